"""Sparsified uploads through the star drivers on gloo: 1 coordinator + 2 clients, tiny shards.

The clients train exactly one round, so the parameters they dump at the end are what they compressed;
the round's global model is the seed-initialised one every participant builds.  The test recomputes
``sparse_combine(theta_g0, topk_delta(dump_k, theta_g0, 0, k) ...)`` with the oracles and expects the
coordinator's ``global_model_round0.pt`` to hold exactly those bits -- with the coordinator combining
the uploads, and with the clients combining among themselves."""
import json

import pytest
import torch

from launch_util import run_ranks

from fedrec_with_pytorchdistributed_amd.config import FedRecConfig
from fedrec_with_pytorchdistributed_amd.ops import reference as ref
from fedrec_with_pytorchdistributed_amd.parallel.sparsify import Sparsifier
from fedrec_with_pytorchdistributed_amd.train.federated import build_model

TINY = ["--data_dir=synthetic:tiny", "--backbone.name=tiny", "--round_timeout_s=120", "--collective_timeout_s=120"]
W = 2


def _ok(outs):
    for rc, out in outs:
        assert rc == 0, out[-3000:]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def star(d, rounds, flags, agg, env=None, timeout=300):
    """Run the star; returns the round records."""
    flags = [*flags, f"--snapshot_path={d}/s.pt"]
    server = ["server.py", str(rounds), *flags]
    client = ["client.py", "1", "16", "1", "0", "c", *flags]
    outs = run_ranks([server] + [client] * W, {"FEDREC_DUMP_FLAT": str(d / "dump"), "FEDREC_STAR_AGG": agg, **(env or {})},
                     timeout=timeout)
    _ok(outs)
    with open(d / "metrics.jsonl") as f:
        rows = [json.loads(ln) for ln in f if ln.strip()]
    return [r for r in rows if not r.get("final_global")]


def expected_round0(d, flags, fraction):
    """(the global model after round 0 by the oracles, the flat layout) from the clients' dumps."""
    cfg = FedRecConfig()
    cfg.apply_overrides(list(flags))
    model = build_model(cfg, torch.device("cpu"))
    theta = model.flat.flat.detach().clone().float()
    n = theta.numel()
    k = Sparsifier(fraction).k_for(n)
    idxs, vals = [], []
    for c in range(W):
        local = torch.load(d / "dump" / f"rank{c + 1}.pt").float()
        assert not torch.equal(local, theta)  # it trained
        idx, val = ref.topk_delta(local, theta, torch.zeros(n), k)
        idxs.append(idx)
        vals.append(val)
    return ref.sparse_combine(theta, torch.stack(idxs), torch.stack(vals), torch.ones(W)), model.flat, n, k


def assert_global_is(d, want, flat):
    g = torch.load(d / "global_model_round0.pt", weights_only=True)
    for name, p, off in flat.views():
        assert torch.equal(_bits(g[name].reshape(-1)), _bits(want[off:off + p.numel()])), name


@pytest.mark.slow
@pytest.mark.parametrize("agg", ["upload", "allreduce"])
def test_one_sparse_round_is_the_oracles_bit_for_bit(tmp_path, agg):
    d = tmp_path / agg
    flags = [*TINY, "--upload_topk=0.05"]
    recs = star(d, 1, flags, agg)
    want, flat, n, k = expected_round0(d, TINY, 0.05)
    assert_global_is(d, want, flat)
    (rec,) = recs
    assert rec["upload_topk"] == 0.05 and rec["clients_accepted"] == W
    assert rec["dense_bytes"] == 4 * n * W and 8 * k * W <= rec["upload_bytes"] < rec["dense_bytes"] // 4


@pytest.mark.slow
def test_two_rounds_carry_a_residual_and_upload_less(tmp_path):
    d = tmp_path / "two"
    recs = star(d, 2, [*TINY, "--upload_topk=0.05"], "upload")
    assert [r["round"] for r in recs] == [0, 1]
    for r in recs:
        assert 0 < r["upload_bytes"] < r["dense_bytes"]
    for c in range(W):
        snap = torch.load(d / f"client{c}_s.pt", weights_only=True)
        res = snap["UPLOAD_RESIDUAL"]
        assert res.dtype == torch.float32 and res.numel() == snap["FLAT_PARAMS"].numel()
        assert bool((res != 0).any()) and bool(torch.isfinite(res).all())
        assert int((res == 0).sum()) >= Sparsifier(0.05).k_for(res.numel())  # what was just sent is cleared


@pytest.mark.slow
def test_the_option_off_leaves_the_records_as_they_were(tmp_path):
    d = tmp_path / "off"
    (rec,) = star(d, 1, [*TINY, "--upload_topk=0"], "upload")
    assert not {"upload_topk", "upload_bytes", "dense_bytes"} & set(rec)
    snap = torch.load(d / "client0_s.pt", weights_only=True)
    assert "UPLOAD_RESIDUAL" not in snap
