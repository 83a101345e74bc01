"""Block-quantized uploads through the star drivers on gloo: 1 coordinator + 2 clients, tiny shards.

The clients train exactly one round, so the parameters they dump at the end are what they compressed;
the round's global model is the seed-initialised one every participant builds.  The test recomputes
``dequant_combine(theta_g0, quantize_delta(dump_k, theta_g0, 0, ...))`` with the oracles -- Philox key
``cfg.seed``, offset ``(client << 32) | round`` -- and expects the coordinator's
``global_model_round0.pt`` to hold exactly those bits, with the coordinator combining the uploads and
with the clients combining among themselves; the same for the form composed with ``--upload_topk``."""
import json

import pytest
import torch

from launch_util import run_ranks

from fedrec_with_pytorchdistributed_amd.config import FedRecConfig
from fedrec_with_pytorchdistributed_amd.ops import reference as ref
from fedrec_with_pytorchdistributed_amd.parallel.control import encode_tensor
from fedrec_with_pytorchdistributed_amd.parallel.quantize import Quantizer, Upload
from fedrec_with_pytorchdistributed_amd.parallel.sparsify import Sparsifier
from fedrec_with_pytorchdistributed_amd.train.federated import build_model

TINY = ["--data_dir=synthetic:tiny", "--backbone.name=tiny", "--round_timeout_s=120", "--collective_timeout_s=120"]
W = 2


def _ok(outs):
    for rc, out in outs:
        assert rc == 0, out[-3000:]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def star(d, rounds, flags, agg, env=None, timeout=300, check=True):
    """Run the star; returns the round records (``check=False``: the ranks' (returncode, output))."""
    flags = [*flags, f"--snapshot_path={d}/s.pt"]
    server = ["server.py", str(rounds), *flags]
    client = ["client.py", "1", "16", "1", "0", "c", *flags]
    outs = run_ranks([server] + [client] * W, {"FEDREC_DUMP_FLAT": str(d / "dump"), "FEDREC_STAR_AGG": agg, **(env or {})},
                     timeout=timeout)
    if not check:
        return outs
    _ok(outs)
    with open(d / "metrics.jsonl") as f:
        rows = [json.loads(ln) for ln in f if ln.strip()]
    return [r for r in rows if not r.get("final_global")]


def expected_round0(d, flags, bits, fraction=0.0):
    """(the global model after round 0 by the oracles, the flat layout, n) from the clients' dumps."""
    cfg = FedRecConfig()
    cfg.apply_overrides(list(flags))
    model = build_model(cfg, torch.device("cpu"))
    theta = model.flat.flat.detach().clone().float()
    n = theta.numel()
    ups = []
    for c in range(W):
        local = torch.load(d / "dump" / f"rank{c + 1}.pt").float()
        assert not torch.equal(local, theta)  # it trained
        offset = (c << 32) | 0
        if fraction:
            k = Sparsifier(fraction).k_for(n)
            idx, val = ref.topk_delta(local, theta, torch.zeros(n), k)
            codes, scales = ref.quantize_delta(val, torch.zeros(k), torch.zeros(k), bits, cfg.seed, offset)
            ups.append((idx, ref.dequantize(codes, scales, bits, k)))
        else:
            ups.append(ref.quantize_delta(local, theta, torch.zeros(n), bits, cfg.seed, offset))
    a, b = (torch.stack(x) for x in zip(*ups))
    if fraction:
        want = ref.sparse_combine(theta, a, b, torch.ones(W))
    else:
        want = ref.dequant_combine(theta, a, b, torch.ones(W), bits)
    assert not torch.equal(want, theta)
    return want, model.flat, n


def assert_global_is(d, want, flat, r=0):
    g = torch.load(d / f"global_model_round{r}.pt", weights_only=True)
    for name, p, off in flat.views():
        assert torch.equal(_bits(g[name].reshape(-1)), _bits(want[off:off + p.numel()])), name


def _header_bytes():
    return len(encode_tensor(torch.zeros(0, dtype=torch.int32)))


@pytest.mark.slow
@pytest.mark.parametrize("agg", ["upload", "allreduce"])
@pytest.mark.parametrize("bits", [8, 4])
def test_one_quantized_round_is_the_oracles_bit_for_bit(tmp_path, bits, agg):
    d = tmp_path / agg
    recs = star(d, 1, [*TINY, f"--upload_bits={bits}"], agg)
    want, flat, n = expected_round0(d, TINY, bits)
    assert_global_is(d, want, flat)
    (rec,) = recs
    assert rec["upload_bits"] == bits and rec["clients_accepted"] == W and "upload_topk" not in rec
    assert rec["dense_bytes"] == 4 * n * W
    payload = W * 4 * (-(-n // 256) + -(-n * bits // 32))
    assert rec["upload_bytes"] >= payload
    # payload / dense is 0.2539 (8 bits) and 0.1289 (4 bits); the rest is the blob's header, which the
    # tiny model's n must leave room for below the bound
    bound = {8: 0.27, 4: 0.15}[bits]
    assert payload + W * _header_bytes() < bound * rec["dense_bytes"], (n, _header_bytes())
    assert rec["upload_bytes"] < bound * rec["dense_bytes"]


@pytest.mark.slow
@pytest.mark.parametrize("agg", ["upload", "allreduce"])
def test_one_round_composed_with_topk_is_the_oracles_bit_for_bit(tmp_path, agg):
    d = tmp_path / agg
    recs = star(d, 1, [*TINY, "--upload_topk=0.05", "--upload_bits=8"], agg)
    want, flat, n = expected_round0(d, TINY, 8, 0.05)
    assert_global_is(d, want, flat)
    (rec,) = recs
    k = Sparsifier(0.05).k_for(n)
    assert rec["upload_bits"] == 8 and rec["upload_topk"] == 0.05 and rec["clients_accepted"] == W
    assert rec["dense_bytes"] == 4 * n * W
    # a sent coordinate costs 5 bytes: idx + one code; then the scales, the padding and the blob's header
    # (an empty tensor's, plus room for the digits of the length it spells out)
    assert W * 4 * (k + -(-k // 256) + -(-k // 4)) <= rec["upload_bytes"] <= W * (5 * k + 4 * (-(-k // 256)) + 4 + _header_bytes() + 16)


@pytest.mark.slow
def test_a_client_restart_between_two_rounds_resumes_the_residual(tmp_path):
    flags = [*TINY, "--upload_bits=4"]
    whole = tmp_path / "whole"
    recs = star(whole, 2, flags, "upload")
    assert [r["round"] for r in recs] == [0, 1]
    cut = tmp_path / "cut"
    star(cut, 1, flags, "upload")
    for c in range(W):
        res = torch.load(cut / f"client{c}_s.pt", weights_only=True)["UPLOAD_RESIDUAL"]
        assert res.dtype == torch.float32 and bool((res != 0).any()) and bool(torch.isfinite(res).all())
    recs = star(cut, 2, flags, "upload")  # every process starts again and resumes at round 1
    assert [r["round"] for r in recs][-1] == 1
    a = torch.load(whole / "global_model_round1.pt", weights_only=True)
    b = torch.load(cut / "global_model_round1.pt", weights_only=True)
    assert set(a) == set(b)
    for name in a:
        assert torch.equal(_bits(a[name].float()), _bits(b[name].float())), name
    for c in range(W):
        ra = torch.load(whole / f"client{c}_s.pt", weights_only=True)["UPLOAD_RESIDUAL"]
        rb = torch.load(cut / f"client{c}_s.pt", weights_only=True)["UPLOAD_RESIDUAL"]
        assert torch.equal(_bits(ra), _bits(rb))


@pytest.mark.slow
def test_a_poisoned_client_is_rejected_and_the_round_completes_on_the_quorum(tmp_path):
    d = tmp_path / "nan"
    outs = star(d, 1, [*TINY, "--upload_bits=8", "--quorum=0.5"], "upload", {"FEDREC_FAULT": "client:1:round:0:nan"},
                check=False)
    _ok(outs)
    assert "dropping client 1" in outs[0][1] and "not a finite value" in outs[0][1]
    with open(d / "metrics.jsonl") as f:
        rec = [json.loads(ln) for ln in f if ln.strip()][0]
    assert rec["clients_accepted"] == 1 and rec["upload_bits"] == 8
    g = torch.load(d / "global_model_round0.pt", weights_only=True)
    assert all(bool(torch.isfinite(v).all()) for v in g.values())
    res = torch.load(d / "client1_s.pt", weights_only=True)["UPLOAD_RESIDUAL"]
    assert not bool(res.any())  # nothing of the poisoned round comes back


def test_the_option_off_is_inactive_and_the_excluded_combinations_fail_at_start_up():
    cfg = FedRecConfig()
    assert cfg.upload_bits == 0 and not Quantizer.from_cfg(cfg, "grad_avg").active
    for flags, driver, text in [
        (["--upload_bits=3"], "fedavg_star", "upload_bits=3: expected 0 (off), 8 or 4"),
        (["--upload_bits=16"], "fedavg_star", "upload_bits=16: expected 0 (off), 8 or 4"),
        (["--upload_bits=8"], "grad_avg", "upload_bits=8 is not available with mode=grad_avg"),
        (["--upload_bits=4"], "param_avg", "upload_bits=4 is not available with mode=param_avg"),
        (["--upload_bits=8", "--secagg.enabled=1"], "fedavg_star", "cannot be combined with secagg.enabled=1"),
        (["--upload_bits=8", "--robust_agg=median"], "fedavg_star", "cannot be combined with robust_agg=median"),
    ]:
        cfg = FedRecConfig()
        cfg.apply_overrides(flags)
        with pytest.raises(ValueError) as e:
            Quantizer.from_cfg(cfg, driver)
        assert text in str(e.value)


@pytest.mark.slow
def test_an_excluded_combination_stops_the_processes_at_start_up(tmp_path):
    outs = star(tmp_path, 1, [*TINY, "--upload_bits=8", "--robust_agg=median"], "upload", check=False, timeout=120)
    assert all(rc not in (0, None) for rc, _ in outs)
    assert all("upload_bits=8 cannot be combined with robust_agg=median" in out for _, out in outs)


def test_pack_and_unpack_round_trip_and_name_what_is_wrong():
    n = 777
    g = torch.Generator().manual_seed(3)
    for bits, fraction in ((8, 0.0), (4, 0.0), (8, 0.05), (4, 0.05)):
        qz = Quantizer(bits, 5, fraction)
        res = torch.zeros(n)
        local, theta = torch.randn(n, generator=g), torch.randn(n, generator=g)
        up = qz.compress(local, theta, res, 1, 2)
        blob = qz.pack(up)
        assert blob.dtype == torch.int32 and blob.dim() == 1 and blob.numel() == qz.words_for(n)
        back = qz.unpack(blob, n)
        assert torch.equal(back.codes, up.codes) and torch.equal(_bits(back.scales), _bits(up.scales))
        assert (back.idx is None) == (fraction == 0.0) and (fraction == 0.0 or torch.equal(back.idx, up.idx))
        # error feedback: what was sent plus what was kept is the delta
        sent = qz.received(torch.zeros(n), back)
        assert bool(((sent + res) - (local - theta)).abs().max() <= (local - theta).abs().max() * 2.0 ** -22)
        with pytest.raises(ValueError, match="expected an int32"):
            qz.unpack(blob[:-1], n)
        bad = blob.clone()
        bad[qz.m_for(n) if fraction else 0] = 0x7FC00000
        with pytest.raises(ValueError, match="not a finite value"):
            qz.unpack(bad, n)
        if ref.quant_sizes(qz.m_for(n), bits)[0] % 4:  # (the top byte of the last word is padding)
            bad = blob.clone()
            bad[-1] |= 0x40000000
            with pytest.raises(ValueError, match="padding bytes"):
                qz.unpack(bad, n)
    up = Upload(None, torch.zeros(3, dtype=torch.uint8), torch.ones(1))
    assert Quantizer.pack(up).tolist() == [0x3F800000, 0]
