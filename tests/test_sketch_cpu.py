"""Count-sketch uploads on the host: the hash's block permutations, planted recovery through one ``combine`` of the
oracles, what ``from_cfg`` rejects and ``unpack`` refuses, and a two-client star on gloo with a coordinator restart."""
import pytest
import torch

from test_quant_star_cpu import TINY, W, star

from fedrec_with_pytorchdistributed_amd.config import FedRecConfig
from fedrec_with_pytorchdistributed_amd.ops import reference as ref
from fedrec_with_pytorchdistributed_amd.parallel.cdp import ClientDP
from fedrec_with_pytorchdistributed_amd.parallel.sketch import SketchUpload
from fedrec_with_pytorchdistributed_amd.parallel.upload import StarUpload
from fedrec_with_pytorchdistributed_amd.train.federated import build_model


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def test_every_row_of_every_block_is_a_permutation_of_the_tile_and_the_inverse_undoes_it():
    T, C, n = ref.SKETCH_T, 4096, 3 * 4096 - 5
    plan = ref.sketch_plan(n, C, 7)
    assert plan.dtype == torch.int32 and tuple(plan.shape) == (3, 8, 4) and torch.equal(plan, ref.sketch_plan(n, C, 7))
    assert not torch.equal(plan, ref.sketch_plan(n, C, 8))
    w = plan.to(torch.int64) & 0xFFFFFFFF
    p = torch.arange(T)
    for q in range(3):
        i = q * C + 2 * T + p  # tile 2 of block q
        j, _ = ref.sketch_hash(plan, i, 5, C)
        assert bool((j // T == ((2 + w[q, 7, 0]) & (C // T - 1))).all())  # one rotation for all rows
        for r in range(5):
            m, o, _, minv = w[q, r]
            j_lo = j[r] % T
            assert j_lo.unique().numel() == T
            assert torch.equal((((j_lo - o) & 0xFFFFFFFF) * minv) & (T - 1), p)
    signs = ref.sketch_hash(plan, torch.arange(n), 5, C)[1].float().mean(1)
    assert bool(((signs - 0.5).abs() < 0.02).all())  # (five fair coins over 12283 coordinates: 4 sigma is 0.018)


def test_sixteen_planted_coordinates_come_back_through_one_combine():
    n, k = 20000, 16
    g = torch.Generator().manual_seed(0)
    sk = SketchUpload(k / n, 5, 4096, seed=0).plan_for(n)
    assert sk.k == k and sk.basis.shape == (5, 4096) and ref.sketch_plan(n, 4096, 0).shape[0] == 5  # nb
    theta = torch.randn(n, generator=g)
    pos = torch.randperm(n, generator=g)[:k].sort().values
    planted = torch.where(torch.rand(k, generator=g) < 0.5, -1.0, 1.0)
    delta = (torch.rand(n, generator=g) * 2 - 1) * 1e-3
    delta[pos] = planted
    up = sk.unpack(sk.pack(sk.compress(theta + delta, theta, None, 0, 0)), n)
    new, dropped = sk.combine(theta, [up], [1.0])
    assert dropped is None
    got = new - theta
    assert torch.equal(got.nonzero().flatten(), pos)
    # a bucket holds one coordinate of each of the nb = 5 blocks: at most 4 noise terms and the roundings of theta
    assert bool(((new[pos] - theta[pos]) - planted).abs().max() <= 5e-3)
    j, _ = ref.sketch_hash(sk._plan("cpu"), pos, 5, 4096)
    assert not bool(torch.stack([sk.basis[r, j[r]] for r in range(5)]).view(torch.int32).any())  # +0.0
    assert bool(sk.basis.any())  # the noise that was not recovered stays


def test_from_cfg_rejects_what_cannot_hold_takes_client_dp_and_unpack_refuses_another_form():
    cfg = FedRecConfig()
    assert cfg.upload_sketch == 0.0 and (cfg.upload_sketch_rows, cfg.upload_sketch_cols) == (5, 0)
    assert not isinstance(StarUpload.from_cfg(cfg, "fedavg_star"), SketchUpload)
    for flags, driver, text in [
        (["--upload_sketch=0.01"], "grad_avg", "upload_sketch=0.01 is not available with mode=grad_avg"),
        (["--upload_sketch=0.01"], "param_avg", "upload_sketch=0.01 is not available with mode=param_avg"),
        (["--upload_sketch=0.01", "--secagg.enabled=1"], "fedavg_star", "cannot be combined with secagg.enabled=1"),
        (["--upload_sketch=0.01", "--robust_agg=median"], "fedavg_star", "cannot be combined with robust_agg=median"),
        (["--upload_sketch=0.01", "--upload_topk=0.1"], "fedavg_star", "cannot be combined with upload_topk=0.1"),
        (["--upload_sketch=0.01", "--upload_bits=8"], "fedavg_star", "cannot be combined with upload_bits=8"),
        (["--upload_sketch=0.01", "--upload_rank=4"], "fedavg_star", "cannot be combined with upload_rank=4"),
        (["--upload_sketch=0.01", "--upload_sketch_rows=2"], "fedavg_star", "upload_sketch_rows=2: expected 1, 3 or 5"),
        (["--upload_sketch=0.01", "--upload_sketch_cols=3000"], "fedavg_star", "upload_sketch_cols=3000: expected 0"),
        (["--upload_sketch=0.01", "--upload_sketch_cols=512"], "fedavg_star", "upload_sketch_cols=512: expected 0"),
        (["--upload_sketch=1.5"], "fedavg_star", "expected 0 <= upload_sketch <= 1"),
    ]:
        cfg = FedRecConfig()
        cfg.apply_overrides(flags)
        with pytest.raises(ValueError) as e:
            StarUpload.from_cfg(cfg, driver)
        assert text in str(e.value)
    cfg = FedRecConfig()
    cfg.apply_overrides(["--upload_sketch=0.01", "--cdp.clip=1.0", "--cdp.noise_multiplier=1.0", "--weighted_fedavg=0"])
    sk = StarUpload.from_cfg(cfg, "fedavg_star")
    assert isinstance(sk, SketchUpload) and not sk.uses_residual and ClientDP.from_cfg(cfg, "fedavg_star", 2).active
    cfg = FedRecConfig()
    cfg.apply_overrides(["--upload_sketch=0.01", "--weighted_fedavg=1"])
    assert isinstance(StarUpload.from_cfg(cfg, "fedavg_star"), SketchUpload)  # (the mean is linear)
    flat = build_model(_tiny_cfg(), torch.device("cpu")).flat
    n = flat.flat.numel()
    sk.bind(flat)
    assert (sk.k, sk.cols) == (-(-n // 100), ref.sketch_cols_for(-(-n // 100))) and sk.cols >= 4 * sk.k > sk.cols // 2
    with pytest.raises(ValueError, match="nothing would be compressed"):
        SketchUpload(0.5, 5, 0).bind(flat)
    blob = sk.pack(torch.zeros(5, sk.cols))
    assert blob.dtype == torch.int32 and blob.shape == (5 * sk.cols,) and sk.unpack(blob, n).shape == (5, sk.cols)
    for bad, m in ((blob.float(), n), (blob[:-1], n), (blob.view(5, -1), n), (blob, n - 1)):
        with pytest.raises(ValueError, match="expected an int32"):
            sk.unpack(bad, m)


def _tiny_cfg():
    cfg = FedRecConfig()
    cfg.apply_overrides(list(TINY))
    return cfg


@pytest.mark.slow
def test_a_two_client_star_sends_tables_keeps_no_client_residual_and_a_restarted_coordinator_keeps_its_error_table(tmp_path):
    flags = [*TINY, "--upload_sketch=0.01", "--upload_sketch_rows=3"]
    whole, cut = tmp_path / "whole", tmp_path / "cut"
    recs = star(whole, 2, flags, "upload")
    assert [r["round"] for r in recs] == [0, 1] and all(r["clients_accepted"] == W for r in recs)
    sk = SketchUpload(0.01, 3).bind(build_model(_tiny_cfg(), torch.device("cpu")).flat)
    for r in recs:
        assert (r["upload_sketch"], r["upload_sketch_rows"], r["upload_sketch_cols"]) == (0.01, 3, sk.cols)
        assert 4 * 3 * sk.cols * W <= r["upload_bytes"] <= (4 * 3 * sk.cols + 256) * W < r["dense_bytes"] == 4 * sk.n * W
    star(cut, 1, flags, "upload")
    first = torch.load(cut / "s.pt", weights_only=True)["EXTRAS"][SketchUpload.STATE]
    assert first.shape == (3, sk.cols) and bool(first.any()) and bool(torch.isfinite(first).all())
    assert [r["round"] for r in star(cut, 2, flags, "upload")][-1] == 1  # every process starts again and resumes at round 1
    for c in range(W):
        snap = torch.load(cut / f"client{c}_s.pt", weights_only=True)
        assert "UPLOAD_RESIDUAL" not in snap
    a, b = (torch.load(d / "s.pt", weights_only=True) for d in (whole, cut))
    assert torch.equal(_bits(a["EXTRAS"][SketchUpload.STATE]), _bits(b["EXTRAS"][SketchUpload.STATE]))
    assert not torch.equal(_bits(first), _bits(b["EXTRAS"][SketchUpload.STATE]))
    ga, gb = (torch.load(d / "global_model_round1.pt", weights_only=True) for d in (whole, cut))
    for name in ga:
        assert torch.equal(_bits(ga[name].float()), _bits(gb[name].float())), name
