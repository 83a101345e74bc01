"""Low-rank (PowerSGD) star uploads on the host: the plan, the wire form, the oracle's properties, the excluded
combinations and one star round over gloo against the oracles bit for bit."""
import pytest
import torch
from torch import nn

from test_quant_star_cpu import TINY, W, assert_global_is, star

from fedrec_with_pytorchdistributed_amd.config import FedRecConfig
from fedrec_with_pytorchdistributed_amd.models.fedrec_model import FlatParams
from fedrec_with_pytorchdistributed_amd.ops import reference as ref
from fedrec_with_pytorchdistributed_amd.parallel.cdp import ClientDP
from fedrec_with_pytorchdistributed_amd.parallel.lowrank import LowRank
from fedrec_with_pytorchdistributed_amd.parallel.upload import StarUpload
from fedrec_with_pytorchdistributed_amd.train.federated import build_model

# one tile; row and column tails; the user tower's att_fc1 (row tail, many K groups); across a 256-column K slab
# and a 64-column group; a [1, 384] vector and a bias, which must land in rest; ALIGN gaps after 24x40, 72x1040, 7
SHAPES = [(16, 16), (384,), (24, 40), (1, 384), (200, 400), (72, 1040), (7,)]


def flat_of(shapes=SHAPES, device="cpu"):
    return FlatParams([(f"p{i}", nn.Parameter(torch.zeros(s, device=device))) for i, s in enumerate(shapes)])


def int_round(plan, seed, rank=1):
    """``(local, theta, residual, basis)`` whose ``a`` and ``Q`` are small integers: ``a`` has exactly ``rank`` on
    every matrix and ``P = a Q`` is exact in fp32, so what orth zeroes does not hang on a summation order."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda *s: torch.randint(-3, 4, s, generator=g).float()  # noqa: E731
    local, basis = ri(plan.n), ri(plan.F)
    for m, (off, rows, cols, _) in enumerate(plan.mats):
        u, v = ri(rows, rank), ri(cols, rank)
        u[0, :], v[0, :] = 1.0, torch.arange(1, rank + 1).float()  # (no zero factor)
        local[off:off + rows * cols] = (u @ v.t()).reshape(-1)
    return local, torch.zeros(plan.n), torch.zeros(plan.n), basis


@pytest.mark.parametrize("R,mats", [(1, [0, 2, 4, 5]), (4, [0, 2, 4, 5]), (8, [4, 5])])
def test_plan_picks_the_matrices_and_rest_covers_everything_else(R, mats):
    flat = flat_of()
    plan = ref.LowRankPlan([(off, tuple(p.shape)) for _, p, off in flat.views()], flat.flat.numel(), R)
    assert [m[0] for m in plan.mats] == [flat.offsets[i] for i in mats]
    cover = torch.zeros(plan.n, dtype=torch.int32)
    for off, rows, cols, _ in plan.mats:
        cover[off:off + rows * cols] += 1
    for start, ln, pay in plan.rest:
        cover[start:start + ln] += 1
        assert plan.F <= pay and pay + ln <= plan.L
    assert bool((cover == 1).all())  # the alignment padding included
    dense = sum(r * c for _, r, c, _ in plan.mats)
    assert plan.F == sum(R * (r + c) for _, r, c, _ in plan.mats) and plan.L == plan.F + plan.n - dense
    assert LowRank(R).bind(flat).plan.tables["mats"].tolist() == plan.tables["mats"].tolist()  # a pure function


def test_the_head_layouts_six_matrices_send_21280_factor_floats_at_rank_4():
    head = [(384, 768), (400, 768), (400, 400), (400, 400), (400, 400), (200, 400)]
    assert LowRank(4).bind(flat_of(head)).plan.F == 21280


def test_pack_and_unpack_round_trip_and_name_what_is_wrong():
    lr = LowRank(2).bind(flat_of())
    up = torch.randn(lr.plan.L)
    blob = lr.pack(up)
    assert blob.dtype == torch.int32 and torch.equal(lr.unpack(blob, lr.plan.n), up)
    for bad, n in [(blob[:-1], lr.plan.n), (up, lr.plan.n), (blob.reshape(1, -1), lr.plan.n), (blob, lr.plan.n + 64)]:
        with pytest.raises(ValueError, match="low-rank upload"):
            lr.unpack(bad, n)


def test_an_exact_rank_2_delta_at_rank_4_is_sent_whole_with_two_zero_columns():
    lr = LowRank(4).bind(flat_of())
    local, theta, res, lr.basis = int_round(lr.plan, 1, rank=2)
    pay = lr.compress(local, theta, res, 0, 0)
    assert lr.finite(pay)
    for m, (off, rows, cols, _) in enumerate(lr.plan.mats):
        P = lr.plan.factors(pay, m)[0]
        assert bool((P[:, 2:] == 0).all()) and bool((P[:, :2] != 0).any(0).all())
        a = local[off:off + rows * cols]
        # Q' carries the dot-product error of its length against sum |a| |P^| <= max|a| sqrt(rows), R of them meet in d
        tol = 4 * (rows + 2) * rows ** 0.5 * 2.0 ** -24 * float(a.abs().max())
        assert float(res[off:off + rows * cols].abs().max()) <= tol < 1e-3 * float(a.abs().max())
    assert torch.equal(lr.received(theta, pay)[lr.plan.rest[0][0]:][:384], local[lr.plan.rest[0][0]:][:384])


def test_a_zero_delta_sends_zeros_and_a_nan_is_not_finite():
    lr = LowRank(4).bind(flat_of())
    basis, theta = lr.basis.clone(), torch.randn(lr.plan.n)
    res = torch.zeros(lr.plan.n)
    local = theta.clone()
    local[lr.plan.mats[1][0] + 5] = float("nan")
    assert not lr.finite(lr.compress(local, theta, res, 0, 0)) and torch.equal(lr.basis, basis)  # the basis stays
    res.zero_()  # (as the driver does)
    pay = lr.compress(theta.clone(), theta, res, 0, 1)
    assert lr.finite(pay) and not bool(pay.any()) and not bool(res.any())


def test_error_feedback_loses_nothing_and_the_aggregate_is_the_mean_of_what_was_sent():
    flat = flat_of()
    theta = torch.randn(flat.flat.numel())
    ups, sent = [], []
    for c in range(3):
        lr = LowRank(4, seed=c).bind(flat)
        local, res = theta + 0.1 * torch.randn_like(theta), 0.01 * torch.randn_like(theta)
        a = (local - theta) + res
        ups.append(lr.compress(local, theta, res, c, 0))
        d = lr.received(torch.zeros_like(theta), ups[-1]).double()
        # residual = fl(a - d): one rounding of the difference, half an ulp of the residual
        assert bool(((d + res.double() - a.double()).abs() <= 2.0 ** -24 * res.abs().double()).all())
        sent.append(d)
    w = torch.tensor([1.0, 2.0, 5.0])
    new, _ = lr.combine(theta, ups, w)
    want = theta.double() + sum(wc * d for wc, d in zip(w.double(), sent)) / 8.0
    assert float((new.double() - want).abs().max()) <= 8 * 2.0 ** -24 * float(want.abs().max())


@pytest.mark.parametrize("flag,match", [("--secagg.enabled=1", "secagg"), ("--robust_agg=median", "robust_agg"),
                                        ("--upload_topk=0.1", "upload_topk"), ("--upload_bits=8", "upload_bits"),
                                        ("--cdp.clip=1.0", "cdp.clip"), ("--upload_rank=3", "expected 0")])
def test_the_excluded_combinations_fail_at_start_up(flag, match):
    cfg = FedRecConfig()
    assert not LowRank.from_cfg(cfg, "grad_avg").active and StarUpload.from_cfg(cfg, "fedavg_star").basis is None
    cfg.apply_overrides(["--upload_rank=2"])
    assert isinstance(StarUpload.from_cfg(cfg, "fedavg_star"), LowRank)
    with pytest.raises(ValueError, match="fedavg_star"):
        StarUpload.from_cfg(cfg, "param_avg")
    cfg.apply_overrides([flag, "--cdp.noise_multiplier=0"])
    with pytest.raises(ValueError, match=match):
        StarUpload.from_cfg(cfg, "fedavg_star")
        ClientDP.from_cfg(cfg, "fedavg_star", 2)


def expected_round0(d, flags, rank):
    """(the global model after round 0 by the oracles, the flat layout, the codec) from the clients' dumps."""
    cfg = FedRecConfig()
    cfg.apply_overrides(list(flags))
    model = build_model(cfg, torch.device("cpu"))
    theta = model.flat.flat.detach().clone().float()
    ups = []
    for c in range(W):
        lr = LowRank(rank, cfg.seed).bind(model.flat)
        ups.append(lr.compress(torch.load(d / "dump" / f"rank{c + 1}.pt").float(), theta, torch.zeros_like(theta), c, 0))
    return lr.combine(theta, ups, torch.ones(W))[0], model.flat, lr


@pytest.mark.slow
def test_one_low_rank_round_is_the_oracles_bit_for_bit_and_a_restart_restores_the_basis(tmp_path):
    flags = [*TINY, "--upload_rank=2"]
    (rec,) = star(tmp_path, 1, flags, "upload")
    want, flat, lr = expected_round0(tmp_path, flags, 2)
    assert_global_is(tmp_path, want, flat)
    assert rec["clients_accepted"] == W and rec["upload_rank"] == 2 and rec["dense_bytes"] == 4 * lr.plan.n * W
    assert 4 * lr.plan.L * W <= rec["upload_bytes"] <= (4 * lr.plan.L + 256) * W  # (a blob's header)
    whole = tmp_path / "whole"
    star(whole, 2, flags, "upload")
    recs = star(tmp_path, 2, flags, "upload")  # every process starts again and resumes at round 1
    assert recs[-1]["round"] == 1 and recs[-1]["clients_accepted"] == W
    for c in range(W):
        a, b = (torch.load(x / f"client{c}_s.pt", weights_only=True)["UPLOAD_BASIS"] for x in (whole, tmp_path))
        assert a.numel() == lr.plan.F and bool(a.any()) and torch.equal(a.view(torch.int32), b.view(torch.int32))
