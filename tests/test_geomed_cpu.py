"""Geometric-median aggregation on the host: the contract recurrence (``ops.reference.geomed_weights``, 32 rounds on
the Gram matrix) against plain Weiszfeld on the stack, ``RobustRule("geomed")`` under a scaled and a NaN client, the
small cases, and the two-bucket gather on gloo.

Optimality residual ``|| sum_c (z - x_c) / ||z - x_c|| || / W`` in fp64 at n = 257, MEASURED for W = 3, 5, 8, 32:
500 plain fp64 Weiszfeld rounds on the stack 1.1e-16, 7.0e-17, 6.2e-17, 8.2e-17; the contract path (32 rounds)
2.0e-07, 8.2e-10, 7.4e-10, 4.6e-08 (64 rounds: 1.1e-09, 8.1e-10, 7.4e-10, 2.6e-10 -- the floor near 8e-10 is the fp32
subtraction of the centre).  RESIDUAL_MARGIN = 1e-6: a residual r leaves the aggregate about r x the clients' mean
distance from the median, and a millionth of the clients' spread is under the fp32 resolution (6e-8) of any
coordinate larger than 6 % of that spread; the issue's ceiling of 1e-3 is asserted as well."""
import pytest
import torch

from launch_util import run_ranks

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.parallel.robust import RobustRule

NAN = float("nan")
RESIDUAL_MARGIN = 1e-6  # what the contract path may add to the residual of 500 plain fp64 Weiszfeld rounds


def _points(W, n, seed):
    """Gaussian rows; the last (W - 1) // 2 are far outliers."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(W, n, generator=g)
    k = (W - 1) // 2
    x[W - k:] = 30.0 + 20.0 * torch.randn(k, n, generator=g)
    return x.contiguous()


def _residual(x, z):
    d = z[None, :] - x.double()
    return float((d / d.norm(dim=1, keepdim=True)).sum(0).norm()) / x.shape[0]


def _weiszfeld(x, iters):
    x = x.double()
    z = x.mean(0)
    for _ in range(iters):
        w = 1.0 / (x - z).norm(dim=1)
        z = (w[:, None] * x).sum(0) / w.sum()
    return z


def _contract_z(x):
    center, _ = ops.trimmed_mean(x, (x.shape[0] - 1) // 2)
    a, _ = ops.geomed_weights(ops.krum_gram(x, center))
    return (a[:, None] * x.double()).sum(0)


@pytest.mark.parametrize("W", [3, 5, 8, 32])
def test_the_recurrence_reaches_the_geometric_median(W):
    x = _points(W, 257, W)
    base, got = _residual(x, _weiszfeld(x, 500)), _residual(x, _contract_z(x))
    print(f"W {W}: residual after 500 plain rounds {base:.3e}, contract path {got:.3e}")
    assert got <= base + RESIDUAL_MARGIN and got < 1e-3


def _honest(W, n, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(n, generator=g)
    return (base + 1e-2 * torch.randn(W, n, generator=g)).contiguous()


@pytest.mark.parametrize("attack", ["scale", "nan"])
def test_rule_holds_against_one_bad_client(attack):
    W, n, b = 6, 2053, 2
    x = _honest(W, n, 3)
    good = [c for c in range(W) if c != b]
    mean, diam = x[good].double().mean(0), float(torch.cdist(x[good].double(), x[good].double()).max())
    x[b] = x[b] * 1e6 if attack == "scale" else torch.full((n,), NAN)
    rule = RobustRule("geomed")
    out, dropped = rule.combine(x)
    assert float((out.double() - mean).norm()) <= diam and bool(torch.isfinite(out).all())
    assert not float((x.mean(0).double() - mean).norm()) <= diam  # the plain mean: far away, or NaN
    rec = rule.record(dropped, n, W)
    aw = rec.pop("agg_weight")
    assert dropped.dtype == torch.int64 and dropped.tolist() == [n if attack == "nan" and c == b else 0 for c in range(W)]
    assert rec == {"robust_agg": "geomed", "robust_trim": 0, "dropped_share": [float(d > 0) for d in dropped.tolist()]}
    assert aw == rule.weights.tolist() and sum(aw) == pytest.approx(1.0, abs=1e-12)
    assert (aw[b] == 0.0 if attack == "nan" else 0.0 < aw[b] < 1e-5) and all(abs(aw[c] - 0.2) < 0.05 for c in good)


def test_small_cases_give_the_row_or_the_midpoint():
    rule = RobustRule("geomed", trim=7, keep=9)  # both ignored
    assert [rule.trim_for(W) for W in (1, 2, 4, 32)] == [0, 0, 0, 0]
    x = _honest(2, 515, 9)
    out, dropped = rule.combine(x[:1])
    assert torch.equal(out, x[0]) and dropped.tolist() == [0] and rule.weights.tolist() == [1.0]
    out, _ = rule.combine(x)
    assert torch.equal(out, 0.5 * x[0] + 0.5 * x[1])
    same = x[:1].expand(5, -1).contiguous()
    out, dropped = rule.combine(same)  # G = 0: uniform weights
    assert rule.weights.tolist() == pytest.approx([0.2] * 5, abs=1e-15) and dropped.tolist() == [0] * 5
    # five products of 2^-24 x 0.2 |x| each, four sums of 2^-24 x (0.4 + 0.6 + 0.8 + 1.0) |x|, 5 fp32(0.2) = 1 + 2^-26
    assert bool(torch.isfinite(out).all()) and bool(((out - x[0]).abs() <= 4.1 * 2.0 ** -24 * x[0].abs()).all())
    a, dist = ops.geomed_weights(torch.full((3, 3), NAN, dtype=torch.float64))  # nobody valid
    assert bool(torch.isnan(a).all()) and dist.tolist() == [float("inf")] * 3
    # rows of weight zero are not read; a NaN weight reaches every coordinate
    x[0] = NAN
    assert torch.equal(ops.geomed_combine(x, torch.tensor([0.0, 1.0], dtype=torch.float64)), x[1])
    assert bool(torch.isnan(ops.geomed_combine(x, torch.tensor([0.0, NAN], dtype=torch.float64))).all())


def test_two_bucket_gather_equals_combine_on_the_whole_stack():
    outs = run_ranks([["tests/_geomed_worker.py"]] * 2, timeout=120)
    assert all(rc == 0 and "GEOMED OK" in out for rc, out in outs), outs[0][1][-2000:]
    assert outs[0][1].split("GEOMED OK")[1].split()[0] == outs[1][1].split("GEOMED OK")[1].split()[0]
