"""``fedrec_agg::trimmed_mean`` (csrc/robust_agg.hip) on the device against its torch oracle.

Shapes: every W with its own sort network shape -- 1, 2, a power of two and one past it up to 32
(W > 16 takes the one-coordinate-per-lane path whatever the alignment) -- and n = 1, 3, 4, 5, 255,
1025, 70001: n % 4 != 0 takes the scalar path, 4 and the multiple-of-4 slices below the 16-byte
path, 70001 more than one block.  Integer-valued operands make every sum exact, so the kernel and
the oracle must agree bit for bit; random operands are held to the sequential-sum bound."""
import pytest
import torch

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import reference as ref
from fedrec_with_pytorchdistributed_amd.parallel.robust import RobustRule

pytestmark = pytest.mark.gpu

WS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32]
NS = [1, 3, 4, 5, 255, 1025, 70001]
NMAX = max(NS) + 3  # one buffer per W, the n are its leading columns; 70004 % 4 == 0
U = 2.0 ** -24
NAN, INF = float("nan"), float("inf")


def _trims(W):
    return sorted({t for t in (0, 1, (W - 1) // 2) if 2 * t < W})


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(got, want):
    """Bitwise equal, but any NaN for a NaN (the kernel rebuilds a kept NaN without its payload)."""
    got, want = got.detach().cpu(), want.detach().cpu()
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(_bits(got)[~nan], _bits(want)[~nan])


def _cols(x, n):
    return x[:, :n].contiguous()


def _run_all(x, dev, check):
    """``check(stack_cpu, trim, out_dev, dropped_dev)`` for every n and valid trim of ``x [W, NMAX]``."""
    W = x.shape[0]
    for n in NS + [NMAX]:  # 70004: the 16-byte path over more than one block
        s = _cols(x, n)
        d = s.to(dev)
        for trim in _trims(W):
            out, dropped = ops.trimmed_mean(d, trim)
            assert out.dtype == torch.float32 and tuple(out.shape) == (n,) and out.device == d.device
            assert dropped.dtype == torch.int64 and tuple(dropped.shape) == (W,)
            check(s, trim, out, dropped)


@pytest.mark.parametrize("W", WS)
def test_integer_operands_match_the_oracle_bitwise(dev, W):
    x = torch.randint(-1024, 1025, (W, NMAX), generator=torch.Generator().manual_seed(W)).float()

    def check(s, trim, out, dropped):
        want, wd = ref.trimmed_mean(s, trim)
        assert torch.equal(_bits(out), _bits(want)), (W, s.shape[1], trim)
        assert torch.equal(dropped.cpu(), wd), (W, s.shape[1], trim)
        assert int(dropped.sum()) == 2 * trim * s.shape[1]

    _run_all(x, dev, check)


@pytest.mark.parametrize("W", WS)
def test_random_operands_stay_within_the_sequential_sum_bound(dev, W):
    """|out - ref64| <= gamma_m sum|kept| / m per element, m = W - 2 trim, gamma_m = m u / (1 - m u),
    u = 2^-24: m - 1 roundings of the sequential sum and one of the division.  Every element."""
    g = torch.Generator().manual_seed(100 + W)
    x = torch.randn(W, NMAX, generator=g) * 10.0 ** (torch.rand(W, NMAX, generator=g) * 6 - 3)

    def check(s, trim, out, dropped):
        m = W - 2 * trim
        r64, wd = ref.trimmed_mean(s, trim, acc_dtype=torch.float64)
        if trim:
            idx = torch.sort(ref.order_keys(s) * 32 + torch.arange(W)[:, None], dim=0).values & 31
            kept = torch.gather(s, 0, idx)[trim:W - trim]
        else:
            kept = s
        bound = (m * U / (1 - m * U)) * kept.double().abs().sum(0) / m
        err = (out.cpu().double() - r64).abs()
        worst = float((err / bound.clamp(min=1e-300)).max())
        print(f"W {W} n {s.shape[1]} trim {trim}: worst err / bound {worst:.3f}")
        assert bool((err <= bound).all()), (W, s.shape[1], trim, worst)
        assert torch.equal(dropped.cpu(), wd), (W, s.shape[1], trim)

    _run_all(x, dev, check)


@pytest.mark.parametrize("W", WS)
def test_ties_go_to_the_lower_client_index(dev, W):
    x = torch.randint(0, 3, (W, NMAX), generator=torch.Generator().manual_seed(200 + W)).float()

    def check(s, trim, out, dropped):
        want, wd = ref.trimmed_mean(s, trim)
        assert torch.equal(_bits(out), _bits(want)), (W, s.shape[1], trim)
        assert torch.equal(dropped.cpu(), wd), (W, s.shape[1], trim)

    _run_all(x, dev, check)


@pytest.mark.parametrize("W", [2, 3, 5, 8, 9, 17, 32])
def test_special_values(dev, W):
    """NaN in <= trim and in > trim clients, +-inf, -0.0 against +0.0, at chosen coordinates of an
    otherwise integer-valued stack: NaN positions, every non-NaN output bit and dropped match."""
    n = 1025
    x = torch.randint(-8, 9, (W, n), generator=torch.Generator().manual_seed(300 + W)).float()
    tmax = (W - 1) // 2
    x[W - 1, 0] = NAN                                  # one NaN client: cut by any trim >= 1
    x[: tmax + 1, 1] = NAN                             # tmax + 1 NaN clients: more than any trim cuts
    x[:tmax, 2] = NAN                                  # exactly tmax (none when tmax = 0)
    x[0, 3], x[W - 1, 3] = INF, -INF
    x[:, 4] = INF                                      # all +inf: stays +inf
    x[0, 5], x[W - 1, 5] = INF, INF                    # inf kept unless trimmed
    x[:, 6] = 0.0
    x[::2, 6] = -0.0                                   # -0.0 ranks below +0.0
    x[:, 7] = -0.0                                     # a sum of -0.0 stays -0.0
    x[0, 8], x[W - 1, 8] = -NAN, NAN                   # the sign of a NaN does not matter
    x[:, 9] = NAN
    x[W // 2, 1000], x[0, 1024] = NAN, -INF            # the same in the last partial vector / tail
    for cols in (slice(0, n), slice(0, 1024)):          # scalar path (n odd), 16-byte path
        s = x[:, cols].contiguous()
        d = s.to(dev)
        for trim in _trims(W):
            out, dropped = ops.trimmed_mean(d, trim)
            want, wd = ref.trimmed_mean(s, trim)
            assert _same(out, want), (W, trim)
            assert torch.equal(dropped.cpu(), wd), (W, trim)
            assert bool(torch.isnan(want[1])) and bool(torch.isnan(want[9]))
            if trim:
                assert bool(torch.isfinite(want[0]))


@pytest.mark.parametrize("W,trim", [(3, 1), (8, 1), (8, 3), (16, 7), (17, 1), (32, 15)])
def test_splitting_the_coordinates_changes_no_bit(dev, W, trim):
    """A contiguous copy of columns [a, b) -- a odd, b - a no multiple of 4: the scalar path -- gives
    the slice of the full (16-byte path) result; the per-client counts of disjoint pieces add up."""
    n = 70000
    g = torch.Generator().manual_seed(400 + W)
    x = (torch.randn(W, n, generator=g) * 10.0 ** (torch.rand(W, n, generator=g) * 6 - 3)).to(dev)
    x[:, ::7] = torch.randint(0, 3, (W, x[:, ::7].shape[1]), generator=g).float().to(dev)  # ties too
    full, dfull = ops.trimmed_mean(x, trim)
    total = torch.zeros_like(dfull)
    for a, b in ((0, 1), (1, 4099), (4099, 4103), (4103, 70000)):
        part, dpart = ops.trimmed_mean(x[:, a:b].contiguous(), trim)
        assert torch.equal(_bits(part), _bits(full[a:b])), (a, b)
        total += dpart
    assert torch.equal(total, dfull)
    # the same columns at a 16-byte-misaligned address (scalar path) and at an aligned one
    buf = torch.empty(W * 4096 + 1, device=dev)
    view = buf[1:].view(W, 4096)
    view.copy_(x[:, :4096])
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    aligned = x[:, :4096].contiguous()
    assert aligned.data_ptr() % 16 == 0
    o1, d1 = ops.trimmed_mean(view, trim)
    o2, d2 = ops.trimmed_mean(aligned, trim)
    assert torch.equal(_bits(o1), _bits(o2)) and torch.equal(d1, d2)
    assert torch.equal(_bits(o2), _bits(full[:4096]))


@pytest.mark.parametrize("kind", ["median", "trimmed_mean"])
def test_rule_combine_on_the_device_equals_the_host(dev, kind):
    rule = RobustRule(kind, 2)
    x = torch.randint(-1024, 1025, (8, 4099), generator=torch.Generator().manual_seed(7)).float()
    x[3] *= -50.0  # a poisoned client
    out, dropped = rule.combine(x.to(dev))
    want, wd = rule.combine(x)
    assert out.is_cuda and torch.equal(_bits(out), _bits(want)) and torch.equal(dropped.cpu(), wd)
    assert int(dropped[3]) == int(dropped.max())


def test_device_op_checks_arguments(dev):
    with pytest.raises(RuntimeError, match="0 <= 2 \\* trim < W"):
        ops.trimmed_mean(torch.zeros(4, 8, device=dev), 2)
    with pytest.raises(RuntimeError, match="must be contiguous"):
        ops.trimmed_mean(torch.zeros(8, 4, device=dev).t(), 1)
