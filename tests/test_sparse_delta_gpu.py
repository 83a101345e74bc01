"""``fedrec_sparse::topk_delta`` / ``combine`` (csrc/sparse_delta.hip) on the device, bit for bit against
their torch oracles.  The contract is exact, so equality with the oracle also proves independence of
grid, block and launch order.  A NaN may stand for any NaN, but only where the oracle's value is one.

Shapes of ``topk_delta``: n = 1, 2, 3, every power of two from 64 to 65536 with both neighbours (one
element either side of every wave, block and tile span the kernel could use), 70001 and 200003 (many
blocks, ragged tail); k in {1, 2, n // 100, n // 2, n - 1, n}.  The value families make each stage of
the radix select decide: distinct keys; almost everything tied; one constant / mixed +-0.0 (the first
k indices win); keys that differ in the lowest digit only, in the top digit only; inf, NaN (more of
them than k), denormals.  Each family draws one buffer; an n is its leading elements."""
import pytest
import torch

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

NS = [1, 2, 3] + [p + d for e in range(6, 17) for p in [1 << e] for d in (-1, 0, 1)] + [70001, 200003]
NMAX = max(NS)
NAN, INF = float("nan"), float("inf")


def _ks(n):
    return sorted({min(max(k, 1), n) for k in (1, 2, max(1, n // 100), n // 2, n - 1, n)})


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(got, want):
    """Bitwise equal, but any NaN where (and only where) the oracle holds a NaN."""
    got, want = got.detach().cpu(), want.detach().cpu()
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(_bits(got)[~nan], _bits(want)[~nan])


def _from_bits(b):
    return b.to(torch.int32).view(torch.float32)


def _family(name):
    """(local, global, residual) of NMAX elements on the host."""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    n = NMAX
    z = torch.zeros(n)
    normal = lambda: torch.randn(n, generator=g) * 2.0 ** torch.randint(-20, 21, (n,), generator=g).float()
    sign = lambda: (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
    if name == "distinct":
        return normal(), normal(), normal()
    if name == "ties":
        ints = lambda: torch.randint(-3, 4, (n,), generator=g).float()
        return ints(), ints(), ints()
    if name == "constant":
        return torch.full((n,), -1.25), z, z
    if name == "zeros":  # (-0 - 0) + -0 = -0, (+0 - 0) + +0 = +0: a keeps the mixed signs
        s = torch.where(torch.randint(0, 2, (n,), generator=g) == 1, torch.tensor(-0.0), torch.tensor(0.0))
        return s, z, s.clone()
    if name == "low_digit":
        return (1.0 + torch.randint(0, 8, (n,), generator=g).float() * 2.0 ** -23) * sign(), z, z
    if name == "top_digit":  # bits 30..21 drawn (finite), bits 20..0 one pattern
        top = torch.randint(1, 1016, (n,), generator=g)
        return _from_bits((top << 21) | 0x0ABCDE) * sign(), z, z
    if name == "special":
        l, gl, e = normal(), normal(), normal()
        l[::5], l[1::7], l[2::11] = NAN, INF, -INF          # n / 5 NaNs: more than the small k
        l[3::13], gl[3::13], e[3::13] = 1e-41, 3e-42, -2e-41  # denormal operands and results
        gl[1::14] = INF                                      # inf - inf: a NaN made by the subtraction
        l[4::17] = -NAN
        return l, gl, e
    raise KeyError(name)


FAMILIES = ["distinct", "ties", "constant", "zeros", "low_digit", "top_digit", "special"]


def _check(l, gl, e, k, dev, views=None):
    want_res = e.clone()
    want_idx, want_val = ref.topk_delta(l, gl, want_res, k)
    dl, dg, de = views if views is not None else (l.to(dev), gl.to(dev), e.to(dev))
    idx, val = ops.topk_delta(dl, dg, de, k)
    n = l.numel()
    assert idx.dtype == torch.int32 and val.dtype == torch.float32 and idx.device == de.device
    assert tuple(idx.shape) == (k,) and tuple(val.shape) == (k,)
    assert torch.equal(idx.cpu(), want_idx), (n, k)
    assert _same(val, want_val), (n, k)
    assert _same(de, want_res), (n, k)


@pytest.mark.parametrize("family", FAMILIES)
def test_topk_delta_matches_the_oracle_bit_for_bit(dev, family):
    L, G, E = _family(family)
    for n in NS:
        l, gl, e = L[:n].clone(), G[:n].clone(), E[:n].clone()
        for k in _ks(n):
            _check(l, gl, e, k, dev)


@pytest.mark.parametrize("family", ["ties", "special"])
def test_topk_delta_on_views_offset_by_one_element(dev, family):
    """``x[1:]``: every pointer 4 bytes past a 16-byte line (the 16-byte body starts 3 elements in), and
    residual alone offset (local / global then take the scalar loads)."""
    L, G, E = _family(family)
    for n in (1, 2, 3, 4, 5, 63, 4096, 4099, 70001):
        l, gl, e = L[:n].clone(), G[:n].clone(), E[:n].clone()
        for k in _ks(n):
            for shift in ((1, 1, 1), (0, 0, 1), (2, 3, 0)):
                views = []
                for t, s in zip((l, gl, e), shift):
                    buf = torch.empty(n + s, device=dev)
                    buf[s:].copy_(t)
                    views.append(buf[s:])
                    assert views[-1].data_ptr() % 16 == 4 * s and views[-1].is_contiguous()
                _check(l, gl, e, k, dev, views)


def test_error_feedback_rounds_on_the_device_equal_the_host(dev):
    """Five rounds with the residual carried: uploads and residual equal the oracle's every round."""
    n, k = 70001, 700
    g = torch.Generator().manual_seed(9)
    res_h, res_d = torch.zeros(n), torch.zeros(n, device=dev)
    for _ in range(5):
        theta = torch.randn(n, generator=g)
        local = theta + 0.01 * torch.randn(n, generator=g)
        wi, wv = ref.topk_delta(local, theta, res_h, k)
        gi, gv = ops.topk_delta(local.to(dev), theta.to(dev), res_d, k)
        assert torch.equal(gi.cpu(), wi) and _same(gv, wv) and _same(res_d, res_h)


# ---- combine -------------------------------------------------------------------------------------
def _lists(W, n, k, g, where="anywhere"):
    rows = []
    for _ in range(W):
        if where == "one_tile" and n > 8192 and k <= 4096:  # all inside the second tile
            pick = 4096 + torch.randperm(4096, generator=g)[:k]
        else:
            pick = torch.randperm(n, generator=g)[:k]
        rows.append(torch.sort(pick).values)
    return torch.stack(rows).to(torch.int32)


@pytest.mark.parametrize("W", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 65, 4097, 70001])
def test_combine_matches_the_oracle_bit_for_bit(dev, W, n):
    g = torch.Generator().manual_seed(W * 100003 + n)
    for k in sorted({1, n // 100 or 1, n}):
        for where in ("anywhere", "one_tile"):  # k = 1 / n // 100: most tiles see no entry at all
            idx = _lists(W, n, k, g, where)
            for kind in ("integer", "random"):
                if kind == "integer":
                    base = torch.randint(-99, 100, (n,), generator=g).float()
                    val = torch.randint(-99, 100, (W, k), generator=g).float()
                    w = torch.ones(W)
                else:
                    base, val = torch.randn(n, generator=g), torch.randn(W, k, generator=g)
                    w = torch.rand(W, generator=g) + 0.25
                want = ref.sparse_combine(base, idx, val, w)
                out = ops.sparse_combine(base.to(dev), idx.to(dev), val.to(dev), w.to(dev))
                assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (n,)
                assert torch.equal(_bits(out), _bits(want)), (W, n, k, where, kind)


def test_combine_on_a_misaligned_base(dev):
    n, W, k = 8200, 2, 100
    g = torch.Generator().manual_seed(4)
    base, val, w = torch.randn(n, generator=g), torch.randn(W, k, generator=g), torch.tensor([2.0, 3.0])
    idx = _lists(W, n, k, g)
    buf = torch.empty(n + 1, device=dev)
    buf[1:].copy_(base)
    out = ops.sparse_combine(buf[1:], idx.to(dev), val.to(dev), w.to(dev))
    assert torch.equal(_bits(out), _bits(ref.sparse_combine(base, idx, val, w)))


def test_combine_stays_in_bounds_whatever_idx_holds(dev):
    """The kernel trusts nothing about idx: unsorted, repeated, negative and >= n entries.  It must
    return, and every coordinate no in-range index names is base + 0 / wsum."""
    n, W, k = 70001, 3, 5000
    g = torch.Generator().manual_seed(6)
    base = torch.randn(n, generator=g)
    idx = torch.randint(-3 * n, 4 * n, (W, k), generator=g).to(torch.int32)
    idx[0, :4] = torch.tensor([-2 ** 31, 2 ** 31 - 1, -1, n], dtype=torch.int32)
    val, w = torch.randn(W, k, generator=g), torch.tensor([1.0, 2.0, 0.5])
    out = ops.sparse_combine(base.to(dev), idx.to(dev), val.to(dev), w.to(dev)).cpu()
    named = torch.zeros(n, dtype=torch.bool)
    inr = idx[(idx >= 0) & (idx < n)].long()
    named[inr] = True
    assert 0 < int(named.sum()) < n
    untouched = base + torch.zeros(n) / (torch.zeros(()) + w[0] + w[1] + w[2])
    assert torch.equal(_bits(out)[~named], _bits(untouched)[~named])
    assert bool(torch.isfinite(out).all())


# ---- the binding's checks come before any launch ---------------------------------------------------
def test_device_ops_check_their_arguments(dev):
    x = lambda n=8: torch.zeros(n, device=dev)
    buf = torch.zeros(16, device=dev)
    for args, msg in [((x().double(), x(), x(), 1), "local must be fp32"),
                      ((x(), x(), x(), 0), r"1 <= k <= n \(got k 0, n 8\)"),
                      ((x(), x(), x(), 9), r"1 <= k <= n \(got k 9, n 8\)"),
                      ((x(), buf[::2], x(), 1), "global must be contiguous"),
                      ((x(), x(), x()[None], 1), r"residual \[n\]"),
                      ((buf[:8], x(), buf[7:15], 1), "residual must not overlap local or global"),
                      ((x(), buf[:8], buf[:8], 1), "residual must not overlap local or global"),
                      ((x(), x(), torch.zeros(8), 1), "must be on one device"),
                      ((torch.zeros(8), torch.zeros(8), torch.zeros(8), 1), "must be device tensors")]:
        with pytest.raises(RuntimeError, match=msg):
            torch.ops.fedrec_sparse.topk_delta(*args)
    idx, val, w = torch.zeros(2, 3, dtype=torch.int32, device=dev), torch.zeros(2, 3, device=dev), torch.ones(2, device=dev)
    for args, msg in [((x(), idx.long(), val, w), "idx must be int32"),
                      ((x(), idx, val, w[:1]), r"weights \[W\]"),
                      ((x(2), idx, val, w), r"1 <= k <= n \(got k 3, n 2\)"),
                      ((x(), idx, val.cpu(), w), "must be on one device")]:
        with pytest.raises(RuntimeError, match=msg):
            torch.ops.fedrec_sparse.combine(*args)
