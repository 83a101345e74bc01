"""``fedrec_quant::quantize_delta`` / ``dequant_combine`` (csrc/quant_delta.hip) on the device, bit for bit
against their torch oracles.  The contract is exact, so equality with the oracle also proves independence
of grid and launch order.  A scale may be any NaN, but only where the oracle's is one.

Sizes of ``quantize_delta``: n = 1, 2, 3, 15, 16, 17 (around a lane's 16 coordinates), every power of two
from 64 to 65536 with both neighbours (one element either side of every scale block, wave span and
workgroup span), 70001 and 200003 (many workgroups, ragged tail); both bit widths; two (seed, offset)
pairs, one with an offset above 2^32.  Each family draws one buffer; an n is its leading elements."""
import pytest
import torch

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import reference as ref

from test_quant_delta_cpu import CLAMP_N, SEEDS, clamp_case, philox_word

pytestmark = pytest.mark.gpu

G = 256
NS = [1, 2, 3, 15, 16, 17] + [p + d for e in range(6, 17) for p in [1 << e] for d in (-1, 0, 1)] + [70001, 200003]
NMAX = max(NS)
NAN, INF = float("nan"), float("inf")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(got, want):
    """Bitwise equal, but any NaN where (and only where) the oracle holds a NaN."""
    got, want = got.detach().cpu(), want.detach().cpu()
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(_bits(got)[~nan], _bits(want)[~nan])


def _family(name, bits):
    """(local, global, residual) of NMAX elements on the host."""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    n = NMAX
    z = torch.zeros(n)
    normal = lambda: torch.randn(n, generator=g) * 2.0 ** torch.randint(-20, 21, (n,), generator=g).float()
    if name == "normal":
        return normal(), normal(), normal()
    if name == "ties":  # small integers and halves: equal keys everywhere, x mostly whole or half
        ints = lambda: torch.randint(-3, 4, (n,), generator=g).float()
        return ints(), ints(), ints() * 0.5
    if name == "constant":
        return torch.full((n,), -1.25), z, z
    if name == "zeros":  # (-0 - 0) + -0 = -0, (+0 - 0) + +0 = +0: a keeps the mixed signs
        s = torch.where(torch.randint(0, 2, (n,), generator=g) == 1, torch.tensor(-0.0), torch.tensor(0.0))
        return s, z, s.clone()
    if name == "denormal":  # denormal operands and results beside a maximum that keeps the block live
        l, gl, e = z.clone(), z.clone(), z.clone()
        l[0::3], gl[0::3], e[0::3] = 1e-41, 3e-42, -2e-41
        l[1::3] = 1e-35
        return l, gl, e
    if name == "tiny_max":  # every block's maximum is below Q 2^-126
        return torch.full((n,), 2.0 ** -126) * torch.randint(-3, 4, (n,), generator=g).float(), z, z
    if name == "special":  # inf, -inf, NaN and inf - inf in every 4th block: the blocks between stay live
        l, gl, e = normal(), normal(), normal()
        for j, (pos, lv, gv) in enumerate([(5, NAN, 0.0), (9, INF, 0.0), (0, -INF, 0.0), (255, INF, INF)]):
            at = torch.arange((4 * j) * G + pos, n, 16 * G)
            l[at], gl[at] = lv, gv
        l[3], gl[3] = NAN, 0.0  # (and the first block at every small n)
        return l, gl, e
    if name == "compare_edge":  # s = 1 and p 2^24 equal to the coordinate's own Philox word >> 8 (n <= 1025)
        Q = ref.quant_levels(bits)
        seed, offset = SEEDS[0]
        head = [float(Q) if i % G == 0 else (philox_word(seed, offset, i) >> 8) / 2.0 ** 24 for i in range(1025)]
        return torch.cat([torch.tensor(head), normal()[1025:]]), z, z
    raise KeyError(name)


FAMILIES = ["normal", "ties", "constant", "zeros", "denormal", "tiny_max", "special", "compare_edge"]


def _check(l, gl, e, bits, seed, offset, dev, views=None):
    want_res = e.clone()
    want_codes, want_scales = ref.quantize_delta(l, gl, want_res, bits, seed, offset)
    dl, dg, de = views if views is not None else (l.to(dev), gl.to(dev), e.to(dev))
    codes, scales = ops.quantize_delta(dl, dg, de, bits, seed, offset)
    n = l.numel()
    assert codes.dtype == torch.uint8 and scales.dtype == torch.float32 and codes.device == de.device
    assert tuple(codes.shape) == (ref.quant_sizes(n, bits)[0],) and tuple(scales.shape) == (ref.quant_sizes(n, bits)[1],)
    assert torch.equal(codes.cpu(), want_codes), (n, bits)
    assert _same(scales, want_scales), (n, bits)
    assert _same(de, want_res), (n, bits)
    return want_codes, want_scales


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("family", FAMILIES)
def test_quantize_delta_matches_the_oracle_bit_for_bit(dev, family, bits):
    L, Gl, E = _family(family, bits)
    for j, n in enumerate(NS):
        l, gl, e = L[:n].clone(), Gl[:n].clone(), E[:n].clone()
        pairs = SEEDS if n in (1, 257, 1025, NMAX) else [SEEDS[0] if family == "compare_edge" else SEEDS[j & 1]]
        for seed, offset in pairs:
            _check(l, gl, e, bits, seed, offset, dev)


def test_the_special_family_keeps_live_blocks_beside_the_dead_ones():
    l, gl, e = _family("special", 8)
    _, scales = ref.quantize_delta(l[:70001], gl[:70001], e[:70001].clone(), 8, *SEEDS[0])
    nan = torch.isnan(scales)
    assert nan[0::4].all() and not nan[1::4].any() and not nan[2::4].any() and not nan[3::4].any()
    assert bool((scales[~nan] > 0).all())


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("bits", [8, 4])
def test_the_clamp_constants_at_the_offset_the_search_found(dev, bits, negative):
    Q = ref.quant_levels(bits)
    c, seed, offset, bad = clamp_case(bits, negative)
    l, z = torch.full((CLAMP_N,), c), torch.zeros(CLAMP_N)
    codes, _ = _check(l, z, z.clone(), bits, seed, offset, dev)
    q = ref.unpack_codes(codes, bits, CLAMP_N)
    assert bool((q[bad].abs() == Q).all()) and int(q.abs().max()) == Q


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("family", ["normal", "special"])
def test_quantize_delta_on_misaligned_views(dev, family, bits):
    """``x[1:]`` / ``x[3:]`` of all three inputs, and of some: the same bits as the contiguous copies (the
    scale blocks start at coordinate 256 b of the tensor whatever its address)."""
    L, Gl, E = _family(family, bits)
    for n in (1, 15, 17, 255, 257, 1024, 4099, 70001):
        l, gl, e = L[:n].clone(), Gl[:n].clone(), E[:n].clone()
        for shift in ((1, 1, 1), (3, 3, 3), (0, 0, 1), (2, 3, 0)):
            views = []
            for t, s in zip((l, gl, e), shift):
                buf = torch.empty(n + s, device=dev)
                buf[s:].copy_(t)
                views.append(buf[s:])
                assert views[-1].data_ptr() % 16 == 4 * s and views[-1].is_contiguous()
            _check(l, gl, e, bits, *SEEDS[1], dev, views)


def test_error_feedback_rounds_on_the_device_equal_the_host(dev):
    """Five rounds with the residual carried: uploads and residual equal the oracle's every round."""
    n = 70001
    g = torch.Generator().manual_seed(9)
    res_h, res_d = torch.zeros(n), torch.zeros(n, device=dev)
    for r in range(5):
        theta = torch.randn(n, generator=g)
        local = theta + 0.01 * torch.randn(n, generator=g)
        wc, ws = ref.quantize_delta(local, theta, res_h, 4, 3, (1 << 32) | r)
        gc, gs = ops.quantize_delta(local.to(dev), theta.to(dev), res_d, 4, 3, (1 << 32) | r)
        assert torch.equal(gc.cpu(), wc) and _same(gs, ws) and _same(res_d, res_h)


# ---- dequant_combine -----------------------------------------------------------------------------
def _uploads(W, n, bits, g):
    """Random bytes as codes (0x80 and the nibble 0x8 among them), finite scales, weights with a zero and
    non-integers."""
    nbytes, nb = ref.quant_sizes(n, bits)
    codes = torch.randint(0, 256, (W, nbytes), generator=g).to(torch.uint8)
    codes[:, 0] = 0x80
    codes[W // 2, nbytes // 2] = 0x88
    scales = torch.rand(W, nb, generator=g) * 2.0 ** torch.randint(-8, 3, (W, nb), generator=g).float()
    w = torch.rand(W, generator=g) * 3 + 0.1
    if W > 1:
        w[1] = 0.0
    return codes, scales, w


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("W", [1, 2, 3, 32, 33])
def test_dequant_combine_matches_the_oracle_bit_for_bit(dev, W, bits):
    g = torch.Generator().manual_seed(W * 1009 + bits)
    for n in (1, 2, 15, 17, 255, 256, 257, 1023, 1025, 4097, 70001):
        codes, scales, w = _uploads(W, n, bits, g)
        base = torch.randn(n, generator=g)
        want = ref.dequant_combine(base, codes, scales, w, bits)
        out = ops.dequant_combine(base.to(dev), codes.to(dev), scales.to(dev), w.to(dev), bits)
        assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (n,)
        assert torch.equal(_bits(out), _bits(want)), (W, n, bits)


@pytest.mark.parametrize("bits", [8, 4])
def test_dequant_combine_with_non_finite_scales_and_a_misaligned_base(dev, bits):
    n, W = 8200, 3
    g = torch.Generator().manual_seed(4)
    codes, scales, w = _uploads(W, n, bits, g)
    scales[0, 3], scales[2, 7], scales[1, 9] = NAN, INF, -0.0
    base = torch.randn(n, generator=g)
    want = ref.dequant_combine(base, codes, scales, w, bits)
    for s in (0, 1, 3):
        buf = torch.empty(n + s, device=dev)
        buf[s:].copy_(base)
        out = ops.dequant_combine(buf[s:], codes.to(dev), scales.to(dev), w.to(dev), bits)
        assert _same(out, want), s
    assert bool(torch.isnan(want[3 * G:4 * G]).all()) and not bool(torch.isnan(want[4 * G:7 * G]).any())


@pytest.mark.parametrize("bits", [8, 4])
def test_dequant_combine_split_at_a_block_boundary_gives_the_same_bits(dev, bits):
    n, W, m = 70001, 3, 13 * G
    g = torch.Generator().manual_seed(8)
    codes, scales, w = _uploads(W, n, bits, g)
    base = torch.randn(n, generator=g)
    dc, ds, dw, db = codes.to(dev), scales.to(dev), w.to(dev), base.to(dev)
    whole = ops.dequant_combine(db, dc, ds, dw, bits)
    mb = m * bits // 8
    head = ops.dequant_combine(db[:m], dc[:, :mb].contiguous(), ds[:, :m // G].contiguous(), dw, bits)
    tail = ops.dequant_combine(db[m:], dc[:, mb:].contiguous(), ds[:, m // G:].contiguous(), dw, bits)
    assert torch.equal(_bits(torch.cat([head, tail])), _bits(whole))
    assert torch.equal(_bits(whole), _bits(ref.dequant_combine(base, codes, scales, w, bits)))


@pytest.mark.parametrize("bits", [8, 4])
def test_dequantize_on_the_device_is_the_host(dev, bits):
    n = 70001
    l, gl, e = (t[:n].clone() for t in _family("normal", bits))
    codes, scales = ref.quantize_delta(l, gl, e, bits, *SEEDS[1])
    d = ops.dequantize(codes.to(dev), scales.to(dev), bits, n)
    assert d.is_cuda and torch.equal(_bits(d), _bits(ref.dequantize(codes, scales, bits, n)))


# ---- the binding's checks come before any launch ---------------------------------------------------
def test_device_ops_check_their_arguments(dev):
    x = lambda n=8: torch.zeros(n, device=dev)
    buf = torch.zeros(16, device=dev)
    for args, msg in [((x().double(), x(), x(), 8, 0, 0), "local must be fp32"),
                      ((x(), x(), x(), 5, 0, 0), r"bits must be 8 or 4 \(got 5\)"),
                      ((x(), buf[::2], x(), 8, 0, 0), "global must be contiguous"),
                      ((x(), x(), x()[None], 8, 0, 0), r"residual \[n\]"),
                      ((buf[:8], x(), buf[7:15], 4, 0, 0), "residual must not overlap local or global"),
                      ((x(), x(), torch.zeros(8), 8, 0, 0), "must be on one device"),
                      ((torch.zeros(8), torch.zeros(8), torch.zeros(8), 8, 0, 0), "must be device tensors")]:
        with pytest.raises(RuntimeError, match=msg):
            torch.ops.fedrec_quant.quantize_delta(*args)
    codes, scales, w = torch.zeros(2, 8, dtype=torch.uint8, device=dev), torch.zeros(2, 1, device=dev), torch.ones(2, device=dev)
    for args, msg in [((x(), codes.to(torch.int8), scales, w, 8), "codes must be uint8"),
                      ((x(), codes, scales, w[:1], 8), r"weights \[W\]"),
                      ((x(), codes, scales, w, 4), r"takes codes \[W, 4\]"),
                      ((x(), codes, scales.cpu(), w, 8), "must be on one device")]:
        with pytest.raises(RuntimeError, match=msg):
            torch.ops.fedrec_quant.dequant_combine(*args)
