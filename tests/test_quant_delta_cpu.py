"""The contract of block-quantized uploads (``ops.reference.quantize_delta`` / ``dequant_combine``, the
oracles of csrc/quant_delta.hip) against an independent per-element loop in Python integers and numpy
fp32 scalars, with its own Philox.  No GPU.

The loop takes a ``mutant`` switch; each mutant is a mistake a kernel or an oracle could make, and the
inputs here must tell every one of them from the contract.  Bounds used below, for a live block with
scale ``s``: ``x = a / s`` carries a relative error of ``2^-24`` at ``|x| <= 128``, the code is within 1
of ``x`` and ``q s`` is rounded once more at ``|q| <= 127``, so ``|residual| <= s (1 + 2^-16)``; ``d +
residual`` is ``a`` up to the rounding of ``a - d`` and of the sum, both below half an ulp of the block
maximum."""
import functools

import numpy as np
import pytest
import torch

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import native
from fedrec_with_pytorchdistributed_amd.ops import reference as ref

G = 256
NAN, INF = float("nan"), float("inf")
M32 = 0xFFFFFFFF
NS = [1, 2, 3, 15, 16, 17, 255, 256, 257, 300, 513, 777]
SEEDS = [(7, 3), (2 ** 40 + 5, (3 << 32) | 9)]  # (one offset above 2^32)
CLAMP_N = 200003
CLAMP_CONST = {8: 1.000003457069397, 4: 1.0000007152557373}


# ---- the independent form ----------------------------------------------------------------------
def philox_word(seed, offset, i, by_element=False):
    """Component ``i & 3`` of Philox-4x32-10 at counter ``i >> 2`` (``by_element``: counter ``i``, a mutant)."""
    ctr = i if by_element else i >> 2
    c = [ctr & M32, (ctr >> 32) & M32, offset & M32, (offset >> 32) & M32]
    k0, k1 = seed & M32, (seed >> 32) & M32
    for _ in range(10):
        p0, p1 = c[0] * 0xD2511F53, c[2] * 0xCD9E8D57
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c[i & 3]


def _key(x):
    return int(np.float32(x).view(np.uint32)) & 0x7FFFFFFF


def loop_quantize(local, global_, residual, bits, seed, offset, mutant=None, first=0):
    """-> (codes uint8, scales fp32, new residual fp32) as numpy arrays, one coordinate at a time.  ``first``
    (a multiple of 256): the coordinate of element 0, for a slice of whole blocks of a longer buffer."""
    f32 = np.float32
    l, g, r = (t.numpy().astype(np.float32) for t in (local, global_, residual))
    n, Q = len(l), (1 << (bits - 1)) - 1
    nb = (n + G - 1) // G
    a = [f32(f32(l[i] - g[i]) + r[i]) for i in range(n)]
    shift = 1 if mutant == "block_offset" else 0
    block_of = lambda i: min((i + shift) // G, nb - 1)
    amax_key = [0] * nb
    for i in range(n):
        amax_key[block_of(i)] = max(amax_key[block_of(i)], _key(a[i]))
    scales = np.zeros(nb, np.float32)
    kind = []
    for b in range(nb):
        if amax_key[b] >= 0x7F800000:
            scales[b] = np.uint32(0x7FC00000).view(np.float32)
            kind.append("nonfinite")
            continue
        s = f32(np.uint32(amax_key[b]).view(np.float32) / f32(Q))
        if s < f32(2.0 ** -126):
            kind.append("zero")
        else:
            scales[b] = s
            kind.append("live")
    q = [0] * n
    res = np.zeros(n, np.float32)
    for i in range(n):
        b = block_of(i)
        if kind[b] == "nonfinite":
            continue  # code 0, residual +0.0
        if kind[b] == "zero":
            res[i] = a[i]
            continue
        s = scales[b]
        x = f32(a[i] / s)
        f = np.floor(x)
        p = f32(x - f)
        w = f32(philox_word(seed, offset, first + i, by_element=mutant == "philox_counter") >> 8)
        up = w <= f32(p * f32(16777216.0)) if mutant == "le" else w < f32(p * f32(16777216.0))
        qi = int(f) + int(up)
        if mutant != "no_clamp":
            qi = max(-Q, min(Q, qi))
        q[i] = qi
        if mutant == "fma":  # a - q s with the product unrounded (exact in fp64)
            res[i] = f32(np.float64(a[i]) - np.float64(qi) * np.float64(s))
        else:
            res[i] = f32(a[i] - f32(f32(qi) * s))
    if bits == 8:
        codes = np.array([v & 0xFF for v in q], np.uint8)
    else:
        nib = [v & 0xF for v in q] + [0] * (n & 1)
        lo, hi = (nib[1::2], nib[0::2]) if mutant == "nibble_swap" else (nib[0::2], nib[1::2])
        codes = np.array([x | (y << 4) for x, y in zip(lo, hi)], np.uint8)
    return codes, scales, res


def loop_combine(base, codes, scales, weights, bits, order=None, fuse=False):
    f32 = np.float32
    n, W = base.numel(), codes.shape[0]
    b, sc, w = base.numpy(), scales.numpy(), weights.numpy()
    q = ref.unpack_codes(codes, bits, n).numpy()
    out = np.zeros(n, np.float32)
    ws = f32(0.0)
    for c in (order or range(W)):
        ws = f32(ws + w[c])
    for i in range(n):
        acc = f32(0.0)
        for c in (order or range(W)):
            if fuse:  # (w q) s: another association of the same product
                acc = f32(acc + f32(f32(w[c] * f32(q[c, i])) * sc[c, i // G]))
            else:
                acc = f32(acc + f32(w[c] * f32(f32(q[c, i]) * sc[c, i // G])))
        out[i] = f32(b[i] + f32(acc / ws))
    return out


# ---- inputs ------------------------------------------------------------------------------------
def family(name, n, bits=8, seed=0, offset=0):
    """(local, global, residual) of n elements on the host."""
    g = torch.Generator().manual_seed(sum(map(ord, name)) + n)
    z = torch.zeros(n)
    normal = lambda: torch.randn(n, generator=g) * 2.0 ** torch.randint(-20, 21, (n,), generator=g).float()
    if name == "normal":
        return normal(), normal(), normal()
    if name == "ties":  # small integers: equal keys everywhere, x mostly a whole number or a half
        ints = lambda: torch.randint(-3, 4, (n,), generator=g).float()
        return ints(), ints(), ints() * 0.5
    if name == "constant":
        return torch.full((n,), -1.25), z, z
    if name == "zeros":  # (-0 - 0) + -0 = -0: a keeps the mixed signs
        s = torch.where(torch.randint(0, 2, (n,), generator=g) == 1, torch.tensor(-0.0), torch.tensor(0.0))
        return s, z, s.clone()
    if name == "denormal":
        l, gl, e = z.clone(), z.clone(), z.clone()
        l[0::3], gl[0::3], e[0::3] = 1e-41, 3e-42, -2e-41
        l[1::3] = 1e-35  # (the block stays live: s = 1e-35 / Q is a normal number)
        return l, gl, e
    if name == "tiny_max":  # the block maximum is below Q 2^-126: s is no normal number
        return torch.full((n,), 2.0 ** -126) * torch.randint(-3, 4, (n,), generator=g).float(), z, z
    if name == "special":  # non-finite values confined to known blocks: their neighbours stay live
        l, gl, e = normal(), normal(), normal()
        for b, (pos, lv, gv) in enumerate([(5, NAN, 0.0), (9, INF, 0.0), (0, -INF, 0.0), (200, INF, INF)]):
            i = (2 * b) * G + pos  # blocks 0, 2, 4, 6
            if i < n:
                l[i], gl[i] = lv, gv
        return l, gl, e
    if name == "compare_edge":  # s = 1 and p 2^24 equal to the coordinate's own Philox word >> 8
        Q = ref.quant_levels(bits)
        l = torch.tensor([float(Q) if i % G == 0 else (philox_word(seed, offset, i) >> 8) / 2.0 ** 24 for i in range(n)])
        return l, z, z
    raise KeyError(name)


FAMILIES = ["normal", "ties", "constant", "zeros", "denormal", "tiny_max", "special", "compare_edge"]


def _bits(t):
    return torch.as_tensor(t).contiguous().view(torch.int32)


def _same(got, want):
    """Bitwise equal, but any NaN where (and only where) the other holds a NaN."""
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    if not want.is_floating_point():
        return torch.equal(got, want)
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(_bits(got)[~nan], _bits(want)[~nan])


def _oracle(l, g, r, bits, seed, offset):
    res = r.clone()
    codes, scales = ref.quantize_delta(l, g, res, bits, seed, offset)
    return codes, scales, res


# ---- packing -----------------------------------------------------------------------------------
def test_byte_and_nibble_packing_by_hand():
    q = torch.tensor([0, 1, -1, 127, -127, -128, 5])
    assert ref.pack_codes(q, 8).tolist() == [0x00, 0x01, 0xFF, 0x7F, 0x81, 0x80, 0x05]
    q4 = torch.tensor([1, -1, 7, -7, 0, 3, -8])
    # low nibble first: (1, -1) -> 0xF1, (7, -7) -> 0x97, (0, 3) -> 0x30, (-8, padding) -> 0x08
    assert ref.pack_codes(q4, 4).tolist() == [0xF1, 0x97, 0x30, 0x08]
    assert ref.unpack_codes(ref.pack_codes(q, 8), 8, 7).tolist() == q.tolist()
    assert ref.unpack_codes(ref.pack_codes(q4, 4), 4, 7).tolist() == q4.tolist()
    assert ref.unpack_codes(torch.tensor([0x80, 0x88], dtype=torch.uint8), 8, 2).tolist() == [-128, -120]
    assert ref.unpack_codes(torch.tensor([0x80, 0x88], dtype=torch.uint8), 4, 4).tolist() == [0, -8, -8, -8]
    assert ref.quant_sizes(513, 8) == (513, 3) and ref.quant_sizes(513, 4) == (257, 3) and ref.quant_sizes(1, 4) == (1, 1)


@pytest.mark.parametrize("n", [1, 3, 257])
def test_the_padding_nibble_of_an_odd_n_is_zero(n):
    l = torch.full((n,), -3.0)  # every code is -Q: every nibble that exists is 0x9
    codes, _, _ = _oracle(l, torch.zeros(n), torch.zeros(n), 4, 1, 2)
    assert codes[-1] == 0x09 and all(c == 0x99 for c in codes[:-1].tolist())


# ---- the oracle is the loop --------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("name", FAMILIES)
def test_the_oracle_is_the_per_element_loop(name, bits):
    for n in NS:
        seed, offset = SEEDS[n & 1]
        l, g, r = family(name, n, bits, seed, offset)
        codes, scales, res = _oracle(l, g, r, bits, seed, offset)
        wc, ws, wr = loop_quantize(l, g, r, bits, seed, offset)
        assert codes.dtype == torch.uint8 and codes.shape == (ref.quant_sizes(n, bits)[0],)
        assert torch.equal(codes, torch.from_numpy(wc)), (name, n)
        assert _same(scales, torch.from_numpy(ws)), (name, n)
        assert _same(res, torch.from_numpy(wr)), (name, n)
        assert 0x80 not in codes.tolist() if bits == 8 else not any(c & 0xF == 8 or c >> 4 == 8 for c in codes.tolist())


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("name", FAMILIES)
def test_block_properties(name, bits):
    Q = ref.quant_levels(bits)
    for n in NS:
        seed, offset = SEEDS[n & 1]
        l, g, r = family(name, n, bits, seed, offset)
        a = (l - g) + r
        codes, scales, res = _oracle(l, g, r, bits, seed, offset)
        d = ops.dequantize(codes, scales, bits, n)
        q = ref.unpack_codes(codes, bits, n)
        for b in range(scales.numel()):
            sl = slice(G * b, min(n, G * b + G))
            ab, s = a[sl], scales[b]
            if not torch.isfinite(ab).all():
                assert int(_bits(s)) == 0x7FC00000
                assert not q[sl].any() and torch.equal(_bits(res[sl]), torch.zeros_like(_bits(res[sl])))
                continue
            amax = ab.abs().max()
            if amax / torch.tensor(float(Q)) < 2.0 ** -126:
                assert int(_bits(s)) == 0 and not q[sl].any() and torch.equal(_bits(res[sl]), _bits(ab))
                continue
            assert _bits(s) == _bits(amax / torch.tensor(float(Q)))
            assert bool((q[sl].abs() <= Q).all())
            assert bool((res[sl].abs().double() <= s.double() * (1 + 2.0 ** -16)).all())
            ulp = float(np.spacing(np.float32(amax)))
            assert bool(((d[sl] + res[sl]) - ab).abs().max() <= ulp)


def test_the_families_hold_what_they_claim():
    l, g, r = family("special", 7 * G + 9)
    _, scales, _ = _oracle(l, g, r, 8, 1, 2)
    assert torch.isnan(scales).tolist() == [True, False, True, False, True, False, True, False]
    _, scales, _ = _oracle(*family("tiny_max", 300), 8, 1, 2)
    assert scales.tolist() == [0.0, 0.0]
    _, scales, res = _oracle(*family("denormal", 300), 8, 1, 2)
    assert bool((scales > 0).all()) and bool(((res != 0) & (res.abs() < 2.0 ** -126)).any())


# ---- the clamp ---------------------------------------------------------------------------------
def _constant_codes(c, bits, seed, offset, clamp):
    """Codes of a constant buffer of CLAMP_N values c, vectorised (every block has the scale |c| / Q)."""
    Q = ref.quant_levels(bits)
    a = torch.full((CLAMP_N,), c)
    s = a.abs() / torch.full_like(a, float(Q))
    x = a / s
    f = torch.floor(x)
    word = ref.philox4x32(seed, offset, torch.arange((CLAMP_N + 3) // 4)).reshape(-1)[:CLAMP_N]
    q = f + ((word >> 8).float() < (x - f) * 16777216.0).float()
    return (torch.clamp(q, -float(Q), float(Q)) if clamp else q).long()


@functools.lru_cache(maxsize=None)
def clamp_case(bits, negative):
    """(constant, seed, offset, coordinates whose unclamped code leaves [-Q, Q]): the first offset at
    which the form without the clamp produces such a code."""
    Q = ref.quant_levels(bits)
    c = -CLAMP_CONST[bits] if negative else CLAMP_CONST[bits]
    for offset in range(64):
        q = _constant_codes(c, bits, 11, offset, clamp=False)
        bad = (q.abs() > Q).nonzero().reshape(-1)
        if bad.numel():
            return c, 11, offset, bad
    raise AssertionError("no offset below 64 produced an out-of-range code")


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("bits", [8, 4])
def test_the_clamp_is_needed_and_holds(bits, negative):
    Q = ref.quant_levels(bits)
    c, seed, offset, bad = clamp_case(bits, negative)
    l, z = torch.full((CLAMP_N,), c), torch.zeros(CLAMP_N)
    codes, scales, res = _oracle(l, z, z, bits, seed, offset)
    q = ref.unpack_codes(codes, bits, CLAMP_N)
    unclamped = _constant_codes(c, bits, seed, offset, clamp=False)
    assert bool((unclamped[bad].abs() == Q + 1).all())
    assert torch.equal(q, _constant_codes(c, bits, seed, offset, clamp=True))
    assert bool((q[bad].abs() == Q).all()) and not torch.equal(q, unclamped)
    # packed without the clamp, the code wraps: +128 reads back as -128, +8 as -8
    wrapped = ref.unpack_codes(ref.pack_codes(unclamped, bits), bits, CLAMP_N)
    assert bool((wrapped[bad] == -(Q + 1)).all())
    assert bool((res.abs() <= scales[0] * (1 + 2.0 ** -16)).all())


# ---- mutants -----------------------------------------------------------------------------------
def _differs(mutant, name, n, bits):
    seed, offset = SEEDS[1]
    l, g, r = family(name, n, bits, seed, offset)
    want = _oracle(l, g, r, bits, seed, offset)
    got = loop_quantize(l, g, r, bits, seed, offset, mutant=mutant)
    return not all(_same(torch.from_numpy(x), y) for x, y in zip(got, want))


@pytest.mark.parametrize("mutant,name,n,bits", [
    ("le", "compare_edge", 300, 8), ("le", "compare_edge", 300, 4),
    ("philox_counter", "normal", 513, 8), ("philox_counter", "normal", 513, 4),
    ("nibble_swap", "normal", 513, 4),
    ("block_offset", "normal", 777, 8), ("block_offset", "normal", 777, 4),
    ("fma", "normal", 777, 8), ("fma", "normal", 777, 4),
])
def test_the_inputs_catch_the_mutant(mutant, name, n, bits):
    assert _differs(mutant, name, n, bits)
    assert not _differs(None, name, n, bits)


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("bits", [8, 4])
def test_the_inputs_catch_the_missing_clamp(bits, negative):
    """The loop over the block of the first out-of-range code, at that block's own coordinates."""
    c, seed, offset, bad = clamp_case(bits, negative)
    l, z = torch.full((CLAMP_N,), c), torch.zeros(CLAMP_N)
    codes, scales, res = _oracle(l, z, z, bits, seed, offset)
    lo = int(bad[0]) // G * G
    hi = min(CLAMP_N, lo + G)
    want = (codes[lo * bits // 8:hi * bits // 8], scales[lo // G:lo // G + 1], res[lo:hi])
    for mutant, same in ((None, True), ("no_clamp", False)):
        got = loop_quantize(l[lo:hi], z[lo:hi], z[lo:hi], bits, seed, offset, mutant=mutant, first=lo)
        assert all(_same(torch.from_numpy(x), y) for x, y in zip(got, want)) == same


# ---- dequant_combine ---------------------------------------------------------------------------
def _uploads(W, n, bits, gen):
    nbytes, nb = ref.quant_sizes(n, bits)
    codes = torch.randint(0, 256, (W, nbytes), generator=gen).to(torch.uint8)
    scales = torch.rand(W, nb, generator=gen) * 2.0 ** torch.randint(-8, 3, (W, nb), generator=gen).float()
    return codes, scales


@pytest.mark.parametrize("bits", [8, 4])
def test_combine_is_the_loop_and_order_and_association_show(bits):
    gen = torch.Generator().manual_seed(5)
    n, W = 300, 3
    codes, scales = _uploads(W, n, bits, gen)
    base = torch.randn(n, generator=gen)
    w = torch.tensor([0.3, 1.7, 2.9])
    got = ref.dequant_combine(base, codes, scales, w, bits)
    assert _same(got, loop_combine(base, codes, scales, w, bits))
    assert not _same(got, loop_combine(base, codes, scales, w, bits, order=[2, 1, 0]))
    assert not _same(got, loop_combine(base, codes, scales, w, bits, fuse=True))
    assert _same(ops.dequant_combine(base, codes, scales, w, bits), got)


@pytest.mark.parametrize("bits", [8, 4])
def test_dequantize_is_code_times_scale(bits):
    n = 513
    l, g, r = family("normal", n)
    codes, scales, _ = _oracle(l, g, r, bits, 1, 2)
    d = ops.dequantize(codes, scales, bits, n)
    want = ref.unpack_codes(codes, bits, n).float() * scales.repeat_interleave(G)[:n]
    assert torch.equal(_bits(d), _bits(want + 0.0))  # (-0.0 reads as +0.0)
    assert not bool((_bits(d) == _bits(torch.tensor(-0.0))).any())


def test_quantize_then_combine_with_one_client_gives_back_the_delta():
    n = 777
    l, g, r = family("normal", n)
    a = (l - g) + r
    codes, scales, res = _oracle(l, g, r, 8, 3, 4)
    out = ref.dequant_combine(torch.zeros(n), codes[None], scales[None], torch.ones(1), 8)
    assert bool(((out + res) - a).abs().max() <= a.abs().max() * 2.0 ** -23)


# ---- checks ------------------------------------------------------------------------------------
def _raises(fn, exc, text):
    with pytest.raises(exc) as e:
        fn()
    assert text in str(e.value), str(e.value)


def _quant_calls(l, g, r, bits):
    return [lambda: ref.quantize_delta_check(l, g, r, bits), lambda: ops.quantize_delta(l, g, r, bits, 0, 0),
            lambda: (native.lib(), torch.ops.fedrec_quant.quantize_delta(l, g, r, bits, 0, 0))]


def test_quantize_delta_argument_messages():
    n = 8
    v = lambda: torch.zeros(n)
    op = "fedrec_quant::quantize_delta: "
    buf = torch.zeros(2 * n)
    cases = [
        ((v().double(), v(), v(), 8), "local must be fp32"),
        ((v(), v().half(), v(), 8), "global must be fp32"),
        ((v(), v(), v().long(), 8), "residual must be fp32"),
        ((torch.zeros(2, 4), v(), v(), 8), "local [n] (got 2 dims)"),
        ((v(), torch.zeros(2 * n)[::2], v(), 8), "global must be contiguous"),
        ((v(), torch.zeros(n + 1), v(), 8), f"local, global and residual must have one length (got {n}, {n + 1}, {n})"),
        ((torch.zeros(0), torch.zeros(0), torch.zeros(0), 8), "1 <= n < 2^31 (got n 0)"),
        ((v(), v(), v(), 6), "bits must be 8 or 4 (got 6)"),
        ((v(), v(), v(), 0), "bits must be 8 or 4 (got 0)"),
        ((buf[:n], v(), buf[n - 1:2 * n - 1], 8), "residual must not overlap local or global"),
        ((v(), buf[1:n + 1], buf[:n], 4), "residual must not overlap local or global"),
    ]
    for args, text in cases:
        for call in _quant_calls(*args):
            _raises(call, RuntimeError, op + text)
    # valid host tensors pass every check and fail the registered op's device check, which comes last
    _raises(_quant_calls(v(), v(), v(), 8)[2], RuntimeError, op + "local, global and residual must be device tensors")
    ref.quantize_delta_check(v(), v(), v(), 4)


def _combine_calls(b, c, s, w, bits):
    return [lambda: ref.dequant_combine_check(b, c, s, w, bits), lambda: ops.dequant_combine(b, c, s, w, bits),
            lambda: (native.lib(), torch.ops.fedrec_quant.dequant_combine(b, c, s, w, bits))]


def test_dequant_combine_argument_messages():
    n, W = 300, 2
    base = lambda: torch.zeros(n)
    codes = lambda bits=8: torch.zeros(W, ref.quant_sizes(n, bits)[0], dtype=torch.uint8)
    scales = lambda: torch.zeros(W, 2)
    w = lambda: torch.ones(W)
    op = "fedrec_quant::dequant_combine: "
    cases = [
        ((base().double(), codes(), scales(), w(), 8), "base must be fp32"),
        ((torch.zeros(2, 150), codes(), scales(), w(), 8), "base [n] (got 2 dims)"),
        ((base(), codes().to(torch.int8), scales(), w(), 8), "codes must be uint8"),
        ((base(), codes(), scales().double(), w(), 8), "scales must be fp32"),
        ((base(), codes()[0], scales(), w(), 8), "codes [W, nbytes] and scales [W, nb]"),
        ((base(), codes(), scales()[0], w(), 8), "codes [W, nbytes] and scales [W, nb]"),
        ((base(), torch.zeros(W, 2 * n, dtype=torch.uint8)[:, ::2], scales(), w(), 8), "codes and scales must be contiguous"),
        ((base(), codes(), scales(), w().double(), 8), "weights must be fp32"),
        ((base(), codes(), scales(), torch.ones(W, 1), 8), "weights [n] (got 2 dims)"),
        ((torch.zeros(0), codes(), scales(), w(), 8), "1 <= n < 2^31 (got n 0)"),
        ((base(), codes(), scales(), w(), 2), "bits must be 8 or 4 (got 2)"),
        ((base(), codes(), scales(), torch.ones(3), 8),
         "1 <= W <= 65536, scales [W, nb] and weights [W] (got W 2, scales 2, weights 3)"),
        ((base(), codes(), torch.zeros(3, 2), w(), 8),
         "1 <= W <= 65536, scales [W, nb] and weights [W] (got W 2, scales 3, weights 2)"),
        ((base(), torch.zeros(0, n, dtype=torch.uint8), torch.zeros(0, 2), torch.ones(0), 8),
         "1 <= W <= 65536, scales [W, nb] and weights [W] (got W 0, scales 0, weights 0)"),
        ((base(), codes(), scales(), w(), 4), "n 300 at 4 bits takes codes [W, 150] and scales [W, 2] (got 300, 2)"),
        ((base(), codes(4), torch.zeros(W, 3), w(), 4), "n 300 at 4 bits takes codes [W, 150] and scales [W, 2] (got 150, 3)"),
    ]
    for args, text in cases:
        for call in _combine_calls(*args):
            _raises(call, RuntimeError, op + text)
    _raises(_combine_calls(base(), codes(), scales(), w(), 8)[2], RuntimeError,
            op + "base, codes, scales and weights must be device tensors")
    ref.dequant_combine_check(base(), codes(4), scales(), w(), 4)


def test_quant_upload_check_names_the_first_violation():
    n, bits = 300, 4
    codes, scales = torch.zeros(150, dtype=torch.uint8), torch.tensor([0.5, 0.0])
    ref.quant_upload_check(codes, scales, n, bits)
    _raises(lambda: ref.quant_upload_check(codes.to(torch.int8), scales, n, bits), ValueError, "codes must be uint8")
    _raises(lambda: ref.quant_upload_check(codes, scales.double(), n, bits), ValueError, "scales must be fp32")
    _raises(lambda: ref.quant_upload_check(codes[:-1], scales, n, bits), ValueError, "codes must have length 150")
    _raises(lambda: ref.quant_upload_check(codes, scales[:1], n, bits), ValueError, "scales must have length 2")
    _raises(lambda: ref.quant_upload_check(codes, torch.tensor([0.5, NAN]), n, bits), ValueError, "scales[1] = nan")
    _raises(lambda: ref.quant_upload_check(codes, torch.tensor([INF, NAN]), n, bits), ValueError, "scales[0] = inf")
    _raises(lambda: ref.quant_upload_check(codes, torch.tensor([0.5, -1.0]), n, bits), ValueError, "scales[1] = -1.0")
    _raises(lambda: ref.quant_upload_check(codes, torch.tensor([-0.0, 1.0]), n, bits), ValueError, "scales[0] = -0.0")
