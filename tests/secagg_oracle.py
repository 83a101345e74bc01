"""Exact twins of the six secure-aggregation kernels (csrc/secagg.hip: ``mask``, ``unmask``, ``hist``
(``amax`` + ``hist``), ``hist_scale``, ``mask_exact``, ``unmask_exact``), with every mask word taken from
``ops.reference.philox4x32`` (a plain helper module for tests/test_secagg_oracle_cpu.py and
tests/test_secagg_oracle_gpu.py, not a conftest; no GPU dependency: numpy / torch on the CPU).

There is no tolerance anywhere: every output is an int32 word or an fp32 value that the kernel and the
twin must form from the same bits.

================================================================================================
1. The twins, line by line.

* ``mask_twin`` (clamped): ``Q = rint(min(max(x, -clip), clip) * scale)`` in fp32, as int32; peer p adds
  ``sign_p * word0(Philox(seed_p, round, i))`` in uint32 wrap-around -- one call per ELEMENT, word 0.
* ``unmask_twin``: ``float32(int32) * inv_scale`` in fp32 (the conversion rounds to nearest even above
  2^24, as ``v_cvt_f32_i32`` does).
* ``hist_twin``: the largest finite ``|x|`` by its fp32 bits, the count of coordinates that fail
  ``|x| <= FLT_MAX``; slot 0 for an all-zero (or empty, or all non-finite) vector, else
  ``max(e, 1) + 1`` with e the exponent field; one-hot at the slot, the count in slot 1; peer p adds
  its four words of counter ``g`` to slots ``4 g .. 4 g + 3``.
* ``hist_scale_twin``: ``smax`` = the largest occupied slot >= 2; none -> scale 2^0;
  ``f = 30 - ceil_log2(W) - (smax - 127)`` clamped to [-120, 60]; ``bad`` = slot 1 non-zero.
* ``mask_exact_twin``: a coordinate failing ``|x| <= FLT_MAX`` becomes 0; ``rint(x * 2^f)`` (exact
  scaling, one rounding); element i takes word ``i % 4`` of counter ``i / 4``, the last group of an
  ``n % 4 != 0`` vector included.
* ``unmask_exact_twin``: the quiet NaN 0x7fc00000 everywhere when ``bad``; else ``float32(int32) * 2^-f``
  (2^120 * q overflows to inf exactly where the kernel's product does).

A float -> int32 conversion outside int32 is undefined in the kernels' language, so the twins assert
that no case reaches one; NaN is left out of the clamped kernel's cases for the same reason (the star
upload zeroes such vectors first), and the ``f = -98`` pair uses ``clip = 2^127`` (W = 2), not the
``clip = 2^128 = inf`` of W = 1, so that +-inf clamps to a finite value.

One remark the no-wrap test documents: the clamp of f at -120 gives up the guarantee
``W max|Q| <= 2^30`` only at W >= 2^23 clients that all hold values near FLT_MAX (the unclamped f
would be -121), where the plain fp32 sum would be inf as well.

================================================================================================
2. Planted defects (``DEFECTS``): every twin takes ``defect=``; tests/test_secagg_oracle_cpu.py shows
for each that at least one named case of the GPU file changes, i.e. the GPU comparison would see a
kernel with that defect.

================================================================================================
3. Cases.  ``MASK_CASES``, ``UNMASK_CASES``, ``HIST_CASES``, ``EXACT_CASES``, ``UNMASK_EXACT_CASES`` and the
fleets are lists of small named tuples; ``*_input`` builds the inputs of a case, ``*_want`` the twin's output
(cached: computed once, shared read-only).  Philox on the CPU costs about 0.14 s per million counters
per peer, so sizes past the first grid-stride trip (4096 blocks x 256 threads = 1 048 576 threads)
run with at most 3 peers and the 64-peer cases at n <= 4099."""
import functools
from collections import namedtuple

import numpy as np
import torch

from fedrec_with_pytorchdistributed_amd.ops import reference as ref

HB = 256  # histogram slots
MAXP = 64  # peers a launch accepts
HIST_ROUND = 1 << 62  # counter space of the histograms: round = 2^62 | r
FLT_MAX = np.float32(3.4028234663852886e38)
TRIP = 4096 * 256  # threads of one grid-stride trip
NAN_BITS = 0x7FC00000

DEFECTS = ("word_reversed", "counter_is_element", "sign_flipped", "seed_hi_dropped", "round_hi_dropped",
           "trunc", "half_away", "floor_log2", "slot_pow2_off_by_one", "nonfinite_kept", "tail_unmasked",
           "zero_mask")

_U32 = 0xFFFFFFFF
_F32 = np.float32


# ================================================================================ Philox words
@functools.lru_cache(maxsize=4096)
def _philox_small(seed, rnd, nc):
    return _philox(seed, rnd, nc)


def _philox(seed, rnd, nc):
    w = ref.philox4x32(seed, rnd, torch.arange(nc, dtype=torch.int64))
    return w.numpy().astype(np.uint32)


def philox_words(seed, rnd, nc):
    """uint32 [nc, 4]: the four words of Philox(seed, round, c) for c = 0 .. nc - 1 (read-only)."""
    seed, rnd, nc = int(seed), int(rnd), int(nc)
    return _philox_small(seed, rnd, nc) if nc <= 8192 else _philox(seed, rnd, nc)


@functools.lru_cache(maxsize=24)
def _net_mask_cached(seeds, signs, rnd, nc, defect):
    acc = np.zeros((nc, 4), dtype=np.uint32)
    if defect == "zero_mask":
        return acc
    for p, (s, g) in enumerate(zip(seeds, signs)):
        if defect == "sign_flipped" and p == 0:
            g = -g
        if defect == "seed_hi_dropped":
            s &= _U32
        r = rnd & _U32 if defect == "round_hi_dropped" else rnd
        w = philox_words(s, r, nc)
        if defect == "word_reversed":
            w = w[:, ::-1]
        acc = acc + w if g > 0 else acc - w  # uint32 wrap-around
    acc.setflags(write=False)
    return acc


def net_mask(seeds, signs, rnd, nc, defect=None):
    """uint32 [nc, 4]: ``sum_p sign_p * Philox(seed_p, round, c)`` in wrap-around."""
    if defect not in ("zero_mask", "sign_flipped", "seed_hi_dropped", "round_hi_dropped", "word_reversed"):
        defect = None
    return _net_mask_cached(tuple(int(s) for s in seeds), tuple(int(g) for g in signs), int(rnd), int(nc), defect)


def element_mask(seeds, signs, rnd, n, defect=None):
    """uint32 [n]: the mask of the 4-per-call kernels -- word ``i % 4`` of counter ``i / 4``."""
    if len(seeds) == 0 or n == 0:
        return np.zeros(n, dtype=np.uint32)
    if defect == "counter_is_element":
        m = net_mask(seeds, signs, rnd, n)
        return m[np.arange(n), np.arange(n) & 3].copy()
    m = net_mask(seeds, signs, rnd, (n + 3) // 4, defect).reshape(-1)[:n].copy()
    if defect == "tail_unmasked" and n % 4:
        m[n - n % 4:] = 0
    return m


# ================================================================================ float steps
def _rint(v, defect=None):
    if defect == "trunc":
        return np.trunc(v)
    if defect == "half_away":
        small = np.abs(v) < _F32(2.0 ** 23)  # larger fp32 values are integers already
        return np.where(small, np.copysign(np.floor(np.abs(v) + _F32(0.5)), v), v).astype(np.float32)
    return np.rint(v)


def _to_u32(r, saturate=False):
    """fp32 integers inside int32 -> their two's-complement words.  ``saturate``: the hardware
    conversion of the ``nonfinite_kept`` defect (inf -> INT_MAX / INT_MIN, NaN -> 0)."""
    if saturate:
        r = np.clip(np.nan_to_num(r.astype(np.float64), nan=0.0, posinf=2.0 ** 31 - 1, neginf=-2.0 ** 31),
                    -2.0 ** 31, 2.0 ** 31 - 1)
    assert bool(((r >= -2.0 ** 31) & (r < 2.0 ** 31)).all()), "a float outside int32: undefined in the kernel"
    return r.astype(np.int64).astype(np.uint32)


def pow2(f):
    """2^f in fp32, exactly (``ldexpf(1.f, f)``)."""
    return np.ldexp(_F32(1.0), int(f)).astype(np.float32)


def ceil_log2(W, defect=None):
    c = 0
    while (1 << c) < W:
        c += 1
    if defect == "floor_log2" and (1 << c) > W:
        c -= 1
    return c


def _finite(x):
    with np.errstate(invalid="ignore"):
        return np.abs(x) <= FLT_MAX  # false for NaN and +-inf, as in the kernels


# ================================================================================ the six twins
def quantize_clamped(x, scale, clip, defect=None):
    x = np.asarray(x, dtype=np.float32)
    v = np.minimum(np.maximum(x, _F32(-clip)), _F32(clip))
    with np.errstate(over="ignore"):
        return _to_u32(_rint(v * _F32(scale), defect))


def mask_twin(x, scale, clip, seeds, signs, rnd, defect=None):
    """``mask_kernel`` -> int32 [n]."""
    acc = quantize_clamped(x, scale, clip, defect)
    if len(seeds) and acc.size:
        acc = acc + net_mask(seeds, signs, rnd, acc.size, defect)[:, 0]
    return acc.view(np.int32)


def unmask_twin(q, inv_scale):
    """``unmask_kernel`` -> fp32 [n]."""
    with np.errstate(over="ignore"):
        return np.asarray(q, dtype=np.int32).astype(np.float32) * _F32(inv_scale)


def hist_plain(x, defect=None):
    """The unmasked histogram (uint32 [HB]) of one client."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    fin = _finite(x)
    bits = int(np.abs(x[fin]).view(np.uint32).max()) if fin.any() else 0
    nf = int((~fin).sum())
    e = bits >> 23
    slot = 0 if bits == 0 else max(e, 1) + 1
    if defect == "slot_pow2_off_by_one" and e >= 1 and (bits & 0x7FFFFF) == 0:
        slot -= 1
    h = np.zeros(HB, dtype=np.uint32)
    h[slot] += 1
    h[1] += np.uint32(nf & _U32)
    return h


def hist_twin(x, seeds, signs, rnd, defect=None):
    """``amax_kernel`` + ``hist_kernel`` -> int32 [HB]."""
    h = hist_plain(x, defect)
    if len(seeds):
        h = h + element_mask(seeds, signs, rnd, HB, defect)
    return h.view(np.int32)


def hist_scale_twin(H, W, defect=None):
    """``hist_scale`` -> (f, bad); ``smax == 0`` gives scale 1.0 = 2^0."""
    H = np.asarray(H).reshape(-1)
    assert H.size == HB
    occ = np.nonzero(H[2:])[0]
    bad = bool(H[1] != 0)
    if occ.size == 0:
        return 0, bad
    smax = int(occ.max()) + 2
    f = 30 - ceil_log2(int(W), defect) - (smax - 127)
    return max(-120, min(60, f)), bad


def quantize_exact(x, f, defect=None):
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    keep = defect == "nonfinite_kept"
    v = x if keep else np.where(_finite(x), x, _F32(0.0))
    with np.errstate(over="ignore", invalid="ignore"):
        return _to_u32(_rint(v * pow2(f), defect), saturate=keep)


def mask_exact_twin(x, H, W, seeds, signs, rnd, defect=None):
    """``mask_exact_kernel`` -> int32 [n]."""
    f, _ = hist_scale_twin(H, W, defect)
    acc = quantize_exact(x, f, defect)
    return (acc + element_mask(seeds, signs, rnd, acc.size, defect)).view(np.int32)


def unmask_exact_twin(q, H, W, defect=None):
    """``unmask_exact_kernel`` -> fp32 [n]."""
    f, bad = hist_scale_twin(H, W, defect)
    q = np.asarray(q, dtype=np.int32).reshape(-1)
    if bad:
        return np.full(q.size, NAN_BITS, dtype=np.uint32).view(np.float32)
    with np.errstate(over="ignore"):
        return q.astype(np.float32) * pow2(-f)


def wrap_sum(parts):
    """int32 wrap-around sum of int32 arrays (what the SUM all-reduce computes)."""
    acc = np.zeros_like(np.asarray(parts[0]), dtype=np.uint32)
    for p in parts:
        acc = acc + np.asarray(p).view(np.uint32)
    return acc.view(np.int32)


def bits(a):
    """The words of an fp32 / int32 array, for a bit-for-bit comparison (-0.0, NaN, inf included)."""
    return np.ascontiguousarray(a).view(np.uint32)


# ================================================================================ seeds and peers
# bit 62 set with a zero low word; a zero high word; bit 62 set with both words busy
SPECIAL_SEEDS = (0x4ABCDEF1 << 32, 0x9E3779B9, (1 << 62) | (0x1357 << 32) | 0x2468ACE1)


def random_seeds(W, salt=0):
    """A symmetric [W, W] int64 matrix of random 63-bit pair seeds (zero diagonal) whose high words are
    non-zero: what ``secagg.pair_seeds`` gives without its 2048-bit exponentiations."""
    rng = np.random.default_rng(1000 + salt)
    m = rng.integers(1 << 40, 1 << 63, size=(W, W), dtype=np.int64)
    m = np.triu(m, 1)
    return m + m.T


def peers_of(i, row):
    """Client i's (seeds, signs) from its row of the pair-seed matrix: +1 towards j > i, -1 towards j < i."""
    js = [j for j in range(len(row)) if j != i]
    return [int(row[j]) for j in js], [1 if i < j else -1 for j in js]


def peers(npeers, salt=0):
    """(seeds, signs) of a direct kernel call: the special seeds first, then random 63-bit ones; signs
    mixed (a lone peer subtracts)."""
    rng = np.random.default_rng(77 + salt)
    extra = rng.integers(1 << 40, 1 << 63, size=max(npeers, 1), dtype=np.int64)
    seeds = (list(SPECIAL_SEEDS) + [int(s) for s in extra])[:npeers]
    signs = [1 if (7 * p + 3) % 5 < 2 else -1 for p in range(npeers)]
    return seeds, signs


ROUNDS = (0, 3, (1 << 32) + 5, (1 << 62) | 7)
NPEERS = (0, 1, 3, 64)
BIG_NPEERS = (0, 1, 3)


# ================================================================================ mask / unmask cases
MaskCase = namedtuple("MaskCase", "name n npeers rnd f clip")
# (f, clip = 2^E) as StarSecureUpload forms them (f = 30 - ceil_log2 W - E), and the defaults
MASK_GRIDS = ((-98, 2.0 ** 127), (0, 2.0 ** 30), (16, 2.0 ** 14), (60, 2.0 ** -30), (16, 1024.0))
MASK_SMALL_N = (1, 255, 256, 257, 4099)
MASK_BIG_N = TRIP + 257  # the second grid-stride trip, partly filled


def _mask_cases():
    out = []
    for n in MASK_SMALL_N:
        for npeers in NPEERS:
            for rnd in ROUNDS:
                for f, clip in MASK_GRIDS:
                    out.append(MaskCase("mask n=%d peers=%d round=%#x f=%d clip=%g" % (n, npeers, rnd, f, clip),
                                        n, npeers, rnd, f, clip))
    for npeers, rnd, (f, clip) in ((0, 0, MASK_GRIDS[0]), (1, ROUNDS[3], MASK_GRIDS[3]), (3, ROUNDS[2], MASK_GRIDS[4])):
        out.append(MaskCase("mask n=%d peers=%d round=%#x f=%d clip=%g" % (MASK_BIG_N, npeers, rnd, f, clip),
                            MASK_BIG_N, npeers, rnd, f, clip))
    return out


MASK_CASES = _mask_cases()


def mask_specials(f, clip):
    """The edge values of a (f, clip) grid: beyond and at +-clip, +-inf, -0.0, denormals, exact ties
    (k + 1/2) 2^-f of both parities and signs, values a quarter off a grid point."""
    c, g = np.float64(clip), np.float64(2.0) ** -f
    v = [2 * c, -2 * c, c, -c, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 1.1754942e-38, -5e-39,
         float(np.nextafter(_F32(c), _F32(0))), -float(np.nextafter(_F32(c), _F32(0)))]
    for k in (0, 1, 2, 3, 6, 7, 100, 101):
        v += [(k + 0.5) * g, -(k + 0.5) * g, (k + 0.25) * g, -(k + 0.75) * g]
    with np.errstate(over="ignore"):
        return np.array(v, dtype=np.float64).astype(np.float32)


@functools.lru_cache(maxsize=8)
def _mask_input(n, f, clip):
    rng = np.random.default_rng(n % 9973 + 17 * (f + 200))
    x = (rng.standard_normal(n) * (clip / 3.0)).astype(np.float32)  # a share beyond +-clip
    sp = mask_specials(f, clip)
    if n == 1:
        x[0] = sp[(f + 200) % sp.size]
    else:
        k = min(n, sp.size)
        x[:k] = sp[:k]
        if n > 2 * sp.size:
            x[-sp.size:] = sp[::-1]  # and in the last (partial) block / the second trip
    x.setflags(write=False)
    return x


def mask_input(case):
    return _mask_input(case.n, case.f, case.clip)


@functools.lru_cache(maxsize=None)
def _mask_want(case):
    seeds, signs = peers(case.npeers)
    w = mask_twin(mask_input(case), 2.0 ** case.f, case.clip, seeds, signs, case.rnd)
    w.setflags(write=False)
    return w


def mask_want(case, defect=None):
    if defect is None:
        return _mask_want(case)
    seeds, signs = peers(case.npeers)
    return mask_twin(mask_input(case), 2.0 ** case.f, case.clip, seeds, signs, case.rnd, defect)


UnmaskCase = namedtuple("UnmaskCase", "name n f")
UNMASK_CASES = [UnmaskCase("unmask n=%d f=%d" % (n, f), n, f)
                for n in (1, 255, 257, 4099, MASK_BIG_N) for f in (-98, 0, 16, 60)]


@functools.lru_cache(maxsize=4)
def unmask_input(n):
    """INT_MIN, INT_MAX, odd values above 2^24 (where the int -> float conversion rounds, ties both
    ways), random words."""
    rng = np.random.default_rng(n)
    q = rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64)
    sp = [-2 ** 31, 2 ** 31 - 1, 2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 + 1), 2 ** 25 + 2, 2 ** 25 + 6, 2 ** 30 + 65,
          2 ** 31 - 65, -(2 ** 31 - 129), 0, -1, 1]
    k = min(n, len(sp))
    q[:k] = sp[:k]
    if n > 2 * len(sp):
        q[-len(sp):] = sp
    q = q.astype(np.int32)
    q.setflags(write=False)
    return q


# ================================================================================ histogram cases
HistCase = namedtuple("HistCase", "name n cls place npeers rnd")
HIST_N = (0, 1, 63, 65, 4099, TRIP + 257)
HIST_MAX = {  # the maximum classes: name -> the largest |x| (None: no finite non-zero value)
    "zero": 0.0,
    "subnormal": 1e-40,
    "subnormal_min": 1e-45,
    "subnormal_max": float(np.nextafter(_F32(1.1754944e-38), _F32(0))),
    "smallest_normal": 1.1754944e-38,
    "pow2_-100": 2.0 ** -100, "pow2_-1": 0.5, "pow2_0": 1.0, "pow2_1": 2.0, "pow2_127": 2.0 ** 127,
    "below_pow2_-100": float(np.nextafter(_F32(2.0 ** -100), _F32(0))),
    "below_pow2_0": float(np.nextafter(_F32(1.0), _F32(0))),
    "below_pow2_127": float(np.nextafter(_F32(2.0 ** 127), _F32(0))),
    "flt_max": float(FLT_MAX),
}
HIST_PLACES = ("first", "last", "partial_wave")
HIST_NPEERS = NPEERS
HIST_ROUNDS = tuple(HIST_ROUND | r for r in ROUNDS)


def _hist_cases():
    out, k = [], 0
    for n in HIST_N:
        for cls in HIST_MAX:
            for place in (HIST_PLACES if n > 1 else ("first",)):
                for npeers in HIST_NPEERS:
                    rnd = HIST_ROUNDS[k % 4]
                    k += 1
                    out.append(HistCase("hist n=%d max=%s at=%s peers=%d round=%#x" % (n, cls, place, npeers, rnd),
                                        n, cls, place, npeers, rnd))
    for n, cls in ((4099, "nonfinite_spread"), (4099, "nonfinite_only"), (65, "nonfinite_only"),
                   (TRIP + 257, "nonfinite_1000"), (TRIP + 257, "nonfinite_only")):
        for npeers in HIST_NPEERS:
            rnd = HIST_ROUNDS[k % 4]
            k += 1
            out.append(HistCase("hist n=%d %s peers=%d round=%#x" % (n, cls, npeers, rnd), n, cls, "first", npeers, rnd))
    return out


HIST_CASES = _hist_cases()
_NONFINITE = np.array([0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0x7F800001, 0xFFFFFFFF],
                      dtype=np.uint32).view(np.float32)  # NaN, -NaN, +-inf, a signalling NaN, all ones


@functools.lru_cache(maxsize=8)
def _hist_input(n, cls, place):
    rng = np.random.default_rng(n % 9973 + 31 * len(cls))
    if cls.startswith("nonfinite"):
        x = rng.standard_normal(n).astype(np.float32)
        if cls == "nonfinite_only":
            x = _NONFINITE[np.arange(n) % _NONFINITE.size].copy()
        else:  # 1000 over many blocks (n > 2^20), or one per wave at n = 4099
            pos = np.linspace(0, n - 1, 1000 if n > TRIP else 65).astype(np.int64)
            x[pos] = _NONFINITE[np.arange(pos.size) % _NONFINITE.size]
        x.setflags(write=False)
        return x
    m = _F32(HIST_MAX[cls])
    # everything else strictly below the maximum in magnitude, of both signs, some of it zero
    with np.errstate(under="ignore"):
        x = (rng.uniform(-0.999, 0.999, n).astype(np.float32) * m).astype(np.float32)
    if n:
        x[rng.integers(0, n, n // 7)] = 0.0
        x = np.where(np.abs(x) >= m, _F32(0.0), x).astype(np.float32)
        at = {"first": 0, "last": n - 1, "partial_wave": max(0, n - 1 - ((n - 1) % 64))}[place]
        x[at] = -m if (n + len(cls)) % 2 else m
    x.setflags(write=False)
    return x


def hist_input(case):
    return _hist_input(case.n, case.cls, case.place)


def hist_want(case, defect=None):
    seeds, signs = peers(case.npeers, salt=1)
    return hist_twin(hist_input(case), seeds, signs, case.rnd, defect)


# ================================================================================ mask_exact cases
ExactCase = namedtuple("ExactCase", "name n W npeers rnd hist")
EXACT_SMALL_N = (1, 2, 3, 4, 5, 4099)
EXACT_BIG_N = 4 * TRIP + 1024 + 3  # the second trip of the 4-element groups, a ragged tail group
EXACT_W = (1, 2, 3, 4, 5, 8, 9, 64, 65, 1 << 23)
# name -> ({slot: count}, W or None for every W, the exponent E that scales the values)
EXACT_HISTS = {
    "natural": ({0: 1, 100: 2, 130: 3}, None),  # slot counts above 1; bound 2^3
    "tiny": ({2: 1, 30: 1}, None),  # bound 2^-97
    "f60_clamp": ({2: 4}, None),  # subnormal maxima: f = 155 - c, clamped to 60
    "f-120_clamp": ({255: 1, 7: 2}, 1 << 23),  # FLT_MAX at W = 2^23: f = -121, clamped to -120
    "huge": ({255: 1}, None),  # bound 2^128: f = -98 - c
    "smax0": ({0: 9}, None),  # every client all zero: scale 1.0
    "slot1": ({1: 2, 127: 1, 0: 1}, None),  # a non-finite coordinate somewhere; bound 2^0
    "negative_count": ({140: -1, 1: 0}, None),  # occupied means non-zero
}


def exact_hist(name):
    h = np.zeros(HB, dtype=np.int32)
    for s, c in EXACT_HISTS[name][0].items():
        h[s] = c
    return h


def _exact_cases():
    out, k = [], 0
    for n in EXACT_SMALL_N:
        for hname, (_, onlyW) in EXACT_HISTS.items():
            for W in (EXACT_W if onlyW is None else (onlyW,)):
                for npeers in NPEERS:
                    if npeers == 64 and n not in (5, 4099):
                        continue
                    rnd = ROUNDS[k % 4]
                    k += 1
                    out.append(ExactCase("exact n=%d W=%d hist=%s peers=%d round=%#x" % (n, W, hname, npeers, rnd),
                                         n, W, npeers, rnd, hname))
    for W, npeers, rnd, hname in ((3, 3, ROUNDS[2], "natural"), (1 << 23, 1, ROUNDS[3], "f-120_clamp"),
                                  (65, 0, 0, "f60_clamp")):
        out.append(ExactCase("exact n=%d W=%d hist=%s peers=%d round=%#x" % (EXACT_BIG_N, W, hname, npeers, rnd),
                             EXACT_BIG_N, W, npeers, rnd, hname))
    return out


EXACT_CASES = _exact_cases()


@functools.lru_cache(maxsize=16)
def _exact_input(n, W, hname):
    H = exact_hist(hname)
    f, _ = hist_scale_twin(H, W)
    occ = np.nonzero(H[2:])[0]
    # values fit the agreed bound 2^E; where no slot is occupied (scale 1.0) or f is clamped to 60 the
    # launcher still takes any value, so small multiples of the grid stand in
    E = int(occ.max()) + 2 - 127 if occ.size else 4
    if f == 60:
        E = -50
    bound, g = np.float64(2.0) ** E, np.float64(2.0) ** -f
    rng = np.random.default_rng(n % 9973 + W % 1009 + len(hname))
    with np.errstate(over="ignore"):
        x = (rng.uniform(-1, 1, n) * bound).astype(np.float32)
        top = float(np.nextafter(_F32(bound), _F32(0))) if np.isfinite(_F32(bound)) else float(FLT_MAX)
        sp = [(0.5) * g, -(1.5) * g, (2.5) * g, -(3.5) * g, np.nan, top, -top, -np.inf, (6.5) * g, (7.5) * g,
              np.inf, -0.0, 1e-45, -1e-40, bound / 2, -bound / 2, (100.5) * g, -(101.5) * g, (0.25) * g, -(0.75) * g]
        if np.isfinite(_F32(bound)):
            sp += [bound, -bound]  # the clip of the star upload: W 2^E 2^f <= 2^30 still
        sp = np.array(sp, dtype=np.float64).astype(np.float32)
    if n <= 5:
        x[:] = np.roll(sp, -(W % 7))[:n]  # the tiny sizes walk through the specials as W varies
    else:
        x[:sp.size] = sp
        x[-sp.size:] = sp[::-1]  # the ragged tail group
    if hname == "f60_clamp" and n > 5:
        sub = rng.integers(1, 1 << 23, n // 2).astype(np.uint32).view(np.float32)  # subnormal inputs
        x[sp.size:sp.size + sub.size] = sub * np.where(rng.uniform(size=sub.size) < 0.5, _F32(-1), _F32(1))
    x.setflags(write=False)
    return x


def exact_input(case):
    return _exact_input(case.n, case.W, case.hist), exact_hist(case.hist)


def exact_want(case, defect=None):
    x, H = exact_input(case)
    seeds, signs = peers(case.npeers, salt=2)
    return mask_exact_twin(x, H, case.W, seeds, signs, case.rnd, defect)


UnmaskExactCase = namedtuple("UnmaskExactCase", "name n W hist")
UNMASK_EXACT_CASES = [UnmaskExactCase("unmask_exact n=%d W=%d hist=%s" % (n, W, h), n, W, h)
                      for n in (1, 2, 3, 4, 5, 4099, EXACT_BIG_N)
                      for h, (_, onlyW) in EXACT_HISTS.items()
                      for W in ((1, 3, 8, 9, 65, 1 << 23) if onlyW is None else (onlyW,))
                      if n <= 4099 or (h, W) in (("natural", 3), ("f-120_clamp", 1 << 23), ("slot1", 9), ("f60_clamp", 1))]


# ================================================================================ fleets: W clients
Fleet = namedtuple("Fleet", "name W n rnd nonfinite")
FLEET_W = (2, 3, 5, 8, 17, 65)  # W = 65: npeers = MAXP
CPU_FLEET_W = (1, 2, 3, 5, 8, 9, 17)
FLEET_N = 1027  # two blocks of 4-element groups, a ragged tail group


def fleet_inputs(W, n=FLEET_N, nonfinite=False, salt=0):
    """W clients' fp32 vectors: scales spread over many binades, the largest coordinate held by one
    client alone, ties on the grid the fleet will agree (the maximum 2^9 fixes it)."""
    rng = np.random.default_rng(5 * W + n + salt)
    xs = []
    for k in range(W):
        x = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 2)).astype(np.float32)
        xs.append(x)
    xs[W // 2][n // 3] = -700.0  # slot 137: E = 10
    f = 30 - ceil_log2(W) - 10
    g = 2.0 ** -f
    for k in range(W):
        xs[k][:8] = np.array([0.5, 1.5, -0.5, -2.5, 3.5, 0.25, -0.75, 1000.5], dtype=np.float64) * g * (1 + k % 3)
    if nonfinite:
        xs[W - 1][n // 2] = np.float32("nan")
        xs[W - 1][n - 1] = np.float32("-inf")
    return xs


def fleet_exact(xs, seeds, rnd, defect=None):
    """The written protocol on the CPU: -> (masked histograms, summed histogram, f, uploads, summed
    payload, dequantised result)."""
    W = len(xs)
    hs = [hist_twin(xs[i], *peers_of(i, seeds[i]), HIST_ROUND | rnd, defect) for i in range(W)]
    H = wrap_sum(hs)
    f, _ = hist_scale_twin(H, W, defect)
    ups = [mask_exact_twin(xs[i], H, W, *peers_of(i, seeds[i]), rnd, defect) for i in range(W)]
    total = wrap_sum(ups)
    return hs, H, f, ups, total, unmask_exact_twin(total, H, W, defect)


def plain_quantized_sum(xs, f):
    """``sum_k round(x_k 2^f)`` in exact integers (fp64 holds x 2^f exactly; non-finite -> 0)."""
    tot = np.zeros(xs[0].size, dtype=np.int64)
    for x in xs:
        v = np.where(_finite(x), x, _F32(0.0)).astype(np.float64)
        tot += np.rint(np.ldexp(v, f)).astype(np.int64)
    return tot
