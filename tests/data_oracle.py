"""Exact twins and fp64 oracles of the batch builder (csrc/batch.hip: ``dedup``, ``sample_batch``,
``multi_copy``) and of the per-news gradient reduction (csrc/news_grad.hip: every segment-sum form,
the LDP clip and noise), with a per-element bound on what the HIP kernels may differ by (a plain
helper module for tests/test_data_oracle_cpu.py and tests/test_data_oracle_gpu.py, not a conftest;
no GPU dependency: everything here runs on the CPU, in numpy, with ``ops.reference.philox4x32`` as
the one source of random words).

================================================================================================
1. Exact twins (integers only: the kernels must agree bit for bit).

* ``dedup_oracle``: ``perm`` is the stable sort of the occurrences by id, ``uniq`` the sorted distinct
  ids, ``inv[r]`` the row of ``uniq`` holding ``ids[r]``, ``seg_ptr`` the offsets of the runs in ``perm``.
* ``sample_oracle``: ``sample_kernel`` line by line.  Row r draws Philox(seed, offset) at counters
  ``(r << 20) + k``, k = 0, 1, ...; each call gives four words and each word one index
  ``(word * n) >> 32`` (unbiased to 2^-32 n, unlike ``word % n``); an index already picked is
  rejected, until ``npratio`` are held.  ``n < npratio``: the negatives in order, then 0.  ``valid``:
  the last ``min(n, npratio)`` negatives, zero padded, no randomness.  History: the last
  ``min(len, H)`` ids (``truncate``) or the first ``min(len, H)`` (compat), zero padded to H.
* ``multi_copy_oracle``: ``dst[i] = src[i]`` for ``i < n_src``, the fill word after, in 4-byte words.

================================================================================================
2. The LDP noise field.  Element (r, d) of the occurrence rows takes one of the four normals of one
Philox(seed, offset + dev_off) call.  There are TWO counter layouts, and the dispatch of
``segment_sum_rows`` (variant, ``D % 4``, 16-byte alignment) selects which one runs -- the same seed
gives a different field in each::

    "fused"  (float4 chunk pass, variant 2, D % 4 == 0, aligned):
             counter (r << 16) | (d / 4),                        component d % 4
    "rows"   (ldp_rows_kernel, every other case; element d = lane + 64 kk):
             counter (r << 16) | (2 lane + kk / 4),              component kk % 4

Words (x, y) make components 0 and 1, words (z, w) components 2 and 3::

    u = ((word >> 8) + 1) / 2^24        exact in fp32 and here: u in (0, 1]
    rad = sqrt(-2 ln u1)    z = rad (cos, sin)(2 pi u2)         fp64 here

Every (row, element-group) counter of a layout is distinct for D <= 512 (the low field stays below
2^16 = the row stride; the CPU test enumerates them).

================================================================================================
3. Bounds.  ``u = 2^-24``, round to nearest, first-order counts with one spare unit, magnitudes
cancellation-free, ``TINY = 1e-30`` so that an exact oracle demands an exact kernel -- all as in
``tests/norm_oracle.py``.

* clip factor ``f = min(1, clip / (||g|| + 1e-12))``.  The D squares and D - 1 adds of ``sum g^2`` are
  all positive: (D + 1) u relative on the sum (taken; 2 D - 1 roundings of partial sums, each of a
  part of the total, count D in the first order), halved by the root.  ``sqrtf`` and the division
  are correctly rounded (no fast-math in this build), 1 u each; the ``+ 1e-12`` add 1 u; one spare::

      rel_f = ((D + 1) / 2 + 4) u

  where the oracle's unclamped ratio is below ``1 + rel_f``; above it both sides clamp to exactly 1
  and the factor carries no error.
* normal ``z``.  ``-2 ln u1`` doubles exactly; ``logf`` (1 ulp = 2 u, halved by the root), ``sqrtf`` and
  the product ``rad * cos`` (1 u each): ``3 u |z|``.  The angle ``2 pi u2`` is formed in fp32: its rounding
  (half an ulp of a value below 8 is 2^-22 < 2 pi u) turns z by up to ``2 pi u`` of its radius.
  ``__sincosf`` compiles to the hardware sine / cosine, whose absolute accuracy is not documented::

      e_z = 3 u |z| + rad (2 pi u + E_TRIG)

  ``E_TRIG`` is measured on the device by the noise-only probe of the GPU test (rows 0, clip 0, std 1,
  one occurrence per segment: the output is z itself) as ``max (|z_gpu - z_64| - 3 u |z| - 2 pi u rad)
  / rad`` (``measure_e_trig``), recorded below as ``E_TRIG_MEASURED`` with the probe size, and used
  as ``E_TRIG = 4 E_TRIG_MEASURED`` (the probe sees ~2^17 of the 2^24 angles).  Whatever is measured,
  the value in use is capped: ``E_TRIG <= 2^-12`` (``E_TRIG_CAP``), or the measurement is a finding.
* transformed occurrence ``t = g f + std z`` (two products and an add, or their fmas)::

      e_t = |g| rel_f + std e_z + 3 u (|g f| + |std z| + |t|)

  Without clip and noise the rows pass through untouched: ``e_t = 0``.
* a segment of n occurrences is an n-term sum, whatever the order (chunk partials, the fix pass's
  4-wave / 32-stride partition, the 16-wave block form)::

      tol = sum e_t + (n - 1) u sum |t| + TINY

  n = 1 leaves ``sum e_t + TINY``: a plain one-occurrence segment is its row bit for bit; n = 0 (the
  padded unique slots of the step graphs) is exactly 0.

================================================================================================
4. Layout cases (``CASES``, chunk length 16) place segments on the chunk grid on purpose; the
occurrences of a segment are scattered through the row order by a seeded permutation.  ``int_rows``
are integers in [-8, 8] (every fp32 sum is exact in any order: a dropped, doubled or misplaced row
is a bit difference); ``float_rows`` are unit Gaussian with row r scaled by ``2^(r % 7 - 3)`` plus an
all-zero row and rows with norms just under, just over (both inside the ``rel_f`` window) and far
over the clip.

5. fp32 numpy models of the kernels' indexing (``model_*``: the chunk pass with its slot rule, the
fix pass, the block-per-row form, both noise layouts, the narrow / wide dedup keys) and their
planted defects (``defect=...``) let the CPU test show that the bounds hold for a correct kernel
and fail for each wrong one.

Judging: ``elem_ratio`` -- ``|cand - ref| / tol``, 0 where equal, infinite for a NaN / inf candidate."""
import math

import numpy as np
import torch

from fedrec_with_pytorchdistributed_amd.ops import reference as ref

U = 2.0 ** -24
TINY = 1e-30
SCH = 16  # chunk length of the chunked segment sums
TWO_PI = 2.0 * math.pi

# measured on the MI355X by test_noise_probe (tests/test_data_oracle_gpu.py), per probe (seed 11,
# offset 3; 1,638,400 and 407,552 normals): 3.691e-8 and 3.360e-8, rounded up.  The derived
# radius and angle terms carry nearly all of the difference; the hardware term is ~0.6 u.
E_TRIG_MEASURED = {"fused R=4096 D=400": 3.70e-8, "rows R=1024 D=398": 3.37e-8}
E_TRIG_CAP = 2.0 ** -12
E_TRIG = 4.0 * max(E_TRIG_MEASURED.values())

F32 = np.float32


# ------------------------------------------------------------------------------------ judging
def elem_ratio(cand, want, tol) -> np.ndarray:
    c = np.asarray(cand, dtype=np.float64)
    d = np.abs(c - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(d == 0, 0.0, d / tol)
    return np.where(np.isfinite(c), r, np.inf)


def check(cand, want, tol, what: str = "") -> float:
    """Assert the worst ratio <= 1 (the message names the worst element); returns it."""
    r = elem_ratio(cand, want, tol)
    w = float(r.max()) if r.size else 0.0
    if not w <= 1.0:
        idx = np.unravel_index(int(r.argmax()), r.shape)
        raise AssertionError("%s: worst element %s: ratio %.4g (got %.9g, want %.9g, bound %.3g); %d of %d above 1"
                             % (what, tuple(int(i) for i in idx), w, float(np.asarray(cand)[idx]), float(want[idx]),
                                float(np.broadcast_to(tol, r.shape)[idx]), int((r > 1).sum()), r.size))
    return w


def words(seed: int, offset: int, ctr) -> np.ndarray:
    """Philox words of int64 counters -> ``[..., 4]`` int64 holding uint32 values."""
    c = torch.from_numpy(np.ascontiguousarray(np.asarray(ctr, dtype=np.int64)))
    return ref.philox4x32(int(seed), int(offset), c).numpy()


# ------------------------------------------------------------------------------------ dedup
def dedup_oracle(ids):
    """-> ``uniq, inv, perm, seg_ptr`` (int64): ``perm`` the stable sort by id."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    R = ids.size
    perm = np.array(sorted(range(R), key=lambda i: (int(ids[i]), i)), dtype=np.int64)
    uniq, seg, inv = [], [], np.zeros(R, dtype=np.int64)
    for p in range(R):
        r = perm[p]
        if p == 0 or ids[r] != ids[perm[p - 1]]:
            uniq.append(int(ids[r]))
            seg.append(p)
        inv[r] = len(uniq) - 1
    seg.append(R)
    return np.array(uniq, dtype=np.int64), inv, perm, np.array(seg, dtype=np.int64)


def model_dedup(ids, num_news: int, defect=None):
    """The kernels' keyed sort: ``id << 13 | i`` in 32 bits when ``0 < num_news <= 2^19``, else
    ``id << 32 | i``; pads (all ones) fill up to a power of two >= 1024 and sort last; the flags run
    over the first R sorted keys.  ``defect="pad_eq"``: the narrow pad key carries occurrence 0, so
    it equals the key of (largest id, occurrence 0) and sorts among the real keys of that id."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    R = ids.size
    narrow = 0 < num_news <= (1 << 19)
    shift, bits = (13, 32) if narrow else (32, 64)
    P = 1024
    while P < R:
        P <<= 1
    pad = (1 << bits) - 1
    if defect == "pad_eq" and narrow:
        pad = ((1 << 19) - 1) << 13
    keys = [((int(ids[i]) & 0xFFFFFFFF) << shift | i) & ((1 << bits) - 1) for i in range(R)] + [pad] * (P - R)
    keys.sort()
    uniq, seg, inv, perm = [], [], np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64)
    for i in range(R):
        r = keys[i] & ((1 << shift) - 1)
        if i == 0 or (keys[i] >> shift) != (keys[i - 1] >> shift):
            uniq.append(keys[i] >> shift)
            seg.append(i)
        perm[i] = r
        if r < R:
            inv[r] = len(uniq) - 1
    seg.append(R)
    return np.array(uniq, dtype=np.int64), inv, perm, np.array(seg, dtype=np.int64)


# ------------------------------------------------------------------------------------ sampler
def sample_oracle(rows, pos, neg_ptr, negs, his_ptr, his, npratio: int, H: int, truncate: bool, seed: int,
                  offset: int, valid: bool = False, defect=None):
    """-> ``cand [B, npratio + 1], hist [B, H]`` (int32).  ``defect``: ``"mod"`` (``word % n``) or
    ``"his_off1"`` (the history window one id early) -- the planted defects of the CPU test."""
    rows = np.asarray(rows, dtype=np.int64)
    pos, negs, his = np.asarray(pos), np.asarray(negs), np.asarray(his)
    neg_ptr, his_ptr = np.asarray(neg_ptr, dtype=np.int64), np.asarray(his_ptr, dtype=np.int64)
    B = rows.size
    cand = np.zeros((B, npratio + 1), dtype=np.int32)
    hist = np.zeros((B, H), dtype=np.int32)
    n_all = neg_ptr[rows + 1] - neg_ptr[rows]
    K = 8  # counters drawn ahead for every random row (more on demand)
    rnd = np.nonzero(n_all >= npratio)[0] if not valid else np.zeros(0, dtype=np.int64)
    ahead = {}
    if rnd.size:
        w = words(seed, offset, (rows[rnd, None] << 20) + np.arange(K)[None, :]).reshape(rnd.size, 4 * K)
        ahead = {int(b): w[i] for i, b in enumerate(rnd)}
    for b in range(B):
        r = int(rows[b])
        n0, n = int(neg_ptr[r]), int(n_all[b])
        cand[b, 0] = pos[r]
        if valid:
            take = min(n, npratio)
            cand[b, 1:1 + take] = negs[n0 + n - take:n0 + n]
        elif n < npratio:
            cand[b, 1:1 + n] = negs[n0:n0 + n]
        else:
            pick, k, w = [], 0, ahead[b]
            while len(pick) < npratio:
                if k == w.size:  # the next block of counters of this row
                    w = np.concatenate([w, words(seed, offset, (r << 20) + k // 4 + np.arange(32)).reshape(-1)])
                x = int(w[k])
                k += 1
                idx = x % n if defect == "mod" else (x * n) >> 32
                if idx not in pick:
                    pick.append(idx)
            cand[b, 1:] = negs[n0 + np.array(pick, dtype=np.int64)]
        h0, hl = int(his_ptr[r]), int(his_ptr[r + 1] - his_ptr[r])
        take = min(hl, H)
        start = h0 + hl - take if truncate else h0
        if defect == "his_off1":
            start = max(start - 1, 0)
        hist[b, :take] = his[start:start + take]
    return cand, hist


def multi_copy_oracle(src, n_dst, fill):
    """``src``: 1-D arrays of a 4-byte dtype; ``n_dst``: words per destination; ``fill``: int32 words.
    -> the destinations, each in its source's dtype."""
    out = []
    for s, nd, f in zip(src, n_dst, fill):
        s = np.ascontiguousarray(s)
        w = s.view(np.int32).reshape(-1)
        d = np.full(int(nd), np.array(int(f), dtype=np.int64).astype(np.int32), dtype=np.int32)
        d[:w.size] = w
        out.append(d.view(s.dtype))
    return out


# ------------------------------------------------------------------------------------ noise field
def noise_counters(R: int, D: int, layout: str, row_ids=None):
    """-> ``low [D]`` (the counter's low field of element d), ``comp [D]`` (its component) and
    ``rid [R]`` (the counter's row field: the occurrence row)."""
    d = np.arange(D, dtype=np.int64)
    if layout == "fused":
        low, comp = d // 4, d % 4
    elif layout == "rows":
        lane, kk = d % 64, d // 64
        low, comp = 2 * lane + kk // 4, kk % 4
    else:
        raise ValueError(layout)
    rid = np.arange(R, dtype=np.int64) if row_ids is None else np.asarray(row_ids, dtype=np.int64)
    return low, comp, rid


def _box_muller(w, dtype, swap=False):
    """Words ``[..., 4]`` -> the four normals and their radii ``[..., 4]`` in ``dtype`` (fp64: the
    oracle; fp32: the kernels' arithmetic, every operation rounded to fp32)."""
    t = dtype
    u = ((w >> 8) + 1).astype(t) * t(1.0 / 16777216.0)
    u1, u2 = u[..., 0::2], u[..., 1::2]
    rad = np.sqrt(t(-2.0) * np.log(u1))
    ang = t(6.283185307179586 if t is F32 else TWO_PI) * u2
    c, s = np.cos(ang), np.sin(ang)
    if swap:
        c, s = s, c
    z = np.stack([rad * c, rad * s], -1).reshape(w.shape)
    return z.astype(t), np.repeat(rad, 2, axis=-1).astype(t)


def _noise(R, D, seed, offset, layout, dtype, row_ids=None, ctr_shift=0, swap=False):
    low, comp, rid = noise_counters(R, D, layout, row_ids)
    lows, where = np.unique(low, return_inverse=True)
    w = words(seed, offset, ((rid[:, None] << 16) | lows[None, :]) + ctr_shift)  # [R, n_low, 4]
    z4, r4 = _box_muller(w, dtype, swap)
    return z4[:, where, comp], r4[:, where, comp]


def ldp_noise_parts(R: int, D: int, seed: int, offset: int, layout: str, row_ids=None, ctr_shift: int = 0):
    """-> ``z, rad`` ``[R, D]`` fp64: the standard normals and the Box-Muller radius of each."""
    return _noise(R, D, seed, offset, layout, np.float64, row_ids, ctr_shift)


def ldp_noise(R: int, D: int, seed: int, offset: int, layout: str) -> np.ndarray:
    return ldp_noise_parts(R, D, seed, offset, layout)[0]


def noise_tol(z, rad, e_trig=None):
    e = E_TRIG if e_trig is None else e_trig
    return 3 * U * np.abs(z) + rad * (TWO_PI * U + e)


def measure_e_trig(z_gpu, z, rad) -> float:
    """The hardware term of the probe: what is left of ``|z_gpu - z|`` after the derived radius and
    angle terms, per unit radius.  rad = 0 (u1 = 1) must give z = 0 exactly."""
    d = np.abs(np.asarray(z_gpu, dtype=np.float64) - z) - 3 * U * np.abs(z) - TWO_PI * U * rad
    assert bool((np.asarray(z_gpu)[rad == 0] == 0).all())
    return float(np.max(np.maximum(d, 0.0)[rad > 0] / rad[rad > 0]))


# ------------------------------------------------------------------------------------ transformed rows
def rel_f(D: int) -> float:
    return ((D + 1) / 2 + 4) * U


def ldp_rows_oracle(rows, clip: float, std: float, seed: int = 0, offset: int = 0, layout: str = "fused",
                    e_trig=None, noise=None):
    """-> ``t, e_t`` ``[R, D]`` fp64: ``t = g f + std z`` and its bound (section 3).  ``noise``: the
    ``(z, rad)`` of ``ldp_noise_parts`` for this (seed, offset, layout), when the caller holds it."""
    g = np.asarray(rows, dtype=np.float64)
    R, D = g.shape
    if clip <= 0 and std <= 0:
        return g.copy(), np.zeros_like(g)
    f, rf = np.ones(R), np.zeros(R)
    if clip > 0:
        ratio = clip / (np.sqrt((g * g).sum(1)) + 1e-12)
        f = np.minimum(1.0, ratio)
        rf = np.where(ratio < 1 + rel_f(D), rel_f(D), 0.0)
    z, e_z = np.zeros_like(g), np.zeros_like(g)
    if std > 0:
        z, rad = ldp_noise_parts(R, D, seed, offset, layout) if noise is None else noise
        e_z = noise_tol(z, rad, e_trig)
    gf = g * f[:, None]
    t = gf + std * z
    e_t = np.abs(g) * rf[:, None] + std * e_z + 3 * U * (np.abs(gf) + np.abs(std * z) + np.abs(t))
    return t, e_t


def segsum_oracle(t, inv, U_out: int) -> np.ndarray:
    """fp64 ``index_add``; empty segments are exactly 0."""
    src = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64))
    idx = torch.from_numpy(np.ascontiguousarray(inv, dtype=np.int64))
    return torch.zeros(U_out, src.shape[1], dtype=torch.float64).index_add_(0, idx, src).numpy()


def segsum_tol(t, e_t, inv, U_out: int) -> np.ndarray:
    inv = np.asarray(inv, dtype=np.int64)
    n = np.bincount(inv, minlength=U_out).astype(np.float64)
    return segsum_oracle(e_t, inv, U_out) + np.maximum(n - 1, 0)[:, None] * U * segsum_oracle(np.abs(t), inv, U_out) + TINY


# ------------------------------------------------------------------------------------ layouts
class Layout:
    """``ids, inv, perm [R]``, ``seg_ptr [U_pad + 1]`` (trailing entries R), ``U`` real segments."""

    def __init__(self, ids, inv, perm, seg_ptr, U_real):
        self.ids, self.inv, self.perm, self.seg_ptr = ids, inv, perm, seg_ptr
        self.U, self.U_pad, self.R = U_real, seg_ptr.size - 1, ids.size


def layout(lengths, scatter_seed: int, trailing: int = 0) -> Layout:
    """Segments of the given lengths, in order, on the position grid; segment s holds id ``3 s`` (the
    first is the pad id 0); its occurrences are scattered through the rows by a seeded permutation
    and listed in ascending row order (the stable sort ``dedup`` produces)."""
    lengths = [int(x) for x in lengths]
    assert min(lengths) >= 1
    R = sum(lengths)
    p = np.random.default_rng(scatter_seed).permutation(R)
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    perm, inv = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64)
    for s in range(len(lengths)):
        perm[ptr[s]:ptr[s + 1]] = np.sort(p[ptr[s]:ptr[s + 1]])
        inv[perm[ptr[s]:ptr[s + 1]]] = s
    seg_ptr = np.concatenate([ptr, np.full(trailing, R, dtype=np.int64)])
    return Layout(3 * inv, inv, perm, seg_ptr, len(lengths))


def _mind_lengths(R=700):
    rng = np.random.default_rng(700)
    n_pad = int(0.3 * R)
    p = 1.0 / np.arange(1, 600)
    tail = rng.choice(599, size=R - n_pad, p=p / p.sum())
    cnt = np.bincount(tail)
    return [n_pad] + [int(c) for c in cnt if c > 0]


CASES = {
    "two_full_chunks": [16, 16],
    "15_2_15": [15, 2, 15],
    "singletons37": [1] * 37,
    "one_segment_34_chunks": [16 * 33 + 5],
    "crossing_70_chunks": [3, 16 * 70, 1, 1, 7],
    "ends_on_edge_next_starts_on_it": [13, 19, 16, 1],
    "starts_on_edge_runs_past": [16, 20, 3],
    "five": [5],
    "one": [1],
    "six_chunks_last_of_one": [16] * 5 + [1],
    "mind_skew_700": _mind_lengths(),
}
TRAILING = (0, 1, 9)


def case_layout(name: str, trailing: int = 0) -> Layout:
    return layout(CASES[name], scatter_seed=len(name) + 17 * len(CASES[name]), trailing=trailing)


# ------------------------------------------------------------------------------------ rows
def int_rows(R: int, D: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(1000 + seed).integers(-8, 9, size=(R, D)).astype(F32)


def float_rows(R: int, D: int, seed: int = 0, clip: float = 2.0) -> np.ndarray:
    g = np.random.default_rng(2000 + seed).standard_normal((R, D))
    g *= (2.0 ** (np.arange(R) % 7 - 3))[:, None]
    if R >= 8:  # an all-zero row; norms just under / just over (inside the rel_f window) / far over the clip
        nrm = lambda r: math.sqrt(float((g[r] * g[r]).sum()))
        g[R // 5] = 0.0
        for r, target in ((2 * R // 5, clip * (1 - 1e-6)), (3 * R // 5, clip * (1 + 1e-6)), (4 * R // 5, 50.0 * clip)):
            g[r] *= target / nrm(r)
    return g.astype(F32)


# ------------------------------------------------------------------------------------ integer inputs
NEG_COUNTS = (0, 1, 3, 4, 5, 16, 17, 1000)


def sampler_csr(n_rows: int, H: int):
    """A CSR shard: negative counts cycle through ``NEG_COUNTS``, history lengths through
    ``0, 1, H - 1, H, H + 1, 3 H`` (every pair of the two within 48 rows); the negatives of a row are
    distinct ids.  -> ``pos, neg_ptr, negs, his_ptr, his`` (int32 ids, int64 pointers)."""
    r = np.arange(n_rows, dtype=np.int64)
    ncnt = np.array(NEG_COUNTS, dtype=np.int64)[r % 8]
    hcnt = np.array([0, 1, H - 1, H, H + 1, 3 * H], dtype=np.int64)[(r // 8) % 6]
    neg_ptr = np.concatenate([[0], np.cumsum(ncnt)]).astype(np.int64)
    his_ptr = np.concatenate([[0], np.cumsum(hcnt)]).astype(np.int64)
    row_of = np.repeat(r, ncnt)
    negs = ((row_of * 7 + (np.arange(neg_ptr[-1]) - neg_ptr[row_of]) * 3) % 100003 + 1).astype(np.int32)
    his = (np.arange(his_ptr[-1], dtype=np.int64) * 11 % 50021 + 1).astype(np.int32)
    pos = (r * 13 % 70001 + 1).astype(np.int32)
    return pos, neg_ptr, negs, his_ptr, his


DEDUP_PATTERNS = ("equal", "descending", "random", "thread_runs", "wave_runs", "top_last", "wide_max")


def dedup_ids(pattern: str, R: int, num_news: int) -> np.ndarray:
    """Id lists of the dedup tests (int64 values below ``num_news``, or below 2^31 for ``num_news``
    0).  ``thread_runs`` / ``wave_runs``: runs of exactly ``ceil(R / 1024)`` ids (64 times that), so the
    "new id" flags sit on the edges of the scan's per-thread / per-wave runs; ``top_last``: random
    ids with ``num_news - 1`` at the last occurrence (the largest key, next to the pad key);
    ``wide_max`` (wide keys only): random ids up to ``2^31 - 1``, that value present."""
    limit = num_news if num_news > 0 else 1 << 31
    rng = np.random.default_rng(R * 31 + limit % 1000003)
    i = np.arange(R, dtype=np.int64)
    if pattern == "equal":
        return np.full(R, limit - 1, dtype=np.int64)
    if pattern == "descending":
        return limit - 1 - i if limit >= R else (R - 1 - i) % limit
    if pattern in ("random", "top_last"):
        pool = rng.integers(0, limit, size=max(1, R // 3))  # ids over the whole range, each ~3 times
        ids = pool[rng.integers(0, pool.size, size=R)]
        if pattern == "top_last":
            ids[-1] = limit - 1
        return ids
    if pattern in ("thread_runs", "wave_runs"):
        run = (R + 1023) // 1024 * (64 if pattern == "wave_runs" else 1)
        return ((R - 1) // run - i // run) % limit
    if pattern == "wide_max":
        assert limit >= 1 << 31
        ids = rng.integers(0, 1 << 31, size=R)
        ids[R // 2] = (1 << 31) - 1
        return ids
    raise ValueError(pattern)


# ------------------------------------------------------------------------------------ fp32 models
def model_transform(rows, clip, std, seed=0, offset=0, layout="fused", defect=None, row_ids=None):
    """The kernels' clip + noise in fp32.  ``defect``: ``"no_noise_hi"`` (elements >= 256, the second
    float4 column group, get no noise), ``"clip_after"`` (the factor scales row + noise),
    ``"swap_sincos"``; ``row_ids`` replaces the occurrence row in the counter."""
    g = np.asarray(rows, dtype=F32)
    R, D = g.shape
    if clip <= 0 and std <= 0:
        return g.copy()
    f = np.ones(R, dtype=F32)
    if clip > 0:
        sq = (g * g).sum(1, dtype=F32)
        f = np.minimum(F32(1.0), F32(clip) / (np.sqrt(sq) + F32(1e-12))).astype(F32)
    z = np.zeros_like(g)
    if std > 0:
        z = _noise(R, D, seed, offset, layout, F32, row_ids, 0, defect == "swap_sincos")[0]
        if defect == "no_noise_hi":
            z[:, 256:] = 0
    if defect == "clip_after":
        return ((g + F32(std) * z) * f[:, None]).astype(F32)
    return (g * f[:, None] + F32(std) * z).astype(F32)


def model_chunk_sum(t32, lay: Layout, defect=None) -> np.ndarray:
    """The chunk pass (one wave per 16 positions, the slot rule) and the fix pass (4 waves, entries
    w, w + 4, ... in rounds of 32) in fp32.  Scratch and output start as NaN: a slot read before it
    is written, or an output row nobody writes, shows.  ``defect``: ``"fix_skip_last"`` (the last
    chunk's slot 0 is not added), ``"fix_32"`` (the fix pass stops after 32 partials)."""
    t32 = np.asarray(t32, dtype=F32)
    R, D = t32.shape
    perm, ptr, inv = lay.perm, lay.seg_ptr, lay.inv
    nch = (R + SCH - 1) // SCH
    scratch = np.full((nch, 2, D), np.nan, dtype=F32)
    out = np.full((lay.U_pad, D), np.nan, dtype=F32)
    for c in range(nch):
        p0, p1 = c * SCH, min(c * SCH + SCH, R)
        u = int(inv[perm[p0]])
        s_beg, s_end = int(ptr[u]), int(ptr[u + 1])
        acc = np.zeros(D, dtype=F32)
        for pp in range(p0, p1):
            acc = acc + t32[perm[pp]]
            if pp + 1 == s_end or pp + 1 == p1:
                if s_beg >= p0 and s_end <= p1:
                    out[u] = acc
                else:
                    scratch[c, 0 if s_beg < p0 else 1] = acc
                acc = np.zeros(D, dtype=F32)
                if pp + 1 == s_end and pp + 1 < p1:
                    u += 1
                    s_beg, s_end = s_end, int(ptr[u + 1])
    for u in range(lay.U_pad):
        beg, end = int(ptr[u]), int(ptr[u + 1])
        if beg == end:
            out[u] = 0
            continue
        c0, c1 = beg // SCH, (end - 1) // SCH
        if c0 == c1:
            continue
        n = c1 - c0 + 1
        part = np.zeros((4, D), dtype=F32)
        for w in range(4):
            for i0 in range(w, n, 32):
                if defect == "fix_32" and i0 >= 32:
                    break
                for j in range(8):
                    i = i0 + 4 * j
                    if i < n and not (defect == "fix_skip_last" and i == n - 1):
                        part[w] = part[w] + (scratch[c0, 1] if i == 0 else scratch[c0 + i, 0])
        out[u] = ((part[0] + part[1]) + part[2]) + part[3]
    return out


def model_block_sum(t32, lay: Layout, zero_empty: bool = True) -> np.ndarray:
    """The block-per-row form: wave w of 16 adds occurrences beg + w, beg + w + 16, ...; the 16
    partials add in order."""
    t32 = np.asarray(t32, dtype=F32)
    D = t32.shape[1]
    out = np.zeros((lay.U_pad, D), dtype=F32)
    for u in range(lay.U_pad):
        beg, end = int(lay.seg_ptr[u]), int(lay.seg_ptr[u + 1])
        tot = np.zeros(D, dtype=F32)
        for w in range(16):
            acc = np.zeros(D, dtype=F32)
            for i in range(beg + w, end, 16):
                acc = acc + t32[lay.perm[i]]
            tot = tot + acc
        out[u] = tot
    return out
