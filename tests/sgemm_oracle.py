"""An fp64 oracle of the small-GEMM family (csrc/small_gemm.hip: every launch form, ``splitk_reduce``,
``colsum_f32``) and of the weight-gradient GEMM (csrc/gemm_wgrad.hip), with a bound per output
element on what the HIP kernels may differ by (a plain helper module of the tests, not a conftest;
every function runs on the device of its arguments).

Operands.  ``C = act(alpha A B^T + bias) o Z (+ C)`` with the logical ``A`` [M, K] and ``B`` [N, K] of a
:class:`ops.Gemm` formed exactly as the kernels form them (``operand``): element ``(r, c)`` of a
stored matrix is ``base + r * ld + c``; ``a_mode`` / ``b_mode`` 1 read it transposed; ``gather_on`` 1 / 2
takes row ``gidx[r]``; a K-segmented B (``kseg``) takes rows ``[i kseg, (i + 1) kseg)`` from block
``i`` of ``(B, bseg[0], bseg[1])``; ``drop_on`` 1 / 2 multiplies an fp32 operand by the Philox scale of
element ``row * drop_ld + col`` -- an fp32 product, 0 or ``v * fp32(1 / (1 - p))`` -- and only then is an
fp32 operand rounded to bf16, once, to nearest even (``f2bf`` is the compiler's conversion).  A bf16
operand is taken as is.  So OPERAND ROUNDING IS NO SOURCE OF TOLERANCE: the oracle is fp64 arithmetic
on the same bf16 values, and what remains is the fp32 accumulation and the epilogue.

Roundings, ``U = 2^-24`` (fp32), first order, one spare unit per count; ``S = |A| |B|^T``.  One term
per line of ``small_gemm_oracle``, in the order of the kernels' epilogue (``gemm_tile``,
``gemm_tile_dma``, ``small_gemm_rd_kernel``, ``splitk_reduce_block`` all apply the same one):

* accumulation: products of bf16 values are exact in fp32; ``v_mfma_f32_16x16x32_bf16`` adds the K
  of them in fp32 (at most one rounding per product added, in any order); split-K adds the
  ``splits`` partials (``splits - 1`` roundings); ``alpha *`` is one more (or none: the compiler may
  contract ``alpha v + bias``): ``e = (K + splits + 2) U |alpha| S`` (K + splits counted, 2 spare);
* the bias add rounds a value of magnitude <= ``|alpha| S + |bias|``; the first part is in the spare
  units above: ``e += U |bias|``;
* tanh carries ``e`` by ``|tanh'| <= 1`` and adds the error of the device's ``tanhf``,
  ``TANH_TERM U max(|y|, TANH_TINY)`` with ``TANH_TERM = ACT_MARGIN * TANHF_MEASURED`` (below);
* the output dropout (``drop_on`` 3) multiplies by exactly 0 or ``fp32(1 / (1 - p))``: ``e`` is scaled
  with it and one rounding ``U |y|`` added; a dropped element is exactly 0 (bound 0);
* accumulate adds the prior ``C`` (taken as exact): one rounding ``U |y|`` (none where the addend
  is an exact 0).

``tol = e + TINY``; C is fp32, there is no bf16 store.

``splits`` is what the launcher picks: ``dispatch`` transcribes ``fr_small_gemm`` / ``launch_rd``
(``fast_ok``, ``mixed_dtypes``, ``dma_ok``, ``rd_ok``, ``choose_tile``, ``choose_splits`` and the kchunk
rule: 64-granular for the LDS forms, 32-granular for the register-direct ones, 1 split when ``N %
4 != 0``) and returns the launch form with each desc's ``(splits, kchunk)``.  The transcription is
trusted for the bound -- a wrong count moves it by ``U S`` in K + 4 -- and it is what says which
form a case reaches (the tests assert the form they name).  The one place the upper count ``MAX_SPLITS``
= 16 is used instead is ``small_gemm_oracle(g, splits=None)``.  A consequence of the conditions,
recorded because the kernel comments suggest otherwise: ``fast_ok`` already requires M % 8 == 0
(N % 8 == 0) of a stored-transposed operand, so ``dma_ok`` never refuses a FAST launch, and a bf16 x
bf16 launch with ``a_mode`` 1 and M % 8 != 0 runs the GENERIC kernel, not the register queue.

``asum`` (a_mode 1): the kernels sum the STORED values of A -- raw fp32 in the register-queue forms
(``as_`` adds the raw words), the bf16 values in the ring (a ones-MFMA) -- K adds and ``splits - 1``
for the partials: ``tol = (K + splits + 2) U sum_k |A|`` around the fp64 sum of the stored values.  A
sum taken from the bf16-rounded copy of an fp32 A is off by up to ``2^-9 sum |A|`` and fails.

``colsum_f32``: rows are added per lane, then 4 waves, then the chunks: < M adds per column,
``tol = (M + 2) U sum_i |x_ij|`` (+ one rounding of the result when accumulating).

``wgrad`` (dW = dy^T x, bf16 operands, fp32 out): M products per element added by the MFMA,
``S_w - 1`` adds of the split partials: ``tol = (M + S_w + 2) U |dy|^T |x|``.  ``wgrad_plan`` transcribes
``plan()`` of gemm_wgrad.hip as a function of the CU count (S, mchunk, 32-row steps per split, rows
of the last split, scratch floats).  ``fr_wgrad_bf16(accumulate = 1)`` is reachable through no
binding (``wgrad`` passes 0) and is not tested.

The ``tanhf`` term is the one number not derived here.  It was measured on the MI355X through the
kernel itself (tests/test_sgemm_oracle_gpu.py ``test_tanhf_term``): K = 8, a one-hot A, ``B[n, :] =
bf16(x_n)`` and ``bias[n] = x_n - bf16(x_n)`` (both exact, and so is their fp32 sum: the pre-activation
IS x_n), x over ``TANH_GRID`` on [-12, 12] plus ``TANH_EDGES``, against ``torch.tanh`` in fp64.  The worst
``|got - tanh(x)| / (U max(|tanh x|, TANH_TINY))`` is recorded as ``TANHF_MEASURED``; the bound uses
``ACT_MARGIN = 2`` times that (gemm_oracle's margin, for the same reason: the grid is a sample).  The
GPU test measures again and holds the measurement to the record.

Judging: ``gemm_oracle.elem_ratio`` per element, worst ratio <= 1; a NaN / inf fails; a non-zero
where the oracle is exactly 0 fails.  ``describe`` names the worst element's 64 x 64 tile, wave
quadrant and 16 x 16 fragment.
"""
import math
from dataclasses import dataclass, replace

import torch

import gemm_oracle as go
from fedrec_with_pytorchdistributed_amd.ops import Gemm
from fedrec_with_pytorchdistributed_amd.ops import reference as ref

U = go.U
UB = go.UB
TINY = go.TINY
ACT_MARGIN = go.ACT_MARGIN
NOMINAL_CUS = go.NOMINAL_CUS
MAX_SPLITS = 16
TANH_TINY = 2.0 ** -100
TANH_GRID = (-12.0, 12.0, (1 << 18) + 1)
TANH_EDGES = (0.0, -0.0, 2.0 ** -60, -2.0 ** -60, 1e-8, -1e-8, 12.5, -12.5, 20.0, -20.0, 40.0, -40.0, 88.0, -88.0,
              89.0, -89.0, 100.0, -100.0, 1e4, -1e4, 1e19, -1e19, 1e30, -1e30)
TANHF_MEASURED = 2.35  # units of U max(|y|, TANH_TINY); measured on the MI355X: 2.3485 at x = -0.63885498
TANH_TERM = ACT_MARGIN * TANHF_MEASURED
SENTINEL = -6.0221e23  # what padded_c fills with (compared bitwise)
POISON = 997.0  # what fills an operand's row padding: finite, so a harmless 0 * pad stays 0


# ------------------------------------------------------------------------------------ operands
def _flat(t: torch.Tensor) -> torch.Tensor:
    n = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()
    return torch.as_strided(t, (n,), (1,), t.storage_offset())


def rows(t, n_rows: int, n_cols: int, ld: int, gidx=None) -> torch.Tensor:
    """``[n_rows, n_cols]`` of the stored matrix at ``t``'s first element, row r at ``r * ld`` (row
    ``gidx[r]`` when gathered), in the stored dtype."""
    r = gidx.long()[:n_rows] if gidx is not None else torch.arange(n_rows, device=t.device)
    idx = r[:, None] * ld + torch.arange(n_cols, device=t.device)[None, :]
    return _flat(t)[idx.reshape(-1)].view(n_rows, n_cols)


def drop_scale(g: Gemm, n_rows: int, n_cols: int, dev_off: int = 0, device="cpu") -> torch.Tensor:
    """fp32 ``[n_rows, n_cols]``: 0 or fp32(1 / (1 - p)) of logical element ``r * drop_ld + c``."""
    idx = torch.arange(n_rows)[:, None] * g.drop_ld + torch.arange(n_cols)[None, :]
    return ref.dropout_scale(idx, g.pdrop, g.seed, g.offset + int(dev_off)).to(device)


def stored_a(g: Gemm) -> torch.Tensor:
    """The logical A [M, K] in its stored dtype (what ``asum`` adds), before dropout / rounding."""
    if g.a_mode == 0:
        return rows(g.A, g.M, g.K, g.lda, g.gidx if g.gather_on == 1 else None)
    return rows(g.A, g.K, g.M, g.lda).t()


def operand(g: Gemm, dev_off: int = 0):
    """``(A [M, K], B [N, K])`` bf16: the values the MFMAs multiply."""
    A = stored_a(g)
    if g.drop_on == 1:
        A = A * drop_scale(g, g.M, g.K, dev_off, A.device)  # the fp32 product, then one rounding
    if g.b_mode == 0:
        B = rows(g.B, g.N, g.K, g.ldb)
    elif g.kseg:
        blocks = (g.B, *g.bseg)
        B = torch.cat([rows(blocks[i], min(g.kseg, g.K - i * g.kseg), g.N, g.ldb)
                       for i in range(3) if i * g.kseg < g.K]).t()
    else:
        Bk = rows(g.B, g.K, g.N, g.ldb, g.gidx if g.gather_on == 2 else None)  # [K, N]
        if g.drop_on == 2:
            Bk = Bk * drop_scale(g, g.K, g.N, dev_off, Bk.device)
        B = Bk.t()
    return A.to(torch.bfloat16), B.to(torch.bfloat16)


# ------------------------------------------------------------------------------------ the launcher
def choose_splits(tiles: int, K: int, dma: bool) -> int:
    mink = 1024 if dma else 384
    if K < 512 or tiles <= 0:
        return 1
    want = (512 + tiles - 1) // tiles
    return max(1, min(want, K // mink, MAX_SPLITS))


def kchunk_rule(t: int, N: int, K: int, dma: bool, gran: int):
    """``(splits, kchunk)`` of a desc with ``t`` output tiles (gran 64: LDS forms, 32: register-direct)."""
    s = choose_splits(t, K, dma)
    kchunk = ((K + s - 1) // s + gran - 1) // gran * gran if s > 1 else K
    if s > 1:
        s = (K + kchunk - 1) // kchunk
    if s > 1 and N % 4 != 0:  # the reduction takes 4 columns per lane
        s, kchunk = 1, K
    return s, kchunk


def _aligned16(t) -> bool:
    return (t.storage_offset() * t.element_size()) % 16 == 0  # allocations are 16-byte aligned


def _bf(t) -> bool:
    return t.dtype == torch.bfloat16


def fast_ok(gs) -> bool:
    for d in gs:
        ea, eb = (8 if _bf(d.A) else 4), (8 if _bf(d.B) else 4)
        ca = d.K if d.a_mode == 0 else d.M
        cb = d.K if d.b_mode == 0 else d.N
        if not (ca % 8 == 0 and cb % 8 == 0 and d.K % 8 == 0 and d.lda % ea == 0 and d.ldb % eb == 0
                and _aligned16(d.A) and _aligned16(d.B) and d.kseg == 0 and d.gather_on == 0
                and d.drop_on not in (1, 2)):
            return False
    return True


def dispatch(gs, tile: int = 0):
    """``(form, [(splits, kchunk)], blocks)`` of ``ops.small_gemm(*gs, tile=tile)``: the transcription of
    ``fr_small_gemm``.  Forms: ``generic``, ``mixed``, ``regq`` (FAST 64 x 64, TRI images, two LDS
    buffers), ``tile2`` / ``tile3`` / ``tile4``, ``ring2`` / ``ring3`` / ``ring4``, ``rd<f><P>`` (+ ``s`` with the
    split digit, + ``a32`` with an fp32 A), ``refused``."""
    fast = fast_ok(gs)
    mixed = any(_bf(d.A) != _bf(gs[0].A) or _bf(d.B) != _bf(gs[0].B) for d in gs)
    if tile >= 1000:  # (tile 0: the automatic register-direct choice is off by default)
        rd = all(_bf(d.A) == _bf(gs[0].A) and _bf(d.B) and d.a_mode == 0 and d.b_mode == 0 and d.asum is None
                 and d.drop_on not in (1, 2) and not d.gather_on and not d.kseg for d in gs)
        if fast and rd:
            allow, f, P = (tile // 100) % 10 != 0, (tile // 10) % 10, tile % 10
            if P < 2 or P > 4 or f > 3:
                return "refused", [], 0
            tm, tn = 32 * (2, 4, 2, 4)[f], 32 * (2, 4, 4, 2)[f]
            sk, blocks = [], 0
            for d in gs:
                t = -(-d.M // tm) * -(-d.N // tn)
                sk.append(kchunk_rule(t, d.N, d.K, True, 32) if allow else (1, d.K))
                blocks += t * sk[-1][0]
            return "rd%d%d%s%s" % (f, P, "s" if allow else "", "" if _bf(gs[0].A) else "a32"), sk, blocks
        tile = 0
    regq = tile == 5
    stg = tile - 4 if 6 <= tile <= 8 else (2 if tile == 9 else 0)
    nosplit = tile == 9
    if 1 <= tile <= 4:
        v = tile
    elif regq or stg:
        v = 1
    else:
        v = 4 if sum(-(-d.M // 64) * -(-d.N // 64) for d in gs) >= 2048 else 1
    if not fast or mixed:
        v = 1
    tm, tn = (128 if v in (2, 4) else 64), (128 if v in (3, 4) else 64)
    dt3 = _bf(gs[0].A) and _bf(gs[0].B)
    dma_ok = all(not ((d.a_mode == 1 and d.M % 8) or (d.b_mode == 1 and d.N % 8)) for d in gs)
    dma_shape = fast and not mixed and v == 1 and dt3 and dma_ok
    dma = dma_shape and not regq
    sk, blocks = [], 0
    for d in gs:
        t = -(-d.M // tm) * -(-d.N // tn)
        sk.append((1, d.K) if nosplit else kchunk_rule(t, d.N, d.K, dma_shape, 64))
        blocks += t * sk[-1][0]
    form = ("generic" if not fast else "mixed" if mixed else "ring%d" % (stg or 2) if dma else "regq" if v == 1
            else "tile%d" % v)
    return form, sk, blocks


def wgrad_plan(M: int, N: int, K: int, cus: int) -> dict:
    """``plan()`` of gemm_wgrad.hip: 256 x 256 output tiles, 32-row stages, S splits of ``mchunk`` rows."""
    ntiles = -(-N // 256) * -(-K // 256)
    smax = (M + 511) // 512
    s = max(1, min(cus // ntiles, smax))
    mchunk = (-(-M // s) + 31) // 32 * 32
    S = max(1, -(-M // mchunk)) if mchunk else 1
    last = M - (S - 1) * mchunk
    return dict(S=S, mchunk=mchunk, steps=-(-min(M, mchunk) // 32), last_rows=last, last_steps=-(-last // 32),
                blocks=S * ntiles, scratch=0 if S == 1 else S * N * K)


def shortest_last_split_m(N: int, K: int, cus: int, lo: int = 513, hi: int = 1600) -> int:
    """The M in [lo, hi] whose last split is the shortest (ties: the smallest M)."""
    return min(range(lo, hi + 1), key=lambda M: (wgrad_plan(M, N, K, cus)["last_rows"], M))


# ------------------------------------------------------------------------------------ oracles
def small_gemm_oracle(g: Gemm, splits=1, dev_off: int = 0):
    """``(ref, tol)`` fp64 [M, N] of the new ``C[:M, :N]`` (``g.C`` is read for ``accumulate``: call
    before the launch).  ``splits=None``: the upper count MAX_SPLITS."""
    splits = MAX_SPLITS if splits is None else splits
    A, B = operand(g, dev_off)
    Ad, Bd = A.double(), B.double()
    y = g.alpha * (Ad @ Bd.t())
    e = (g.K + splits + 2) * U * abs(g.alpha) * (Ad.abs() @ Bd.abs().t())  # K MFMA adds, splits partials, alpha
    if g.bias is not None:
        b = g.bias.double()[:g.N]
        y = y + b
        e = e + U * b.abs()  # the bias add
    if g.act == 1:
        y = torch.tanh(y)  # e carried by |tanh'| <= 1
        e = e + TANH_TERM * U * y.abs().clamp(min=TANH_TINY)  # tanhf
    dropped = None
    if g.drop_on == 3:
        z = drop_scale(g, g.M, g.N, dev_off, y.device).double()
        dropped = z == 0
        y = y * z
        e = e * z + U * y.abs()  # v *= scale
    if g.accumulate:
        c = rows(g.C, g.M, g.N, g.ldc).double()
        y = y + c
        r = U * y.abs()  # v += C
        e = e + (r if dropped is None else torch.where(dropped, torch.zeros_like(r), r))  # 0 + c is exact
    tol = e + TINY
    if dropped is not None and not g.accumulate:
        tol = torch.where(dropped, torch.zeros_like(tol), tol)  # a dropped element is exactly 0
    return y, tol


def asum_oracle(g: Gemm, splits: int = 1):
    """``(ref, tol)`` fp64 [M]: the sums over k of the STORED A values."""
    a = stored_a(g).double()
    return a.sum(1), (g.K + splits + 2) * U * a.abs().sum(1) + TINY


def colsum_oracle(X, M: int, N: int, ld: int, prior=None):
    """``(ref, tol)`` fp64 [N] of ``colsum_f32`` (``prior``: the out values when accumulating)."""
    x = rows(X, M, N, ld).double() if M > 0 else torch.zeros(0, N, dtype=torch.float64, device=X.device)
    y, tol = x.sum(0), (M + 2) * U * x.abs().sum(0)
    if prior is not None:
        y = y + prior.double()[:N]
        tol = tol + U * y.abs()
    return y, tol + TINY


def wgrad_oracle(dy, x, S: int = 1):
    """``(ref, tol)`` fp64 [N, K] of ``wgrad(dy [M, N], x [M, K])`` run in ``S`` splits."""
    d, xx = dy.double(), x.double()
    return d.t() @ xx, (dy.shape[0] + S + 2) * U * (d.abs().t() @ xx.abs()) + TINY


# ------------------------------------------------------------------------------------ judging
def describe(cand, ref_, tol) -> str:
    r = go.elem_ratio(cand, ref_, tol)
    if r.dim() == 1:
        j = int(r.argmax())
        return ("worst index %d (64-tile %d): ratio %.4g (got %.9g, want %.9g, bound %.3g); %d of %d above 1"
                % (j, j // 64, float(r[j]), float(cand[j]), float(ref_[j]), float(tol[j]), int((r > 1).sum()),
                   r.numel()))
    N = r.shape[1]
    k = int(r.argmax())
    i, j = k // N, k % N
    return ("worst (row %d, column %d) = 64 x 64 tile (%d, %d), wave quadrant (%d, %d), 16 x 16 fragment (%d, %d) of "
            "the tile: ratio %.4g (got %.9g, want %.9g, bound %.3g); %d of %d elements above 1"
            % (i, j, i // 64, j // 64, i % 64 // 32, j % 64 // 32, i % 64 // 16, j % 64 // 16, float(r[i, j]),
               float(cand[i, j]), float(ref_[i, j]), float(tol[i, j]), int((r > 1).sum()), r.numel()))


def worst_ratio(cand, ref_, tol) -> float:
    r = go.elem_ratio(cand, ref_, tol)
    return float(r.max()) if r.numel() else 0.0


def check(cand, ref_, tol, what: str = "") -> float:
    """Assert every element within its bound and no non-zero where the oracle is exactly 0."""
    w = worst_ratio(cand, ref_, tol)
    if not w <= 1.0:
        raise AssertionError("%s: %s" % (what, describe(cand, ref_, tol)))
    stray = (ref_ == 0) & (cand.double() != 0)
    if bool(stray.any()):
        raise AssertionError("%s: %d non-zero elements where the oracle is exactly 0" % (what, int(stray.sum())))
    return w


# ------------------------------------------------------------------------------------ builders
def _uniform(gen, *shape):
    return torch.rand(*shape, generator=gen) * 2 - 1


def _store(logical: torch.Tensor, mode: int, bf16: bool, pad: int, off: int):
    """The logical [R, K] matrix stored row-major (mode 0) or transposed (mode 1) with ``pad`` POISON
    elements after each row and ``off`` elements before the first -> (tensor view at the base, ld)."""
    m = logical if mode == 0 else logical.t()
    r, c = m.shape
    ld = c + pad
    buf = torch.full((off + max(r, 1) * ld,), POISON, dtype=torch.bfloat16 if bf16 else torch.float32)
    if r:
        buf[off:off + r * ld].view(r, ld)[:, :c] = m.to(buf.dtype)
    return buf[off:], ld


def make_gidx(n: int, n_src: int, gen) -> torch.Tensor:
    """int32 [n] into ``n_src`` rows: index 0 first, the largest last, duplicates in between."""
    g = torch.randint(0, n_src, (n,), generator=gen, dtype=torch.int64)
    if n > 2:
        g[n // 2] = g[n // 2 - 1]  # an adjacent duplicate
    g[0] = 0
    g[-1] = n_src - 1
    return g.to(torch.int32)


def make_operands(M, N, K, a_mode=0, b_mode=0, a_dtype=torch.bfloat16, b_dtype=torch.bfloat16, lda_pad=0, ldb_pad=0,
                  seed=0, regime="", a_off=0, b_off=0):
    """``(A, lda, B, ldb)`` on the CPU.  Logical A [M, K] uniform in +-1, B [N, K] in +-1 / sqrt(K)
    (a product sum has standard deviation 1/3), rounded to the stored dtype.  Regimes: ``col30``: k
    column 1 of A and the last k column of B are 30 x the rest; ``zero``: an all-zero A row (M // 2) and
    B row (N - 1); ``exact``: the position-coded integers of ``exact_expected``."""
    gen = torch.Generator().manual_seed(7919 * seed + 104729 * M + 1299709 * N + 31 * K + 2 * a_mode + b_mode)
    if regime == "exact":
        Al = torch.zeros(M, K)
        Al[torch.arange(M), (5 * torch.arange(M) + 3) % K] = 1.0
        Bl = ((37 * torch.arange(N)[:, None] + 11 * torch.arange(K)[None, :]) % 251 - 125).float()
    else:
        Al = _uniform(gen, M, K)
        Bl = _uniform(gen, N, K) / math.sqrt(K)
        if regime == "col30":
            Al[:, min(1, K - 1)] *= 30.0
            Bl[:, K - 1] *= 30.0
        elif regime == "zero":
            Al[M // 2] = 0.0
            Bl[N - 1] = 0.0
    A, lda = _store(Al, a_mode, a_dtype == torch.bfloat16, lda_pad, a_off)
    B, ldb = _store(Bl, b_mode, b_dtype == torch.bfloat16, ldb_pad, b_off)
    return A, lda, B, ldb


def exact_expected(M, N, K, bias: bool, accumulate: bool) -> torch.Tensor:
    """fp32 [M, N] integers of magnitude <= 255 the ``exact`` regime must give, bit for bit."""
    i, j = torch.arange(M), torch.arange(N)
    want = (37 * j[None, :] + 11 * ((5 * i + 3) % K)[:, None]) % 251 - 125
    if bias:
        want = want + exact_bias(N).long()[None, :]
    if accumulate:
        want = want + exact_prior(M, N).long()
    assert M == 0 or N == 0 or int(want.abs().max()) <= 255
    return want.float()


def exact_bias(N):
    return ((torch.arange(N) * 7) % 121 - 60).float()


def exact_prior(M, N):
    return ((torch.arange(M)[:, None] * 3 + torch.arange(N)[None, :] * 5) % 141 - 70).float()


def padded_c(M, N, ldc, guard_rows=2, base_offset=0, prior=None, device="cpu"):
    """``(flat, C)``: a SENTINEL-filled buffer and the view at C's first element -- ``guard_rows`` rows
    (rounded up to 16 bytes) before it, then ``base_offset`` floats, M rows of ``ldc``, and the guard
    rows after.  ``prior`` [M, N] is copied into ``C[:M, :N]`` (accumulate)."""
    lead = (guard_rows * ldc + 3) // 4 * 4 + base_offset
    flat = torch.full((lead + (M + guard_rows) * ldc,), SENTINEL, dtype=torch.float32, device=device)
    C = flat[lead:]
    if prior is not None and M:
        C[:M * ldc].view(M, ldc)[:, :N] = prior.to(device)
    return flat, C


def c_view(C, M, N, ldc):
    return C[:M * ldc].view(M, ldc)[:, :N]


def check_padding(flat, C, M, N, ldc, what="") -> None:
    """Everything of ``flat`` outside ``C[:M, :N]`` is still bitwise the sentinel."""
    keep = torch.ones(flat.numel(), dtype=torch.bool, device=flat.device)
    lead = C.storage_offset() - flat.storage_offset()
    if M and N:
        keep[lead:lead + M * ldc].view(M, ldc)[:, :N] = False
    s = torch.tensor(SENTINEL, dtype=torch.float32, device=flat.device).view(torch.int32)
    bad = (flat.view(torch.int32) != s) & keep
    if bool(bad.any()):
        k = int(bad.nonzero()[0]) - lead
        raise AssertionError("%s: %d floats outside C[:M, :N] written; the first at row %d, column %d (ldc %d)"
                             % (what, int(bad.sum()), k // ldc, k % ldc, ldc))


# ------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Spec:
    """One GEMM of a launch, by value (tests build it with ``build`` on the CPU and move it)."""
    M: int
    N: int
    K: int
    a_mode: int = 0
    b_mode: int = 0
    a_bf16: bool = True
    b_bf16: bool = True
    lda_pad: int = 8
    ldb_pad: int = 0
    a_off: int = 0
    b_off: int = 0
    alpha: float = 1.0
    bias: bool = False
    wide: bool = False  # the bias spans +-20: tanh saturates both ways
    act: int = 0
    accumulate: bool = False
    drop_on: int = 0
    pdrop: float = 0.2
    drop_extra: int = 16  # drop_ld = round_up(row length, 16) + drop_extra
    gather: int = 0
    kseg: int = 0
    asum: bool = False
    regime: str = ""
    seed: int = 0


@dataclass
class Built:
    spec: Spec
    A: torch.Tensor
    B: torch.Tensor
    lda: int
    ldb: int
    bias: torch.Tensor
    gidx: torch.Tensor
    bseg: tuple
    prior: torch.Tensor
    drop_ld: int

    def to(self, device):
        mv = lambda t: None if t is None else t.to(device)  # noqa: E731
        return Built(self.spec, mv(self.A), mv(self.B), self.lda, self.ldb, mv(self.bias), mv(self.gidx),
                     tuple(mv(t) for t in self.bseg), mv(self.prior), self.drop_ld)

    def gemm(self, C, ldc, asum=None) -> Gemm:
        s = self.spec
        return Gemm(self.A, self.B, C, s.M, s.N, s.K, self.lda, self.ldb, ldc, a_mode=s.a_mode, b_mode=s.b_mode,
                    act=s.act, accumulate=s.accumulate, alpha=s.alpha, bias=self.bias, gidx=self.gidx,
                    gather_on=s.gather, pdrop=s.pdrop if s.drop_on else 0.0, drop_on=s.drop_on, drop_ld=self.drop_ld,
                    seed=11 + s.seed, offset=3 + 2 * s.seed, bseg=self.bseg, kseg=s.kseg, asum=asum)


def build(s: Spec) -> Built:
    """The tensors of a Spec, drawn on the CPU (the same values wherever they are used)."""
    gen = torch.Generator().manual_seed(15485863 * s.seed + 611953 * s.M + 7 * s.N + 13 * s.K + 1)
    f32, b16 = torch.float32, torch.bfloat16
    A, lda, B, ldb = make_operands(s.M, s.N, s.K, s.a_mode, s.b_mode, b16 if s.a_bf16 else f32,
                                   b16 if s.b_bf16 else f32, s.lda_pad, s.ldb_pad, s.seed, s.regime, s.a_off, s.b_off)
    gidx, bseg = None, ()
    if s.gather == 1:  # A rows from a table of n_src rows: row m of the logical A is table row gidx[m]
        assert s.a_mode == 0
        n_src = max(4, s.M // 2 + 3)
        gidx = make_gidx(s.M, n_src, gen)
        tab = _uniform(gen, n_src, s.K)
        A, lda = _store(tab, 0, s.a_bf16, s.lda_pad, s.a_off)
    elif s.gather == 2:
        assert s.b_mode == 1 and not s.kseg
        n_src = max(4, s.K // 2 + 3)
        gidx = make_gidx(s.K, n_src, gen)
        tab = _uniform(gen, n_src, s.N) / math.sqrt(s.K)
        B, ldb = _store(tab, 0, s.b_bf16, s.ldb_pad, s.b_off)  # stored [rows, N] = the K-major layout
    if s.kseg:  # B's K rows split over three separately stored blocks of kseg rows
        assert s.b_mode == 1 and s.K <= 3 * s.kseg
        full = rows(B, s.K, s.N, ldb)
        blocks = []
        for i in range(3):
            blk = torch.full((s.kseg, ldb), POISON, dtype=B.dtype)
            n = max(0, min(s.kseg, s.K - i * s.kseg))
            blk[:n, :s.N] = full[i * s.kseg:i * s.kseg + n]
            blocks.append(blk)
        B, bseg = blocks[0], (blocks[1], blocks[2])
    bias = None
    if s.regime == "exact":
        bias = exact_bias(s.N) if s.bias else None
        prior = exact_prior(s.M, s.N) if s.accumulate else None
    else:
        if s.bias:
            bias = (torch.randperm(s.N, generator=gen).float() / max(s.N - 1, 1) * 40.0 - 20.0) if s.wide \
                else torch.randn(s.N, generator=gen)
        prior = torch.randn(s.M, s.N, generator=gen) if s.accumulate else None
    row_len = {0: 0, 1: s.K, 2: s.N, 3: s.N}[s.drop_on]
    drop_ld = (row_len + 15) // 16 * 16 + s.drop_extra if s.drop_on else 0
    return Built(s, A, B, lda, ldb, bias, gidx, bseg, prior, drop_ld)


# Each list below is built from constants alone, so tests/test_sgemm_oracle_cpu.py runs its
# rounding model over the input sets of tests/test_sgemm_oracle_gpu.py.  A case: (name, [Spec], tile,
# the form ``dispatch`` must report[, dict(splits=[per desc] | blocks=the launch's tile count)]).
PAIRS = [(1, 129), (15, 64), (16, 17), (17, 16), (63, 65), (64, 1), (65, 63), (127, 128), (128, 15), (129, 127)]
K_LDS = [8, 56, 64, 72, 128, 192, 200, 264]  # 1, 1, 1, 2, 2, 3, 4, 5 k-tiles of 64: every ring stage count wraps
K_RD = [8, 40, 72, 104, 136, 168, 200, 232, 264, 64, 128]  # 1 .. 9 k-steps of 32 (2 P + 1 for P = 4); 8 / 40 / 72:
#                                                            a last k-step with lanes past kend
RD_CODES = [1002, 1003, 1004, 1012, 1013, 1023, 1033, 1103]
LDS_FORMS = {1: "regq", 2: "tile2", 3: "tile3", 4: "tile4", 5: "regq", 0: "ring2", 7: "ring3", 8: "ring4", 9: "ring2"}


def rd_form(code: int, a_bf16: bool = True) -> str:
    return "rd%d%d%s%s" % ((code // 10) % 10, code % 10, "s" if (code // 100) % 10 else "", "" if a_bf16 else "a32")


def edge_cases(tile: int):
    """Row / column / k edges of one tile code.  Codes 1-4 take an fp32 A (a bf16 x bf16 launch under
    tile 1 is the ring's); 5, the ring and the register-direct codes bf16 x bf16; every third
    register-direct case an fp32 A."""
    ks = K_RD if tile >= 1000 else K_LDS
    out = []
    for i in range(max(len(PAIRS), len(ks))):
        M, N = PAIRS[(i + tile) % len(PAIRS)]
        K = ks[i % len(ks)]
        a_bf16 = (i % 3 != 2) if tile >= 1000 else tile not in (1, 2, 3, 4)
        s = Spec(M, N, K, a_bf16=a_bf16, bias=True, seed=i)
        form = rd_form(tile, a_bf16) if tile >= 1000 else LDS_FORMS[tile]
        out.append(("edge tile %d %dx%dx%d" % (tile, M, N, K), [s], tile, form))
    return out


LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]


def quadrant_cases(tile: int):
    """The four dtype quadrants x the four layouts at M, N multiples of 8 and not of 16."""
    out = []
    for (am, bm) in LAYOUTS:
        for ab in (False, True):
            for bb in (False, True):
                for (M, N, K) in ((72, 136, 200), (136, 72, 72)):
                    s = Spec(M, N, K, a_mode=am, b_mode=bm, a_bf16=ab, b_bf16=bb, ldb_pad=8, bias=True,
                             seed=am + 2 * bm)
                    if tile in (2, 3, 4):
                        form = "tile%d" % tile
                    else:
                        form = "ring2" if (ab and bb and tile != 5) else "regq"
                    out.append(("quadrant tile %d a%d b%d %s x %s %dx%dx%d" % (tile, am, bm, "bf16" if ab else "fp32",
                                                                                 "bf16" if bb else "fp32", M, N, K),
                                [s], tile, form))
    return out


def generic_cases():
    S = Spec
    return [
        ("generic K 131 odd lda", [S(77, 45, 131, a_bf16=False, b_bf16=False, lda_pad=2, b_mode=1, bias=True)], 0,
         "generic"),
        ("generic K 5", [S(17, 33, 5, a_bf16=False, b_bf16=False, lda_pad=0, alpha=0.5)], 0, "generic"),
        ("generic bf16 at an odd offset", [S(77, 45, 131, a_off=1, lda_pad=0, b_mode=1, b_off=3)], 0, "generic"),
        ("generic a_mode 1 M % 8 != 0 bf16 x bf16", [S(68, 40, 72, a_mode=1, b_mode=1, lda_pad=0, asum=True)], 0,
         "generic"),
        ("generic gather A", [S(70, 40, 200, a_bf16=False, gather=1, bias=True)], 0, "generic"),
        ("generic gather A bf16", [S(65, 64, 72, gather=1)], 0, "generic"),
        ("generic gather B", [S(40, 72, 130, a_mode=1, b_mode=1, b_bf16=False, lda_pad=0, gather=2)], 0, "generic"),
        ("generic kseg two segments", [S(66, 48, 144, b_mode=1, kseg=72, accumulate=True)], 0, "generic"),
        ("generic kseg three segments", [S(66, 48, 200, b_mode=1, kseg=72, b_bf16=False)], 0, "generic"),
        ("generic K = 2 kseg + 8", [S(33, 40, 152, b_mode=1, kseg=72, a_bf16=False, drop_on=3)], 0, "generic"),
        ("generic drop_on 1", [S(70, 40, 200, a_bf16=False, drop_on=1, gather=1, bias=True, act=1)], 0, "generic"),
        ("generic drop_on 1 p 0.5", [S(3, 130, 72, a_bf16=False, drop_on=1, pdrop=0.5)], 0, "generic"),
        ("generic drop_on 2", [S(40, 72, 130, a_mode=1, b_mode=1, b_bf16=False, lda_pad=0, drop_on=2, gather=2)], 0,
         "generic"),
        ("generic col30", [S(70, 41, 131, a_bf16=False, regime="col30", bias=True)], 0, "generic"),
        ("generic zero rows", [S(70, 41, 131, b_bf16=False, regime="zero")], 0, "generic"),
    ]


EPI = [dict(alpha=0.5), dict(bias=True), dict(bias=True, wide=True, act=1), dict(drop_on=3), dict(accumulate=True),
       dict(alpha=0.5, bias=True, wide=True, act=1, drop_on=3, accumulate=True)]
# (tile, form, fp32 A?, K): one per form that has an epilogue of its own, and splitk_reduce behind three
EPI_FORMS = [(1, "regq", True, 200), (4, "tile4", True, 200), (5, "regq", False, 72), (0, "ring2", False, 200),
             (1003, "rd03", False, 200), (1033, "rd33a32", True, 72), (0, "generic", False, 68),
             (1, "regq", True, 800), (0, "ring2", False, 2048), (1103, "rd03s", False, 2056)]


def epilogue_cases():
    out = []
    for (tile, form, a32, K) in EPI_FORMS:
        for i, kw in enumerate(EPI):
            if K >= 800:  # splitk_reduce behind it: N % 4 == 0 (133: the split is declined)
                ns = (132, 136, 133) if i == len(EPI) - 1 else (132,)
            else:
                ns = (132, 133, 134, 135) if i == len(EPI) - 1 else (132 + (i + 1) % 4,)
            for N in ns:
                s = Spec(70, N, K, a_bf16=not a32, seed=i, **kw)
                out.append(("epilogue tile %d K %d N %d %s" % (tile, K, N, sorted(kw)), [s], tile, form))
    return out


def split_cases():
    """(name, [Spec], tile, form, dict(splits=the expected split counts)).  Register-queue forms split at 384 per
    split, the
    ring and the register-direct form at 1,024."""
    S = Spec
    out = []
    for tile, form in ((1, "regq"), (2, "tile2"), (3, "tile3"), (4, "tile4")):
        for K, sp in ((768, 2), (800, 2), (1200, 3)):
            out.append(("split tile %d K %d" % (tile, K), [S(70, 132, K, a_bf16=False, bias=True)], tile, form,
                        dict(splits=[sp])))
    for K, sp in ((2048, 2), (2056, 2), (3200, 3)):
        out.append(("split ring K %d" % K, [S(130, 64, K, accumulate=True)], 0, "ring2", dict(splits=[sp])))
        out.append(("split ring3 K %d" % K, [S(70, 132, K)], 7, "ring3", dict(splits=[sp])))
        out.append(("split regq bf16 K %d" % K, [S(130, 64, K, accumulate=True)], 5, "regq", dict(splits=[sp])))
        out.append(("split rd K %d" % K, [S(70, 132, K, bias=True)], 1103, "rd03s", dict(splits=[sp])))
        out.append(("ring tile 9 never splits K %d" % K, [S(64, 64, K)], 9, "ring2", dict(splits=[1])))
        out.append(("rd without the split digit K %d" % K, [S(64, 68, K)], 1003, "rd03", dict(splits=[1])))
    out += [
        ("split asum fp32 A", [S(72, 136, 800, a_mode=1, b_mode=1, a_bf16=False, lda_pad=0, asum=True)], 1, "regq",
         dict(splits=[2])),
        ("split asum bf16 A regq", [S(72, 136, 2048, a_mode=1, b_mode=1, lda_pad=0, asum=True)], 5, "regq",
         dict(splits=[2])),
        ("split asum ring", [S(136, 72, 3200, a_mode=1, b_mode=1, lda_pad=8, ldb_pad=8, asum=True, accumulate=True)], 0,
         "ring2", dict(splits=[3])),
        ("split asum mixed", [S(72, 136, 800, a_mode=1, b_mode=1, a_bf16=False, lda_pad=0, asum=True),
                              S(8, 72, 1200, a_mode=1, b_mode=1, lda_pad=0, asum=True, seed=1)], 0, "mixed",
         dict(splits=[2, 3])),
        ("split declined N 42", [S(70, 42, 800, a_bf16=False, bias=True)], 1, "regq", dict(splits=[1])),
        ("split col30", [S(70, 132, 800, a_bf16=False, regime="col30")], 1, "regq", dict(splits=[2])),
        ("split zero rows", [S(70, 132, 2048, regime="zero", bias=True)], 0, "ring2", dict(splits=[2])),
    ]
    return out


def grouped_cases():
    S = Spec
    six = [S(17, 33, 8, a_bf16=False, b_bf16=False, lda_pad=0, alpha=0.5), S(64, 64, 64, bias=True),
           S(0, 40, 72, a_bf16=False), S(65, 72, 200, a_mode=1, b_mode=1, b_bf16=False, lda_pad=3, ldb_pad=0, seed=2),
           S(72, 136, 800, a_mode=1, b_mode=1, a_bf16=False, lda_pad=0, asum=True, seed=3),
           S(3, 200, 1200, b_mode=1, accumulate=True, seed=4)]
    out = [("grouped six descs, M = 0 in the middle", six, 0, "generic")]
    six_fast = [replace(six[0], M=16), six[1], six[2], replace(six[3], M=72, lda_pad=0), six[4], six[5]]
    out.append(("grouped six descs mixed kernel", six_fast, 0, "mixed"))
    # tile totals 1, 7, 8, 9: the XCD remap with 0, 7, 0 and 1 blocks of remainder
    for total, shapes in ((1, [(64, 64)]), (7, [(65, 128), (64, 129)]), (8, [(128, 128), (65, 65)]),
                          (9, [(129, 129)])):
        for tile, form, a32 in ((1, "regq", True), (0, "ring2", False), (1002, "rd02", False)):
            gs = [S(M, N, 72, a_bf16=not a32, bias=True, seed=i) for i, (M, N) in enumerate(shapes)]
            out.append(("grouped %d tiles tile %d" % (total, tile), gs, tile, form, dict(blocks=total)))
    return out


def step_cases(BH: int = 130, D: int = 400, Qd: int = 200, nT: int = 130, Dt: int = 768, Qt: int = 200):
    """The training step's own descriptors (ops/functional.py) with BH = 130 history rows and n T =
    130 token rows in place of 3200 / ~78,000."""
    S = Spec
    D3 = 3 * D
    wg = [S(D3, D, BH, a_mode=1, b_mode=1, lda_pad=0, asum=True),
          S(Qd, D, BH, a_mode=1, b_mode=1, a_bf16=False, lda_pad=0, asum=True, seed=1),
          S(8, Qd, BH, a_mode=1, b_mode=1, a_bf16=False, b_bf16=False, lda_pad=0, asum=True, seed=2)]
    dgrad = S(BH, D, D3, b_mode=1, lda_pad=0, drop_on=3, drop_extra=0)
    # a weight gradient reduces over the rows: K = BH (n T) must be a multiple of 8 for the FAST
    # loads the step's 3200 rows get; 130 rows run the same descriptors through the generic kernel
    wmix = "mixed" if BH % 8 == 0 else "generic"
    tbwd = "regq" if nT % 8 == 0 else "generic"
    return [
        ("step QKV projection", [S(BH, D3, D, lda_pad=0, bias=True)], 0, "ring2"),
        ("step att_fc1 RD_ATT_FC1", [S(BH, Qd, D, lda_pad=0, bias=True, act=1)], 1002, "rd02"),
        ("step dctx RD_DCTX", [S(BH, D, Qd, lda_pad=0, accumulate=True)], 1004, "rd04"),
        ("step dctx K-major W1", [S(BH, D, Qd, lda_pad=0, b_mode=1, accumulate=True)], 0, "ring2"),
        ("step dgrad dropout epilogue", [dgrad], 0, "ring2"),
        ("step dgrad + weight gradients BH %d" % BH, [dgrad] + wg, 0, wmix),
        ("step weight-gradient group BH %d" % BH, wg, 0, wmix),
        ("step text fc forward", [S(nT, Qt, Dt, a_bf16=False, b_bf16=False, lda_pad=0, bias=True, act=1)], 0, "regq"),
        ("step text fc backward n T %d" % nT, [S(nT, Dt, Qt, a_bf16=False, b_bf16=False, b_mode=1, lda_pad=0),
                                   S(Qt, Dt, nT, a_mode=1, b_mode=1, a_bf16=False, b_bf16=False, lda_pad=0, asum=True)],
         0, tbwd),
    ]


def all_step_cases():
    """130 rows, and 136 for the descriptors that reduce over the rows (the
    weight-gradient groups and the text fc: entries 5 .. 8), which only then take the step's forms."""
    return step_cases() + step_cases(136, nT=136)[5:]


def exact_cases():
    """Position-coded integers under every tile code and layout: ``torch.equal``."""
    out = []
    for tile in (1, 2, 3, 4, 5, 0, 7, 8, 9):
        for (am, bm) in LAYOUTS:
            a32 = tile in (1, 2, 3, 4)
            s = Spec(136, 72, 200, a_mode=am, b_mode=bm, a_bf16=not a32, lda_pad=8, ldb_pad=8, bias=True,
                     accumulate=True,
                     regime="exact", asum=am == 1)
            form = LDS_FORMS[tile]
            out.append(("exact tile %d a%d b%d" % (tile, am, bm), [s], tile, form))
    for tile in RD_CODES:
        for a32 in (False, True):
            s = Spec(129, 67, 200, a_bf16=not a32, bias=True, accumulate=True, regime="exact")
            out.append(("exact tile %d%s" % (tile, " fp32 A" if a32 else ""), [s], tile, rd_form(tile, not a32)))
    out.append(("exact generic", [Spec(77, 45, 131, a_bf16=False, b_mode=1, lda_pad=2, bias=True, accumulate=True,
                                       regime="exact")], 0, "generic"))
    out.append(("exact split", [Spec(70, 132, 800, a_bf16=False, bias=True, accumulate=True, regime="exact")], 1,
                "regq"))
    out.append(("exact split ring", [Spec(72, 136, 2048, a_mode=1, b_mode=1, lda_pad=0, bias=True, accumulate=True,
                                          regime="exact", asum=True)], 0, "ring2"))
    return out


def all_gemm_cases():
    c = []
    for t in list(LDS_FORMS) + RD_CODES:
        c += edge_cases(t)
    for t in (1, 5, 2, 3, 4):
        c += quadrant_cases(t)
    return (c + generic_cases() + epilogue_cases() + split_cases() + grouped_cases() + all_step_cases()
            + exact_cases())


COLSUM_M = [1, 127, 128, 129, 513]
COLSUM_N = [1, 33, 64, 256, 260, 1203]
WGRAD_M_SMALL = [1, 31, 32, 33, 64, 65, 96, 97, 129]  # 1 .. 5 stages of one split: prologue, its fill, the ring wrap
WGRAD_M_SPLIT = [513, 577, 1025, 1537]
WGRAD_NK = [(8, 8), (248, 256), (256, 264), (264, 248), (520, 8), (8, 520), (264, 520)]


def wgrad_inputs(M, N, K, regime="", seed=0):
    """``(dy [M, N], x [M, K])`` bf16 on the CPU: dy uniform in +-1 / sqrt(M), x in +-1."""
    gen = torch.Generator().manual_seed(92821 * seed + 1009 * M + 31 * N + K)
    if regime == "exact":  # one-hot dy rows, integer x: every sum an integer below 2^24
        dy = torch.zeros(M, N)
        dy[torch.arange(M), (5 * torch.arange(M) + 3) % N] = 1.0
        x = ((37 * torch.arange(M)[:, None] + 11 * torch.arange(K)[None, :]) % 251 - 125).float()
    else:
        dy = _uniform(gen, M, N) / math.sqrt(max(M, 1))
        x = _uniform(gen, M, K)
        if regime == "col30":
            dy[:, N - 1] *= 30.0
            x[:, 0] *= 30.0
        elif regime == "zero" and M:
            dy[M // 2] = 0.0
            x[M - 1] = 0.0
            dy[:, N // 2] = 0.0
    return dy.to(torch.bfloat16), x.to(torch.bfloat16)
