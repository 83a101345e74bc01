"""An fp64 oracle of the bf16 GEMM family (csrc/gemm_bf16.hip) that carries, per output element,
a bound on what the HIP kernels may differ by (a plain helper module for the GEMM tests, not a
conftest; no GPU dependency: every function runs on the device of its arguments).

The operations (``A`` [M, K] and ``W`` [N, K] bf16, ``bias`` [N] fp32, ``R`` [M, N] bf16, all taken
as exact)::

    pre = A W^T + bias                                   S = |A| |W|^T + |bias|  >= |pre|
    act 0: y = pre + R        act 1: y = GELU(pre) + R    act 2: y = tanh(pre) + R
    act 3: y = (A W^T) GELU'(R)                           (R = the saved pre-activation z; no bias)
    linear_gelu_dual:  z = pre, h = GELU(pre)             linear_gelu_bwd: dz = act 3, colsum_j = sum_i dz_ij

GELU is the exact erf form, ``x Phi(x)``; ``GELU'(x) = Phi(x) + x phi(x)``.  ``S`` is the
cancellation-free magnitude: a rounding acts on a partial sum, which ``|pre|`` does not bound.

Roundings.  ``UB = 2^-8`` is the unit roundoff of bf16 and ``U = 2^-24`` of fp32, both round to
nearest even (the bf16 conversion is the compiler's ``v_cvt_pk_bf16_f32``: ``f2bf`` in common.h is a
plain cast).  Every count is first order; one spare unit per count covers the U^2 terms.  The
terms, in the order the kernels apply them (``linear_oracle`` has one line per term):

* accumulation: the products of two bf16 values are exact in fp32, the K of them are added by
  ``v_mfma_f32_16x16x32_bf16`` in fp32 (at most one rounding per product added, in any order) and
  the bias is one more add -- in the epilogue (variants 0, 6, 9) or as the accumulators' starting
  value (12, 13), the same count either way: ``e_acc = (K + 2) U S`` (K + 1 counted, 1 spare);
* the activation carries ``e_acc`` by its derivative, ``|GELU'| <= 1.13`` and ``|tanh'| <= 1``, and
  adds its own approximation error (below);
* act 3 multiplies by GELU'(z): ``|GELU'(z)| e_acc``, the approximation error of GELU' times
  ``|A W^T|``, and the rounding of the product, ``U |y|``;
* the residual add (act 0-2) rounds once: ``U |y|``;
* the bf16 store rounds the COMPUTED value: ``UB (|y| + e)`` with e the sum of the above.

So ``tol = UB |y| + (1 + UB) e + TINY``: away from cancellation the bound is the bf16 rounding
itself, which is what makes it sharp -- a lost K-step, a neighbour's bias or residual, or two
swapped column groups move an element by hundreds of bounds (tests/test_gemm_oracle_cpu.py).

Activation approximation terms.  The kernels use Abramowitz-Stegun 7.1.26 for erf with the
hardware ``v_rcp_f32`` / ``v_exp_f32``: ``gelu_pair`` (act 1, every kernel: ``act4`` takes the
packed form for the 128x128 kernel too -- the scalar ``gelu_erf`` / ``gelu_grad`` of gemm_bf16.hip
are reached by no launch), ``gelu_grad_pair`` (act 3), ``tanh_fast`` (act 2), and, in the
``linear_gelu_dual`` fallback, the scalar form ``erf_fast2`` of ``fr_gelu_bf16`` (layernorm.hip).
Each formula is transcribed below in fp32 (``*_f32``) and was compared with the exact function
in fp64 by ``measure_activation_eps`` over ``ACT_GRID``: 2^22 + 1 equally spaced points on
[-12, 12] rounded to fp32, plus the saturation points ``ACT_EDGES``.  The worst absolute error,
divided by max(1, |x|) for the GELU forms (their error is that of Phi, times x), is recorded in
``EPS_MEASURED``; the bound uses ``ACT_MARGIN = 2`` times that, because the transcription runs
correctly rounded fp32 ``1 / x`` and libm-grade ``exp2`` where the hardware instructions are ~1 ulp
approximations, and fuses no multiply-adds where the compiler does.  The CPU test measures
again and holds the record to it.  The comments in gemm_bf16.hip used to quote A&S's figure for erf in
exact arithmetic ("|error| <= 1.5e-7") and "~1e-7" for tanh; in fp32 the forms measure 1.7e-7 to
3.0e-7 (the polynomial's terms reach 1.45, so its own roundings are of the size of its error).

GELU has NO relative accuracy in the negative tail, in the kernels or in this bound: GELU(-5) is
about -1.4e-6 against an absolute term of ``2 EPS max(1, |x|)`` ~ 1e-6, so there the bound says
"about zero" and nothing about the digits.  The same holds for tanh near 0 (``1 - 2 / (1 + e)``
cancels) and for GELU' in its tails.  The outputs are consumed in sums with O(1) terms, which is
what an absolute bound fits.

``linear_gelu_dual``.  ``z = bf16(pre)`` and, in the fused kernels, ``h = bf16(GELU(pre in fp32))``:
the act 0 and act 1 bounds.  Below M = 4096 (and under variants 0 / 6) the op runs the GEMM and
then ``fr_gelu_bf16`` on the ROUNDED z: ``|z~ - pre| <= tol_z``, carried by 1.13, plus the scalar
form's approximation term -- a bound of its own (``tol_h_fallback``), about 2.1 x the fused one
for |pre| >~ 1; the fused bound is not loosened (mutant (g) of the CPU test is that fallback
judged by the fused bound).

``linear_gelu_bwd`` colsum.  ``gemm_nt_pp2_kernel`` adds the fp32 values ``v`` (before the bf16
rounding) of the rows m < M -- the clamped rows of the last row tile are excluded -- 8 per lane, then
16 lanes by ``__shfl_xor``, one partial per (row tile, wave row); the op sums the partials in fp32.
The reference is the fp64 sum of the bf16 ``dz`` the same launch stored, so per column::

    tol_j = M U sum_i |dz_ij|  +  UB / (1 - UB) sum_i |dz_ij|     (< M adds; |v - bf16(v)| <= UB |v|)

Judging.  ``ratio = |y - ref| / tol``; a candidate passes when the worst ratio is <= 1; a NaN / inf
candidate is an infinite ratio.  ``describe`` names the worst element's row, column, 256x256
tile, 128x64 wave block and 16x16 fragment.
"""
import math

import torch

UB = 2.0 ** -8
U = 2.0 ** -24
TINY = 1e-30
GELU_D_MAX = 1.13  # max |GELU'| = 1.1290, at x = sqrt(2)
NOMINAL_CUS = 256  # what the CPU tests size the walk cases by (the GPU tests ask the device)
PP2_MAXN = 3072
ACT = {"none": 0, "gelu": 1, "tanh": 2, "gelu_bwd": 3}

# ------------------------------------------------------------------ activations: fp32 transcriptions
_P = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)  # A&S 7.1.26
_H = (0.127414796, -0.142248368, 0.7107068705, -0.7265760135, 0.5307027145)  # the same, halved
_RSQRT2 = 0.70710678118654752
_LOG2E = 1.44269504088896341
_RSQRT2PI = 0.3989422804014327


def _f(c: float) -> torch.Tensor:
    return torch.tensor(c, dtype=torch.float32)  # a literal as the compiler rounds it


def _poly(t: torch.Tensor, c) -> torch.Tensor:
    return t * (_f(c[0]) + t * (_f(c[1]) + t * (_f(c[2]) + t * (_f(c[3]) + t * _f(c[4])))))


def _pair_core(x: torch.Tensor):
    z = x.abs() * _f(_RSQRT2)
    t = torch.reciprocal(z * _f(0.3275911) + _f(1.0))  # v_rcp_f32
    e = torch.exp2(z * z * _f(-_LOG2E))  # v_exp_f32
    return _poly(t, _H), e


def gelu_pair_f32(x: torch.Tensor) -> torch.Tensor:
    """``gelu_pair`` of gemm_bf16.hip."""
    P, e = _pair_core(x)
    r = x * (P * e)
    return torch.where(x >= 0, x - r, r)


def gelu_grad_pair_f32(x: torch.Tensor) -> torch.Tensor:
    """``gelu_grad_pair`` of gemm_bf16.hip."""
    P, e = _pair_core(x)
    h = P * e
    g = x * e * _f(_RSQRT2PI)
    return torch.where(x >= 0, _f(1.0) - h, h) + g


def _erf_fast_f32(x: torch.Tensor) -> torch.Tensor:
    ax = x.abs()
    t = torch.reciprocal(_f(1.0) + _f(0.3275911) * ax)  # __frcp_rn
    r = _f(1.0) - _poly(t, _P) * torch.exp(-ax * ax)  # __expf
    return torch.copysign(r, x)


def gelu_scalar_f32(x: torch.Tensor) -> torch.Tensor:
    """``gelu_erf`` of gemm_bf16.hip = the forward of ``gelu_kernel`` in layernorm.hip."""
    return _f(0.5) * x * (_f(1.0) + _erf_fast_f32(x * _f(_RSQRT2)))


def gelu_grad_scalar_f32(x: torch.Tensor) -> torch.Tensor:
    """``gelu_grad`` of gemm_bf16.hip."""
    cdf = _f(0.5) * (_f(1.0) + _erf_fast_f32(x * _f(_RSQRT2)))
    return cdf + x * _f(_RSQRT2PI) * torch.exp(_f(-0.5) * x * x)


def tanh_fast_f32(x: torch.Tensor) -> torch.Tensor:
    """``tanh_fast`` of gemm_bf16.hip (e = inf -> 1, e = 0 -> -1)."""
    e = torch.exp2(x * _f(2.8853900817779268))
    return _f(1.0) - _f(2.0) * torch.reciprocal(_f(1.0) + e)


# ------------------------------------------------------------------ activations: exact, fp64
def gelu_exact(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * torch.special.erfc(-x * _RSQRT2)  # erfc: the negative tail keeps its digits


def gelu_grad_exact(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * torch.special.erfc(-x * _RSQRT2) + x * _RSQRT2PI * torch.exp(-0.5 * x * x)


# The grid the EPS values were measured on, and the values: worst |transcription - exact|, over
# max(1, |x|) for the four GELU forms.  measure_activation_eps() reproduces them (a few seconds).
ACT_GRID = (-12.0, 12.0, (1 << 22) + 1)
ACT_EDGES = (0.0, -0.0, 12.5, -12.5, 13.2, -13.2, 20.0, -20.0, 40.0, -40.0, 43.7, -43.7, 44.5, -44.5, 64.0, -64.0,
             88.0, -88.0, 89.0, -89.0, 100.0, -100.0, 1e4, -1e4, 1e19, -1e19, 1e30, -1e30)
EPS_MEASURED = {
    "gelu_pair": 1.68e-7,
    "gelu_scalar": 1.86e-7,
    "gelu_grad_pair": 2.99e-7,
    "gelu_grad_scalar": 2.99e-7,
    "tanh_fast": 1.83e-7,
}
ACT_MARGIN = 2.0
EPS = {k: ACT_MARGIN * v for k, v in EPS_MEASURED.items()}


def act_grid() -> torch.Tensor:
    lo, hi, n = ACT_GRID
    g = torch.linspace(lo, hi, n, dtype=torch.float64).float()
    return torch.cat([g, torch.tensor(ACT_EDGES, dtype=torch.float32)])


def measure_activation_eps() -> dict:
    x = act_grid()
    xd = x.double()
    sc = xd.abs().clamp(min=1.0)
    forms = {"gelu_pair": (gelu_pair_f32, gelu_exact, sc), "gelu_scalar": (gelu_scalar_f32, gelu_exact, sc),
             "gelu_grad_pair": (gelu_grad_pair_f32, gelu_grad_exact, sc),
             "gelu_grad_scalar": (gelu_grad_scalar_f32, gelu_grad_exact, sc),
             "tanh_fast": (tanh_fast_f32, torch.tanh, torch.ones_like(sc))}
    out = {}
    for name, (f32, exact, scale) in forms.items():
        d = (f32(x).double() - exact(xd)).abs() / scale
        assert bool(torch.isfinite(d).all()), name
        out[name] = float(d.max())
    return out


# ------------------------------------------------------------------------------------ inputs
def make_inputs(M: int, N: int, K: int, bias: bool = True, res: bool = False, act: int = 0, wide: bool = False,
                seed: int = 0, device="cpu"):
    """``(x bf16 [M, K], w bf16 [N, K], b fp32 [N] | None, r bf16 [M, N] | None)``, drawn on the CPU
    (the same values wherever they are used) and moved to ``device``.  x is uniform in +-1 and w
    in +-1 / sqrt(K) (``pre - bias`` has standard deviation 1/3); the bias is N(0, 1), distinct
    per column.  ``wide``: the bias (for act 3 the saved z) instead spans +-40 in N distinct steps,
    shuffled over the columns -- tanh saturates both ways (e^{2x} = inf and 0), GELU and GELU' run
    through their tails.  The residual rows (for act 3: the z rows) cycle through a 509-row N(0, 1)
    (z: N(0, 4)) table with stride 7, so neighbouring rows differ and a large M costs nothing.
    Act 3 takes ``res`` (its z) and no bias."""
    assert act != 3 or (res and not bias)
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * N + 31 * K + 4 * act + 2 * bias + res + 8 * wide)
    gx = torch.Generator().manual_seed(2000003 * seed + 104729 * M + K)
    x = (torch.rand(M, K, generator=gx) * 2 - 1).to(torch.bfloat16)
    w = ((torch.rand(N, K, generator=g) * 2 - 1) / math.sqrt(K)).to(torch.bfloat16)
    span = (torch.randperm(N, generator=g).float() / max(N - 1, 1) * 80.0 - 40.0)
    b = None
    if bias:
        b = span if wide else torch.randn(N, generator=g)
    r = None
    if res:
        table = torch.randn(509, N, generator=g) * (2.0 if act == 3 else 1.0)
        if wide and act == 3:
            table = table + span * (torch.rand(509, 1, generator=g) < 0.5)  # half the rows in the tails
        r = table.to(torch.bfloat16).to(device)[(torch.arange(M, device=device) * 7) % 509]
    return x.to(device), w.to(device), None if b is None else b.to(device), r


def exact_inputs(M: int, N: int, K: int, bias: bool, res: bool, device="cpu"):
    """The position-coded case: ``x[i]`` one-hot at ``(5 i + 3) mod K``, ``w[j, k] = ((37 j + 11 k) mod
    251) - 125``, bias in [-60, 60] and residual in [-70, 70] (integers): every product, sum and
    output is an integer of magnitude <= 255, exact in fp32 and in bf16.  Returns the inputs and the
    expected output (bf16)."""
    i = torch.arange(M, device=device)
    j = torch.arange(N, device=device)
    k = torch.arange(K, device=device)
    hot = (5 * i + 3) % K
    x = torch.zeros(M, K, device=device, dtype=torch.bfloat16)
    x[i, hot] = 1.0
    w = ((37 * j[:, None] + 11 * k[None, :]) % 251 - 125)
    want = w.t()[hot]  # [M, N]: w[j, hot_i]
    b = r = None
    if bias:
        b = ((j * 7) % 121 - 60).float()
        want = want + b.long()
    if res:
        rr = (i[:, None] * 3 + j[None, :] * 5) % 141 - 70
        want = want + rr
        r = rr.to(torch.bfloat16)
    assert int(want.abs().max()) <= 256
    return x, w.to(torch.bfloat16), b, r, want.to(torch.bfloat16)


# ------------------------------------------------------------------------------------ oracle
def linear_oracle(x, w, b=None, act: int = 0, r=None, gelu_eps: float = None):
    """``(ref, tol)`` fp64 [M, N] of ``linear(x, w, b, act, r)`` on the device of ``x``."""
    K = x.shape[1]
    xd, wd = x.double(), w.double()
    pre = xd @ wd.t()
    S = xd.abs() @ wd.abs().t()
    del xd, wd
    if b is not None:
        pre += b.double()
        S += b.double().abs()
    e = S.mul_((K + 2) * U)  # K adds inside v_mfma_f32_16x16x32_bf16 + the bias add (epilogue or armed) + 1 spare
    if act == 0:
        y = pre
    elif act == 1:
        y = gelu_exact(pre)
        e *= GELU_D_MAX  # e_acc carried by |GELU'| <= 1.13
        e += (EPS["gelu_pair"] if gelu_eps is None else gelu_eps) * pre.abs().clamp_(min=1.0)  # gelu_pair
    elif act == 2:
        y = torch.tanh(pre)  # e_acc carried by |tanh'| <= 1
        e += EPS["tanh_fast"]  # tanh_fast
    elif act == 3:
        zd = r.double()
        gp = gelu_grad_exact(zd)
        y = pre * gp
        e *= gp.abs()  # e_acc carried by the factor GELU'(z)
        e += (pre.abs() + e) * (EPS["gelu_grad_pair"] * zd.abs().clamp_(min=1.0))  # gelu_grad_pair, times |A W^T|
        e += U * y.abs()  # res4<3>: v *= GELU'(z)
        del zd, gp
    else:
        raise ValueError(act)
    if r is not None and act != 3:
        y = y + r.double()
        e += U * y.abs()  # res4: v += r
    tol = y.abs().mul_(UB).add_(e.mul_(1 + UB)).add_(TINY)  # f2bf rounds the computed value
    return y, tol


def dual_oracle(x, w, b):
    """fp64 ``dict(z, tol_z, h, tol_h, tol_h_fallback)`` of ``linear_gelu_dual(x, w, b)``."""
    z, tol_z = linear_oracle(x, w, b, 0)
    h, tol_h = linear_oracle(x, w, b, 1)
    # the fallback: fr_gelu_bf16 reads the stored z~ = bf16(pre in fp32), |z~ - pre| <= tol_z
    e = GELU_D_MAX * tol_z  # carried by |GELU'| <= 1.13
    e = e + EPS["gelu_scalar"] * (z.abs() + tol_z).clamp_(min=1.0)  # gelu_kernel: erf_fast2
    tol_fb = h.abs() * UB + (1 + UB) * e + TINY  # its f2bf
    return dict(z=z, tol_z=tol_z, h=h, tol_h=tol_h, tol_h_fallback=tol_fb)


def colsum_oracle(dz):
    """``(ref, tol)`` fp64 [N] for the fused column sums, from the ``dz`` [M, N] bf16 the same launch
    stored (see the module docstring)."""
    d = dz.double()
    a = d.abs().sum(0)
    M = dz.shape[0]
    return d.sum(0), M * U * a + UB / (1 - UB) * a + TINY


# ------------------------------------------------------------------------------------ judging
def elem_ratio(cand, ref, tol) -> torch.Tensor:
    d = (cand.detach().double() - ref).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / tol)
    return torch.where(torch.isfinite(d), r, torch.full_like(r, math.inf))  # a NaN / inf candidate fails


def describe(cand, ref, tol, rows=None, cols=None) -> str:
    r = elem_ratio(cand, ref, tol)
    if r.dim() == 1:
        j = int(r.argmax())
        return ("worst column %d (column tile %d, wave column %d): ratio %.4g (got %.9g, want %.9g, bound %.3g); "
                "%d of %d columns above 1" % (j, j // 256, j % 256 // 64, float(r[j]), float(cand[j]), float(ref[j]),
                                              float(tol[j]), int((r > 1).sum()), r.numel()))
    if rows is not None:
        r[rows:, cols:] = 0.0
    N = r.shape[1]
    k = int(r.argmax())
    i, j = k // N, k % N
    return ("worst (row %d, column %d) = tile (%d, %d), wave block (wr %d, wc %d), fragment (%d, %d) of the tile: "
            "ratio %.4g (got %.9g, want %.9g, bound %.3g); %d of %d elements above 1"
            % (i, j, i // 256, j // 256, i % 256 // 128, j % 256 // 64, i % 256 // 16, j % 256 // 16, float(r[i, j]),
               float(cand[i, j]), float(ref[i, j]), float(tol[i, j]), int((r > 1).sum()), r.numel()))


def worst_ratio(cand, ref, tol, rows=None, cols=None) -> float:
    """max |cand - ref| / tol.  With ``rows`` / ``cols`` (``linear_split``): over all columns of the
    rows < ``rows`` and the first ``cols`` columns of every row -- the rest is unwritten."""
    r = elem_ratio(cand, ref, tol)
    if rows is not None:
        r[rows:, cols:] = 0.0
    return float(r.max()) if r.numel() else 0.0


def check(cand, ref, tol, what: str = "", rows=None, cols=None) -> float:
    """Assert the worst ratio <= 1 (the message names the worst element); returns it."""
    w = worst_ratio(cand, ref, tol, rows, cols)
    if not w <= 1.0:
        raise AssertionError("%s: %s" % (what, describe(cand, ref, tol, rows, cols)))
    return w


# ------------------------------------------------------------------------------------ the GPU cases
# Every list below is built from the CU count alone, so tests/test_gemm_oracle_cpu.py can run its
# rounding model over the input sets of tests/test_gemm_oracle_gpu.py (at NOMINAL_CUS).
# A linear case: (M, N, K, act, bias, res, wide, variant).
K_ZOO = [64, 128, 192, 256, 768, 3072]  # 64: one K-step, the 128x128 kernel; 192: odd step count
PP_VARIANTS = [6, 9, 12, 13]
ALL_VARIANTS = [-1, 0, 6, 9, 12, 13]


def k_cases():
    c = [(512, N, K, 0, True, False, False, v) for N in (256, 768) for K in K_ZOO for v in PP_VARIANTS]
    c += [(512, 128, K, 0, True, False, False, 0) for K in K_ZOO]
    return c + [(4096, 768, 3072, 0, True, False, False, -1)]  # auto: K >= 2048 -> variant 9


def m_cases():
    c = [(M, 768, 192, 0, True, False, False, v) for M in (1, 255, 256, 257, 513) for v in PP_VARIANTS]
    return c + [(M, 768, 192, 0, True, False, False, -1) for M in (4095, 4096, 4097)]


def n_cases():
    c = [(512, N, 192, 2, True, False, False, -1) for N in (128, 384)]  # auto: the 128x128 kernel
    c += [(512, N, 192, 2, True, False, False, 9) for N in (384, 640)]  # partial last column tile
    c += [(512, N, 192, 1, True, False, False, v) for N in (PP2_MAXN, 3200) for v in (9, 12)]  # 3200: falls back
    return c


def _tile_grid(count: int):
    """(tiles_m, N) with tiles_m * N / 256 == count: the most column tiles of 9, 3, 4, 2, 1 that divide it."""
    tn = next(t for t in (9, 3, 4, 2, 1) if count % t == 0)
    return count // tn, tn * 256


def walk_shapes(cus: int):
    """``[(tiles_m, N)]``.  Tile counts 7, 8, 9: one tile per block, G % 8 != 0, == 0, != 0.  Then the
    counts CUs - 1, CUs, CUs + 1 and 3 CUs + 1 exactly, with as many column tiles as divide them (at
    256 CUs: 255 = 85 x 3, 256 = 64 x 4, 257 and 769 are prime: one column tile), and -- so that a
    block's consecutive tiles also CHANGE column tile and the re-armed bias differs -- the nearest
    counts with three or nine column tiles: the multiple of 3 just above the CU count (N = 768) and
    the multiple of 9 just above three times it (N = 2304; blocks walk 3 or 4 tiles, the last
    stride is part-filled)."""
    above = (cus + 3) // 3
    multi = (3 * cus + 9) // 9
    assert cus < above * 3 <= cus + 3 and 3 * cus < multi * 9 <= 3 * cus + 9
    exact = [_tile_grid(c) for c in (cus - 1, cus, cus + 1, 3 * cus + 1)]
    return [(1, 7 * 256), (4, 2 * 256), (3, 3 * 256)] + exact + [(above, 768), (multi, 2304)]


def walk_cases(cus: int):
    c = []
    for tm, N in walk_shapes(cus):
        M = tm * 256 - 5  # the last row tile is part-filled
        for K in (128, 192):
            c += [(M, N, K, 0, True, False, False, v) for v in (6, 9, 12, 13)]
            c += [(M, N, K, 0, False, False, False, v) for v in (6, 9, 13)]
            c += [(M, N, K, 0, True, True, False, v) for v in (6, 9)]
    return c


def epilogue_cases():
    c = []
    for v in ALL_VARIANTS:
        for act in (0, 1, 2):
            c += [(500, 512, 192, act, bias, res, False, v) for bias in (True, False) for res in (True, False)]
            c += [(500, 512, 192, act, True, res, True, v) for res in (True, False)]
        c += [(500, 512, 192, 3, False, True, wide, v) for wide in (False, True)]
    return c


SPLIT_M = [4352, 22 * 256]
SPLIT_N = 2304
SPLIT_K = [128, 768]
SPLIT_NP = [256, 768, SPLIT_N]
SPLIT_VARIANTS = [-1, 9, 12]


def split_full_rows(M: int):
    return [0, 1, 255, 256, 257, M - 1, M]


FFN_N = 3072
FFN_K = [128, 768]
FFN_M = [300, 4096, 4097, 22 * 256]  # 300: the fallbacks; 22 * 256 rows: 264 tiles
FFN_VARIANTS = [-1, 9, 12]


def exact_shape(cus: int):
    """(M, N, K) of the position-coded case: K = 192, three column tiles, more than two tiles per
    block, the last row tile part-filled."""
    return ((2 * cus + 3) // 3 + 1) * 256 - 7, 768, 192


def input_key(case):
    """The input set of a linear case (the variant does not change the inputs)."""
    return case[:7]


def family(case) -> str:
    M, N, K, act, bias, res, wide, v = case
    return {0: "residual" if res else "plain", 1: "gelu", 2: "tanh", 3: "act3"}[act]
