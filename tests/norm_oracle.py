"""fp64 oracles of the LayerNorm file (csrc/layernorm.hip: every LayerNorm forward form, the
LayerNorm backward with its fused column sums and dropout, the streaming GELU) and of the
gradient reductions (csrc/train_grad.hip: ``colsum``, ``gelu_bwd_colsum``, ``embed_grad``) that
carry, per output element, a bound on what the HIP kernels may differ by (a plain helper module
for tests/test_norm_oracle_cpu.py and tests/test_norm_oracle_gpu.py, not a conftest; no GPU
dependency: everything here runs on the CPU).

The values are those of ``ops.reference`` / ``torch.nn.functional.layer_norm`` / ``F.gelu`` in
fp64, with the bf16 (or fp32: w, b) inputs taken as exact.  The intermediates are formed
explicitly (the CPU test holds them to fp64 autograd), because the bounds need magnitudes.

Roundings.  ``u = 2^-24`` (fp32) and ``ub = 2^-8`` (bf16), round to nearest.  Every count is first
order with one spare unit ("taken").  A rounding acts on a partial sum, so the magnitudes are
cancellation-free (``sum |v|`` where the usual statement has ``|sum v|``).  An n-term fp32 sum is
n - 1 adds in any order (per lane, butterfly, LDS, atomics alike): ``(n - 1) u sum |t|``.
``TINY = 1e-30`` keeps every bound positive, so where the oracle is exactly 0 with no error term
(a pad or absent embedding row, GELU of a saturated negative input) the kernel must give 0.

================================================================================================
1. LayerNorm forward (plain, ``+ residual``, ``embed_ln``, ``embed_ln_rows``,
``layer_norm_scatter``; eps = 1e-12 inside the sqrt, biased variance).  Per row of D elements::

    v = x (+ r)      mean = sum v / D      d = v - mean      var = sum d^2 / D
    rstd = 1 / sqrt(var + eps)      xhat = d rstd      y = xhat w + b
    A = sum |v| / D  (>= |mean|)

* ``v = x + r`` (residual, or word + position) is one fp32 rounding: ``e_in = u |v|`` (0 without).
* mean: the input rounding (1), D - 1 adds, the ``1 / D`` constant of the wide forms (not exact for
  D = 768) and its product -- or the generic form's division -- (2): D + 2 of A::

      e_mean = (D + 3) u A                                                   (taken: + 1)

* ``d = v - mean``.  The computed mean is ONE value per row (the xor butterfly leaves the same sum
  in every lane), off by ``delta``, ``|delta| <= e_mean``; each element adds ``eta = e_in + u |d|``
  (its input rounding and the subtraction's).  The error of d is absolute -- it matters most
  where ``|d|`` is small::

      e_d = e_mean + eta

* var.  ``sum (d - delta + eta)^2 = sum d^2 + D delta^2 + 2 sum d eta - 2 delta sum eta`` (sum d = 0:
  the shift enters squared, exactly -- kept because delta^2 is what is left of a constant row);
  the squares (1), D - 1 adds, ``1 / D`` and its product (2): D + 2 of var::

      e_var = e_mean^2 + 2 mean(|d| eta) + 2 e_mean mean(eta) + (D + 3) u var      (taken: + 1)

* rstd: the eps add (u of var + eps, halved by the root), ``rsqrtf`` (v_rsq_f32, one ulp = 2 u)::

      rel = e_var / (2 (var + eps)) + 4 u                                    (2.5 counted, taken 4)

* ``xhat = d rstd`` (1 product), ``y = xhat w + b`` (a product and an add, or one fma)::

      e_xhat = e_d rstd + |xhat| (rel + u)
      e_y    = |w| e_xhat + u |xhat w| + u |y| + u (|xhat w| + |b|)           (the last: spare)
      tol_y  = ub |y| + (1 + ub) e_y + TINY                                  (f2bf rounds the computed value)

Every term scales with the row's own magnitudes (A, |d|, var, rstd): no regime constant.  An
all-zero row has A = d = 0: every term but ``ub |b|`` vanishes, the kernel must return bf16(b).
A constant non-zero row c has d = 0 and rstd = 1e6: ``e_d rstd |w| ~ (D + 3) u |c| 1e6 |w|``, of
order 100 |w| -- loose by construction (the fp32 sum of D equal values is not D c, and whatever
is left is multiplied by 1e6); there the check is "finite and not absurd".

================================================================================================
2. LayerNorm backward (``g = dy w``; the statistics as above, from x alone: e_in = 0)::

    mg = sum g / D      mgx = sum g xhat / D      dx = rstd (g - mg - xhat mgx)
    dw = sum_rows dy xhat      db = sum_rows dy

    e_g   = u |g|                         e_mg = (D + 3) u mean |g|
    e_mgx = mean(|g| e_xhat) + (D + 4) u mean |g xhat|       (g, the product, D - 1 adds, 1 / D: D + 3)
    e_t   = e_g + e_mg + e_xhat |mgx| + |xhat| e_mgx + 3 u (|g| + |mg| + |xhat mgx|)
    e_dx  = rstd e_t + |dx| (rel + 2 u)           tol_dx = ub |dx| + (1 + ub) e_dx + TINY
    tol_dw = sum_rows |dy| e_xhat + (n + 1) u sum_rows |dy xhat| + TINY      (product, n - 1 adds)
    tol_db = n u sum_rows |dy| + TINY                                        (n - 1 adds)

(e_t: the product ``xhat mgx`` and the two subtractions round once each, 2 u of each magnitude,
taken 3.)  dw and db are added per lane over the rows of its stride, over the 4 waves in LDS, then
by one float atomic per block: an n-row sum in any order.  An all-zero row gives
``dx = rstd (g - mg)`` with rstd = 1e6, finite in bf16.

``dxs`` (and ``cs`` of the drop form) are the column sums of the bf16 tensor the kernel WROTE
(dx, or ``dxz = bf16(bf16(dx) Z)``): they are judged against the fp64 column sum of that written
tensor with ``n u sum |t|`` (``written_colsum``) -- a summation error is not mixed with a dx error.
dxz itself is a bit-exact function of the written dx (``ops.dropout_add``).

================================================================================================
3. Streaming GELU (``fr_gelu_bf16``) and ``gelu_bwd_colsum``.  GELU is ``x Phi(x)``, ``GELU' = Phi + x
phi``; the exact values are ``gemm_oracle.gelu_exact`` / ``gelu_grad_exact`` (erfc forms).  The
kernels use Abramowitz-Stegun 7.1.26 in fp32; the approximation term is ``EPS max(1, |x|)`` with
the constants measured by the method of ``gemm_oracle.measure_activation_eps`` (fp32
transcription against the exact function over ``gemm_oracle.act_grid()``, on the CPU) and doubled
(``ACT_MARGIN``: the hardware rcp / exp are ~1 ulp, the compiler fuses multiply-adds)::

    forward:   tol = ub |y| + (1 + ub) EPS_fwd max(1, |x|) + TINY
    backward:  tol = ub |y| + (1 + ub) (|dh| EPS_bwd max(1, |x|) + u |y|) + TINY     (y = dh GELU'(x))

* ``gelu_kernel`` forward is ``gemm_oracle.gelu_scalar_f32``: the recorded ``EPS["gelu_scalar"]``.
* ``gelu_grad_s`` (train_grad.hip) is ``gemm_oracle.gelu_grad_scalar_f32`` operation for operation
  (``(x c) exp(-x^2 / 2)``): the recorded ``EPS["gelu_grad_scalar"]``.
* ``gelu_kernel`` backward associates ``x (c exp(-x^2 / 2))``: ``gelu_grad_stream_f32`` below, measured
  on its own: 2.99e-7, the same figure (``EPS_MEASURED_STREAM``; the CPU test measures again).

GELU has NO relative accuracy in the negative tail, in the kernels or here: GELU(-5) = -1.4e-6
against an absolute term of 2 EPS |x| ~ 2e-6 -- the bound says "about zero".  The same holds for
GELU' in both tails.  Where fp32 saturates (x <= -13.2: 1 + erf = 0) the kernels give exactly 0.
The comment in train_grad.hip used to quote A&S's exact-arithmetic figure (1.5e-7) for this form.

The column sums of ``gelu_bwd_colsum`` are judged against the written dz (``written_colsum``).

================================================================================================
4. ``colsum`` (contiguous, or a column slice with ld > N): the fp64 sum; M - 1 adds in any order
(unrolled, tail, 4 waves, chunks): ``tol = M u sum_rows |x| + TINY`` per column.

5. ``embed_grad``: the fp64 ``index_add`` over the occurrences of each token, the pad token 0
excluded; a segment of L rows is L - 1 adds: ``tol = L u sum_seg |dx| + TINY``.  Row 0 and every
token absent from the batch have ref = 0 and tol = TINY: exactly zero, checked on the kernel's
output as it stands.

Judging: ``gemm_oracle.elem_ratio`` -- ``|cand - ref| / tol``, a NaN / inf candidate is infinite."""
import functools
import math

import torch

import gemm_oracle as go
from gemm_oracle import TINY, U, UB

BF = torch.bfloat16
LN_EPS = 1e-12
SENTINEL = -60000.0  # what unwritten bf16 rows are filled with
NOMINAL_CUS = go.NOMINAL_CUS

# gelu_kernel's backward association, measured as gemm_oracle.EPS_MEASURED was (see section 3)
EPS_MEASURED_STREAM = {"gelu_grad_stream": 2.99e-7}
EPS_STREAM = {k: go.ACT_MARGIN * v for k, v in EPS_MEASURED_STREAM.items()}


def gelu_grad_stream_f32(x: torch.Tensor) -> torch.Tensor:
    """The backward of ``gelu_kernel`` (layernorm.hip): ``cdf + x * (c * __expf(-0.5f * x * x))``."""
    f = go._f
    cdf = f(0.5) * (f(1.0) + go._erf_fast_f32(x * f(go._RSQRT2)))
    pdf = f(go._RSQRT2PI) * torch.exp(f(-0.5) * x * x)
    return cdf + x * pdf


def measure_stream_eps() -> dict:
    x = go.act_grid()
    xd = x.double()
    d = (gelu_grad_stream_f32(x).double() - go.gelu_grad_exact(xd)).abs() / xd.abs().clamp(min=1.0)
    assert bool(torch.isfinite(d).all())
    return {"gelu_grad_stream": float(d.max())}


# ------------------------------------------------------------------------------------ judging
def ratio(cand, ref, tol) -> float:
    r = go.elem_ratio(cand.cpu(), ref, tol)
    return float(r.max()) if r.numel() else 0.0


def check(cand, ref, tol, what: str = "") -> float:
    """Assert the worst ratio <= 1 (the message names the worst element); returns it."""
    r = go.elem_ratio(cand.cpu(), ref, tol)
    w = float(r.max()) if r.numel() else 0.0
    if not w <= 1.0:
        k = int(r.reshape(-1).argmax())
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(k), r.shape))
        raise AssertionError("%s: worst element %s: ratio %.4g (got %.9g, want %.9g, bound %.3g); %d of %d above 1"
                             % (what, idx, w, float(cand.cpu()[idx]), float(ref[idx]), float(tol[idx]),
                                int((r > 1).sum()), r.numel()))
    return w


def scatter_ratio(buf, ref, tol, dst, fill=SENTINEL) -> float:
    """``buf`` [>= rows, D] was filled with ``fill`` and given to a form that stores row r at
    ``dst[r]`` (None: r).  The written rows against (ref, tol); every other row of buf -- rows no dst
    names and the guard rows past the end -- must still hold ``fill``: else the ratio is infinite."""
    buf = buf.cpu()
    rows = ref.shape[0]
    d = torch.arange(rows) if dst is None else dst.cpu().long()
    untouched = torch.ones(buf.shape[0], dtype=torch.bool)
    untouched[d] = False
    want = torch.full((), fill, dtype=buf.dtype)
    if not bool((buf[untouched] == want).all()):
        return math.inf
    return ratio(buf[d], ref, tol)


# ================================================================================== LayerNorm
def _stats(v, e_in, eps):
    """fp64 statistics of the rows of v and their error terms (section 1)."""
    D = v.shape[-1]
    mean = v.mean(-1, keepdim=True)
    d = v - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = d * rstd
    A = v.abs().mean(-1, keepdim=True)
    e_mean = (D + 3) * U * A  # the input rounding, D - 1 adds, 1 / D and its product; 1 spare
    eta = e_in + U * d.abs()  # v = x + r, and the subtraction
    e_d = e_mean + eta
    e_var = (e_mean ** 2 + 2 * (d.abs() * eta).mean(-1, keepdim=True) + 2 * e_mean * eta.mean(-1, keepdim=True)
             + (D + 3) * U * var)  # the squares, D - 1 adds, 1 / D and its product; 1 spare
    rel = 0.5 * e_var / (var + eps) + 4 * U  # the eps add (halved), rsqrtf 2 u; taken 4
    e_xhat = e_d * rstd + xhat.abs() * (rel + U)  # the product d * rstd
    return dict(mean=mean, d=d, var=var, rstd=rstd, xhat=xhat, rel=rel, e_xhat=e_xhat)


def ln_oracle(x, w, b, r=None, eps: float = LN_EPS):
    """LN(x [+ r]) w + b -> dict(y, tol, mean, var, rstd, xhat) in fp64.  ``r``: the residual, or the
    position rows of an embedding (x = the gathered word rows): one fp32 rounding of the sum."""
    v = x.double()
    e_in = 0.0
    if r is not None:
        v = v + r.double()
        e_in = U * v.abs()
    s = _stats(v, e_in, eps)
    wd, bd = w.double(), b.double()
    xw = s["xhat"] * wd
    y = xw + bd
    e_y = wd.abs() * s["e_xhat"] + U * xw.abs() + U * y.abs() + U * (xw.abs() + bd.abs())  # product, add, spare
    s.update(y=y, tol=UB * y.abs() + (1 + UB) * e_y + TINY)  # f2bf rounds the computed value
    return s


def embed_oracle(tok, word, pos, w, b, T: int, src=None, eps: float = LN_EPS):
    """``LN(word[tok[s]] + pos[s % T])`` for row r, s = src[r] (None: r); tok is the flat [n * T] list."""
    s = torch.arange(tok.numel()) if src is None else src.long()
    return ln_oracle(word[tok.reshape(-1).long()[s]], w, b, pos[s % T], eps)


def ln_bwd_oracle(x, w, dy, eps: float = LN_EPS):
    """-> dict(dx, tol_dx, dw, tol_dw, db, tol_db, rstd, xhat, g, mg, mgx) in fp64 (section 2)."""
    s = _stats(x.double(), 0.0, eps)
    D, n = x.shape[-1], x.shape[0]
    xhat, rstd, e_xhat, rel = s["xhat"], s["rstd"], s["e_xhat"], s["rel"]
    dyd = dy.double()
    g = dyd * w.double()
    mg = g.mean(-1, keepdim=True)
    gx = g * xhat
    mgx = gx.mean(-1, keepdim=True)
    p = xhat * mgx
    dx = rstd * (g - mg - p)
    e_g = U * g.abs()
    e_mg = (D + 3) * U * g.abs().mean(-1, keepdim=True)
    e_mgx = (g.abs() * e_xhat).mean(-1, keepdim=True) + (D + 4) * U * gx.abs().mean(-1, keepdim=True)
    e_t = e_g + e_mg + e_xhat * mgx.abs() + xhat.abs() * e_mgx + 3 * U * (g.abs() + mg.abs() + p.abs())
    e_dx = rstd * e_t + dx.abs() * (rel + 2 * U)
    tol_dx = UB * dx.abs() + (1 + UB) * e_dx + TINY
    dyx = dyd * xhat
    tol_dw = (dyd.abs() * e_xhat).sum(0) + (n + 1) * U * dyx.abs().sum(0) + TINY
    tol_db = n * U * dyd.abs().sum(0) + TINY
    return dict(dx=dx, tol_dx=tol_dx, dw=dyx.sum(0), tol_dw=tol_dw, db=dyd.sum(0), tol_db=tol_db, rstd=rstd,
                xhat=xhat, g=g, mg=mg, mgx=mgx)


def written_colsum(t):
    """(ref, tol) fp64 [N] of the fused column sums of a tensor ``t`` [n, N] the kernel wrote."""
    d = t.cpu().double()
    return d.sum(0), d.shape[0] * U * d.abs().sum(0) + TINY


def drop_kept_limits(n: int, p: float):
    """The kept count of n compared elements: within 5 standard deviations of Binomial(n, 1 - p)."""
    m, sd = n * (1.0 - p), math.sqrt(n * p * (1.0 - p))
    return m - 5.0 * sd, m + 5.0 * sd


# ----------------------------------------------------------------------------- LayerNorm inputs
REGIMES = ("gauss", "bigmean", "outlier", "tinyvar", "zero", "const")
N_REG = len(REGIMES)


def _gen(*key):
    h = 1469598103
    for k in key:
        h = (h * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(h)


def regime_of(rows: int, start: int = 0, regimes=REGIMES):
    return [regimes[(i + start) % len(regimes)] for i in range(rows)]


def regime_rows(rows: int, D: int, g, start: int = 0, residual: bool = False, regimes=REGIMES):
    """bf16 [rows, D]: row i is of regime ``regimes[(i + start) % len]``.  gauss: N(0, 1); bigmean:
    50 + 0.1 N (in bf16 the values are 49.75 / 50 / 50.25); outlier: N(0, 1) with column D // 3 at
    about 30 (the DistilBERT shape); tinyvar: 1e-6 N (var ~ 1e-12 = eps); zero; const: 3.  With
    ``residual`` the same regimes as the second summand: bigmean adds 0.1 N (a spread finer than the
    bf16 spacing at 50), const adds 0.5, zero adds 0."""
    z = torch.randn(rows, D, generator=g)
    kinds = regime_of(rows, start, regimes)
    out = torch.empty(rows, D)
    for name in set(kinds):
        idx = torch.tensor([i for i, k in enumerate(kinds) if k == name])
        zz = z[idx]
        if name == "gauss":
            val = zz
        elif name == "bigmean":
            val = 0.1 * zz if residual else 50.0 + 0.1 * zz
        elif name == "outlier":
            val = zz.clone()
            val[:, D // 3] = (0.0 if residual else 30.0) + zz[:, D // 3]
        elif name == "tinyvar":
            val = 1e-6 * zz
        elif name == "zero":
            val = torch.zeros_like(zz)
        else:
            val = torch.full_like(zz, 0.5 if residual else 3.0)
        out[idx] = val
    return out.to(BF)


def affine(D: int, g):
    """(w, b) fp32: w ~ N(0, 1) (negative entries) with every 5th entry 0; b ~ 0.5 + N(0, 1), never 0."""
    w = torch.randn(D, generator=g)
    w[::5] = 0.0
    b = 0.5 + torch.randn(D, generator=g)
    b[b == 0] = 0.25
    return w, b


@functools.lru_cache(maxsize=None)
def ln_inputs(rows: int, D: int):
    """-> (x, r, w, b, kinds): the shared forward input set of a shape, every regime in turn (which
    regime the first row has depends on the shape)."""
    g = _gen(1, rows, D)
    start = (rows + D // 4) % N_REG
    x = regime_rows(rows, D, g, start)
    r = regime_rows(rows, D, g, start, residual=True)
    w, b = affine(D, g)
    return x, r, w, b, regime_of(rows, start)


BWD_REGIMES = REGIMES[:5]  # a constant row makes tol_dw of EVERY column loose: only where asked for


@functools.lru_cache(maxsize=None)
def ln_bwd_inputs(rows: int, D: int, with_const: bool = False):
    """-> (x, w, dy, kinds)."""
    g = _gen(2, rows, D, with_const)
    regs = REGIMES if with_const else BWD_REGIMES
    start = (rows + D // 4) % len(regs)
    if with_const and rows < N_REG:
        start = N_REG - rows  # the constant row is among them
    x = regime_rows(rows, D, g, start, regimes=regs)
    w, _ = affine(D, g)
    dy = torch.randn(rows, D, generator=g).to(BF)
    return x, w, dy, regime_of(rows, start, regs)


# forward cases: (wide, rows, D)
FWD_ROWS = (1, 3, 7, 9, 31, 33, 65)  # the tails of 4-, 8-, 16- and 32-row blocks
# ln_kernel (wide = 0): 4: one lane; 36 / 252 / 260 / 400 / 1000: D % 256 != 0, the ``i < D`` masking inside a
# chunk; 256 / 768 / 1024: whole chunks
FWD_D_GENERIC = (4, 36, 252, 256, 260, 400, 768, 1000, 1024)
FWD_D_WIDE = (256, 512, 768, 1024, 400)  # 400: D % 256 != 0 falls through to the generic kernel


def fwd_shapes(wide: int):
    return [(rows, D) for D in (FWD_D_GENERIC if wide == 0 else FWD_D_WIDE) for rows in FWD_ROWS]


def walk_rows(cus: int):
    """ln16p_kernel (wide = 4) at D = 256: its grid is min(8 CUs, ceil(rows / 8)) blocks of 8
    half-waves, so a half-wave takes a second row past 64 CUs rows and a third past 128 CUs."""
    return [64 * cus + 11, 128 * cus + 3]


BWD_D = (36, 256, 400, 768, 1024)  # 36, 400: ln_bwd_kernel's masked lanes read row 0 and discard it
BWD_ROWS = (1, 4, 5, 1000)  # 1, 4: one block (a part-filled one, a full one); 5: the second block has one row
BWD_WALK_ROWS = (4096 + 5, 2 * 4096 + 1)  # D = 256: the 1024-block grid strides 4096 rows
DROP_P = (0.1, 0.5)
DROP_SEED, DROP_OFFSET = 99, 5


def bwd_cases():
    """(rows, D, with_const)."""
    c = [(rows, D, False) for D in BWD_D for rows in BWD_ROWS]
    c += [(rows, 256, False) for rows in BWD_WALK_ROWS]
    return c + [(4, 36, True), (5, 256, True), (5, 768, True)]


# embedding cases: (n, T, D); the vocabulary is small, tokens repeat.  n * T = 1, 5, 7, 15, 33, 50, 150 rows:
# tails of the 4-row (ln_kernel) and 8- / 16- / 32-row (ln16_kernel) blocks; T = 1: row % T == 0 always
EMBED_V = 13
EMBED_T = (1, 5, 50)


def embed_shapes(wide: int):
    Ds = (36, 400, 768) if wide == 0 else (256, 768, 400)
    return [(n, T, D) for D in Ds for T in EMBED_T for n in ((1, 7, 33) if T == 1 else (1, 3))]


@functools.lru_cache(maxsize=None)
def embed_inputs(n: int, T: int, D: int):
    """-> (tok [n, T] int32, word [V, D], pos [T + 3, D], w, b, src [n * T] int32).  Word rows cycle
    through the regimes (row 0 gauss, row 4 all zero); position rows are 0.02 N, every third one
    zero.  Token 0, the last vocabulary row and position T - 1 occur; ``src`` is a permutation of
    the flat tokens (never the identity for n * T > 1)."""
    g = _gen(3, n, T, D)
    word = regime_rows(EMBED_V, D, g)
    pos = (0.02 * torch.randn(T + 3, D, generator=g))
    pos[::3] = 0.0
    tok = torch.randint(0, EMBED_V, (n, T), generator=g, dtype=torch.int32)
    flat = tok.view(-1)
    flat[-1] = EMBED_V - 1
    flat[0] = 0
    if n * T > 2:
        flat[1] = 4
    w, b = affine(D, g)
    src = torch.roll(torch.randperm(n * T, generator=g), 1).to(torch.int32)
    if n * T > 1 and bool((src.long() == torch.arange(n * T)).all()):
        src = torch.roll(src, 1)
    return tok, word, pos.to(BF), w, b, src


SCATTER_D = (256, 768)


def scatter_dst(rows: int, g):
    """-> (dst int32 [rows], dup): a partial permutation.  Rows rows-1 and rows-2 (when rows >= 4) are
    to be made copies of rows 0 and 1 and share their destinations, so two destination rows stay
    unwritten; ``dup`` is that count."""
    p = torch.randperm(rows, generator=g)
    dup = 2 if rows >= 4 else 0
    dst = p.clone()
    for k in range(dup):
        dst[rows - 1 - k] = p[k]
    return dst.to(torch.int32), dup


@functools.lru_cache(maxsize=None)
def scatter_inputs(rows: int, D: int):
    x, r, w, b, _ = ln_inputs(rows, D)
    dst, dup = scatter_dst(rows, _gen(4, rows, D))
    x, r = x.clone(), r.clone()
    for k in range(dup):
        x[rows - 1 - k], r[rows - 1 - k] = x[k], r[k]
    return x, r, w, b, dst


# ======================================================================================= GELU
GELU_N = (4, 4 * 63, 4 * 257)
GELU_N_STRIDE = 4 * (4096 * 256 + 37)  # past the 4096-block cap of fr_gelu_bf16: the grid-stride loop


@functools.lru_cache(maxsize=None)
def gelu_inputs(n: int):
    """-> (z, dh) bf16 [n]: gemm_oracle's saturation points, then a sweep of [-12, 12] (rounded to
    bf16), in an order that puts edge values in every size; dh ~ N(0, 1)."""
    g = _gen(5, n)
    edges = torch.tensor(go.ACT_EDGES, dtype=torch.float32)
    m = max(n - edges.numel(), 2)
    z = torch.cat([torch.linspace(-12.0, 12.0, m), edges])
    z = z[torch.randperm(z.numel(), generator=g)][:n]
    if n >= 4:
        z[:4] = torch.tensor([-13.25, -0.0, 0.7, 1e30])
    return z.to(BF), torch.randn(n, generator=g).to(BF)


def gelu_fwd_oracle(z):
    x = z.double()
    y = go.gelu_exact(x)
    return y, UB * y.abs() + (1 + UB) * go.EPS["gelu_scalar"] * x.abs().clamp(min=1.0) + TINY


def gelu_bwd_oracle(z, dh, form: str):
    """``form``: "stream" (gelu_kernel's backward) or "colsum" (gelu_grad_s of train_grad.hip)."""
    eps = EPS_STREAM["gelu_grad_stream"] if form == "stream" else go.EPS["gelu_grad_scalar"]
    x, d = z.double(), dh.double()
    y = d * go.gelu_grad_exact(x)
    e = d.abs() * eps * x.abs().clamp(min=1.0) + U * y.abs()  # the approximation; the product with dh
    return y, UB * y.abs() + (1 + UB) * e + TINY


# ===================================================================================== colsum
CS_MAX_CHUNKS = 256


def cs_chunks(M: int, N: int, budget: int) -> int:
    """The launchers' rule (train_grad.hip): cb = ceil(N / 512) column blocks; chunks = budget / cb
    (budget 1024 for colsum, 2048 for gelu_bwd_colsum) clamped to [16, 256], then to M; a chunk
    is rows_per = ceil(M / chunks) rows."""
    cb = (N + 511) // 512
    c = min(max(budget // cb, 16), CS_MAX_CHUNKS)
    return min(c, M)


CS_N = (8, 64, 520, 768, 3072)
CS_SMALL_M = (1, 3, 17)


def cs_mixed_M(N: int, budget: int, unroll: int) -> int:
    """An M at which one launch has: full chunks that run the unrolled loop (``unroll`` rows per
    trip: 16 in colsum, 8 in gelu_bwd_colsum) twice and then a ragged tail (the 4 waves end on
    different trips); one chunk of 5 (colsum) or 3 rows that runs the tail loop only; and empty
    chunks after it.  rows_per = 2 * unroll + 3 (colsum: 35; gelu: 19 -- wave 0 trips at rows 0, 8,
    then one tail row 16; wave 3 has no tail row), M = rows_per * k + (5 or 3) with k the largest
    count that keeps ceil(M / chunks) = rows_per."""
    chunks = min(max(budget // ((N + 511) // 512), 16), CS_MAX_CHUNKS)
    rp = 2 * unroll + 3
    rest = 5 if unroll == 16 else 3
    k = (chunks * rp - rest) // rp - 1
    M = rp * k + rest
    assert cs_chunks(M, N, budget) == chunks and (M + chunks - 1) // chunks == rp and k + 1 < chunks
    return M


def colsum_cases():
    """(M, N, sliced): sliced = the middle third of a [M, 3 N] tensor (ld = 3 N).  The mixed-loop M
    is sliced for N <= 520 (at N >= 768 the parent tensor would be 40 - 100 MB for the same loops)."""
    c = []
    for N in CS_N:
        Ms = CS_SMALL_M + (cs_mixed_M(N, 1024, 16),)
        c += [(M, N, False) for M in Ms]
        c += [(M, N, True) for M in Ms if M in (3, 17) or (M > 17 and N <= 520)]
    return c


def gelu_colsum_cases():
    return [(M, N) for N in CS_N for M in CS_SMALL_M + (cs_mixed_M(N, 2048, 8),)]


@functools.lru_cache(maxsize=4)
def colsum_inputs(M: int, N: int, sliced: bool):
    """bf16 [M, N] N(0, 1) -- for ``sliced`` the [M, 3 N] parent: the case is ``parent[:, N:2 * N]``."""
    return torch.randn(M, 3 * N if sliced else N, generator=_gen(6, M, N, sliced)).to(BF)


@functools.lru_cache(maxsize=2)
def gelu_colsum_inputs(M: int, N: int):
    """(df, z) bf16 [M, N]: z ~ N(0, 4) with every 7th column scaled into the tails."""
    g = _gen(7, M, N)
    z = 2.0 * torch.randn(M, N, generator=g)
    z[:, ::7] *= 4.0
    return torch.randn(M, N, generator=g).to(BF), z.to(BF)


def colsum_oracle(x):
    d = x.double()
    return d.sum(0), d.shape[0] * U * d.abs().sum(0) + TINY


# ================================================================================= embed_grad
EG_HEAVY = 64
EG_LENGTHS = (1, 63, 64, 65, 66, 1000)
# (name, D, segment lengths of tokens 2, 4, 6, ... in id order, pad rows)
EG_CASES = (
    ("zoo-768", 768, EG_LENGTHS, 40),  # the last token (1000 rows, heavy kernel) ends at R
    ("end64-512", 512, (65, 1000, 66, 1, 63, 64), 7),  # the last segment is exactly EG_HEAVY rows and ends at R
    ("end65-256", 256, (64, 1, 1000, 66, 63, 65), 0),  # no pad row at all; the last segment is heavy by one row
    ("end1-256", 256, (66, 65, 64, 63, 1), 3),
    ("heavy-stride-256", 256, (65,) * 261 + (3, 64), 50),  # 261 heavy tokens > the 256-block grid
)


@functools.lru_cache(maxsize=None)
def embed_grad_inputs(name: str):
    """-> (dx bf16 [R, D], tok int32 [R], V).  Token ids are 2, 4, 6, ...: every odd id (and V - 1)
    is absent from the batch; token 0 is the pad.  The rows are shuffled, so ``perm`` is no
    identity; a stable sort restores occurrence order."""
    _, D, lengths, pad = next(c for c in EG_CASES if c[0] == name)
    g = _gen(8, D, len(lengths), pad)
    tok = torch.cat([torch.zeros(pad, dtype=torch.int32)]
                    + [torch.full((L,), 2 * (i + 1), dtype=torch.int32) for i, L in enumerate(lengths)])
    tok = tok[torch.randperm(tok.numel(), generator=g)]
    V = 2 * len(lengths) + 2
    return torch.randn(tok.numel(), D, generator=g).to(BF), tok, V


def embed_grad_oracle(dx, tok, V: int):
    d = dx.double()
    t = tok.long()
    ref = torch.zeros(V, d.shape[1], dtype=torch.float64).index_add_(0, t, d)
    mag = torch.zeros(V, d.shape[1], dtype=torch.float64).index_add_(0, t, d.abs())
    L = torch.bincount(t, minlength=V).double().unsqueeze(1)
    ref[0] = 0.0  # padding_idx
    mag[0] = 0.0
    return ref, L * U * mag + TINY
