"""fp64 oracles of the user tower -- the multi-head attention over the clicked news
(csrc/user_attn.hip), the additive pool's fp32 user forms (csrc/additive_pool.hip) and the score +
cross-entropy (csrc/score_ce.hip, with its fused tail ``user_pool_score``) -- that carry, per
output element, a bound on what the HIP kernels may differ by (a plain helper module for
tests/test_user_oracle_cpu.py and tests/test_user_oracle_gpu.py, not a conftest).

The values are those of ``ops.reference`` run in fp64 with the fp32 (or bf16) inputs taken as
exact; the intermediates are also formed explicitly (a CPU test holds them to fp64 autograd
through ``ops.reference``), because the bounds need magnitudes, not only values.

Roundings.  ``u = 2^-24`` is the unit roundoff of fp32 and ``ub = 2^-8`` of bf16, both round to
nearest.  Every count is first order; one spare unit per count covers the u^2 terms ("taken").
A rounding acts on a partial sum, so the magnitudes are cancellation-free: ``sum |q||k|`` where the
usual statement has ``|S|``, ``|dA| + sum A |dA|`` where it has ``|dA - D|``.  An n-term fp32 dot
product or weighted sum is counted as n products and n adds, ``2 n u`` of its magnitude, in any
order (MFMA, lane-strided or sequential; with fused multiply-adds it is half that).  ``__expf(x)``
is ``exp2(x log2 e)``: the product and the constant round (2 u |x|) and the hardware exp2 is good
to one ulp (2 u); an absolute error d in the argument is a relative error d in the result.
``1 / x`` and ``a / b`` by the fast forms: 2 u, with the product 3 u.  ``TINY = 1e-30`` keeps every
bound positive -- it also covers fp32 underflow (a flushed term is below 2^-126 of a sum whose
largest term is 1) -- so where the oracle is exactly 0 (the gradients of a masked key, the ctx of
an all-masked impression) any non-zero candidate is a ratio far above 1.

================================================================================================
1. User attention.  d_k = 20, per (impression, head), query t, key s, ``kp_s`` the key mask::

    S_ts = q_t . k_s / sqrt(20)        A_ts = kp_s exp(S_ts) / (sum_s kp_s exp(S_ts) + 1e-8)
    ctx_t = sum_s A_ts v_s             dA = dctx V^T ;  D_t = sum_s A_ts dA_ts
    dS_ts = A_ts (dA_ts - D_t) / sqrt(20) ;  dQ = dS K ;  dK = dS^T Q ;  dV = A^T dctx

evaluated literally in fp64 (exp(-100) is 4e-44 there).  The kernels evaluate the stabilised form
``e_s = exp(S_s - m)``, ``l = sum_s e_s + 1e-8 exp(-m)``, ``A = e / l`` with m the largest kept score
(0 when every key is masked) and save ``(m, 1 / l)``; the oracle gives those too.

    sabs_ts = sum_d |q_td| |k_sd| / sqrt(20) >= |S_ts| ;  smax_t = max over kept s of sabs_ts (>= |m_t|)
    G_ts    = sum_d |dctx_td| |v_sd| >= |dA_ts| ;         Gbar_t = sum_s A_ts G_ts >= |D_t|
    MdS_ts  = A_ts (G_ts + Gbar_t) / sqrt(20) >= |dS_ts|

Scores: a 20-term dot product (40 u) and the scale ``rsqrtf(20)`` with its product (3 u), before or
after the sum: ``|d S_ts| <= 43 u sabs_ts``, taken 44.  The kernel's m is the maximum of its own
scores, so ``|d m| <= 44 u smax`` (+ TINY: ``tol_m``).  In ``e_s`` and in the eps term the SAME m
appears, so its error cancels in A; ``x = S - m`` rounds (u |x|), ``__expf`` adds 2 u |x| + 2 u,
|x| <= 2 smax::

    eps_e = u (44 smax + 6 smax + 2) = u (50 smax + 2)                      taken: u (50 smax + 3)

The eps term ``1e-8f * __expf(-m)``: the fp32 constant (u), ``__expf`` (2 u |m| + 2 u), the
product (u) -- an error of its own, proportional to |m|, that counts wherever the term is a
visible share ``fE = 1e-8 / (sum exp(S) + 1e-8) = 1 - sum_s A_ts`` of l::

    eps_E = u (2 |m| + 4)                                                   taken: u (2 |m| + 5)
    eps_l = (1 - fE) eps_e + fE eps_E + n_l u

with ``n_l`` the adds of l.  Short forms (H <= 64, one 16-lane row per query): 4 adds in the lane,
4 DPP adds, the eps add: n_l = 9, taken 10.  Long forms (H > 64, online softmax over nch =
ceil(H / 64) chunks): H sequential adds, the eps add, and per chunk the rescale
``alpha = __expf(m_old - m_new)`` (|arg| <= 2 smax: u (6 smax + 2)) with its product (u):
``n_l = H + 1 + nch (6 smax + 3)``, taken + 1.  The rescale is applied to l and to the accumulator
alike; against the eps term and in the saved 1 / l it does not cancel, so it is counted in full.
The saved ``1 / l`` (2 u, taken 3) is held to the oracle's at the oracle's m, which moves it by
d m: ``tol_inv = inv (eps_l + 3 u + 44 u smax) + TINY``.  The weights, ``A = e (1 / l)``::

    eps_A = eps_e + eps_l + 4 u                                             taken: + 5 u

Overflow.  ``__expf(-m)`` is +inf once ``-m log2 e >= 128``, i.e. ``-m >= 88.72``: then l = inf,
1 / l = 0 and every weight of the row is exactly 0, where the true ones are below
``exp(-88) / 1e-8 = 6e-31``.  Rows with ``-m >= 88`` (the margin covers d m) take ``eps_A = 1 +
eps_A`` and ``tol_inv = inv (1 + ...)``: the kernel may return the weight or 0, nothing else --
in particular nothing non-finite.

Forward.  ``ctx = (sum_s e_s v_s) (1 / l)``: H products and adds (2 H u), the long form's nch
rescale products of the accumulator::

    tol_ctx = (eps_A + (2 H + nch + 1) u) sum_s A_ts |v_sd| + TINY          (nch = 0 for H <= 64)
    tol_ctx_b = ub |ctx| + (1 + ub) tol_ctx                                 (ctx_b: rounded from the computed value)

Backward.  The weights are recomputed from the saved stats, ``A = __expf(S - m) (1 / l)``: eps_A
again (the stats are stored unrounded).  ``dA`` is a 20-term dot product (40 u G).  Short forms:
``D_t`` sums products A dA (eps_A + 41 u of Gbar) over 4 adds in the lane and 4 DPP adds:
``|d D| <= Gbar (eps_A + 49 u)``; the subtraction rounds (u (G + Gbar)); the products with A
(eps_A + u) and the scale (3 u)::

    |d dS_ts| <= MdS_ts c_dS_t ;   c_dS = 2 eps_A + 54 u                    taken: + 55 u
    E_dQ_td = sum_s MdS_ts (c_dS_t + (2 H + 1) u) |k_sd|     E_dK_sd = sum_t MdS_ts (c_dS_t + (2 H + 1) u) |q_td|
    E_dV_sd = sum_t A_ts (eps_A_t + (2 H + 1) u) |dctx_td|   tol_x = E_x + TINY

(the three products are H-term sums; |dS| <= MdS bounds their partial sums).  ``bf16_out`` rounds
the computed value once: ``tol_x = ub |x| + (1 + ub) E_x + TINY``.  Long forms: D_t is an H-term
sequential sum (``|d D| <= Gbar (eps_A + (41 + H) u)``); ``dQ = (U - D W) / sqrt(20)`` with U = sum A
dA k (a term: eps_A + 42 u, H adds) and W = sum A k (eps_A + (1 + H) u), the product D W, the
subtraction and the scale (5 u): ``2 eps_A + (2 H + 48) u`` of MdS; dK forms dS per (key, query)
(``2 eps_A + (H + 48) u``) and sums H terms (2 H u)::

    c_long = 2 eps_A + (3 H + 49) u   for dQ and dK                         taken: + 50 u
    E_dV   = sum_t A_ts (eps_A_t + (2 H + 1) u) |dctx_td|

================================================================================================
2. Additive pool, fp32 user forms.  Per sequence, position t, ``kp_t`` the position mask::

    a_t = w2 . e_t + b2        alpha_t = kp_t exp(a_t) / (sum_t kp_t exp(a_t) + 1e-8)
    pooled = sum_t alpha_t x_t
    dalpha_t = x_t . g ;  da_t = alpha_t (dalpha_t - sum_k alpha_k dalpha_k) ;  dx_t = alpha_t g
    dpre_t = da_t w2 (1 - e_t^2) ;  dw2 = sum_{n,t} da_t e_t ;  db2 = sum_{n,t} da_t

    aabs_t = sum_q |e_tq| |w2_q| + |b2| ;  amax = max over kept t of aabs_t

``a_t`` is a Q-term dot product (split over 4 or 16 lanes per row, any order) and the bias add:
``|d a_t| <= (2 Q + 2) u aabs_t``.  The wave softmax is the attention's with that argument error::

    eps_e = u ((2 Q + 2) amax + 6 amax + 2)   taken + 3 ;   eps_E = u (2 |m| + 5)
    eps_l = (1 - fE) eps_e + fE eps_E + (ceil(T / 64) + 7) u                (lane adds, 6 wave adds, eps add)
    eps_alpha = eps_e + eps_l + 5 u ;   tol_alpha = alpha eps_alpha + TINY
    tol_pooled = sum_t alpha_t |x_td| (eps_alpha + (2 T + 1) u) + TINY      (T terms, over 8 or 16 t-groups or in order)

The user forms split D over US = 4 blocks per sequence; every block recomputes the same alpha, so
the split changes no count.  The backward reads alpha and g as inputs.  They are exact for the
separate kernels (the test passes the alpha the forward wrote); the fused tail forms them in the
same launch, so the bound carries their errors ``ta_t``, ``tg_d`` (0 otherwise)::

    Mdal_t = sum_d |x_td| |g_d|         E_dal_t = (2 D + 1) u Mdal_t + sum_d |x_td| tg_d
    Msd    = sum_t alpha_t Mdal_t       E_sd    = sum_t (ta_t Mdal_t + alpha_t E_dal_t) + (ceil(T / 64) + 8) u Msd
    Mda_t  = alpha_t (Mdal_t + Msd)     E_da_t  = ta_t (Mdal_t + Msd) + alpha_t (E_dal_t + E_sd) + 3 u Mda_t
    tol_dx_td   = ta_t |g_d| + alpha_t tg_d + 2 u |alpha_t g_d| + TINY
    tol_dpre_tq = E_da_t |w2_q| (1 - e^2) + |da_t w2_q| (2 u + 3 u (1 - e^2)) + TINY

(``e e`` and ``1 - e^2`` round to an absolute u (e^2 + (1 - e^2)) = u, taken 2 u: the factor has no
relative accuracy near |e| = 1; the two products 2 u, taken 3.)  The bf16 copy of dpre rounds the
computed value once: ``ub |dpre| + (1 + ub) tol_dpre``.  ``da8[:, 0]`` is da: ``E_da + TINY``.  The
dw2 / db2 partial rows (one per block) are summed by ``colsum_f32``: at most T + US n adds and a
product per term, on magnitudes (``sum_t da_t`` cancels to ``(1 - sum alpha) sum alpha dalpha``)::

    tol_dw2_q = sum_{n,t} (E_da_t + (T + 4 n + 3) u Mda_t) |e_tq| + TINY
    tol_db2   = sum_{n,t} (E_da_t + (T + 4 n + 3) u Mda_t) + TINY

(The bf16 text-head forms take the same bounds on their bf16 operands: ``tests/text_pool_oracle.py``.)

================================================================================================
3. Score + CE.  Per impression b, candidate c, label column 0::

    z_c = cand_c . user ;  s = sigmoid(z) or z ;  p = softmax_c(s) ;  loss_b = (logsumexp_c s - s_0) / B
    ds_c = (p_c - [c = 0]) / B ;  dz = ds s (1 - s) or ds ;  dcand_c = dz_c user ;  duser = sum_c dz_c cand_c
    loss = sum_b loss_b

``z`` is a D-term dot product: ``E_z = (2 D + 1) u sum_d |cand||user|`` (+ the carried error of a
``user`` formed in the same launch: ``sum_d |cand_cd| tu_d``).  Sigmoid ``1 / (1 + __expf(-z))``:
t = exp(-z) has the relative error ``E_z + u (2 |z| + 2)``, the add and the reciprocal 3 u, and
``d s / d t = -s^2``::

    E_s = s (1 - s) (E_z + u (2 |z| + 3)) + 3 u s + TINY          (identity: E_s = E_z + TINY)

with ``1 - s`` formed as sigmoid(-z): at |z| = 30 the fp64 ``1 - s`` itself has three digits.
Saturation is inside the bound: for z >= 17 the kernel's s is exactly 1 and dz exactly 0 (true
dz ~ ds e^-z, below 3 u s |ds|); for z <= -88.7 ``__expf`` overflows and s is exactly 0 (true s
below 3e-39 < TINY).  Softmax over C <= 16: the common maximum cancels; ``x = s_c - mx`` with
``__expf`` (3 u |x| + 2 u); C adds (taken 16); the division (3 u)::

    r_c  = E_s_c + u (3 |s_c - mx| + 2) ;  r_se = max_c r_c + 16 u ;  E_p_c = p_c (r_c + r_se + 3 u)
    E_ds_c = (E_p_c + 4 u |p_c - [c = 0]|) / B                    (the subtraction, 1 / B and its product)
    E_dz_c = E_ds_c s (1 - s) + |ds_c| E_s_c + 3 u |dz_c| + TINY   (identity: E_ds_c + TINY)

(``d (s (1 - s)) <= E_s (s + (1 - s)) = E_s``, ``1 - s`` and two products 3 u.)  The loss share
``(mx + __logf(se) - s_0) / B``: the logarithm carries r_se absolutely and adds ``u (3 log se + 4)``
of its own, the two adds and the scale ``u (2 (|mx| + log se) + 2 (|lse| + |s_0|) + 3 |lse - s_0|)``
-- at most ``10 u Mloss`` with ``Mloss = |mx| + log se + |s_0|``::

    E_loss_b = (r_se + E_s_0 + u (4 + 10 Mloss_b)) / B
    tol_loss = sum_b E_loss_b + (B + 1) u sum_b loss_b + TINY      (the batch loss: a B-term sum in any order)
    tol_dcand_cd = E_dz_c |user_d| + |dz_c| tu_d + 2 u |dz_c user_d| + TINY
    tol_duser_d  = sum_c (E_dz_c + (2 C + 1) u |dz_c|) |cand_cd| + TINY

================================================================================================
4. The fused tail ``user_pool_score`` = pool forward -> score + CE -> pool backward for duser, in
one launch.  Its bound is the composition of the three above: ``tu = tol_pooled`` enters the scores,
``tg = tol_duser`` and ``ta = tol_alpha`` enter the pool backward (``tail_oracle``).

Judging.  ``ratios`` gives max |candidate - oracle| / bound per (impression, head) for the
attention and per impression (sequence) for pool and score; a candidate passes when every
group's ratio is <= 1; a NaN / inf candidate is an infinite ratio.

Shared inputs (seeded, CPU-built, ``lru_cache``d): a mask zoo per batch -- a random mask (about
30 % dropped), an impression with every key masked, only key 0 kept, only the last key kept, key
0 masked; for H > 64 also the whole first 64-key chunk masked, a whole middle chunk masked (H >
128) and a single key of the last chunk kept -- each also run without a mask; the score regimes
``randn``, ``q4`` (q x 4), ``eps`` (q = a w, k = -b w + noise: every score in about [-25, -10], so
``1e-8 exp(-m)`` is comparable to or larger than l) and ``ovf`` (eps, with query row 0 at scores
near -100, where ``__expf(-m)`` overflows).
"""
import functools
import math

import torch

UB = 2.0 ** -8
U = 2.0 ** -24
TINY = 1e-30
DK = 20
EPS = 1e-8
OVF_M = 88.0  # rows with -m >= 88 (< 128 ln 2 = 88.72): __expf(-m) may be +inf
SQ = math.sqrt(DK)

REGIMES = ("randn", "q4", "eps", "ovf")
H_SHORT = [1, 15, 16, 17, 33, 48, 50, 63, 64]
H_LONG = [65, 76, 128, 129, 200, 2048]
H_FUSED = [1, 16, 17, 50, 64]


# ---------------------------------------------------------------------------------- the inputs
def zoo_mask(T: int, gen: torch.Generator) -> torch.Tensor:
    """``[n, T]`` int32, one sequence per pattern (the module docstring lists them)."""
    ar = torch.arange(T)
    pats = [torch.rand(T, generator=gen) < 0.7, ar < 0, ar == 0, ar == T - 1, ar != 0]
    if T > 64:
        last0 = 64 * ((T - 1) // 64)
        pats.append(ar >= 64)  # the whole first chunk masked
        if T > 128:
            pats.append((ar < 64) | (ar >= 128))  # a whole middle chunk masked
        pats.append(ar == last0 + (T - 1 - last0) // 2)  # one key inside the last (partial) chunk
    return torch.stack(pats).to(torch.int32)


def one_mask(T: int, gen: torch.Generator) -> torch.Tensor:
    """``[1, T]``: the B = 1 case (H = 2048) -- first and a middle chunk masked, 30 % of the rest."""
    ar = torch.arange(T)
    m = (torch.rand(T, generator=gen) < 0.7) & (ar >= 64) & ~((ar >= 640) & (ar < 704))
    return m.view(1, T).to(torch.int32)


def attn_batch(H: int) -> int:
    return 1 if H >= 2048 else 5


@functools.lru_cache(maxsize=None)
def attn_inputs(H: int, NH: int, regime: str, masked: bool):
    """``(qkv fp32 [B, H, 3 NH 20], keep int32 [B, H] | None, dctx fp32 [B, H, NH 20])``."""
    g = torch.Generator().manual_seed(7919 * H + 31 * NH + REGIMES.index(regime))
    keep = None
    B = attn_batch(H)
    if masked:
        keep = one_mask(H, g) if B == 1 else zoo_mask(H, g)
        B = keep.shape[0]
    D = NH * DK
    if regime in ("randn", "q4"):
        q = torch.randn(B, H, NH, DK, generator=g) * (4.0 if regime == "q4" else 1.0)
        k = torch.randn(B, H, NH, DK, generator=g)
    else:  # S_ts = -a_t b_s + noise
        w = torch.randn(B, 1, NH, DK, generator=g)
        w = w / w.norm(dim=-1, keepdim=True) * math.sqrt(SQ)
        a = 3.3 + 1.6 * torch.rand(B, H, NH, 1, generator=g)
        b = 3.3 + 1.6 * torch.rand(B, H, NH, 1, generator=g)
        if regime == "ovf":
            b = 3.9 + 0.2 * torch.rand(B, H, NH, 1, generator=g)
            a[:, 0] = 25.0
        q = a * w
        k = -b * w + 0.01 * torch.randn(B, H, NH, DK, generator=g)
    v = torch.randn(B, H, NH, DK, generator=g)
    qkv = torch.stack([q, k, v], 2).reshape(B, H, 3 * D).contiguous()
    dctx = torch.randn(B, H, D, generator=g)
    return qkv, keep, dctx


def attn_cases():
    """(H, NH, regime): every H with every regime at NH = 3 (2 at H = 2048), and NH = 20 at the
    plain and the eps regime.  Each runs with the mask zoo and without a mask."""
    out = []
    for H in H_SHORT + H_LONG:
        small = 2 if H >= 2048 else 3
        out += [(H, small, r) for r in REGIMES]
        if H < 2048:
            out += [(H, 20, r) for r in ("randn", "eps")]
    return out


POOL_SHAPES = [(T, D, Q) for T in (1, 17, 50, 64) for (D, Q) in ((400, 200), (256, 4), (512, 256))]
POOL_LONG = [(T, 400, 200) for T in (65, 76, 300)]


@functools.lru_cache(maxsize=None)
def pool_inputs(T: int, D: int, Q: int, masked: bool, n: int = 0):
    """``(x [n, T, D], e [n, T, Q], w2 [Q], b2 [1], keep | None, g [n, D])`` fp32.  ``sum |w2| = 40``;
    the last sequence has every ``a_t`` near -20 (the pool's eps regime).  ``n`` = 0: one sequence
    per mask pattern (5 for T <= 64)."""
    gen = torch.Generator().manual_seed(104729 * T + 13 * D + Q + (1 if masked else 0))
    zoo = zoo_mask(T, gen)
    n = n or zoo.shape[0]
    keep = None
    if masked:
        keep = zoo[torch.arange(n) % zoo.shape[0]].contiguous()
    x = torch.randn(n, T, D, generator=gen)
    e = torch.tanh(torch.randn(n, T, Q, generator=gen))
    w2 = torch.randn(Q, generator=gen)
    w2 = w2 * (40.0 / w2.abs().sum())
    b2 = torch.randn(1, generator=gen)
    e[n - 1] = -0.5 * torch.sign(w2) + 0.02 * torch.randn(T, Q, generator=gen)
    g = torch.randn(n, D, generator=gen)
    return x, e.contiguous(), w2, b2, keep, g


SCORE_KINDS = ("small", "sat", "wide")  # |z| ~ 1; |z| near 30 (sigmoid saturated); z over +-60
SCORE_REGIMES = [("small", "sigmoid"), ("sat", "sigmoid"), ("small", "identity"), ("wide", "identity")]  # (kind, act)
SCORE_B, SCORE_C, SCORE_D = [1, 5, 33, 130], [1, 2, 5, 15, 16], [400, 256, 64]
ROWS_B, ROWS_CD = [1, 70, 130], [(5, 400), (16, 256), (1, 64)]
# the fused tail, (B, T, D, Q, C, act, masked, want_bwd): every value of every axis with masks and want_bwd
TAIL_CASES = [(3, 17, 400, 200, 5, "sigmoid", True, True), (1, 1, 256, 4, 1, "identity", True, True),
              (70, 64, 512, 200, 16, "sigmoid", True, True), (3, 50, 400, 4, 5, "identity", True, True),
              (1, 64, 256, 200, 16, "sigmoid", True, True), (70, 1, 400, 4, 1, "sigmoid", True, True),
              (3, 50, 512, 200, 1, "identity", True, True), (3, 17, 256, 4, 16, "identity", True, True),
              (3, 50, 400, 200, 5, "sigmoid", False, True), (3, 17, 400, 200, 5, "sigmoid", True, False),
              (70, 64, 512, 4, 16, "identity", False, False)]


@functools.lru_cache(maxsize=None)
def score_inputs(B: int, C: int, D: int, kind: str):
    """``(cand [B, C, D], user [B, D])`` fp32 with z of the given kind."""
    gen = torch.Generator().manual_seed(15485863 + 1009 * B + 17 * C + D + SCORE_KINDS.index(kind))
    u = torch.randn(B, D, generator=gen)
    cand = torch.randn(B, C, D, generator=gen) / math.sqrt(D)
    if kind != "small":
        un = u / (u * u).sum(-1, keepdim=True)  # cand += t un moves z by t
        if kind == "sat":
            t = 30.0 * (torch.randint(0, 2, (B, C, 1), generator=gen) * 2.0 - 1.0)
        else:
            t = 120.0 * torch.rand(B, C, 1, generator=gen) - 60.0
        cand = cand + t * un.unsqueeze(1)
    return cand.contiguous(), u


@functools.lru_cache(maxsize=None)
def rows_inputs(B: int, C: int, D: int, kind: str, rows: int = 0):
    """``(table [R, D], ci int32 [B C], user [B, D])``: fewer rows than candidates, so rows repeat
    within and across impressions (row 0 is every impression's candidate 1 when C > 1)."""
    R = rows or max(2, (B * C) // 3)
    gen = torch.Generator().manual_seed(32452843 + 1009 * B + 17 * C + D + SCORE_KINDS.index(kind))
    u = torch.randn(B, D, generator=gen)
    table = torch.randn(R, D, generator=gen) / math.sqrt(D)
    if kind != "small":  # users and rows share one direction: user . dirn = 6 (8) +- 1, so z = 5 r (6 +- 1) + O(1)
        dirn = torch.randn(D, generator=gen)
        dirn = dirn / dirn.norm()
        u = u + (6.0 if kind == "sat" else 8.0) * dirn
        r = torch.rand(R, 1, generator=gen) * 2 - 1
        table = table + (torch.sign(r) * 5.0 if kind == "sat" else r * 7.5) * dirn  # z near +-30 / over +-60
    ci = torch.randint(0, R, (B * C,), generator=gen).to(torch.int32)
    if C > 1:
        ci.view(B, C)[:, 1] = 0
        ci.view(B, C)[0, 0] = 0  # a repeat inside an impression
    return table.contiguous(), ci, u.contiguous()


# ------------------------------------------------------------------------------------ judging
def elem_ratio(cand, want, tol) -> torch.Tensor:
    d = (cand.detach().double().cpu().reshape(want.shape) - want).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / tol)
    return torch.where(torch.isfinite(d), r, torch.full_like(r, math.inf))  # a NaN / inf candidate fails


def ratios(cand, want, tol, lead: int = 1) -> torch.Tensor:
    """max |cand - want| / tol per group: the group is the first ``lead`` dims of ``want``."""
    r = elem_ratio(cand, want, tol)
    if r.dim() <= lead:
        return r
    return r.reshape(r.shape[:lead] + (-1,)).amax(-1)


def describe(cand, want, tol) -> str:
    r = elem_ratio(cand, want, tol)
    i = int(r.argmax())
    idx = tuple(int(j) for j in torch.unravel_index(torch.tensor(i), r.shape)) if r.dim() else ()
    c = cand.detach().double().cpu().reshape(want.shape)
    return ("worst element %s of %s: ratio %.4g (got %.9g, want %.9g, bound %.3g); %d of %d elements above 1"
            % (idx, tuple(r.shape), float(r.reshape(-1)[i]), float(c.reshape(-1)[i]), float(want.reshape(-1)[i]),
               float(tol.expand_as(want).reshape(-1)[i]), int((r > 1).sum()), r.numel()))


def check(cand, want, tol, what: str = "", lead: int = 1) -> float:
    """Assert every group's ratio <= 1 (the message names the worst element); returns the worst."""
    tol = tol.expand_as(want)
    w = float(ratios(cand, want, tol, lead).max()) if want.numel() else 0.0
    if not w <= 1.0:
        raise AssertionError("%s: %s" % (what, describe(cand, want, tol)))
    return w


# ---------------------------------------------------------------------------------- attention
def _heads(x: torch.Tensor, NH: int) -> torch.Tensor:
    B, H, _ = x.shape
    return x.reshape(B, H, NH, DK).permute(0, 2, 1, 3)  # [B, NH, H, DK]


def _rows(x: torch.Tensor) -> torch.Tensor:
    B, NH, H, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, H, NH * DK)


def _per_head(x: torch.Tensor, NH: int) -> torch.Tensor:
    """[B, H, NH DK] -> [B, NH, H DK]: (impression, head) leading, for ``ratios(lead=2)``."""
    B, H, _ = x.shape
    return x.reshape(B, H, NH, DK).permute(0, 2, 1, 3).reshape(B, NH, H * DK)


class AttnOracle:
    """fp64 values and bounds of the user attention on ``qkv`` [B, H, 3 NH 20] (fp32, exact):
    ``ctx``, ``m``, ``inv`` (+ ``tol_*``; ``tol_ctx_b``), and with ``dctx``: ``dq``, ``dk``, ``dv``
    [B, H, NH 20] with ``tol_d*`` (fp32 outputs) and ``tolb_d*`` (``bf16_out``).  ``keep_x``: ``self.x``
    keeps the explicit intermediates."""

    def __init__(self, qkv, keep, NH: int, dctx=None, keep_x: bool = False):
        qkv = qkv.detach().cpu().double()
        B, H, _ = qkv.shape
        D = NH * DK
        assert qkv.shape[2] == 3 * D
        self.B, self.H, self.NH, self.D = B, H, NH, D
        self.long = H > 64
        nch = (H + 63) // 64 if self.long else 0
        q, k, v = qkv.view(B, H, 3, NH, DK).permute(2, 0, 3, 1, 4)
        kp = torch.ones(B, 1, 1, H, dtype=torch.bool) if keep is None else (keep.detach().cpu() != 0).view(B, 1, 1, H)
        self.kp = kp
        kf = kp.double()
        S = q @ k.transpose(-1, -2) / SQ
        sabs = q.abs() @ k.abs().transpose(-1, -2) / SQ
        smax = sabs.masked_fill(~kp, 0.0).amax(-1, keepdim=True)
        Ex = torch.exp(S) * kf
        den = Ex.sum(-1, keepdim=True) + EPS
        A = Ex / den  # the eps form, literally
        fE = EPS / den
        m = S.masked_fill(~kp, -math.inf).amax(-1, keepdim=True)
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        inv = 1.0 / ((torch.exp(S - m) * kf).sum(-1, keepdim=True) + EPS * torch.exp(-m))
        eps_e = U * (50 * smax + 3)
        eps_E = U * (2 * m.abs() + 5)
        n_l = (H + 2 + nch * (6 * smax + 3)) if self.long else 10
        eps_l = (1 - fE) * eps_e + fE * eps_E + n_l * U
        ovf = (-m >= OVF_M).double()
        eps_A = eps_e + eps_l + 5 * U + ovf
        self.ctx = _rows(A @ v)
        self.tol_ctx = _rows((eps_A + (2 * H + nch + 1) * U) * (A @ v.abs()) + TINY)
        self.tol_ctx_b = UB * self.ctx.abs() + (1 + UB) * self.tol_ctx
        self.m, self.inv = m.squeeze(-1), inv.squeeze(-1)  # [B, NH, H]
        self.tol_m = (44 * U * smax + TINY).squeeze(-1)
        self.tol_inv = (inv * (eps_l + 3 * U + 44 * U * smax + ovf) + TINY).squeeze(-1)
        self.x = dict(S=S, A=A, smax=smax, fE=fE) if keep_x else None
        if dctx is None:
            return
        g = _heads(dctx.detach().cpu().double(), NH)
        dA = g @ v.transpose(-1, -2)
        G = g.abs() @ v.abs().transpose(-1, -2)
        Dt = (A * dA).sum(-1, keepdim=True)
        Gbar = (A * G).sum(-1, keepdim=True)
        dS = A * (dA - Dt) / SQ
        MdS = A * (G + Gbar) / SQ
        if self.long:
            c = 2 * eps_A + (3 * H + 50) * U
        else:
            c = 2 * eps_A + 55 * U
        wS = MdS * (c + (0 if self.long else (2 * H + 1) * U))
        wA = A * (eps_A + (2 * H + 1) * U)
        vals = (dS @ k, dS.transpose(-1, -2) @ q, A.transpose(-1, -2) @ g)
        errs = (wS @ k.abs(), wS.transpose(-1, -2) @ q.abs(), wA.transpose(-1, -2) @ g.abs())
        for name, val, E in zip(("dq", "dk", "dv"), vals, errs):
            val, E = _rows(val), _rows(E)
            setattr(self, name, val)
            setattr(self, "tol_" + name, E + TINY)
            setattr(self, "tolb_" + name, UB * val.abs() + (1 + UB) * E + TINY)
        self.dqkv = torch.cat([self.dq, self.dk, self.dv], 2)
        if keep_x:
            self.x.update(dA=dA, D=Dt, dS=dS)

    # ``what`` -> worst ratio over the (impression, head) groups
    def _chk(self, cand, want, tol, what):
        NH = self.NH
        return check(_per_head(cand.detach().double().cpu().reshape(want.shape), NH), _per_head(want, NH),
                     _per_head(tol, NH), what, lead=2)

    def check_ctx(self, ctx, what="ctx", bf16=False):
        return self._chk(ctx, self.ctx, self.tol_ctx_b if bf16 else self.tol_ctx, what)

    def check_stats(self, stats, what="stats"):
        s = stats.detach().double().cpu().reshape(self.B, self.NH, self.H, 2)
        return max(check(s[..., 0], self.m, self.tol_m, what + " m", lead=2),
                   check(s[..., 1], self.inv, self.tol_inv, what + " 1/l", lead=2))

    def check_bwd(self, dqkv, what="bwd", bf16=False):
        """-> {"dQ" | "dK" | "dV": worst ratio}, each judged on its own."""
        D = self.D
        c = dqkv.detach().double().cpu().reshape(self.B, self.H, 3 * D)
        pre = "tolb_" if bf16 else "tol_"
        return {n[0] + n[1].upper():
                self._chk(c[..., i * D:(i + 1) * D], getattr(self, n), getattr(self, pre + n), "%s %s" % (what, n))
                for i, n in enumerate(("dq", "dk", "dv"))}

    def masked_rows(self):
        """bool [B, H]: rows of dK / dV that must be exactly 0 (masked keys)."""
        return ~self.kp.view(self.B, self.H)


# --------------------------------------------------------------------------------------- pool
class PoolOracle:
    """fp64 values and bounds of the additive pool's forward: ``alpha`` [n, T], ``pooled`` [n, D];
    ``backward(g, ...)`` gives the gradients."""

    def __init__(self, x, e, w2, b2, keep=None):
        self.xd, self.ed = x.detach().cpu().double(), e.detach().cpu().double()
        self.w2, self.b2 = w2.detach().cpu().double().reshape(-1), float(b2.detach().cpu().double().reshape(-1)[0])
        n, T, D = self.xd.shape
        Q = self.ed.shape[2]
        self.n, self.T, self.D, self.Q = n, T, D, Q
        kp = torch.ones(n, T, dtype=torch.bool) if keep is None else (keep.detach().cpu() != 0).view(n, T)
        self.kp = kp
        a = self.ed @ self.w2 + self.b2
        aabs = self.ed.abs() @ self.w2.abs() + abs(self.b2)
        amax = aabs.masked_fill(~kp, 0.0).amax(-1, keepdim=True)
        Ex = torch.exp(a) * kp.double()
        den = Ex.sum(-1, keepdim=True) + EPS
        self.alpha = Ex / den
        fE = EPS / den
        m = a.masked_fill(~kp, -math.inf).amax(-1, keepdim=True)
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        eps_e = U * ((2 * Q + 2) * amax + 6 * amax + 3)
        eps_E = U * (2 * m.abs() + 5)
        eps_l = (1 - fE) * eps_e + fE * eps_E + ((T + 63) // 64 + 7) * U
        eps_al = eps_e + eps_l + 5 * U
        self.tol_alpha = self.alpha * eps_al + TINY
        self.pooled = torch.einsum("nt,ntd->nd", self.alpha, self.xd)
        self.tol_pooled = torch.einsum("nt,ntd->nd", self.alpha * (eps_al + (2 * T + 1) * U), self.xd.abs()) + TINY
        self.x = dict(a=a, fE=fE, m=m)

    def backward(self, g, alpha=None, ta=None, tg=None):
        """Gradients for ``g`` [n, D] with the weights ``alpha`` (default: the oracle's own; the
        tests pass the fp32 alpha the forward kernel wrote, taken as exact).  ``ta`` / ``tg``: carried
        absolute errors of alpha / g.  -> dict of (value, tol) per output + ``dpre_b`` tol."""
        n, T, D, Q = self.n, self.T, self.D, self.Q
        x, e, w2 = self.xd, self.ed, self.w2
        g = g.detach().cpu().double().reshape(n, D)
        al = self.alpha if alpha is None else alpha.detach().cpu().double().reshape(n, T)
        ta = torch.zeros(n, T, dtype=torch.float64) if ta is None else ta
        tg = torch.zeros(n, D, dtype=torch.float64) if tg is None else tg
        dal = torch.einsum("ntd,nd->nt", x, g)
        Mdal = torch.einsum("ntd,nd->nt", x.abs(), g.abs())
        Edal = (2 * D + 1) * U * Mdal + torch.einsum("ntd,nd->nt", x.abs(), tg)
        sd = (al * dal).sum(-1, keepdim=True)
        Msd = (al * Mdal).sum(-1, keepdim=True)
        Esd = (ta * Mdal + al * Edal).sum(-1, keepdim=True) + ((T + 63) // 64 + 8) * U * Msd
        da = al * (dal - sd)
        Mda = al * (Mdal + Msd)
        Eda = ta * (Mdal + Msd) + al * (Edal + Esd) + 3 * U * Mda
        dx = al.unsqueeze(-1) * g.unsqueeze(1)
        tol_dx = ta.unsqueeze(-1) * g.abs().unsqueeze(1) + al.unsqueeze(-1) * tg.unsqueeze(1) + 2 * U * dx.abs() + TINY
        f = 1.0 - e * e
        dw = da.unsqueeze(-1) * w2
        dpre = dw * f
        tol_dpre = Eda.unsqueeze(-1) * w2.abs() * f + dw.abs() * (2 * U + 3 * U * f) + TINY
        wsum = Eda + (T + 4 * n + 3) * U * Mda
        out = dict(da=(da, Eda + TINY), dx=(dx, tol_dx), dpre=(dpre, tol_dpre),
                   dpre_b=(dpre, UB * dpre.abs() + (1 + UB) * tol_dpre),
                   dw2=(torch.einsum("nt,ntq->q", da, e), torch.einsum("nt,ntq->q", wsum, e.abs()) + TINY),
                   db2=(da.sum().reshape(1), wsum.sum().reshape(1) + TINY))
        out["x"] = dict(dal=dal, sd=sd)
        return out


# ----------------------------------------------------------------------------------- score + CE
class ScoreOracle:
    """fp64 values and bounds of score + CE for ``cand`` [B, C, D], ``user`` [B, D], ``act`` in
    ("sigmoid", "identity"), label column 0: ``scores`` [B, C], ``lossb`` [B], ``loss`` [1], ``dcand``
    [B, C, D], ``duser`` [B, D] (+ ``tol_*``).  ``tu`` [B, D]: carried absolute error of ``user``."""

    def __init__(self, cand, user, act: str, tu=None):
        c, u = cand.detach().cpu().double(), user.detach().cpu().double()
        B, C, D = c.shape
        self.B, self.C, self.D = B, C, D
        tu = torch.zeros(B, D, dtype=torch.float64) if tu is None else tu
        z = torch.einsum("bcd,bd->bc", c, u)
        Ez = (2 * D + 1) * U * torch.einsum("bcd,bd->bc", c.abs(), u.abs()) + torch.einsum("bcd,bd->bc", c.abs(), tu)
        if act == "sigmoid":
            s, s1 = torch.sigmoid(z), torch.sigmoid(-z)  # s and 1 - s, each to full precision
            Es = s * s1 * (Ez + U * (2 * z.abs() + 3)) + 3 * U * s + TINY
        else:
            s, s1, Es = z, None, Ez + TINY
        mx = s.amax(-1, keepdim=True)
        ex = torch.exp(s - mx)
        se = ex.sum(-1, keepdim=True)
        p = ex / se
        r = Es + U * (3 * (s - mx).abs() + 2)
        rse = r.amax(-1, keepdim=True) + 16 * U
        Ep = p * (r + rse + 3 * U)
        pm = p.clone()
        pm[:, 0] = -(p[:, 1:].sum(-1))  # p_0 - 1 without the cancellation
        ds = pm / B
        Eds = (Ep + 4 * U * pm.abs()) / B
        if act == "sigmoid":
            dz = ds * s * s1
            Edz = Eds * s * s1 + ds.abs() * Es + 3 * U * dz.abs() + TINY
        else:
            dz, Edz = ds, Eds + TINY
        lse = mx + torch.log(se)
        self.lossb = ((lse - s[:, :1]) / B).squeeze(-1)
        Mloss = mx.abs() + torch.log(se) + s[:, :1].abs()
        Eloss = ((rse + Es[:, :1] + U * (4 + 10 * Mloss)) / B).squeeze(-1)
        self.tol_lossb = Eloss + TINY
        self.loss = self.lossb.sum().reshape(1)
        self.tol_loss = (Eloss.sum() + (B + 1) * U * self.lossb.abs().sum() + TINY).reshape(1)
        self.scores, self.tol_scores = s, Es
        self.dcand = dz.unsqueeze(-1) * u.unsqueeze(1)
        self.tol_dcand = (Edz.unsqueeze(-1) * u.abs().unsqueeze(1) + dz.abs().unsqueeze(-1) * tu.unsqueeze(1)
                          + 2 * U * self.dcand.abs() + TINY)
        self.duser = torch.einsum("bc,bcd->bd", dz, c)
        self.tol_duser = torch.einsum("bc,bcd->bd", Edz + (2 * C + 1) * U * dz.abs(), c.abs()) + TINY
        self.x = dict(z=z, dz=dz, p=p)

    def check(self, loss, scores, dcand, duser, what="score") -> float:
        w = [check(loss.reshape(1), self.loss, self.tol_loss, what + " loss", lead=1),
             check(scores, self.scores, self.tol_scores, what + " scores"),
             check(dcand, self.dcand, self.tol_dcand, what + " dcand"),
             check(duser, self.duser, self.tol_duser, what + " duser")]
        return max(w)


def tail_inputs(B: int, T: int, D: int, Q: int, C: int, masked: bool):
    """``(x, e, w2, b2, keep, table, ci)`` of a fused-tail case."""
    x, e, w2, b2, keep, _ = pool_inputs(T, D, Q, masked, n=B)
    table, ci, _ = rows_inputs(B, C, D, "small")
    return x, e, w2, b2, keep, table, ci


def tail_oracle(x, e, w2, b2, keep, table, ci, act: str, want_bwd: bool = True):
    """The composed oracle of ``user_pool_score``: ``(pool, score, bwd | None)`` with the carried
    errors of section 4."""
    po = PoolOracle(x, e, w2, b2, keep)
    B = po.n
    cand = table.detach().cpu().double().index_select(0, ci.detach().cpu().long().reshape(-1)).view(B, -1, po.D)
    so = ScoreOracle(cand, po.pooled, act, tu=po.tol_pooled)
    bw = po.backward(so.duser, ta=po.tol_alpha, tg=so.tol_duser) if want_bwd else None
    return po, so, bw
