"""An fp64 oracle of the fused text head (csrc/text_head.hip) that carries, per output element, a
bound on what the HIP kernels may differ by (a plain helper module for the head tests, not a
conftest; no GPU dependency: every function runs on the device of its arguments).

Every op is judged stage-wise: the oracle of a stage receives the exact tensors the kernel
received, and where a stage consumes a previous kernel's output it receives that kernel's ACTUAL
output, taken as exact.  ``U = 2^-24`` / ``UB = 2^-8`` are the unit roundoffs of fp32 / bf16,
``TINY`` the absolute floor, ``tanh_fast_f32`` / ``EPS["tanh_fast"]`` / ``ACT_MARGIN`` and the
judging helpers are those of tests/gemm_oracle.py (the head's ``tanh_fast`` is the same formula).
Magnitudes are sums of absolute values (never ``|result|``: a rounding acts on a partial sum);
every count is first order with one spare unit.  The terms, in the order the kernels apply them:

``head_score`` (``score_oracle``): X [M, D] the cache rows by title index, W1 [Q, D] bf16.
* accumulation: bf16 products are exact in fp32, D of them added by the MFMAs and b1 once:
  ``e_acc = (D + 2) U (|X| |W1|^T + |b1|)``;
* tanh carries ``e_acc`` by its derivative -- ``1 - tanh^2 <= min(1, 1 - e^2 + 2 e_acc)`` within e_acc of
  pre -- and adds ``EPS["tanh_fast"]``: ``e32``;
* e is stored in bf16: ``tol_e = UB |e| + (1 + UB) e32``;
* a = w2 . e + b2 from the FP32 tanh values: ``tol_a = sum_q |w2_q| e32_q + (Q + 2) U (sum |w2| |e| +
  |b2|)``.  The accumulation term dominates: the bound is 2^-10 of the score's magnitude at D = 768 and
  2^-12 at D = 256 (not the 2^-16 of the last term alone), so a score built from the bf16 e -- off by
  up to 2^-8 sum |w2| |e|, but with random signs by 1 / sqrt(Q) of that -- leaves it only where the
  roundings align: the "aligned" input set (mutant (a): 7.0 there, 0.39 on the plain set).

``head_pool`` (``pool_oracle``): alpha_t = keep_t exp(a_t) / (sum keep exp(a) + 1e-8), in fp64
straight from this definition (the reference's formula, not the shifted form the kernel runs).
* ``a_t - m`` rounds once, ``__expf(x)`` is ``v_exp_f32(x log2 e)`` with relative error
  ``EPS["expf"] max(1, |x|)`` (the argument's rounding scales with |x|; measured below):
  ``ex(x) = EPS["expf"] max(1, |x|) + U |x|``;
* the denominator: the terms' errors weighted by their share, ``sum_s alpha_s ex(a_s - m)``, the
  eps term's share ``1 - sum alpha`` times ``ex(m) + 2 U`` (``__expf(-m)``, the constant 1e-8f, the
  product), and T + 2 adds of positive terms: ``(T + 2) U``;
* the reciprocal and the product ``p inv``: ``3 U`` (one spare);
  ``tol_alpha = alpha (ex(a_t - m) + den + (T + 5) U) + TINY``.  TINY is the absolute floor: a weight
  below 2^-126 may be flushed, and for m < -88.7 ``__expf(-m)`` overflows and the kernel returns
  alpha = 0 where the true value is at most e^-88.7 / 1e-8 = 2.9e-31;
* ``pooled = sum_t alpha_t x_t``: ``(T + 2) U sum |alpha| |x| + sum tol_alpha_t |x_t|``.  A title with
  no kept token and a padded title (u >= nreal) give exact zeros; ``pooled_b`` is bf16(pooled).

``head_pool_bwd`` and da / db2p of ``head_pool_bwd_g`` (``pool_bwd_oracle``): the kernel's alpha
[U, T] and g [U, D] fp32 are exact.  ``A_t = sum_d |g_d| |x_td|``, ``B = sum_s alpha_s A_s``.
* ``dalpha_t = g . x_t``: ``(D + 2) U A_t`` (any order);
* ``sm = sum alpha dalpha``: ``(D + 2) U B`` carried plus ``(T + 2) U B`` of its own;
* ``da_t = alpha_t (dalpha_t - sm)``: the subtraction and the product, one spare: ``3 U (A_t + B)``;
  ``tol_da = alpha_t ((D + 2) U A_t + (D + T + 4) U B + 3 U (A_t + B)) + TINY`` -- never ``|da|``;
* ``db2p = sum_t da_t`` against the fp64 sum of the fp64 da: ``sum_t tol_da_t + (T + 2) U sum_t
  alpha_t (A_t + B)``.

The rewrite of ``head_pool_bwd_g`` (``g_oracle``): from the kernel's own fp32 da and the bf16 e.
* ``g = bf16(da (1 - e^2))``: ``1 - f f`` and the product round once each, one spare, then the
  store: ``tol_g = UB |g| + 3 U |g| + TINY`` (tighter than one bf16 ulp);
* ``cs[0] = sum_t da_t e_t``: ``(T + 2) U sum |da| |e|``;
* ``cs[1] = sum_t g_t`` of the STORED g, against the fp64 sum of what the launch wrote:
  ``(T + 2) U sum |g|``.

``head_wgrad_g`` (``wgrad_g_oracle``): G bf16 [U T, Q], R real titles in S splits of tps whole titles.
A term passes through the adds of ITS split and then the reduction's, not through every add of
the sum, so the count is per split -- never more than the R T + S + 3 of the whole sum, and at
1577 titles of 50 tokens 40 times less, which is what lets the bound see a lost stage there:
* ``dW1[q][k] = w2_q sum_{m < R T} G_mq x_mk``: tps T adds in the split's MFMAs, S in the reduction,
  the w2 product, one spare: ``(tps T + S + 3) U |w2_q| sum |G| |x|``;
* ``dw2 = sum_{u < R} cs[0]``: ``(tps + S + 2) U sum |cs[0]|``; ``db1 = w2 sum_{u < R} cs[1]``: ``(tps + S + 3)
  U |w2| sum |cs[1]|``; ``db2 = sum_{u < U} db2p`` (every slot: the pool backward writes 0 for the
  padded ones): ``(U + S + 2) U sum |db2p|``.

``head_wgrad`` (``wgrad_oracle``, g formed inside from e and da; S splits of mchunk rows):
* g is rounded to bf16 in LDS: ``UB |g| + 3 U |g|`` per term, so ``dW1``: ``(UB + (mchunk + S + 6) U)
  |w2_q| sum |g| |x|`` and ``db1 = w2 sum bf16(g)``: ``(UB + (mchunk + S + 6) U) |w2_q| sum |g|``;
* ``dw2 = sum da e`` has no bf16 term: ``(mchunk + S + 2) U sum |da| |e|``; db2 as above.
Under nreal both kernels re-split the real rows over the same grid; tps and mchunk are the
re-split values (``wgrad_g_resplit`` / ``wgrad_resplit``).

``__expf``.  ``expf_f32`` transcribes it in fp32; ``measure_expf_eps`` compares it with fp64 over
``EXPF_GRID`` (2^23 + 1 points of [-100, 100]: the arguments ``a - m`` <= 0 that occur and the arguments
``-m``) plus ``EXPF_EDGES``: relative error over max(1, |x|) wherever the exact value is a
normal fp32 number (below 2^-126 and past the overflow the transcription must be within TINY of
the exact value / be inf).  The worst is recorded in ``EPS_MEASURED["expf"]``; the bound uses
``ACT_MARGIN`` times it, as for the GEMM activations.  The CPU test measures again.

Judging.  ``check`` asserts ``max |cand - ref| / tol <= 1`` (NaN / inf: an infinite ratio) over every
element; the rows of padded titles of e and a (m >= nreal T) are the one exception -- the
launcher's contract leaves them unwritten -- and are cut off by the caller (``[: nreal * T]``).
"""
import math

import torch

import gemm_oracle as go
from gemm_oracle import ACT_MARGIN, NOMINAL_CUS, TINY, U, UB, tanh_fast_f32  # noqa: F401 (re-exported)

EPS_MEASURED = {"expf": 1.15e-7}
EPS = {"tanh_fast": go.EPS["tanh_fast"], "expf": ACT_MARGIN * EPS_MEASURED["expf"]}
_LOG2E = 1.44269504088896341
EXPF_GRID = (-100.0, 100.0, (1 << 23) + 1)
EXPF_EDGES = (0.0, -0.0, -87.0, -87.3, -87.33654, -87.4, -88.0, -88.7, -89.0, -103.0, -104.0, -110.0, -1e4, 87.0, 88.0,
              88.7, 88.72, 88.73, 89.0, 100.0, 1e4)
MAXT = 128
MAX_SPLIT_TITLES = 1024
WTM = 32  # rows per stage of both weight-gradient kernels


def expf_f32(x: torch.Tensor) -> torch.Tensor:
    """``__expf`` = ``v_exp_f32(x * log2(e))``, in fp32."""
    return torch.exp2(x * torch.tensor(_LOG2E, dtype=torch.float32, device=x.device))


def expf_grid() -> torch.Tensor:
    lo, hi, n = EXPF_GRID
    g = torch.linspace(lo, hi, n, dtype=torch.float64).float()
    return torch.cat([g, torch.tensor(EXPF_EDGES, dtype=torch.float32)])


def measure_expf_eps() -> float:
    x = expf_grid()
    xd = x.double()
    got, want = expf_f32(x).double(), torch.exp(xd)
    normal = (want >= 2.0 ** -126) & (want < 2.0 ** 127)
    rel = (got - want).abs() / (want * xd.abs().clamp(min=1.0))
    assert bool(torch.isfinite(rel[normal]).all())
    low = want < 2.0 ** -126
    assert float((got - want)[low].abs().max()) <= TINY  # the flushed range: inside the absolute floor
    assert bool((got[want >= 2.0 ** 128] == math.inf).all())
    return float(rel[normal].max())


# ------------------------------------------------------------------------------------ launch rules
def score_tile(M: int, T: int, Q: int, cus: int, forced: int = 0, padded: bool = False) -> int:
    """Rows per block of ``head_score`` (fr_head_score's rounds rule)."""
    if Q != 384:
        return 128
    Me = max(M - 64 * T, T) if padded else M
    r192 = ((Me + 191) // 192 + cus - 1) // cus
    r160 = ((Me + 159) // 160 + cus - 1) // cus
    return 160 if forced == 160 or (forced == 0 and r160 * (160 + 384) < r192 * (192 + 384)) else 192


def pool_tpt(T: int, D: int) -> int:
    TG = 384 // (D // 8)
    return (T + TG - 1) // TG


def supported(D: int, Q: int, T: int) -> bool:
    return D % 256 == 0 and D <= 1024 and Q in (128, 256, 384) and 1 <= T <= MAXT and pool_tpt(T, D) <= 32


def wgrad_g_split(Un: int, D: int, cus: int):
    """``(S, tps)`` of fr_head_wgrad_g: S splits of ``tps`` whole titles."""
    S = max(1, cus // (D // 128))
    tps = min(max(1, (Un + S - 1) // S), MAX_SPLIT_TITLES - 2)
    return ((Un + tps - 1) // tps if Un > 0 else 1), tps


def wgrad_split(M: int, T: int, D: int, Q: int, cus: int):
    """``(S, mchunk)`` of fr_head_wgrad: S splits of ``mchunk`` rows (seams fall inside titles)."""
    ntiles = (Q // 128) * (D // 256)
    S = max(1, min(cus // ntiles, (M + 8 * WTM - 1) // (8 * WTM)))
    mchunk = max(WTM, ((M + S - 1) // S + WTM - 1) // WTM * WTM)
    cap = (MAX_SPLIT_TITLES - 2) * T // WTM * WTM
    if mchunk > cap:
        mchunk = 64 if cap < 64 else cap // 64 * 64
    return max(1, (M + mchunk - 1) // mchunk), mchunk


def wgrad_resplit(M: int, T: int, R: int, S: int, mchunk: int):
    """The kernel's re-split of the real rows under ``nreal = R``: ``(M', mchunk')``."""
    Mr = min(M, R * T)
    c = ((Mr + S - 1) // S + WTM - 1) // WTM * WTM
    return Mr, max(WTM, min(mchunk, c))


def wgrad_g_resplit(Un: int, R: int, S: int, tps: int):
    Ur = min(Un, R)
    return Ur, max(1, min(tps, (Ur + S - 1) // S))


# ------------------------------------------------------------------------------------ inputs
N_TABLE = 37  # titles in the hidden-state table: ids repeat to reach the row counts


def zoo_mask(n: int, T: int, gen: torch.Generator) -> torch.Tensor:
    """``[n, T]`` int32 keep masks, one title per pattern and then random ones: lengths T, 0, 1, T - 1,
    only the last token, every other token, a random prefix, random at 0.4; for T > 64 only the
    tokens >= 64, only token 63, only token 64.  Title 1 is all masked in every set."""
    ar = torch.arange(T)
    pats = [torch.ones(T), torch.zeros(T), (ar < 1).float(), (ar < T - 1).float(), (ar == T - 1).float(),
            (ar % 2 == 0).float(), (ar < int(torch.randint(1, T + 1, (1,), generator=gen))).float(),
            (torch.rand(T, generator=gen) < 0.4).float()]
    if T > 64:
        pats += [(ar >= 64).float(), (ar == 63).float(), (ar == 64).float()]
    rows = []
    for i in range(n):
        if i < len(pats):
            rows.append(pats[i])
        elif i % 2:
            rows.append((ar < int(torch.randint(1, T + 1, (1,), generator=gen))).float())
        else:
            rows.append((torch.rand(T, generator=gen) < 0.7).float())
    return torch.stack(rows).to(torch.int32)


def make_ids(Un: int, N: int, gen: torch.Generator) -> torch.Tensor:
    """``[Un]`` int32 with duplicates, id 0 in the first slots, then ids 1 ... 11 (the mask patterns), the
    largest id N - 1 in the middle and last; with Un >= N every table title occurs."""
    ids = torch.randint(0, N, (Un,), generator=gen, dtype=torch.int32)
    if Un >= N:
        ids[torch.randperm(Un, generator=gen)[:N]] = torch.arange(N, dtype=torch.int32)
    ids[: min(Un, 3)] = 0
    n = min(11, N - 1, max(0, Un - 5))  # the titles that carry zoo_mask's patterns, where the slots allow
    ids[3:3 + n] = torch.arange(1, n + 1, dtype=torch.int32)
    if Un > 3:
        ids[Un // 2] = N - 1
        ids[Un - 1] = N - 1
    return ids


KINDS = ("plain", "wide", "shifted", "aligned")


def make_inputs(Un: int, T: int, D: int, Q: int, kind: str = "plain", masked: bool = False, seed: int = 0,
                device="cpu", gout: bool = True):
    """A dict of what the head consumes, drawn on the CPU (the same values wherever they are used):
    ``table`` bf16 [N T, D], ``ids`` int32 [Un], ``tokens`` int32 [N, 2, T] | None and ``keep`` bool
    [N, T], ``w1`` bf16 [Q, D], ``b1`` / ``w2`` [Q], ``b2`` [1], ``gout`` fp32 [Un, D].

    * plain: pre ~ N(0, 1); w2 is scaled x3 so that alpha is peaked (scores ~ N(0, 1.9^2));
    * wide: pre ~ N(0, 4^2): tanh saturates, 1 - e^2 reaches 0 and 2^-7;
    * shifted: plain with b2 = -20 (|b2| dominates the score's magnitude); the pools' shifted
      scores are made per title by ``shift_scores`` from the scores they are given;
    * aligned: plain with the sign of w2_q that of the bf16 rounding error of e_q in table row 0 (=
      row 0 of every set: ids start with 0): a score summed from the ROUNDED e is off by sum |w2|
      |e - bf16(e)| there, its worst case, where random signs hide it in the accumulation term."""
    assert kind in KINDS and supported(D, Q, T)
    N = N_TABLE
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * T + 31 * D + Q + 104729 * KINDS.index(kind))
    gu = torch.Generator().manual_seed(2000003 * seed + 15485863 * Un + T)
    table = torch.randn(N * T, D, generator=g).to(torch.bfloat16)
    w1 = (torch.randn(Q, D, generator=g) / math.sqrt(D) * (4.0 if kind == "wide" else 1.0)).to(torch.bfloat16)
    b1 = torch.randn(Q, generator=g) * 0.1
    w2 = torch.randn(Q, generator=g) / math.sqrt(Q) * 3
    b2 = torch.randn(1, generator=g)
    if kind == "shifted":
        b2 = b2 * 0 - 20.0
    if kind == "aligned":
        ev = torch.tanh(table[0].double() @ w1.double().t() + b1.double())
        w2 = w2.abs() * torch.sign(ev.to(torch.bfloat16).double() - ev).float()
    keep = zoo_mask(N, T, g) if masked else torch.ones(N, T, dtype=torch.int32)
    tokens = torch.stack([keep * 7, keep], 1).contiguous() if masked else None
    ids = make_ids(Un, N, gu)
    gout = torch.randn(509, D, generator=g)[(torch.arange(Un if gout else 1) * 7) % 509].contiguous()
    d = dict(table=table, ids=ids, tokens=tokens, keep=keep.bool(), w1=w1, b1=b1, w2=w2, b2=b2, gout=gout)
    return {k: (v if v is None else v.to(device)) for k, v in d.items()}


def gather(table, ids, T: int) -> torch.Tensor:
    """The cache rows by title index: ``[Un, T, D]`` (in the table's type)."""
    return table.view(-1, T, table.shape[1])[ids.long()]


def title_keep(keep, ids) -> torch.Tensor:
    return keep[ids.long()]


SHIFTS = ("eps", "high", "low", "none")


def shift_scores(a, keep):
    """The shifted set of the pools, from scores ``a`` fp32 [Un, T] and ``keep`` bool [Un, T]: title u
    takes ``SHIFTS[u % 4]`` -- eps: moved so that sum keep exp(a) = 1e-8 (scores near -20; the eps
    term carries half of the denominator); high: the maximum moved to +60 (the eps term vanishes);
    low: the maximum moved to -100 (``__expf(-m)`` overflows: alpha about 0); none: as given."""
    ad = a.double().masked_fill(~keep, -math.inf)
    m = ad.amax(1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    lse = m + torch.log(torch.exp(ad - m).sum(1, keepdim=True).clamp(min=1e-300))
    cls = (torch.arange(a.shape[0], device=a.device) % 4).view(-1, 1)
    s = torch.where(cls == 0, math.log(1e-8) - lse, torch.where(cls == 1, 60.0 - m, torch.where(cls == 2, -100.0 - m, 0.0 * m)))
    return (a.double() + s).float().contiguous()


def cycle_rows(rows: int, cols: int, table_rows: int, seed: int, scale: float = 1.0, device="cpu") -> torch.Tensor:
    """``[rows, cols]`` fp32: a ``table_rows`` x cols N(0, scale^2) table cycled with stride 7 (neighbouring
    rows differ and a large row count costs nothing to draw)."""
    g = torch.Generator().manual_seed(seed)
    t = (torch.randn(table_rows, cols, generator=g) * scale).to(device)
    return t[(torch.arange(rows, device=device) * 7) % table_rows]


def make_wgrad_g_inputs(Un: int, T: int, D: int, nreal=None, device="cpu"):
    """``head_wgrad_g``'s operands drawn directly: make_inputs' table / ids / w2 (Q = 384) plus ``G`` bf16
    [Un T, Q] ~ N(0, 0.1^2), ``cs`` fp32 [2, Un, Q] ~ N(0, 1), ``db2p`` fp32 [Un] -- nonzero in the rows of
    padded titles too (they must add nothing), except db2p, which the pool backward zeroes there."""
    d = make_inputs(Un, T, D, 384, seed=5, device=device, gout=False)
    d["G"] = cycle_rows(Un * T, 384, 509, 11, 0.1, device).to(torch.bfloat16)
    d["cs"] = cycle_rows(2 * Un, 384, 509, 12, 1.0, device).view(2, Un, 384).contiguous()
    d["db2p"] = cycle_rows(Un, 1, 1021, 13, 1.0, device).reshape(-1).contiguous()
    if nreal is not None:
        d["db2p"][nreal:] = 0.0
    return d


def make_wgrad_inputs(Un: int, T: int, D: int, Q: int, nreal=None, device="cpu"):
    """The round-4 ``head_wgrad``'s operands drawn directly: ``e`` = bf16(tanh N(0, 1.5^2)) [Un T, Q] (saturated
    values included), ``da`` fp32 [Un T] ~ N(0, 0.05^2), ``db2p`` as above."""
    d = make_inputs(Un, T, D, Q, seed=6, device=device, gout=False)
    d["e"] = torch.tanh(cycle_rows(Un * T, Q, 509, 21, 1.5, device)).to(torch.bfloat16)
    d["da"] = cycle_rows(Un * T, 1, 1021, 22, 0.05, device).reshape(-1).contiguous()
    d["db2p"] = cycle_rows(Un, 1, 1021, 23, 1.0, device).reshape(-1).contiguous()
    if nreal is not None:
        d["db2p"][nreal:] = 0.0
    return d


# ------------------------------------------------------------------------------------ oracles
def score_oracle(x, w1, b1, w2, b2):
    """fp64 ``dict(e, tol_e, a, tol_a)`` of ``head_score`` for the rows ``x`` [M, D] bf16."""
    D, Q = x.shape[1], w1.shape[0]
    xd, wd, bd, w2d = x.double(), w1.double(), b1.double(), w2.double().reshape(-1)
    pre = xd @ wd.t() + bd
    S = xd.abs() @ wd.abs().t() + bd.abs()
    del xd, wd
    e_acc = S.mul_((D + 2) * U)  # D adds in the MFMAs + b1 + 1 spare
    e = torch.tanh(pre)
    del pre
    # carried by tanh' = 1 - tanh^2 <= 1 - e^2 + 2 e_acc anywhere within e_acc of pre (and <= 1)
    e32 = e_acc * (1.0 - e * e + 2.0 * e_acc).clamp_(max=1.0)
    e32 += EPS["tanh_fast"]  # tanh_fast
    tol_e = e.abs() * UB + (1 + UB) * e32 + TINY  # the bf16 store rounds the computed value
    a = e @ w2d + b2.double().reshape(())
    mag = e.abs() @ w2d.abs() + b2.double().abs().reshape(())
    tol_a = e32 @ w2d.abs() + (Q + 2) * U * mag + TINY  # the fp32 tanh values; Q products-and-adds, b2, 1 spare
    return dict(e=e, tol_e=tol_e, a=a, tol_a=tol_a)


def _ex(x):
    return EPS["expf"] * x.abs().clamp(min=1.0) + U * x.abs()


def pool_oracle(x, a, keep=None):
    """fp64 ``dict(alpha, tol_alpha, pooled, tol_pooled)`` of ``head_pool``: ``x`` [Un, T, D] bf16 (the
    gathered rows), ``a`` fp32 [Un, T] (exact), ``keep`` bool [Un, T] | None."""
    Un, T, D = x.shape
    ad = a.double().view(Un, T)
    kp = torch.ones_like(ad, dtype=torch.bool) if keep is None else keep
    p = torch.exp(ad) * kp
    den = p.sum(1, keepdim=True) + 1e-8
    alpha = p / den  # the definition, unshifted
    m = ad.masked_fill(~kp, -math.inf).amax(1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    ext = _ex(ad - m) * kp  # a_t - m rounds once, then __expf
    w8 = 1e-8 / den  # the eps term's share of the denominator = 1 - sum alpha
    dent = (alpha * ext).sum(1, keepdim=True) + w8 * (_ex(m) + 2 * U)  # __expf(-m), the constant 1e-8f, their product
    tol_alpha = alpha * (ext + dent + (T + 5) * U) + TINY  # T + 2 adds; reciprocal, product, 1 spare; the floor
    ax = x.double().abs()
    xd = x.double()
    pooled = torch.einsum("ut,utd->ud", alpha, xd)
    tol_pooled = (T + 2) * U * torch.einsum("ut,utd->ud", alpha, ax) + torch.einsum("ut,utd->ud", tol_alpha, ax) + TINY
    return dict(alpha=alpha, tol_alpha=tol_alpha, pooled=pooled, tol_pooled=tol_pooled)


def pool_bwd_oracle(x, alpha, g):
    """fp64 ``dict(da, tol_da, db2p, tol_db2p)``: ``x`` [Un, T, D] bf16, ``alpha`` fp32 [Un, T] (the pool's
    output, exact), ``g`` fp32 [Un, D]."""
    Un, T, D = x.shape
    xd, gd, al = x.double(), g.double(), alpha.double().view(Un, T)
    dalpha = torch.einsum("ud,utd->ut", gd, xd)
    A = torch.einsum("ud,utd->ut", gd.abs(), xd.abs())
    del xd
    B = (al * A).sum(1, keepdim=True)
    sm = (al * dalpha).sum(1, keepdim=True)
    da = al * (dalpha - sm)
    tol_da = al * ((D + 2) * U * A + (D + T + 4) * U * B + 3 * U * (A + B)) + TINY
    db2p = da.sum(1)
    tol_db2p = tol_da.sum(1) + (T + 2) * U * (al * (A + B)).sum(1)
    return dict(da=da, tol_da=tol_da, db2p=db2p, tol_db2p=tol_db2p)


def g_oracle(da, e, T: int):
    """fp64 ``dict(g, tol_g, cs0, tol_cs0)`` of the rewrite of ``head_pool_bwd_g``: ``da`` fp32 [M] (the
    kernel's own, exact), ``e`` bf16 [M, Q] as given.  ``cs[1]`` is judged by ``cs1_oracle``."""
    dad, ed = da.double().view(-1, 1), e.double()
    Q = e.shape[1]
    g = dad * (1.0 - ed * ed)
    tol_g = g.abs() * (UB + 3 * U) + TINY
    t = dad * ed
    cs0 = t.view(-1, T, Q).sum(1)
    tol_cs0 = (T + 2) * U * t.abs().view(-1, T, Q).sum(1) + TINY
    return dict(g=g, tol_g=tol_g, cs0=cs0, tol_cs0=tol_cs0)


def cs1_oracle(g_stored, T: int):
    """``(ref, tol)`` fp64 [titles, Q] of ``cs[1]`` from the bf16 g the same launch stored."""
    gd = g_stored.double().view(-1, T, g_stored.shape[1])
    return gd.sum(1), (T + 2) * U * gd.abs().sum(1) + TINY


def _small_sums(cs, w2, db2p, R: int, Un: int, S: int, tp: int):
    w2d = w2.double().reshape(-1)
    c = cs.double()[:, :R]
    dw2, tol_dw2 = c[0].sum(0), (tp + S + 2) * U * c[0].abs().sum(0) + TINY
    db1, tol_db1 = w2d * c[1].sum(0), (tp + S + 3) * U * w2d.abs() * c[1].abs().sum(0) + TINY
    return dict(dw2=dw2, tol_dw2=tol_dw2, db1=db1, tol_db1=tol_db1, **_db2(db2p, Un, S))


def _db2(db2p, Un: int, S: int):
    d = db2p.double().reshape(-1)[:Un]
    return dict(db2=d.sum().reshape(1), tol_db2=((Un + S + 2) * U * d.abs().sum() + TINY).reshape(1))


def wgrad_g_oracle(x, G, cs, w2, db2p, T: int, R: int, S: int, tps: int):
    """fp64 ``dict(dW1, db1, dw2, db2 and tol_*)`` of ``head_wgrad_g``: ``x`` [Un T, D'] bf16 (the gathered
    rows, or a column slice of them), ``G`` bf16 [Un T, Q], ``cs`` fp32 [2, Un, Q], ``db2p`` [>= Un];
    R real titles, the launcher's S splits of ``tps`` titles.  With R = 0 every value and bound but db2's
    is 0 (+ TINY)."""
    Un = x.shape[0] // T
    n = R * T
    _, tp = wgrad_g_resplit(Un, R, S, tps)
    xd, gd, w2d = x[:n].double(), G[:n].double(), w2.double().reshape(-1, 1)
    dW1 = w2d * (gd.t() @ xd)
    tol = (tp * T + S + 3) * U * w2d.abs() * (gd.abs().t() @ xd.abs()) + TINY
    return dict(dW1=dW1, tol_dW1=tol, **_small_sums(cs, w2, db2p, R, Un, S, tp))


def wgrad_oracle(x, e, da, w2, db2p, T: int, R: int, S: int, mchunk: int):
    """fp64 outputs and bounds of the round-4 ``head_wgrad``: ``e`` bf16 [Un T, Q], ``da`` fp32 [Un T]; the
    launcher's S splits of ``mchunk`` rows."""
    Un = x.shape[0] // T
    n = R * T
    _, mc = wgrad_resplit(Un * T, T, R, S, mchunk)
    xd, ed, dad, w2d = x[:n].double(), e[:n].double(), da.double().reshape(-1)[:n].view(-1, 1), w2.double().reshape(-1)
    g = dad * (1.0 - ed * ed)
    rel = UB + (mc + S + 6) * U  # g rounded to bf16 in LDS (UB + 3 U), then mc + S adds, w2, 1 spare
    dW1 = w2d.view(-1, 1) * (g.t() @ xd)
    tol_dW1 = rel * w2d.abs().view(-1, 1) * (g.abs().t() @ xd.abs()) + TINY
    db1, tol_db1 = w2d * g.sum(0), rel * w2d.abs() * g.abs().sum(0) + TINY
    t = dad * ed
    dw2, tol_dw2 = t.sum(0), (mc + S + 2) * U * t.abs().sum(0) + TINY
    return dict(dW1=dW1, tol_dW1=tol_dW1, db1=db1, tol_db1=tol_db1, dw2=dw2, tol_dw2=tol_dw2, **_db2(db2p, Un, S))


# ------------------------------------------------------------------------------------ judging
def worst_ratio(cand, ref, tol) -> float:
    return go.worst_ratio(cand.reshape(ref.shape), ref, tol)


def describe(cand, ref, tol, T: int = 0, tile: int = 0) -> str:
    """The worst element; with ``T`` the leading index is a token row: its title slot, token, 32-row
    stage and (with the score's row ``tile``) its block, row in the block and 16 x 16 fragment."""
    cand = cand.reshape(ref.shape)
    r = go.elem_ratio(cand, ref, tol)
    k = int(r.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(k), ref.shape))
    s = ("worst element %s: ratio %.4g (got %.9g, want %.9g, bound %.3g); %d of %d elements above 1"
         % (idx, float(r[idx]), float(cand[idx]), float(ref[idx]), float(tol[idx]), int((r > 1).sum()), r.numel()))
    if T:
        i = idx[0]
        s += "; row %d = title slot %d, token %d, 32-row stage %d" % (i, i // T, i % T, i // WTM)
        if tile:
            s += ", block %d row %d, fragment (%d, %d)" % (i // tile, i % tile, i % tile // 16, (idx[1] if len(idx) > 1 else 0) // 16)
    return s


def check(cand, ref, tol, what: str = "", T: int = 0, tile: int = 0) -> float:
    """Assert the worst ratio <= 1 over every element (the message names the worst one); returns it."""
    assert cand.numel() == ref.numel(), (what, cand.shape, ref.shape)
    w = worst_ratio(cand, ref, tol)
    if not w <= 1.0:
        raise AssertionError("%s: %s" % (what, describe(cand, ref, tol, T, tile)))
    return w


# ------------------------------------------------------------------------------------ the GPU cases
# Every list is built from the CU count alone, so tests/test_head_oracle_cpu.py can run its rounding
# model over the input sets of tests/test_head_oracle_gpu.py (at NOMINAL_CUS).
DQ = [(256, 128), (512, 256), (768, 384), (1024, 384), (256, 384)]


def score_cases(cus: int):
    """``(Un, T, D, Q, kind, forced rows, nreal | None)``.  T = 1: every row its own title (the gather is
    per row) with Un at tile - 1 / tile / tile + 1 of every row tile and one row; D = 256 ... 1024: 4
    to 16 k-tiles; at D = 768 titles of 17 / 50 / 128 rows straddle the tile seams; the wide and
    shifted sets; nreal 1 / Un - 37 / Un; the walk: CUs + 1 blocks (the grid's second round)."""
    c = []
    for D, Q in DQ:
        tiles = (160, 192) if Q == 384 else (128,)
        for n in sorted({1} | {t + d for t in tiles for d in (-1, 0, 1)}):
            for f in ((160, 192, 0) if Q == 384 and D == 768 else (0,)):
                c.append((n, 1, D, Q, "plain", f, None))
    c += [(23, 17, 768, 384, "plain", f, None) for f in (160, 192, 0)]
    c += [(9, 50, 768, 384, k, 0, None) for k in ("plain", "wide", "shifted")]
    c += [(9, 50, D, 384, "aligned", 0, None) for D in (256, 768)]
    c += [(4, 128, 768, 384, "plain", f, None) for f in (160, 192)]
    c += [(5, 96, 1024, 384, "wide", 0, None), (6, 50, 512, 256, "wide", 0, None), (6, 50, 256, 128, "shifted", 0, None),
          (5, 128, 512, 384, "plain", 0, None)]
    for Un, T, D, Q in ((60, 17, 768, 384), (60, 17, 256, 128)):
        c += [(Un, T, D, Q, "plain", 0, r) for r in (1, Un - 37, Un)]
    c += [(cus * 192 + 1, 1, 256, 384, "plain", f, None) for f in (192, 0)]  # the walk
    return c


def pool_cases():
    """``(Un, T, D, kind, masked, nreal | None)``; kind "shifted" = ``shift_scores`` of the plain scores.
    Every tpt dispatch (13 / 16 / 32) at each D, T = 1 / 63 / 64 / 65 / 127 / 128 with the masks of
    tokens >= 64, TG = 12 (D = 256) to 3 (D = 1024), padded titles."""
    c = []
    for D, Ts in ((768, (1, 52, 53, 63, 64, 65, 127, 128)), (1024, (1, 39, 40, 48, 49, 96)), (256, (1, 50, 65, 128)),
                  (512, (50, 78, 79, 96, 97, 128))):
        for T in Ts:
            c += [(40, T, D, "plain", False, None), (40, T, D, "shifted", True, None)]
    c += [(40, 50, 768, "wide", True, None), (40, 128, 768, "shifted", False, None), (40, 50, 768, "shifted", False, None)]
    c += [(60, 50, 768, "plain", True, r) for r in (1, 23, 60)] + [(60, 65, 1024, "shifted", True, 23)]
    return c


def pool_bwd_cases():
    """``(Un, T, D, kind, nreal | None)`` for ``head_pool_bwd`` / ``head_pool_bwd_g`` (Q = 384 where the G path
    exists: D % 128 == 0): tpw 9 / 11 / 22 at T = 54 / 55, 66 / 67, 128; etp 7 / 8 / 16 at T = 56 / 57,
    64 / 65, 128; T = 1; D = 1024 (both 64-lane column chunks live) and D = 256 (the second dead)."""
    c = [(24, T, 768, "plain", None) for T in (1, 54, 55, 56, 57, 64, 65, 66, 67, 128)]
    c += [(24, T, 768, "wide", None) for T in (50, 128)]
    c += [(24, T, 1024, "plain", None) for T in (1, 55, 96)] + [(24, T, 256, "wide", None) for T in (1, 57, 128)]
    c += [(24, 50, 512, "plain", None)]
    c += [(60, 50, 768, "plain", r) for r in (1, 23, 60)]
    return c


def wgrad_g_cases(cus: int):
    """``(Un, T, D, nreal | None)`` for ``head_wgrad_g`` (Q = 384): Un around the split count S = CUs / (D /
    128), titles smaller and larger than the 32-row stage with a part-filled last stage, nreal 0 /
    1 / Un - 37 / Un, and the cap: T = 1 with tps clamped at MAX_SPLIT_TITLES - 2."""
    c = []
    S = max(1, cus // 6)
    for Un in (1, S - 1, S, S + 1, 2 * S + 1):
        c += [(Un, T, 768, None) for T in (1, 17, 33)]
    c += [(2 * S + 1, T, 768, None) for T in (32, 50, 128)]
    c += [(3 * max(1, cus // 2) + 2, 50, 256, None), (2 * max(1, cus // 8) + 1, 96, 1024, None)]
    Un = 2 * S + 40
    c += [(Un, T, 768, r) for T in (17, 50) for r in (0, 1, Un - 37, Un)]
    c += [(S * (MAX_SPLIT_TITLES - 2) + 1, 1, 768, None)]  # the cap
    return c


def wgrad_cases(cus: int):
    """``(Un, T, D, Q, nreal | None)`` for the round-4 ``head_wgrad``: M <= 256 (S = 1), M no multiple of 32,
    seams inside titles, nreal, and the ``mchunk > cap`` clamp at T = 1 and T = 3 with the smallest tile
    grid (Q = 128, D = 256: S = CUs)."""
    c = [(5, 50, 256, 128, None), (3, 17, 512, 256, None), (1, 1, 768, 384, None), (7, 33, 768, 384, None)]
    c += [(77, 50, D, Q, None) for D, Q in ((256, 128), (512, 256), (768, 384), (512, 128))]
    c += [(300, 17, 256, 128, None), (41, 128, 768, 384, None)]
    c += [(120, 50, D, Q, r) for D, Q in ((256, 128), (768, 384)) for r in (0, 1, 120 - 37, 120)]
    for T in (1, 3):
        cap = (MAX_SPLIT_TITLES - 2) * T // WTM * WTM
        c.append(((cus * cap) // T + 40, T, 256, 128, None))  # mchunk > cap: clamped, S grows past the CU count
    return c
