"""An fp64 oracle of the title self-attention that carries, per output element, a bound on what
the HIP kernels may differ by (a plain helper module for the attention tests, not a conftest).

The operation (``ops.reference.title_attention``, head dim 64, ``keep_s`` = mask of key s, Z the
Philox dropout multipliers or 1), per (title, head), query t, key s::

    score_ts = q_t . k_s / 8 ;  P = softmax_s(score, masked keys at finfo.min) ;  P~ = P o Z
    o_t = sum_s P~_ts v_s
    dP~ = (dO V^T) o Z ;  D_t = sum_s P_ts dP~_ts ;  dS_ts = keep_s P_ts (dP~_ts - D_t) / 8
    dQ = dS K ;  dK = dS^T Q ;  dV = P~^T dO

The values come from ``ops.reference.title_attention`` run in fp64 on the CPU, and fp64 autograd
through it, with the bf16 inputs taken as exact.  The intermediates above are also formed
explicitly (``AttnOracle(..., keep=True)`` keeps them; a CPU test holds the explicit gradients
to autograd): the bounds need magnitudes, not only values.

Roundings.  ``ub = 2^-8`` is the unit roundoff of bf16, ``u = 2^-24`` of fp32, both round to
nearest.  Every count below is first order; one spare unit per count covers the u^2 terms.
Magnitudes are cancellation-free wherever a rounding acts on a partial sum:

    sabs_ts = sum_d |q_td| |k_sd| / 8  >= |score_ts| ;    smax_t = max over kept s of sabs_ts
    G_ts    = Z_ts sum_d |dO_td| |v_sd| >= |dP~_ts| ;     Gbar_t = sum_s P_ts G_ts >= |D_t|
    MdS_ts  = keep_s P_ts (G_ts + Gbar_t) / 8 >= |dS_ts|   (the cancellation in dP~ - D is bounded
                                                            by |dP| + sum P |dP|, not by the difference)

``max_s |score_ts|`` of the usual statement of such a bound is taken as ``smax_t``: a 64-term
fp32 dot product errs by up to 64 u sabs, which |score| itself does not bound.

The probabilities (all kernels).  The products of two bf16 values are exact in fp32, so a
64-term dot product makes 64 roundings: ``|d score_ts| <= 64 u sabs_ts``, and the scale 1/8 is
exact.  ``x = score - m`` rounds once (u |x|), ``__expf(x)`` rounds ``x log2(e)`` and log2(e)
itself (2 u |x|) and the hardware exp2 is good to one ulp (2 u); |x| <= 2 smax; an absolute
error d in the argument is a relative error d in the result.  The running maximum m cancels
between numerator and denominator.  So ``e_s = exp(score_s - m)`` has the relative error

    eps_e = u (64 smax + 6 smax + 2) = u (70 smax + 2)

MFMA kernels, T <= 64 (title_attn.hip, title_attn_bwd.hip).  ``l = sum_s e_s`` is 16 adds in a
lane and 2 across lanes (18 u) on top of eps_e; ``1 / l`` is good to one ulp (2 u); ``e * inv``
rounds (u); the dropout multiplier is one more product and the kernel's ``1 / (1 - p)`` may be
one ulp from the oracle's (3 u, counted with or without dropout)::

    eps_P = 2 eps_e + (18 + 2 + 1 + 3) u = u (140 smax + 28)        taken: u (140 smax + 29)

P~ is rounded to bf16 (ub |P~|), the 64-term P~.V dot product rounds 64 times, and the output
is rounded to bf16 *from the computed value* (hence the factor 1 + ub on the inner error)::

    A_td    = sum_s |P~_ts| |v_sd|
    E_o     = ub A_td + (eps_P_t + 65 u) A_td                        (64 counted + 1 spare)
    tol_out = ub |o_td| + (1 + ub) E_o + tiny

i.e. ``ub (|o| + A) + c32 u (1 + smax) A`` with c32 = 140 (and 94 for the constant part), plus
the second-order ub^2 A.  Backward.  ``dP~`` is a 64-term dot product and a product with Z
(64 u + 3 u of G); D adds a product and 18 adds to that and to eps_P: ``|dD| <= Gbar (eps_P +
86 u)``; the subtraction rounds (u (G + Gbar)); the two products with P (eps_P + u) and u; keep
and 1/8 are exact::

    |d dS_ts| <= MdS_ts c_dS_t ,   c_dS_t = 2 eps_P_t + 88 u        taken: 2 eps_P_t + 89 u

dS and P~ are rounded to bf16, the three products are 64-term dot products (zero rows pad the
tiles), the outputs are rounded to bf16::

    E_dQ_td = (ub + 65 u) sum_s |dS_ts| |k_sd| + sum_s MdS_ts c_dS_t |k_sd|
    E_dK_sd = (ub + 65 u) sum_t |dS_ts| |q_td| + sum_t MdS_ts c_dS_t |q_td|
    E_dV_sd = (ub + 65 u) sum_t |P~_ts| |dO_td| + sum_t |P~_ts| eps_P_t |dO_td|
    tol_x   = ub |x| + (1 + ub) E_x + tiny

Long kernels, T > 64 (title_attn_long.hip): fp32 on the VALU throughout, online softmax over
nch = ceil(T / 64) key chunks; the only bf16 rounding is the output.  Forward: l and the
accumulator are rescaled by the same ``alpha`` per chunk (its own error cancels; its product
rounds, nch u each); l takes T adds, the accumulator T products and T adds; ``1 / l`` (2 u) and
the product with it (u)::

    tol_out = ub |o| + (1 + ub) u (2 (70 smax + 2) + 3 T + 2 nch + 3) A     taken: ... + 4

Backward.  (m, l) are recomputed with ``l = l alpha + l_chunk``: here alpha's error stays
(u (6 smax + 2)), with its product and add (2 u), per chunk; a chunk sum is 64 adds;
``A_ts = e_s / l``: 2 u + u::

    eps_A = 2 eps_e + 64 u + nch u (6 smax + 4) + 3 u = u ((140 + 6 nch) smax + 71 + 4 nch)
                                                             taken: ... + 72 + 4 nch

D_t sums T terms A dA (dA: 64 u of G; product u; T adds): ``|dD| <= Gbar (eps_A + (66 + T) u)``.
``dQ = (U - D W) / 8`` with U = sum A dA k (a term: eps_A + 64 u + 3 u, T adds), W = sum A k
(eps_A + (1 + T) u), the product D W and the subtraction (2 u); dK sums T terms
A (dA - D) q (eps_A + 64 u + 4 u, T adds, and D's error); dV sums T terms A dO (a product, an
add)::

    c_dS  = 2 eps_A + (2 T + 136) u                                  taken: ... + 137
    E_dQ  = sum_s MdS_ts c_dS_t |k_sd| ;   E_dK = sum_t MdS_ts c_dS_t |q_td|
    E_dV  = sum_t P_ts (eps_A_t + (T + 3) u) |dO_td|                 (T + 2 counted)
    tol_x = ub |x| + (1 + ub) E_x + tiny

``tiny`` = 1e-30 keeps the bound positive; where everything else is 0 (dQ and dK of an
all-masked title: dS is exactly 0) any non-zero candidate is a ratio far above 1.

``ratios`` returns, per output, max |candidate - oracle| / bound **per (title, head)**: a
candidate passes when every pair's ratio is <= 1.
"""
import math

import torch

from fedrec_with_pytorchdistributed_amd.ops import reference as ref

UB = 2.0 ** -8
U = 2.0 ** -24
TINY = 1e-30
DH = 64
FMIN = torch.finfo(torch.float32).min

# (seed, offset) of the dropout cases: the project's usual draw, and one with the high words of
# both (Philox k1, c3) non-zero
DROP_SEEDS = [(4242, 3), (0x123456789ABC, 2 ** 33 + 5)]
P_DROP = [0.1, 0.5]
WALK_DROPS = [(0.1,) + DROP_SEEDS[0], (0.5,) + DROP_SEEDS[1]]  # (p, seed, offset) of the walk cases
NOMINAL_CUS = 256  # what the CPU tests size the walk cases by (the GPU tests ask the device)


# ------------------------------------------------------------------------------------ inputs
def zoo_mask(n: int, T: int, gen: torch.Generator) -> torch.Tensor:
    """``[n, T]`` int32: one title per pattern, then random ones (alternately a random prefix
    and random keys at 0.7).  Title 1 is all masked in every set."""
    ar = torch.arange(T)
    pats = [torch.ones(T), torch.zeros(T), (ar == 0).float(), (ar == T - 1).float(), (ar != 0).float(),
            (ar % 2 == 0).float(), (ar < int(torch.randint(1, T + 1, (1,), generator=gen))).float(),
            (torch.rand(T, generator=gen) < 0.4).float()]
    if T > 64:
        pats.append((ar >= 64).float())  # the whole first chunk masked
        if T >= 192:
            pats.append(((ar < 64) | (ar >= 128)).float())  # a whole middle chunk masked
        pats[3] = (ar == T - 1).float()  # only the last key kept: every chunk but the last masked
    rows = []
    for i in range(n):
        if i < len(pats):
            rows.append(pats[i])
        elif i % 2:
            rows.append((ar < int(torch.randint(1, T + 1, (1,), generator=gen))).float())
        else:
            rows.append((torch.rand(T, generator=gen) < 0.7).float())
    return torch.stack(rows).to(torch.int32)


def n_patterns(T: int) -> int:
    return 8 + (T > 64) + (T >= 192)


def make_inputs(n: int, H: int, T: int, qscale: float = 1.0, seed: int = 0):
    """(qkv bf16 [n*T, 3D], mask int32 [n, T], dout bf16 [n*T, D]) on the CPU."""
    D = H * DH
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * n + 31 * T + H)
    qkv = torch.randn(n * T, 3 * D, generator=g)
    qkv[:, :D] *= qscale
    dout = torch.randn(n * T, D, generator=g)
    mask = zoo_mask(n, T, g)
    return qkv.to(torch.bfloat16), mask, dout.to(torch.bfloat16)


def walk_titles(cus: int, H: int, blocks_per_cu: int = 1) -> int:
    """n with 12 * blocks < n * H < 16 * blocks for a persistent grid of ``blocks`` 4-wave blocks:
    every wave walks 3 or 4 (title, head) pairs and the last stride is part-filled."""
    blocks = cus * blocks_per_cu
    n = (14 * blocks) // H + 1
    assert 12 * blocks < n * H < 16 * blocks, (cus, H, n)
    return n


# The input sets of the GPU tests, by name -> (n, H, T, qscale).  tests/test_attn_oracle_cpu.py
# runs its rounding model over every one of them, so the bound is checked where it is used.
T_SHORT = [1, 15, 16, 17, 31, 32, 33, 48, 50, 63, 64]
T_DROP = [1, 17, 32, 50, 64]
T_PACKED = [1, 16, 17, 50, 64]
T_LONG = [65, 127, 128, 129, 200, 512]
SHAPES = [(12, 12), (11, 5)]  # (n, H): 144 pairs, and 55 (odd: the last block is part-filled)
WALK_T = 33


def small_cases():
    return [(n, H, T, qs) for (n, H) in SHAPES for T in T_SHORT for qs in (1.0, 4.0)]


def drop_cases():
    return [(n, H, T, 1.0) for (n, H) in SHAPES for T in T_DROP]


def packed_cases():
    return [(n, H, T, qs) for (n, H) in SHAPES for T in T_PACKED for qs in (1.0, 4.0)]


def long_cases():
    return [(n_patterns(T) + 2, 2, T, qs) for T in T_LONG for qs in (1.0, 4.0)] + [(n_patterns(130), 12, 130, 1.0)]


# ------------------------------------------------------------------------------------ oracle
def _heads(x: torch.Tensor, n: int, T: int, H: int) -> torch.Tensor:
    return x.reshape(n, T, H, DH).permute(0, 2, 1, 3)  # [n, H, T, 64]


def _rows(x: torch.Tensor) -> torch.Tensor:
    n, H, T, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(n * T, H * DH)


class AttnOracle:
    """fp64 values (``o`` [n*T, D]; ``dqkv`` [n*T, 3D] when ``dout`` is given) and their bounds
    (``tol_o``, ``tol_dqkv``).  ``drop = (p, seed, offset)``.  ``keep=True`` also keeps the
    explicit intermediates of the whole batch in ``self.x`` (small cases only)."""

    def __init__(self, qkv, mask, H: int, dout=None, drop=None, keep: bool = False):
        qkv = qkv.detach().cpu().double()
        mask = mask.detach().cpu()
        n, T = mask.shape
        D = H * DH
        assert qkv.shape == (n * T, 3 * D)
        self.n, self.H, self.T, self.D, self.long = n, H, T, D, T > 64
        assert drop is None or not self.long
        x = qkv.clone().requires_grad_(dout is not None)
        y = ref.title_attention(x, mask, H, drop)
        self.o = y.detach()
        self.dqkv = None
        if dout is not None:
            dout = dout.detach().cpu().double()
            y.backward(dout)
            self.dqkv = x.grad
        del x, y
        Z = None if drop is None else ref.attention_dropout_scale(n, H, T, *drop).double()
        step = max(1, (1 << 21) // (H * T * T))  # titles per slab: the [., H, T, T] tensors stay ~16 MB
        tol_o, tol_g, xs = [], [], []
        for a in range(0, n, step):
            b = min(n, a + step)
            t = self._slab(qkv[a * T:b * T], mask[a:b], None if dout is None else dout[a * T:b * T],
                           None if Z is None else Z[a:b], keep)
            tol_o.append(t[0])
            tol_g.append(t[1])
            xs.append(t[2])
        self.tol_o = torch.cat(tol_o)
        self.tol_dqkv = None if dout is None else torch.cat(tol_g)
        self.x = {k: torch.cat([d[k] for d in xs]) for k in xs[0]} if keep else None

    def _slab(self, qkv, mask, dout, Z, keep):
        n, T = mask.shape
        H, long = self.H, self.long
        q, k, v = qkv.view(n, T, 3, H, DH).permute(2, 0, 3, 1, 4)
        kp = (mask != 0).view(n, 1, 1, T)
        sc = q @ k.transpose(-1, -2) / 8.0
        sabs = q.abs() @ k.abs().transpose(-1, -2) / 8.0
        smax = sabs.masked_fill(~kp, 0.0).amax(-1, keepdim=True)
        P = torch.softmax(sc.masked_fill(~kp, FMIN), -1)
        Pt = P if Z is None else P * Z
        A = Pt.abs() @ v.abs()
        o = Pt @ v
        nch = (T + 63) // 64
        if long:
            eps_o = U * (140 * smax + 3 * T + 2 * nch + 8)
            eps_p = U * ((140 + 6 * nch) * smax + 72 + 4 * nch)
            E_o = eps_o * A
        else:
            eps_p = U * (140 * smax + 29)
            E_o = (UB + eps_p + 65 * U) * A
        tol_o = _rows(UB * o.abs() + (1 + UB) * E_o + TINY)
        x = dict(P=P, Pt=Pt, o=_rows(o)) if keep else {}
        if dout is None:
            return tol_o, None, x
        g = _heads(dout, n, T, H)
        dPt = g @ v.transpose(-1, -2)
        G = g.abs() @ v.abs().transpose(-1, -2)
        if Z is not None:
            dPt, G = dPt * Z, G * Z
        Dt = (P * dPt).sum(-1, keepdim=True)
        Gbar = (P * G).sum(-1, keepdim=True)
        kf = kp.double()
        dS = kf * P * (dPt - Dt) / 8.0
        MdS = kf * P * (G + Gbar) / 8.0
        dQ, dK, dV = dS @ k, dS.transpose(-1, -2) @ q, Pt.transpose(-1, -2) @ g
        if long:
            c_ds = 2 * eps_p + (2 * T + 137) * U
            E_q = (MdS * c_ds) @ k.abs()
            E_k = (MdS * c_ds).transpose(-1, -2) @ q.abs()
            E_v = (P * (eps_p + (T + 3) * U)).transpose(-1, -2) @ g.abs()
        else:
            c_ds = 2 * eps_p + 89 * U
            r = UB + 65 * U
            E_q = r * (dS.abs() @ k.abs()) + (MdS * c_ds) @ k.abs()
            E_k = r * (dS.abs().transpose(-1, -2) @ q.abs()) + (MdS * c_ds).transpose(-1, -2) @ q.abs()
            E_v = r * (Pt.abs().transpose(-1, -2) @ g.abs()) + (Pt.abs() * eps_p).transpose(-1, -2) @ g.abs()
        tol_g = torch.cat([_rows(UB * w.abs() + (1 + UB) * E + TINY) for w, E in ((dQ, E_q), (dK, E_k), (dV, E_v))], 1)
        if keep:
            x.update(dPt=dPt, D=Dt, dS=dS, dqkv=torch.cat([_rows(dQ), _rows(dK), _rows(dV)], 1))
        return tol_o, tol_g, x

    # --------------------------------------------------------------------------- comparing
    def ratios_fwd(self, out):
        """``{"out": [n, H]}``: per (title, head), max |out - o| / tol_out."""
        return {"out": ratios(out, self.o, self.tol_o, self.n, self.H)}

    def ratios_bwd(self, dqkv):
        """``{"dQ" | "dK" | "dV": [n, H]}``."""
        D = self.D
        c = dqkv.detach().double().cpu()
        return {name: ratios(c[:, i * D:(i + 1) * D], self.dqkv[:, i * D:(i + 1) * D],
                             self.tol_dqkv[:, i * D:(i + 1) * D], self.n, self.H)
                for i, name in enumerate(("dQ", "dK", "dV"))}

    def check_fwd(self, out, what: str = "") -> float:
        return self._check(self.ratios_fwd(out), {"out": (out, self.o, self.tol_o)}, what)

    def check_bwd(self, dqkv, what: str = "") -> float:
        D = self.D
        parts = {name: (dqkv[:, i * D:(i + 1) * D], self.dqkv[:, i * D:(i + 1) * D], self.tol_dqkv[:, i * D:(i + 1) * D])
                 for i, name in enumerate(("dQ", "dK", "dV"))}
        return self._check(self.ratios_bwd(dqkv), parts, what)

    def _check(self, rs, parts, what) -> float:
        """Assert every pair's ratio <= 1; the message names the worst element.  Returns the
        worst ratio (for the record)."""
        worst = 0.0
        for name, r in rs.items():
            w = float(r.max())
            if not w <= 1.0:
                raise AssertionError("%s %s: %s" % (what, name, describe_worst(*parts[name], self.n, self.H)))
            worst = max(worst, w)
        return worst


def _elem_ratio(cand, want, tol):
    d = (cand.detach().double().cpu() - want).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / tol)
    return torch.where(torch.isfinite(d), r, torch.full_like(r, math.inf))  # a NaN / inf candidate fails


def ratios(cand, want, tol, n: int, H: int) -> torch.Tensor:
    """``[n, H]``: per (title, head), the maximum over its [T, 64] block of
    |cand - want| / tol (``cand``, ``want``, ``tol``: ``[n*T, H*64]``)."""
    T = want.shape[0] // n
    return _elem_ratio(cand, want, tol).view(n, T, H, DH).amax((1, 3))


def describe_worst(cand, want, tol, n: int, H: int) -> str:
    T = want.shape[0] // n
    r = _elem_ratio(cand, want, tol).view(n, T, H, DH)
    i = int(r.argmax())
    title, t, h, d = i // (T * H * DH), i // (H * DH) % T, i // DH % H, i % DH
    row, col = title * T + t, h * DH + d
    bad = int((r.amax((1, 3)) > 1).sum())
    return ("worst (title %d, head %d, row %d, column %d): ratio %.3g (got %.6g, want %.6g, bound %.3g); "
            "%d of %d (title, head) pairs above 1" % (title, h, t, d, float(r.view(-1)[i]),
                                                     float(cand.detach().double().cpu()[row, col]),
                                                     float(want[row, col]), float(tol[row, col]), bad, n * H))
