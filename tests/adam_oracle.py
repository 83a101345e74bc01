"""An fp64 Adam oracle that carries, per element, a bound on what an fp32 implementation of
the same operation may differ by (a plain helper module for the Adam tests, not a conftest).

The operation (``torch.optim.Adam``: no weight decay, no amsgrad), with the REAL -- Python
double -- hyperparameters, the step count ``t`` and the gradient scale ``gs``::

    x = g * gs;  m = b1 m + (1 - b1) x;  v = b2 v + (1 - b2) x^2
    den = sqrt(v) / sqrt(1 - b2^t) + eps;  upd = lr / (1 - b1^t) * m / den;  p -= upd

The inputs (p0, g, and m0 / v0 when given) are fp32 values taken as exact.  An fp32
implementation rounds every scalar it is handed once and every arithmetic result once, each
with a relative error of at most u = 2^-24 (round to nearest; a fused multiply-add only drops
a rounding).  Counting those roundings gives the bounds below; second-order terms (u^2) are
covered by the spare unit in each count.

First moment.  ``x`` carries 2u (the rounding of ``gs`` and the product ``g * gs``); the new
term ``(1 - b1) x`` adds the rounding of ``1 - b1`` and its multiply: 4u of ``(1 - b1)|x|``.
The old term ``b1 m`` carries the rounding of ``b1`` and its multiply: 2u of ``b1 |m|``, plus
``b1`` times the error m already had.  The add rounds the sum: u.  m can cancel (a gradient
that flips sign), so the magnitudes are bounded by the cancellation-free recurrence
``ma = b1 ma + (1 - b1)|x| >= |m|``, not by ``|m|``::

    ma = b1 ma + (1 - b1) |x|
    em = b1 em + 6u ma                      # |m_fp32 - m| <= em     (5 counted + 1 spare)

Second moment.  The same with ``x`` used twice (4u) -- every term is non-negative, so ``v``
is its own magnitude::

    ev = b2 ev + 9u v                       # |v_fp32 - v| <= ev     (4 + 2 + 2 counted + 1)

The step.  ``sqrt(v)`` inherits the relative error ``ev / (2 v)`` of v (0 where v = 0: then
v_fp32 = 0 too), and ``den >= sqrt(v) / sqrt(bc2)``, so that is also a bound on the relative
error it causes in ``den`` and in ``upd``.  The error of m enters as ``(lr / bc1) em / den``.
The roundings: ``bc1``, ``bc2``, ``lr`` (3), ``lr / bc1`` (1), ``1 / sqrt(bc2)`` (its square
root and its divide, 2; halved by the square root, counted whole), ``sqrt(v)`` (1), the
multiply by ``1 / sqrt(bc2)`` and the add of ``eps`` with eps's own rounding (3), the
multiply ``step_size * m`` and the divide by ``den`` (2): 12 counted, 14 taken.  The final
``p - upd`` rounds to the stored p: u |p_new|::

    tol_step = |upd| (ev / (2 v) + 14u) + (lr / bc1) em / den + c u |p_new| + 1e-37

``c = 1`` where p starts at 0 (p is then of the size of the updates).  For a realistic p0
(|p| >> |upd|) use ``c = 2``: the rounding of p itself costs up to u |p| per step, so a run
from p0 ~ N(0, 1) legitimately sits at a ratio of about 1 on that term alone, and the bound
would then measure nothing but the luck of p's last bit.  p keeps the errors of earlier
steps (they propagate with factor 1), so the bound on p after several steps is the sum of
the steps' ``tol_step``.  1e-37 (about the smallest normal fp32) keeps the bound positive
where everything else is 0.

``ratios(p, m, v)`` returns the three maxima of |candidate - oracle| / bound: a candidate
passes when all three are <= 1.  Where a bound is exactly 0 (an element whose gradient was
always 0) the candidate must be exact: any difference there is an infinite ratio.
"""
import math

import torch

U = 2.0 ** -24

# the project's hyperparameters, and a second set with short memories and a large eps
HPARAMS = [dict(lr=5e-5, b1=0.9, b2=0.999, eps=1e-8), dict(lr=1e-3, b1=0.8, b2=0.95, eps=1e-6)]


def grad_stream(n: int, steps: int, seed: int = 1234):
    """The test gradients: fp32 CPU tensors, one per step.  Per element and step
    g = randn * 10^U(-9, 2) (eleven decades: v spans twenty-two, on either side of eps);
    every 17th element is exactly 0 on every step (m, v, p must not move); every third step is
    the negation of the step before it (m cancels)."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for i in range(steps):
        if i % 3 == 2:
            out.append(-out[-1])
            continue
        g = torch.randn(n, generator=gen, dtype=torch.float64)
        g = g * 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 11.0 - 9.0)
        g[::17] = 0.0
        out.append(g.float())
    return out


def _ratio(cand: torch.Tensor, want: torch.Tensor, bound: torch.Tensor) -> float:
    d = (cand.detach().double().cpu().reshape(-1) - want).abs()
    if not bool(torch.isfinite(d).all()):
        return math.inf
    r = torch.where(d == 0, torch.zeros_like(d), d / bound)  # 0 / 0 = exact; d / 0 = inf
    return float(r.max()) if r.numel() else 0.0


class AdamOracle:
    """fp64 Adam state (``p``, ``m``, ``v``) and the fp32 error bounds (``ep``, ``em``, ``ev``)."""

    def __init__(self, p0: torch.Tensor, lr: float, b1: float, b2: float, eps: float, grad_scale: float = 1.0,
                 c: float = 2.0, m0: torch.Tensor = None, v0: torch.Tensor = None):
        self.lr, self.b1, self.b2, self.eps, self.gs, self.c = lr, b1, b2, eps, grad_scale, c
        self.p = p0.detach().double().cpu().reshape(-1).clone()
        z = torch.zeros_like(self.p)
        self.m = z.clone() if m0 is None else m0.detach().double().cpu().reshape(-1).clone()
        self.v = z.clone() if v0 is None else v0.detach().double().cpu().reshape(-1).clone()
        self.ma = self.m.abs()  # exact fp32 inputs: no error yet, but m0 can be cancelled from
        self.em, self.ev, self.ep = z.clone(), z.clone(), z.clone()

    def step(self, g: torch.Tensor, t: int) -> None:
        lr, b1, b2, eps = self.lr, self.b1, self.b2, self.eps
        x = g.detach().double().cpu().reshape(-1) * self.gs
        self.m = b1 * self.m + (1 - b1) * x
        self.v = b2 * self.v + (1 - b2) * x * x
        self.ma = b1 * self.ma + (1 - b1) * x.abs()
        self.em = b1 * self.em + 6 * U * self.ma
        self.ev = b2 * self.ev + 9 * U * self.v
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        den = self.v.sqrt() / math.sqrt(bc2) + eps
        upd = lr / bc1 * self.m / den
        self.p = self.p - upd
        relv = torch.where(self.v > 0, self.ev / (2 * self.v), torch.zeros_like(self.v))
        tol = upd.abs() * (relv + 14 * U) + (lr / bc1) * self.em / den + self.c * U * self.p.abs() + 1e-37
        self.ep = self.ep + tol

    def ratios(self, p: torch.Tensor, m: torch.Tensor, v: torch.Tensor):
        """(ratio m, ratio v, ratio step): max |candidate - oracle| / bound, each <= 1 to pass."""
        return _ratio(m, self.m, self.em), _ratio(v, self.v, self.ev), _ratio(p, self.p, self.ep)
