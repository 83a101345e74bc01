"""Byzantine-robust aggregation rule (``cfg.robust_agg``): the coordinate-wise trimmed mean or
median of the clients' vectors (Yin et al. 2018) in place of the mean.

A mean moves by 1/W of whatever one client sends, and a NaN from one client reaches every
coordinate of everybody.  The trimmed mean drops, per coordinate, the ``trim`` lowest and ``trim``
highest of the W values before it averages (NaN ranks highest: up to ``trim`` NaN clients are cut);
the median is the largest trim a given W allows.  The rule needs every client's individual vector:
the drivers all-gather where the mean all-reduced (:meth:`RobustRule.gather_combine_`), or stack the
uploads on the coordinator.  The arithmetic is :func:`ops.trimmed_mean` -- the HIP kernel on device
stacks, the torch oracle on the host -- so every client that combines the same stack holds the same
bits.

``multi_krum`` (Blanchard et al. 2017) judges a client by its whole vector instead: a sign-flipped,
scaled or colluding update lies inside the honest spread at every single coordinate and still far from
everybody as a vector.  Each client is scored by the sum of its squared distances to its ``W - f - 2``
nearest peers (``f = robust_trim``, the assumed number of Byzantine clients; ``W >= 2 f + 3``), the
``robust_keep`` best-scored clients (0: ``W - f``; 1: plain Krum) are kept and averaged.  The distances
come from the Gram matrix of the rows centred on their coordinate-wise median (:func:`ops.krum_gram`,
:func:`ops.krum_select`, :func:`ops.krum_mean`: csrc/krum.hip on the device); ``dropped[c]`` is ``n`` for
a client that was not kept and 0 for one that was, so its ``dropped_share`` reads 1.0.

``geomed`` is the geometric median of the clients' vectors (RFA: Pillutla, Kakade, Harchaoui 2022), the
point with the least sum of distances to them: breakdown point 1/2 with no ``f`` to guess, defined for
every ``W >= 1`` (``robust_trim`` and ``robust_keep`` are ignored), and a soft re-weighting ``sum_c a_c x_c``
with ``a_c`` proportional to ``1 / ||x_c - z||`` -- an honest client that is merely far counts less instead of
not at all.  Weiszfeld's iteration runs on the same centred Gram matrix (:func:`ops.geomed_weights`, 32 rounds in
``W`` dimensions, no pass over the stack per round), :func:`ops.geomed_combine` takes the weighted sum
(csrc/geomed.hip on the device).  A client whose row is not finite gets weight 0 and ``dropped[c] = n``; the
record gains ``agg_weight``, the last aggregation's weights.
"""
from __future__ import annotations

from typing import List, Sequence

import torch
from torch._utils import _flatten_dense_tensors, _unflatten_dense_tensors

from .. import ops
from . import comm

KINDS = ("none", "trimmed_mean", "median", "multi_krum", "geomed")


class RobustRule:
    def __init__(self, kind: str = "none", trim: int = 1, keep: int = 0):
        if kind not in KINDS:
            raise ValueError(f"robust_agg={kind!r}: expected {' | '.join(KINDS)}")
        if kind in ("trimmed_mean", "multi_krum") and int(trim) < 0:
            raise ValueError(f"robust_trim={trim}: must be >= 0")
        if kind == "multi_krum" and int(keep) < 0:
            raise ValueError(f"robust_keep={keep}: must be >= 0")
        self.kind, self.trim, self.keep = kind, int(trim), int(keep)
        self.weights = None  # geomed: a [W] fp64 of the last aggregation

    @classmethod
    def from_cfg(cls, cfg, driver: str = "") -> "RobustRule":
        """The rule of ``cfg``; an active rule is rejected where it cannot hold (``driver``: the
        federation driver that asks)."""
        rule = cls(cfg.robust_agg, cfg.robust_trim, cfg.robust_keep)
        if rule.active:
            if cfg.secagg.enabled:
                raise ValueError(f"robust_agg={cfg.robust_agg} cannot be combined with secagg.enabled=1: under secure "
                                 "aggregation nobody sees an individual update, and the rule ranks them")
            if cfg.weighted_fedavg:
                raise ValueError(f"robust_agg={cfg.robust_agg} cannot be combined with weighted_fedavg=1: the rule is "
                                 "unweighted")
            if driver == "grad_avg":
                raise ValueError(f"robust_agg={cfg.robust_agg} is not available with mode=grad_avg: the gradient "
                                 "all-reduce runs inside the captured step (use param_avg or fedavg_star)")
        return rule

    @property
    def active(self) -> bool:
        return self.kind != "none"

    def trim_for(self, W: int) -> int:
        """Values cut on each side among ``W`` clients; raises where the rule leaves nothing."""
        W = int(W)
        if self.kind == "multi_krum":  # f Byzantine clients assumed; Krum's guarantee needs W >= 2 f + 3
            if W < 2 * self.trim + 3 or not 0 <= self.keep <= W - self.trim:
                raise ValueError(f"robust_agg=multi_krum with robust_trim={self.trim}, robust_keep={self.keep} needs "
                                 f"at least {2 * self.trim + 3} clients and robust_keep <= clients - robust_trim "
                                 f"(got {W})")
            return self.trim
        if self.kind == "geomed":
            if W < 1:
                raise ValueError(f"robust_agg=geomed needs at least 1 client (got {W})")
            return 0
        trim = (W - 1) // 2 if self.kind == "median" else self.trim
        if W < 1 or 2 * trim >= W:
            raise ValueError(f"robust_agg={self.kind} with robust_trim={trim} needs more than {2 * trim} clients "
                             f"(got {W})")
        return trim

    def combine(self, stack: torch.Tensor):
        """``stack [W, n]`` fp32 -> ``(out [n], dropped [W] int64)`` on the stack's device."""
        if self.kind == "multi_krum":
            stack = stack.contiguous()
            sel = self._krum_select(self._krum_gram(stack), stack.shape[0])
            return ops.krum_mean(stack, sel), self._krum_dropped(sel, stack.shape[1])
        if self.kind == "geomed":
            stack = stack.contiguous()
            self.trim_for(stack.shape[0])
            return self._geomed_combine(stack, self._geomed_weights(self._krum_gram(stack)))
        return ops.trimmed_mean(stack.contiguous(), self.trim_for(stack.shape[0]))

    # multi-Krum in pieces (a multi-bucket gather adds the buckets' Gram matrices before it selects)
    def _krum_gram(self, stack: torch.Tensor) -> torch.Tensor:
        center, _ = ops.trimmed_mean(stack, (stack.shape[0] - 1) // 2)  # the coordinate-wise median
        return ops.krum_gram(stack, center)

    def _krum_select(self, G: torch.Tensor, W: int) -> torch.Tensor:
        f = self.trim_for(W)
        return ops.krum_select(G, f, self.keep or W - f)[0]

    @staticmethod
    def _krum_dropped(sel: torch.Tensor, n: int) -> torch.Tensor:
        return (sel == 0).to(torch.int64) * int(n)

    # the geometric median in pieces (the Gram matrix as multi-Krum's; weights: (a, invalid) of one aggregation)
    def _geomed_weights(self, G: torch.Tensor):
        a, dist = ops.geomed_weights(G)
        self.weights = a
        return a, torch.isinf(dist).to(torch.int64)

    @staticmethod
    def _geomed_combine(stack: torch.Tensor, weights):
        return ops.geomed_combine(stack, weights[0]), weights[1] * int(stack.shape[1])

    def gather_combine_(self, tensors: Sequence[torch.Tensor], group, W: int,
                        bucket_bytes: int = comm.BUCKET_BYTES) -> torch.Tensor:
        """In place: every tensor becomes the rule's aggregate of the group's W copies of it.  The
        tensors travel flattened in ~28 MB buckets, one all-gather into a ``[W, len]`` stack each; at
        most one bucket's stack exists at a time.  Returns the summed ``dropped [W]`` (int64, host).

        ``multi_krum`` selects on whole vectors, so with more than one bucket it makes two passes and
        moves every byte TWICE: pass 1 gathers each bucket and adds the buckets' Gram matrices in bucket
        order (fp64, on the stack's device), one select follows, pass 2 gathers each bucket again and
        averages the selected rows.  A single bucket is gathered once.  ``geomed`` weighs whole vectors and
        takes the same two passes: one :func:`ops.geomed_weights` on the summed Gram matrix, then every bucket
        combined with those weights."""
        self.trim_for(W)  # before the first collective: every member raises alike
        dropped = torch.zeros(W, dtype=torch.int64)
        buckets = list(comm._buckets(list(tensors), bucket_bytes))
        sel = wts = None
        if self.kind in ("multi_krum", "geomed") and len(buckets) > 1:
            G = None
            for b in buckets:
                stack = comm.allgather_stack(_flatten_dense_tensors(b).float(), group, W)
                g = self._krum_gram(stack)
                del stack
                G = g if G is None else G + g
            if self.kind == "geomed":
                wts = self._geomed_weights(G)
            else:
                sel = self._krum_select(G, W)
        for b in buckets:
            one = len(b) == 1 and b[0].is_contiguous()
            flat = b[0].reshape(-1) if one else _flatten_dense_tensors(b)
            stack = comm.allgather_stack(flat.float(), group, W)
            if sel is not None:
                out, d = ops.krum_mean(stack, sel), self._krum_dropped(sel, stack.shape[1])
            else:
                out, d = self._geomed_combine(stack, wts) if wts is not None else self.combine(stack)
            del stack
            dropped += d.cpu()
            if one:
                b[0].copy_(out.view_as(b[0]))
            else:
                for t, s in zip(b, _unflatten_dense_tensors(out, b)):
                    t.copy_(s)
        return dropped

    def record(self, dropped, n: int, W: int) -> dict:
        """The keys a round / epoch record gains: ``dropped_share[c]`` is the fraction of the ``n``
        aggregated coordinates at which client ``c`` was cut (an honest client sits near
        ``2 trim / W``, a poisoned one near 1; under multi_krum 0 for a kept client, 1 for one left out).
        ``geomed`` adds ``agg_weight``: the last aggregation's weight of every client (they sum to 1)."""
        share: List[float] = [float(x) / max(int(n), 1) for x in dropped]
        rec = {"robust_agg": self.kind, "robust_trim": self.trim_for(W), "dropped_share": share}
        if self.kind == "geomed" and self.weights is not None:
            rec["agg_weight"] = [float(x) for x in self.weights.cpu()]
        return rec
