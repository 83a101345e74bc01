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
"""
from __future__ import annotations

from typing import List, Sequence

import torch
from torch._utils import _flatten_dense_tensors, _unflatten_dense_tensors

from .. import ops
from . import comm

KINDS = ("none", "trimmed_mean", "median")


class RobustRule:
    def __init__(self, kind: str = "none", trim: int = 1):
        if kind not in KINDS:
            raise ValueError(f"robust_agg={kind!r}: expected {' | '.join(KINDS)}")
        if kind == "trimmed_mean" and int(trim) < 0:
            raise ValueError(f"robust_trim={trim}: must be >= 0")
        self.kind, self.trim = kind, int(trim)

    @classmethod
    def from_cfg(cls, cfg, driver: str = "") -> "RobustRule":
        """The rule of ``cfg``; an active rule is rejected where it cannot hold (``driver``: the
        federation driver that asks)."""
        rule = cls(cfg.robust_agg, cfg.robust_trim)
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
        trim = (W - 1) // 2 if self.kind == "median" else self.trim
        if W < 1 or 2 * trim >= W:
            raise ValueError(f"robust_agg={self.kind} with robust_trim={trim} needs more than {2 * trim} clients "
                             f"(got {W})")
        return trim

    def combine(self, stack: torch.Tensor):
        """``stack [W, n]`` fp32 -> ``(out [n], dropped [W] int64)`` on the stack's device."""
        return ops.trimmed_mean(stack.contiguous(), self.trim_for(stack.shape[0]))

    def gather_combine_(self, tensors: Sequence[torch.Tensor], group, W: int,
                        bucket_bytes: int = comm.BUCKET_BYTES) -> torch.Tensor:
        """In place: every tensor becomes the rule's aggregate of the group's W copies of it.  The
        tensors travel flattened in ~28 MB buckets, one all-gather into a ``[W, len]`` stack each; at
        most one bucket's stack exists at a time.  Returns the summed ``dropped [W]`` (int64, host)."""
        self.trim_for(W)  # before the first collective: every member raises alike
        dropped = torch.zeros(W, dtype=torch.int64)
        for b in comm._buckets(list(tensors), bucket_bytes):
            one = len(b) == 1 and b[0].is_contiguous()
            flat = b[0].reshape(-1) if one else _flatten_dense_tensors(b)
            stack = comm.allgather_stack(flat.float(), group, W)
            out, d = self.combine(stack)
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
        ``2 trim / W``, a poisoned one near 1)."""
        share: List[float] = [float(x) / max(int(n), 1) for x in dropped]
        return {"robust_agg": self.kind, "robust_trim": self.trim_for(W), "dropped_share": share}
