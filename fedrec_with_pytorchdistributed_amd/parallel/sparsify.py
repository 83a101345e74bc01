"""Top-k sparsified uploads with error feedback (``cfg.upload_topk``) for the star topology.

A star client uploads its whole flat trainable buffer every round.  With ``upload_topk = F`` it
sends only the ``k = max(1, ceil(F n))`` largest-magnitude coordinates of ``(theta_k - theta_g) +
residual`` and keeps the rest as its residual, which joins the next round's delta (Stich et al.
2018; Lin et al. 2018): nothing is lost, only delayed, and the upload is ``8 k`` bytes instead of
``4 n``.  The aggregate is ``theta_g + (sum_c w_c scatter(idx_c, val_c)) / sum_c w_c``.

The arithmetic is :func:`ops.topk_delta` and :func:`ops.sparse_combine` -- the HIP kernels on
device tensors, the torch oracles on the host, one bitwise contract -- so the coordinator (host)
and clients that combine among themselves (device) hold the same bits.
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import torch

from .. import ops
from ..ops import reference as ref
from . import comm


class Sparsifier:
    def __init__(self, fraction: float = 0.0):
        f = float(fraction)
        if not (0.0 <= f <= 1.0):  # (NaN fails here too)
            raise ValueError(f"upload_topk={fraction}: expected 0 <= upload_topk <= 1")
        self.fraction = f

    @classmethod
    def from_cfg(cls, cfg, driver: str = "") -> "Sparsifier":
        """The sparsifier of ``cfg``; an active one is rejected where it cannot hold (``driver``: the
        federation driver that asks)."""
        sp = cls(cfg.upload_topk)
        if sp.active:
            if driver != "fedavg_star":
                raise ValueError(f"upload_topk={cfg.upload_topk} is not available with mode={driver}: only the star "
                                 "clients upload a model; sparsified gradient or parameter averaging is out of scope "
                                 "(use fedavg_star)")
            if cfg.secagg.enabled:
                raise ValueError(f"upload_topk={cfg.upload_topk} cannot be combined with secagg.enabled=1: masked sums "
                                 "need dense vectors aligned over the clients, and each client picks its own coordinates")
            if cfg.robust_agg != "none":
                raise ValueError(f"upload_topk={cfg.upload_topk} cannot be combined with robust_agg={cfg.robust_agg}: "
                                 "the rule ranks dense stacks of every client's value per coordinate")
        return sp

    @property
    def active(self) -> bool:
        return self.fraction > 0.0

    def k_for(self, n: int) -> int:
        """Coordinates sent out of ``n``."""
        return min(int(n), max(1, int(math.ceil(self.fraction * int(n)))))

    # ---- client ------------------------------------------------------------------------------
    def compress(self, local: torch.Tensor, theta_g: torch.Tensor, residual: torch.Tensor):
        """``(idx [k] int32 ascending, val [k] fp32)`` of this round; ``residual`` is updated in place."""
        return ops.topk_delta(local.contiguous(), theta_g.contiguous(), residual, self.k_for(local.numel()))

    @staticmethod
    def pack(idx: torch.Tensor, val: torch.Tensor) -> torch.Tensor:
        """One int32 ``[2, k]`` tensor: ``idx``, then the bits of ``val``."""
        return torch.stack([idx, val.view(torch.int32)])

    @staticmethod
    def unpack(blob: torch.Tensor, n: int, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(idx, val)`` of a packed upload, validated (:func:`ops.reference.sparse_upload_check`);
        ``ValueError`` names what is wrong with it."""
        if blob.dtype != torch.int32 or blob.dim() != 2 or blob.shape[0] != 2:
            raise ValueError(f"sparse upload: expected an int32 [2, {k}] tensor (got {blob.dtype} "
                             f"{tuple(blob.shape)})")
        idx, val = blob[0].contiguous(), blob[1].contiguous().view(torch.float32)
        ref.sparse_upload_check(idx, val, n, k)
        return idx, val

    def gather(self, idx: torch.Tensor, val: torch.Tensor, weight: float, group, W: int, n: int):
        """All-gather the group's W lists and weights -> ``(idx [W, k], val [W, k], weights [W])``, every
        list validated: each member ends up with the same three tensors."""
        k = idx.numel()
        mine = torch.cat([self.pack(idx, val).reshape(-1),
                          torch.tensor([weight], dtype=torch.float32, device=idx.device).view(torch.int32)])
        both = comm.allgather_stack(mine, group, W)
        lists = both[:, :2 * k].reshape(W, 2, k)
        for c in range(W):
            try:
                self.unpack(lists[c], n, k)
            except ValueError as e:
                raise RuntimeError(f"client {c}: {e}")
        return (lists[:, 0].contiguous(), lists[:, 1].contiguous().view(torch.float32),
                both[:, 2 * k].contiguous().view(torch.float32))

    # ---- aggregation -------------------------------------------------------------------------
    @staticmethod
    def combine(base: torch.Tensor, idxs: Sequence[torch.Tensor], vals: Sequence[torch.Tensor],
                weights: Sequence[float]) -> torch.Tensor:
        """``base + (sum_c w_c scatter(idx_c, val_c)) / sum_c w_c`` on ``base``'s device."""
        w = torch.tensor([float(x) for x in weights], dtype=torch.float32, device=base.device)
        return ops.sparse_combine(base.contiguous(), torch.stack(list(idxs)).contiguous(),
                                  torch.stack(list(vals)).contiguous(), w)

    @staticmethod
    def scatter(base: torch.Tensor, idx: torch.Tensor, val: torch.Tensor) -> torch.Tensor:
        """``base`` plus one client's sparse delta (that client's model as the coordinator sees it)."""
        out = base.detach().clone()
        out[idx.long()] += val
        return out

    def record(self, n: int, upload_bytes: List[int]) -> dict:
        """The keys a round record gains: the bytes the accepted clients sent against the dense form."""
        return {"upload_topk": self.fraction, "upload_bytes": int(sum(upload_bytes)),
                "dense_bytes": 4 * int(n) * len(upload_bytes)}
