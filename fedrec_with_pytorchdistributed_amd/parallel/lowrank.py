"""Low-rank uploads with error feedback (``cfg.upload_rank``) for the star topology.

Top-k sends fewer coordinates and quantisation fewer bits per coordinate; both treat the model as one long row.
But almost all of the flat buffer is a handful of matrices, and with ``upload_rank = R`` (1, 2, 4 or 8) a star
client sends each matrix' round delta ``a = (theta_k - theta_g) + residual`` as rank-``R`` factors (PowerSGD:
Vogels, Karimireddy, Jaggi 2019): ``P = a Q``, ``P^ = orth(P)``, ``Q' = a^T P^``; the coordinator decodes ``d = P^
Q'^T``.  What the factors miss stays in the residual and joins the next round's delta (error feedback), and ``Q'``
is the next round's ``Q`` (warm start: one power-iteration step per round).  ``R (rows + cols)`` floats travel
instead of ``rows cols``; biases, vectors and the alignment padding ("rest") travel dense.

Which parameters are matrices, and the payload's layout, is the plan (:class:`ops.reference.LowRankPlan`), a pure
function of the flat layout and ``R``: :meth:`LowRank.bind` builds it on a client and on the coordinator alike.  The
decode and the aggregate are a bitwise contract between host and device (what the coordinator reconstructs is
exactly what the client subtracted from its residual: nothing is lost, only delayed); the two projections are
bounded by the dot-product error of their length.  The arithmetic is ``ops.lowrank_*``; :class:`LowRank` is a codec
of parallel/upload.py.
"""
from __future__ import annotations

import torch

from .. import ops
from ..ops import reference as ref
from .upload import StarUpload


class LowRank(StarUpload):  # (its payload: fp32 [plan.L])
    def __init__(self, rank: int = 0, seed: int = 0):
        if rank not in (0, *ref.LOWRANK_RANKS):
            raise ValueError(f"upload_rank={rank}: expected 0 (off), 1, 2, 4 or 8")
        self.rank, self.seed = int(rank), int(seed)
        self.options = {"upload_rank": self.rank}
        self.plan = None
        self.basis = None   # fp32 [plan.F] on the client's device: this round's Q of every matrix
        self._seen = (None, False)  # the last payload of compress and whether it is finite

    @classmethod
    def from_cfg(cls, cfg, driver: str = "") -> "LowRank":
        """The codec of ``cfg``; an active one is rejected where it cannot hold (``driver``: the federation driver
        that asks)."""
        lr = cls(cfg.upload_rank, cfg.seed)
        if lr.active:
            if driver != "fedavg_star":
                raise ValueError(f"upload_rank={cfg.upload_rank} is not available with mode={driver}: only the star "
                                 "clients upload a model; low-rank gradient or parameter averaging is out of scope "
                                 "(use fedavg_star)")
            if cfg.secagg.enabled:
                raise ValueError(f"upload_rank={cfg.upload_rank} cannot be combined with secagg.enabled=1: masked sums "
                                 "add the clients' values coordinate by coordinate, and factors of different bases do not add")
            if cfg.robust_agg != "none":
                raise ValueError(f"upload_rank={cfg.upload_rank} cannot be combined with robust_agg={cfg.robust_agg}: "
                                 "the rule ranks dense fp32 stacks of every client's value per coordinate")
            if cfg.upload_topk:
                raise ValueError(f"upload_rank={cfg.upload_rank} cannot be combined with upload_topk={cfg.upload_topk}: "
                                 "sparsified factors are out of scope, and one residual cannot serve two compressors")
            if cfg.upload_bits:
                raise ValueError(f"upload_rank={cfg.upload_rank} cannot be combined with upload_bits={cfg.upload_bits}: "
                                 "quantised factors are out of scope, and one residual cannot serve two compressors")
        return lr

    @property
    def active(self) -> bool:
        return self.rank != 0

    def bind(self, flat_params) -> "LowRank":
        """The plan of ``flat_params``' layout and the round-1 basis on its device."""
        self.plan = ref.LowRankPlan([(off, tuple(p.shape)) for _, p, off in flat_params.views()],
                                    flat_params.flat.numel(), self.rank)
        self.basis = self.plan.initial_basis(self.seed).to(flat_params.flat.device)
        return self

    def _plan(self):
        if self.plan is None:
            raise RuntimeError("low-rank upload: bind(flat_params) has not been called")
        return self.plan

    # ---- client ------------------------------------------------------------------------------
    def compress(self, local, theta_g, residual, client, round_idx):
        """This round's payload; ``residual`` is updated in place.  The basis moves on to ``Q'`` only when the
        payload is finite (a non-finite one is sent as it is and rejected; the driver zeroes the residual)."""
        plan = self._plan()
        pay = ops.lowrank_compress(local.contiguous(), theta_g.contiguous(), residual, self.basis, plan)
        ok = bool(torch.isfinite(pay).all())
        self._seen = (pay, ok)
        if ok:
            self.basis = pay[:plan.F].clone()
        return pay

    def finite(self, up) -> bool:
        return self._seen[1] if up is self._seen[0] else bool(torch.isfinite(up).all())

    def pack(self, up):
        """One int32 1-D tensor: the payload's bits."""
        return up.view(torch.int32)

    def unpack(self, blob, n):
        plan = self._plan()
        if blob.dtype != torch.int32 or blob.dim() != 1 or blob.numel() != plan.L or int(n) != plan.n:
            raise ValueError(f"low-rank upload: expected an int32 [{plan.L}] tensor for a model of {plan.n} (got "
                             f"{blob.dtype} {tuple(blob.shape)} for {n})")
        return blob.contiguous().view(torch.float32)

    # ---- aggregation -------------------------------------------------------------------------
    def combine(self, base, ups, weights):
        """``(base + (sum_c w_c d_c) / sum_c w_c, None)`` on ``base``'s device, in the order of ``ups``."""
        w = weights if isinstance(weights, torch.Tensor) else torch.tensor([float(x) for x in weights], dtype=torch.float32,
                                                                              device=base.device)
        return ops.lowrank_combine(base.contiguous(), torch.stack(list(ups)).contiguous(), w, self._plan()), None

    def received(self, base, up):
        """``base`` plus one client's decoded delta (that client's model as the coordinator sees it)."""
        return ops.lowrank_combine(base.detach().contiguous(), up.reshape(1, -1).contiguous(),
                                   torch.ones(1, dtype=torch.float32, device=base.device), self._plan())
