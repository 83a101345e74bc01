"""The form of a star client's upload, chosen once per run (:meth:`StarUpload.from_cfg`): the dense fp32 model
(under the robust rule of parallel/robust.py, when one is set), the top-k list of parallel/sparsify.py, the
quantised codes of parallel/quantize.py (of the rotated delta: parallel/rotate.py), the sign bits of parallel/sign.py, the
low-rank factors of parallel/lowrank.py or the count sketch of parallel/sketch.py -- one interface, so that the star drivers hold one path for all six.  ``bind(flat_params)``, once
after the model is built, gives a codec the layout of the flat buffer (the low-rank and the sketch codec need it).
With ``upload_index=ef`` the three forms that carry an index list are wrapped by parallel/index_code.py, which codes that list.

``compress(local, theta_g, residual, client, round)`` makes the payload (the flat model, ``(idx, val)``, an ``Upload``),
``finite`` tells whether a coordinator may take it, ``pack`` / ``unpack(blob, n)`` are its wire tensor (``unpack``
validates: ``ValueError``), ``combine(base, payloads, weights)`` the aggregate in client order -> ``(new, dropped or
None)``, ``received(base, payload)`` one client's model as far as its upload tells.  The arithmetic is ``ops.*``: HIP
kernels on device tensors, torch oracles on the host, one bitwise contract -- the coordinator (host) and clients that
combine among themselves (device) hold the same bits.  Secure aggregation is a protocol, not a payload: parallel/secagg.py.
"""
from __future__ import annotations

import torch

from .. import ops
from . import comm
from .control import encode_tensor
from .dist import data_ipc
from .robust import RobustRule
from .sparsify import Sparsifier


class StarUpload:
    uses_residual = True  # the driver keeps an fp32 error-feedback residual (checkpointed as UPLOAD_RESIDUAL)
    options: dict = {}  # the option keys of this form in a round record
    rule = RobustRule()  # (inactive: the dense codec holds the run's)
    # the low-rank codec's per-matrix basis, the sketch codec's error table, the rotated quantiser's residual
    # (checkpointed as UPLOAD_BASIS); None on the others
    basis = None

    @staticmethod
    def from_cfg(cfg, driver: str) -> "StarUpload":
        """The codec of ``cfg``; every option is rejected where it cannot hold (``driver``: the federation
        driver that asks).  Outside the star only the dense codec's ``rule`` means anything."""
        from .index_code import IndexCoded  # (StarUploads themselves: these modules import this one)
        from .lowrank import LowRank
        from .quantize import Quantizer
        from .rotate import RotatedQuantizer
        from .sign import SignUpload
        from .sketch import SketchUpload
        coded = IndexCoded.check_cfg(cfg, driver)
        rule = RobustRule.from_cfg(cfg, driver)
        sparse = Sparsifier.from_cfg(cfg, driver)
        quant = Quantizer.from_cfg(cfg, driver)
        rot = RotatedQuantizer.from_cfg(cfg, driver)
        low = LowRank.from_cfg(cfg, driver)
        sketch = SketchUpload.from_cfg(cfg, driver)
        sign = SignUpload.from_cfg(cfg, driver)
        if sign.active:
            return IndexCoded(sign) if coded else sign
        if sketch.active:
            return sketch
        if low.active:
            return low
        if rot.active:
            return rot
        if coded:  # (with upload_topk > 0: check_cfg)
            return IndexCoded(quant if quant.active else TopkUpload(sparse))
        return quant if quant.active else TopkUpload(sparse) if sparse.active else DenseUpload(rule)

    def bind(self, flat_params) -> "StarUpload":
        """Called once with the model's ``FlatParams``: a codec that needs the layout plans here."""
        return self

    def state(self):
        """What a coordinator's snapshot keeps of this codec between the rounds (a dict for its extras), or None."""
        return None

    def load(self, st) -> None:
        """Take back what :meth:`state` gave (``st``: the snapshot's extras)."""

    def check_clients(self, W: int) -> None:
        """``ValueError`` where ``W`` payloads are too few to combine."""
        if self.rule.active:
            self.rule.trim_for(W)

    def combine_among(self, payload, weight: float, ctx, base: torch.Tensor, timeout_s: float):
        """All-gather the clients' packed payloads and weights, validate every row, combine: the same bits on each."""
        blob = self.pack(payload)
        word = torch.tensor([weight], dtype=torch.float32, device=blob.device).view(torch.int32)
        both = comm.allgather_stack(torch.cat([blob.reshape(-1), word]), ctx.data_group, ctx.num_clients)
        ups = []
        for c in range(ctx.num_clients):
            try:
                ups.append(self.unpack(both[c, :-1].view(blob.shape), base.numel()))
            except ValueError as e:
                raise RuntimeError(f"client {c}: {e}")
        return self.combine(base, ups, both[:, -1].contiguous().view(torch.float32))

    def meta(self, payload, blob: bytes = None) -> dict:
        """``blob``: the encoded upload where the client has sent one."""
        return {"upload_bytes": len(encode_tensor(self.pack(payload)) if blob is None else blob)}

    def record(self, n: int, metas, dropped=None) -> dict:
        """The form's options, and the bytes the accepted clients sent against the dense form."""
        return {**self.options, "upload_bytes": sum(int(m.get("upload_bytes", 0)) for m in metas), "dense_bytes": 4 * int(n) * len(metas)}


class DenseUpload(StarUpload):
    """The flat model as it is; ``combine`` is the mean of the reference (``server.py:46-50``; weighted with
    ``weighted_fedavg``) or the robust rule's aggregate, and ``dropped`` the rule's cut counts."""
    uses_residual = False

    def __init__(self, rule: RobustRule):
        self.rule = rule

    def compress(self, local, theta_g, residual, client, round_idx):
        return local

    def finite(self, up) -> bool:
        return bool(torch.isfinite(up).all())

    def pack(self, up):
        return up

    def unpack(self, blob, n):
        return blob

    def received(self, base, up):
        return up

    def combine(self, base, ups, weights):
        if self.rule.active:
            return self.rule.combine(torch.stack([t.float() for t in ups]))
        acc = torch.zeros_like(ups[0], dtype=torch.float64)
        for t, w in zip(ups, weights):
            acc += t.double() * w
        return (acc / sum(weights)).float(), None

    def combine_among(self, up, weight, ctx, base, timeout_s):
        """In place.  The rule gathers (every client combines the same stack); the mean stays an all-reduce."""
        if self.rule.active:
            return up, self.rule.gather_combine_([up], ctx.data_group, ctx.num_clients)
        wt = torch.tensor([weight], device=up.device, dtype=torch.float32)
        up.mul_(wt)
        ipc = data_ipc(ctx, timeout_s) if ctx.device.type == "cuda" else None
        comm.allreduce_([up, wt], ctx.data_group, ipc=ipc)
        if ipc is not None:
            ipc.check()
        return up.div_(wt), None

    def meta(self, up, blob=None):
        return {}

    def record(self, n, metas, dropped=None):
        return self.rule.record(dropped, n, len(metas)) if dropped is not None else {}


class TopkUpload(StarUpload):
    """``(idx, val)`` of a :class:`Sparsifier`."""

    def __init__(self, sparse: Sparsifier):
        self.sparse, self.options = sparse, {"upload_topk": sparse.fraction}

    def compress(self, local, theta_g, residual, client, round_idx):
        return self.sparse.compress(local, theta_g, residual)

    def finite(self, up) -> bool:
        return bool(torch.isfinite(up[1]).all())

    def pack(self, up):
        return Sparsifier.pack(*up)

    def unpack(self, blob, n):
        return Sparsifier.unpack(blob, n, self.sparse.k_for(n))

    def words_for(self, n: int) -> int:
        """int32 words of a packed upload."""
        return 2 * self.sparse.k_for(n)

    def received(self, base, up):
        out = base.detach().clone()
        out[up[0].long()] += up[1]
        return out

    def combine(self, base, ups, weights):
        w = weights if isinstance(weights, torch.Tensor) else torch.tensor([float(x) for x in weights], dtype=torch.float32,
                                                                              device=base.device)
        return ops.sparse_combine(base.contiguous(), torch.stack([u[0] for u in ups]).contiguous(),
                                  torch.stack([u[1] for u in ups]).contiguous(), w), None

    def meta(self, up, blob=None):
        return {"upload_k": int(up[0].numel()), **super().meta(up, blob)}
