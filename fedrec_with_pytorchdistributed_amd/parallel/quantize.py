"""Block-quantized uploads with error feedback (``cfg.upload_bits``) for the star topology.

A star client uploads fp32 for every coordinate it sends.  With ``upload_bits = B`` (8 or 4) it sends
``(theta_k - theta_g) + residual`` as stochastic ``B``-bit codes with one fp32 scale per 256 coordinates
(QSGD, Alistarh et al. 2017) and keeps the quantisation error as its residual, which joins the next
round's delta (error feedback: Stich et al. 2018; Karimireddy et al. 2019): ``4 ceil(n / 256) + n B / 8``
bytes instead of ``4 n``.  The aggregate is ``theta_g + (sum_c w_c d_c) / sum_c w_c`` with ``d_c`` the
dequantised delta.

With ``upload_topk = F`` as well, ``topk_delta`` selects ``k`` coordinates first and their values are
quantised as a list of their own (scale blocks over the list positions); the ``k`` quantisation errors
go back into the residual at the selected coordinates.  The upload is then ``4 k + 4 ceil(k / 256) + k B /
8`` bytes, and the aggregation dequantises each list and scatters it as the sparse path does.

The arithmetic is :func:`ops.quantize_delta` and :func:`ops.dequant_combine` -- the HIP kernels on device
tensors, the torch oracles on the host, one bitwise contract -- so the coordinator (host) and clients
that combine among themselves (device) hold the same bits.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

import torch

from .. import ops
from ..ops import reference as ref
from . import comm
from .sparsify import Sparsifier


class Upload(NamedTuple):
    idx: Optional[torch.Tensor]  # int32 [k] ascending (composed with upload_topk), else None
    codes: torch.Tensor          # uint8 [ceil(m bits / 8)], m = k or n
    scales: torch.Tensor         # fp32 [ceil(m / 256)]


class Quantizer:
    def __init__(self, bits: int = 0, seed: int = 0, fraction: float = 0.0):
        if bits not in (0, 8, 4):
            raise ValueError(f"upload_bits={bits}: expected 0 (off), 8 or 4")
        self.bits = int(bits)
        self.seed = int(seed)
        self.sparse = Sparsifier(fraction)

    @classmethod
    def from_cfg(cls, cfg, driver: str = "") -> "Quantizer":
        """The quantizer of ``cfg``; an active one is rejected where it cannot hold (``driver``: the
        federation driver that asks)."""
        qz = cls(cfg.upload_bits, cfg.seed, cfg.upload_topk)
        if qz.active:
            if driver != "fedavg_star":
                raise ValueError(f"upload_bits={cfg.upload_bits} is not available with mode={driver}: only the star "
                                 "clients upload a model; quantised gradient or parameter averaging is out of scope "
                                 "(use fedavg_star)")
            if cfg.secagg.enabled:
                raise ValueError(f"upload_bits={cfg.upload_bits} cannot be combined with secagg.enabled=1: masked sums "
                                 "need every client's values on one fixed-point grid, and each client scales its own blocks")
            if cfg.robust_agg != "none":
                raise ValueError(f"upload_bits={cfg.upload_bits} cannot be combined with robust_agg={cfg.robust_agg}: "
                                 "the rule ranks dense fp32 stacks of every client's value per coordinate")
        return qz

    @property
    def active(self) -> bool:
        return self.bits != 0

    def m_for(self, n: int) -> int:
        """Quantised values out of ``n`` coordinates: ``k`` when composed with top-k, else ``n``."""
        return self.sparse.k_for(n) if self.sparse.active else int(n)

    def words_for(self, n: int) -> int:
        """int32 words of a packed upload."""
        m = self.m_for(n)
        nbytes, nb = ref.quant_sizes(m, self.bits)
        return (m if self.sparse.active else 0) + nb + (nbytes + 3) // 4

    # ---- client ------------------------------------------------------------------------------
    def compress(self, local: torch.Tensor, theta_g: torch.Tensor, residual: torch.Tensor, client: int,
                 round_idx: int) -> Upload:
        """This round's upload; ``residual`` is updated in place.  The Philox key is the run's seed, the
        offset ``(client << 32) | round``: no two uploads of a run share a stream."""
        offset = (int(client) << 32) | int(round_idx)
        local, theta_g = local.contiguous(), theta_g.contiguous()
        if not self.sparse.active:
            return Upload(None, *ops.quantize_delta(local, theta_g, residual, self.bits, self.seed, offset))
        idx, val = self.sparse.compress(local, theta_g, residual)
        err = torch.zeros_like(val)
        codes, scales = ops.quantize_delta(val, torch.zeros_like(val), err, self.bits, self.seed, offset)
        residual[idx.long()] += err  # (+0.0 there since topk_delta sent them)
        return Upload(idx, codes, scales)

    @staticmethod
    def finite(up: Upload) -> bool:
        return bool(torch.isfinite(up.scales).all())

    @staticmethod
    def pack(up: Upload) -> torch.Tensor:
        """One int32 1-D tensor: ``idx`` (composed form only), the scales' bits, then the codes padded with
        zero bytes to a multiple of 4."""
        codes = up.codes
        pad = -codes.numel() % 4
        if pad:
            codes = torch.cat([codes, codes.new_zeros(pad)])
        parts = [up.scales.view(torch.int32), codes.view(torch.int32)]
        return torch.cat(parts if up.idx is None else [up.idx, *parts])

    def unpack(self, blob: torch.Tensor, n: int) -> Upload:
        """The parts of a packed upload, validated (:func:`ops.reference.quant_upload_check`, and
        :func:`ops.reference.sparse_upload_check` on the composed form's ``idx``); ``ValueError`` names what
        is wrong with it."""
        L = self.words_for(n)
        if blob.dtype != torch.int32 or blob.dim() != 1 or blob.numel() != L:
            raise ValueError(f"quantized upload: expected an int32 [{L}] tensor (got {blob.dtype} {tuple(blob.shape)})")
        m = self.m_for(n)
        nbytes, nb = ref.quant_sizes(m, self.bits)
        o = m if self.sparse.active else 0
        idx = blob[:o].contiguous() if self.sparse.active else None
        scales = blob[o:o + nb].contiguous().view(torch.float32)
        tail = blob[o + nb:].contiguous().view(torch.uint8)
        if bool(tail[nbytes:].any()):
            raise ValueError("quantized upload: the padding bytes after the codes are not zero")
        codes = tail[:nbytes].contiguous()
        if idx is not None:
            ref.sparse_upload_check(idx, torch.zeros(m, dtype=torch.float32), n, m)
        ref.quant_upload_check(codes, scales, m, self.bits)
        return Upload(idx, codes, scales)

    def gather(self, up: Upload, weight: float, group, W: int, n: int):
        """All-gather the group's W packed uploads and weights -> ``(uploads, weights [W])``, every row
        validated: each member ends up with the same tensors."""
        mine = torch.cat([self.pack(up), torch.tensor([weight], dtype=torch.float32, device=up.codes.device).view(torch.int32)])
        both = comm.allgather_stack(mine, group, W)
        ups = []
        for c in range(W):
            try:
                ups.append(self.unpack(both[c, :-1], n))
            except ValueError as e:
                raise RuntimeError(f"client {c}: {e}")
        return ups, both[:, -1].contiguous().view(torch.float32)

    # ---- aggregation -------------------------------------------------------------------------
    def combine(self, base: torch.Tensor, ups: Sequence[Upload], weights) -> torch.Tensor:
        """``base + (sum_c w_c d_c) / sum_c w_c`` on ``base``'s device, in the order of ``ups``."""
        w = weights if isinstance(weights, torch.Tensor) else torch.tensor([float(x) for x in weights], dtype=torch.float32,
                                                                              device=base.device)
        base = base.contiguous()
        if not self.sparse.active:
            return ops.dequant_combine(base, torch.stack([u.codes for u in ups]), torch.stack([u.scales for u in ups]),
                                       w, self.bits)
        k = self.m_for(base.numel())
        vals = [ops.dequantize(u.codes, u.scales, self.bits, k) for u in ups]
        return ops.sparse_combine(base, torch.stack([u.idx for u in ups]).contiguous(), torch.stack(vals).contiguous(), w)

    def received(self, base: torch.Tensor, up: Upload) -> torch.Tensor:
        """``base`` plus one client's dequantised delta (that client's model as the coordinator sees it)."""
        m = self.m_for(base.numel())
        d = ops.dequantize(up.codes, up.scales, self.bits, m)
        if up.idx is None:
            return base.detach() + d
        return Sparsifier.scatter(base, up.idx, d)

    def record(self, n: int, upload_bytes: List[int]) -> dict:
        """The keys a round record gains: the bytes the accepted clients sent against the dense form."""
        rec = {"upload_bits": self.bits, "upload_bytes": int(sum(upload_bytes)), "dense_bytes": 4 * int(n) * len(upload_bytes)}
        if self.sparse.active:
            rec["upload_topk"] = self.sparse.fraction
        return rec
