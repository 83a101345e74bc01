"""Randomized-Hadamard rotation of quantised uploads (``cfg.upload_rotate``, with ``cfg.upload_bits``) for the star
topology: Konecny et al. 2016 ("structured updates"); Suresh, Yu, Kumar, McMahan 2017; DRIVE / EDEN, Vargaftik et al.
2021/22.

The block quantiser's step is ``max|a| / Q`` per 256 coordinates: a few large coordinates set the step of all the small
ones, and the error-feedback residual is where the outliers of earlier rounds collect.  ``R = 2^-6 H D`` over chunks of
4096 coordinates (``H`` the Hadamard matrix, ``D`` signs from ``cfg.seed``, the same on every client and in every round)
makes every rotated coordinate a signed average of its chunk: max / rms is about 3 per block whatever the input looked
like, and the error follows the chunk's norm.  ``R`` is orthonormal and linear, so the residual lives in the rotated
domain (``R delta + r_rot``: one transform per round, not two) and whoever combines averages the rotated uploads and
rotates back once.

The payload is the quantiser's ``Upload(None, codes, scales)`` over ``n_pad = 4096 ceil(n / 4096)`` rotated
coordinates; the residual, fp32 ``[n_pad]``, is :attr:`RotatedQuantizer.basis` and travels in the client snapshot as
``UPLOAD_BASIS``.  The arithmetic is :func:`ops.rotate_quantize` and :func:`ops.rotate_combine`, bitwise contracts
between host and device as the quantiser's are.
"""
from __future__ import annotations

from typing import Sequence

import torch

from .. import ops
from ..ops import reference as ref
from .quantize import Quantizer, Upload


class RotatedQuantizer(Quantizer):  # (its payload: an Upload over n_pad coordinates)
    uses_residual = False  # the driver's [n] residual does not fit: the residual is ``basis``

    def __init__(self, bits: int = 0, seed: int = 0):
        super().__init__(bits, seed)
        if self.active:
            self.options = {**self.options, "upload_rotate": 1}
        self.basis = None  # fp32 [n_pad]: the error-feedback residual in the rotated domain (bind)

    @classmethod
    def from_cfg(cls, cfg, driver: str = "") -> "RotatedQuantizer":
        """The codec of ``cfg``, inactive with ``upload_rotate=0``; an active one holds wherever
        :meth:`Quantizer.from_cfg` holds, without ``upload_topk``."""
        rot = cfg.upload_rotate
        if rot not in (0, 1):
            raise ValueError(f"upload_rotate={rot}: expected 0 (off) or 1")
        if not rot:
            return cls(0, cfg.seed)
        if not cfg.upload_bits:
            if cfg.upload_sign:  # the rotated sign code: parallel/sign.py owns it
                return cls(0, cfg.seed)
            raise ValueError("upload_rotate=1 needs upload_bits=8 or 4, or upload_sign=1: the rotation prepares the round "
                             "delta for the block quantiser or the sign coder and does nothing for an fp32 upload")
        if cfg.upload_topk:
            raise ValueError(f"upload_rotate=1 cannot be combined with upload_topk={cfg.upload_topk}: the quantiser then "
                             "codes a list of selected values, and list positions are not coordinates to rotate")
        Quantizer.from_cfg(cfg, driver)  # every exclusion of the quantiser holds
        return cls(cfg.upload_bits, cfg.seed)

    def bind(self, flat_params) -> "RotatedQuantizer":
        flat = flat_params.flat
        return self.plan_for(flat.numel(), flat.device)

    def plan_for(self, n: int, device="cpu") -> "RotatedQuantizer":
        """A zero residual for ``n`` coordinates on ``device``."""
        self.basis = torch.zeros(ref.rotate_pad(n), dtype=torch.float32, device=device)
        return self

    def m_for(self, n: int) -> int:
        """Quantised values out of ``n`` coordinates: ``n_pad`` (``pack``, ``unpack`` and ``words_for`` work on it)."""
        return ref.rotate_pad(n)

    # ---- client ------------------------------------------------------------------------------
    def compress(self, local, theta_g, residual, client: int, round_idx: int) -> Upload:
        """This round's upload; the residual updated in place is :attr:`basis` (``residual`` is the driver's: None)."""
        if self.basis is None or self.basis.numel() != ref.rotate_pad(local.numel()):
            raise RuntimeError("rotated upload: bind(flat_params) has not been called for this model")
        if self.basis.device != local.device:
            self.basis = self.basis.to(local.device)
        offset = (int(client) << 32) | int(round_idx)
        return Upload(None, *ops.rotate_quantize(local.contiguous(), theta_g.contiguous(), self.basis, self.bits,
                                                 self.seed, offset))

    # ---- aggregation -------------------------------------------------------------------------
    def combine(self, base: torch.Tensor, ups: Sequence[Upload], weights):
        """``(base + R^-1 ((sum_c w_c d_c) / sum_c w_c), None)`` on ``base``'s device, in the order of ``ups``."""
        w = weights if isinstance(weights, torch.Tensor) else torch.tensor([float(x) for x in weights], dtype=torch.float32,
                                                                              device=base.device)
        return ops.rotate_combine(base.detach().contiguous(), torch.stack([u.codes for u in ups]),
                                  torch.stack([u.scales for u in ups]), w, self.bits, self.seed), None

    def received(self, base: torch.Tensor, up: Upload) -> torch.Tensor:
        """``base`` plus one client's dequantised delta rotated back: :meth:`combine` of it alone with weight 1."""
        return self.combine(base, [up], [1.0])[0]
