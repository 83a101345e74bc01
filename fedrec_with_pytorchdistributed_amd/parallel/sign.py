"""1-bit scaled-sign uploads with error feedback (``cfg.upload_sign``) for the star topology: signSGD (Bernstein et al.
2018) with the error feedback that makes it converge (EF-signSGD, Karimireddy et al. 2019).

A client sends the sign of every coordinate of ``(theta_k - theta_g) + residual`` and one fp32 mean magnitude per 256
coordinates -- ``ceil(n / 8) + 4 ceil(n / 256)`` bytes, 0.035 of ``4 n`` -- and keeps ``a - copysign(scale, a)`` as its
residual.  The sign with the mean magnitude is the L2-optimal 1-bit code of a block: its relative error is ``sqrt(1 -
mean|a|^2 / mean(a^2))``, near 0 on a delta whose coordinates share one magnitude (Adam's do) and 0.60 on a Gaussian one.
The coding is deterministic.

With ``upload_topk = F`` as well (STC, Sattler et al. 2019) ``topk_delta`` selects ``k`` coordinates first and their
values are sign-coded as a list of their own (scale blocks over list positions); the ``k`` errors go back into the
residual at the selected coordinates: ``4 k + ceil(k / 8) + 4 ceil(k / 256)`` bytes.

With ``upload_rotate = 1`` (DRIVE, Vargaftik et al. 2021) every 4096 coordinates are rotated by the randomized Hadamard
transform of parallel/rotate.py first, the residual lives in the rotated domain (:attr:`SignUpload.basis`, ``[n_pad]``,
``UPLOAD_BASIS`` in the client snapshot) and whoever combines averages rotated uploads and rotates back once.  On a
heavy-tailed delta, where a block's mean magnitude is far below its rms and the plain sign code says little, the
rotation is what makes one bit work.

The payload is the quantiser's ``Upload``; ``pack``, ``unpack`` and ``words_for`` are :class:`Quantizer`'s at one bit.
The arithmetic is :func:`ops.sign_quantize` / :func:`ops.sign_combine` and their ``rotate_`` forms, bitwise contracts
between host and device.
"""
from __future__ import annotations

from typing import Sequence

import torch

from .. import ops
from ..ops import reference as ref
from .quantize import Quantizer, Upload
from .sparsify import Sparsifier


class SignUpload(Quantizer):  # (its payload: an Upload at one bit per coded value)
    def __init__(self, sign: int = 0, seed: int = 0, fraction: float = 0.0, rotate: int = 0):
        if sign not in (0, 1):
            raise ValueError(f"upload_sign={sign}: expected 0 (off) or 1")
        self.bits = int(sign)  # one bit per coded value: Quantizer's sizes, pack and unpack hold
        self.seed = int(seed)
        self.sparse = Sparsifier(fraction if sign else 0.0)
        self.rotate = bool(rotate) and self.active
        self.uses_residual = not self.rotate  # rotated: the driver's [n] residual does not fit, the residual is ``basis``
        self.basis = None  # fp32 [n_pad]: the error-feedback residual in the rotated domain (bind)
        self.options = {"upload_sign": self.bits, **({"upload_topk": self.sparse.fraction} if self.sparse.active else {}),
                        **({"upload_rotate": 1} if self.rotate else {})}

    @classmethod
    def from_cfg(cls, cfg, driver: str = "") -> "SignUpload":
        """The codec of ``cfg``, inactive with ``upload_sign=0``; an active one is rejected where it cannot hold."""
        if cfg.upload_sign not in (0, 1):
            raise ValueError(f"upload_sign={cfg.upload_sign}: expected 0 (off) or 1")
        if not cfg.upload_sign:
            return cls(0, cfg.seed)
        if driver != "fedavg_star":
            raise ValueError(f"upload_sign=1 is not available with mode={driver}: only the star clients upload a model; "
                             "sign-coded gradient or parameter averaging is out of scope (use fedavg_star)")
        if cfg.upload_bits:
            raise ValueError(f"upload_sign=1 cannot be combined with upload_bits={cfg.upload_bits}: the sign code is the "
                             "1-bit form of its own, not a width of the stochastic quantiser")
        if cfg.upload_rank:
            raise ValueError(f"upload_sign=1 cannot be combined with upload_rank={cfg.upload_rank}: the factors are "
                             "orthonormalised and decoded in fp32")
        if cfg.upload_sketch:
            raise ValueError(f"upload_sign=1 cannot be combined with upload_sketch={cfg.upload_sketch}: sketch tables "
                             "are added, and signs of buckets do not add")
        if cfg.secagg.enabled:
            raise ValueError("upload_sign=1 cannot be combined with secagg.enabled=1: masked sums need every client's "
                             "values on one fixed-point grid, and each client scales its own blocks")
        if cfg.robust_agg != "none":
            raise ValueError(f"upload_sign=1 cannot be combined with robust_agg={cfg.robust_agg}: the rule ranks dense "
                             "fp32 stacks of every client's value per coordinate")
        if cfg.cdp.clip:
            raise ValueError(f"upload_sign=1 cannot be combined with cdp.clip={cfg.cdp.clip}: the error-feedback "
                             "residual is unprivatised state")
        if cfg.upload_rotate not in (0, 1):
            raise ValueError(f"upload_rotate={cfg.upload_rotate}: expected 0 (off) or 1")
        if cfg.upload_rotate and cfg.upload_topk:
            raise ValueError(f"upload_rotate=1 cannot be combined with upload_topk={cfg.upload_topk}: the quantiser then "
                             "codes a list of selected values, and list positions are not coordinates to rotate")
        return cls(1, cfg.seed, cfg.upload_topk, cfg.upload_rotate)

    def bind(self, flat_params) -> "SignUpload":
        flat = flat_params.flat
        return self.plan_for(flat.numel(), flat.device)

    def plan_for(self, n: int, device="cpu") -> "SignUpload":
        """Rotated form: a zero residual for ``n`` coordinates on ``device``."""
        if self.rotate:
            self.basis = torch.zeros(ref.rotate_pad(n), dtype=torch.float32, device=device)
        return self

    def m_for(self, n: int) -> int:
        """Coded values out of ``n`` coordinates: ``n_pad`` rotated, ``k`` composed with top-k, else ``n``."""
        return ref.rotate_pad(n) if self.rotate else super().m_for(n)

    # ---- client ------------------------------------------------------------------------------
    def compress(self, local, theta_g, residual, client: int, round_idx: int) -> Upload:
        """This round's upload; ``residual`` (rotated: :attr:`basis`, ``residual`` is None) is updated in place."""
        local, theta_g = local.contiguous(), theta_g.contiguous()
        if self.rotate:
            if self.basis is None or self.basis.numel() != ref.rotate_pad(local.numel()):
                raise RuntimeError("rotated sign upload: bind(flat_params) has not been called for this model")
            if self.basis.device != local.device:
                self.basis = self.basis.to(local.device)
            return Upload(None, *ops.rotate_sign_quantize(local, theta_g, self.basis, self.seed))
        if not self.sparse.active:
            return Upload(None, *ops.sign_quantize(local, theta_g, residual))
        idx, val = self.sparse.compress(local, theta_g, residual)
        err = torch.zeros_like(val)
        codes, scales = ops.sign_quantize(val, torch.zeros_like(val), err)
        residual[idx.long()] += err  # (+0.0 there since topk_delta sent them)
        return Upload(idx, codes, scales)

    # ---- aggregation -------------------------------------------------------------------------
    def combine(self, base: torch.Tensor, ups: Sequence[Upload], weights):
        """``(base + (sum_c w_c d_c) / sum_c w_c, None)`` on ``base``'s device, in the order of ``ups`` (rotated: the
        mean is taken over rotated coordinates and rotated back once)."""
        w = weights if isinstance(weights, torch.Tensor) else torch.tensor([float(x) for x in weights], dtype=torch.float32,
                                                                              device=base.device)
        base = base.detach().contiguous()
        if self.sparse.active:
            k = self.m_for(base.numel())
            vals = [ops.sign_dequantize(u.codes, u.scales, k) for u in ups]
            return ops.sparse_combine(base, torch.stack([u.idx for u in ups]).contiguous(), torch.stack(vals).contiguous(), w), None
        codes, scales = torch.stack([u.codes for u in ups]), torch.stack([u.scales for u in ups])
        if self.rotate:
            return ops.rotate_sign_combine(base, codes, scales, w, self.seed), None
        return ops.sign_combine(base, codes, scales, w), None

    def received(self, base: torch.Tensor, up: Upload) -> torch.Tensor:
        """``base`` plus one client's decoded delta: :meth:`combine` of it alone with weight 1."""
        return self.combine(base, [up], [1.0])[0]
