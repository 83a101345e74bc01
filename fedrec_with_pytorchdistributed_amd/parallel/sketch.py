"""Count-sketch uploads (``cfg.upload_sketch``) for the star topology: FetchSGD (Rothchild, Panda, Ullah, Ivkin, Stoica,
Braverman, Gonzalez, Arora, ICML 2020).

Top-k, quantised and low-rank uploads keep an fp32 error-feedback residual on every client, and every payload must be
decoded before the payloads can be added.  A count sketch is the compressor that is linear: a client sends the ``R x
C`` table ``S(theta_k - theta_g)`` (``4 R C`` bytes; ``R`` rows of ``C`` signed hash buckets) and keeps nothing; the
aggregating side adds the tables -- the sketch of the weighted mean is the weighted mean of the sketches -- onto an
error table ``E`` that it keeps between the rounds, estimates every coordinate of ``E`` as the median of its ``R``
buckets, takes the ``k = max(1, ceil(F n))`` largest estimates as the round's update and zeroes their buckets in
``E``; what the round did not recover stays in ``E`` (error feedback in sketch space).  So the clients are stateless,
and ``E`` is post-processing of the clients' sum: the codec composes with client-level DP (parallel/cdp.py), which
no compressor with a client-side residual can.

The hash is a block permutation (:func:`ops.reference.sketch_plan`), a pure function of ``(n, C, cfg.seed)`` that a
client and the coordinator derive alike in :meth:`SketchUpload.bind`.  Every step is a bitwise contract between host
and device (``ops.sketch_*``, ``ops.topk_delta``, ``ops.sparse_combine``): a coordinator on the host and clients that
combine among themselves on the device hold the same model and the same ``E``.  ``E`` travels in the coordinator's
snapshot and, as :attr:`SketchUpload.basis`, in the snapshot of clients that combine among themselves.

Not here: secure aggregation over the tables (masks cancel in a sum of tables -- ``combine`` is "add tables, decode
once" so that it can follow), an all-reduce of the tables in place of the all-gather, FetchSGD's momentum sketch
(the server-side step applies to the round's update as it stands) and the averaging modes.
"""
from __future__ import annotations

import math

import torch

from .. import ops
from ..ops import reference as ref
from ..utils import obs
from .upload import StarUpload


class SketchUpload(StarUpload):  # (its payload: the table, fp32 [R, C])
    uses_residual = False  # the clients are stateless
    STATE = "UPLOAD_SKETCH_ERROR"  # E in a coordinator's snapshot extras

    def __init__(self, fraction: float = 0.0, rows: int = 5, cols: int = 0, seed: int = 0):
        f = float(fraction)
        if not (0.0 <= f <= 1.0):  # (NaN fails here too)
            raise ValueError(f"upload_sketch={fraction}: expected 0 <= upload_sketch <= 1")
        if f and rows not in ref.SKETCH_ROWS:
            raise ValueError(f"upload_sketch_rows={rows}: expected 1, 3 or 5")
        if f and cols and (cols < ref.SKETCH_T or cols & (cols - 1)):
            raise ValueError(f"upload_sketch_cols={cols}: expected 0 (auto) or a power of two >= {ref.SKETCH_T}")
        self.fraction, self.rows, self.cols, self.seed = f, int(rows), int(cols), int(seed)
        self.options = {"upload_sketch": f, "upload_sketch_rows": self.rows, "upload_sketch_cols": self.cols}
        self.n = self.k = 0
        self.basis = None  # E, fp32 [R, C]: the error table of whoever combines (zeros until then)
        self._plans = {}

    @classmethod
    def from_cfg(cls, cfg, driver: str = "") -> "SketchUpload":
        """The codec of ``cfg``; an active one is rejected where it cannot hold (``driver``: the federation driver
        that asks)."""
        sk = cls(cfg.upload_sketch, cfg.upload_sketch_rows, cfg.upload_sketch_cols, cfg.seed)
        if sk.active:
            what = f"upload_sketch={cfg.upload_sketch}"
            if driver != "fedavg_star":
                raise ValueError(f"{what} is not available with mode={driver}: only the star clients upload a model; "
                                 "sketched gradient or parameter averaging is out of scope (use fedavg_star)")
            if cfg.secagg.enabled:
                raise ValueError(f"{what} cannot be combined with secagg.enabled=1: the secure upload masks the flat "
                                 "delta; masking the table instead is out of scope")
            if cfg.robust_agg != "none":
                raise ValueError(f"{what} cannot be combined with robust_agg={cfg.robust_agg}: the rule ranks dense "
                                 "fp32 stacks of every client's value per coordinate")
            for name in ("upload_topk", "upload_bits", "upload_rank"):
                if getattr(cfg, name):
                    raise ValueError(f"{what} cannot be combined with {name}={getattr(cfg, name)}: the sketch is "
                                     "linear and its clients keep no residual; a compressor in front of it is neither")
        return sk

    @property
    def active(self) -> bool:
        return self.fraction > 0.0

    def bind(self, flat_params) -> "SketchUpload":
        """:meth:`plan_for` the flat buffer; a table that is no smaller than the buffer is a configuration error."""
        flat = flat_params.flat
        self.plan_for(flat.numel(), flat.device)
        if self.rows * self.cols >= self.n:
            raise ValueError(f"upload_sketch={self.fraction}: a {self.rows} x {self.cols} table is no smaller than the "
                             f"model's {self.n} coordinates: nothing would be compressed (fewer rows, columns or a smaller fraction)")
        return self

    def plan_for(self, n: int, device="cpu") -> "SketchUpload":
        """The table's shape and the hash for ``n`` coordinates, and a zero ``E`` on ``device``."""
        self.n = n = int(n)
        self.k = min(n, max(1, int(math.ceil(self.fraction * n))))
        self.cols = self.cols or ref.sketch_cols_for(self.k)
        self.options = {**self.options, "upload_sketch_cols": self.cols}
        self._plans = {torch.device("cpu"): ref.sketch_plan(n, self.cols, self.seed)}
        self.basis = torch.zeros(self.rows, self.cols, dtype=torch.float32, device=device)
        return self

    def _plan(self, device) -> torch.Tensor:
        """The hash words on ``device`` (copied once)."""
        if not self._plans:
            raise RuntimeError("sketch upload: bind(flat_params) has not been called")
        device = torch.device(device)
        if device not in self._plans:
            self._plans[device] = self._plans[torch.device("cpu")].to(device)
        return self._plans[device]

    # ---- client ------------------------------------------------------------------------------
    def compress(self, local, theta_g, residual, client, round_idx):
        return ops.sketch_delta(local.contiguous(), theta_g.contiguous(), self._plan(local.device), self.rows, self.cols)

    def finite(self, up) -> bool:
        return bool(torch.isfinite(up).all())

    def pack(self, up):
        """One int32 1-D tensor: the table's bits."""
        return up.reshape(-1).view(torch.int32)

    def unpack(self, blob, n):
        L = self.rows * self.cols
        if blob.dtype != torch.int32 or blob.dim() != 1 or blob.numel() != L or int(n) != self.n:
            raise ValueError(f"sketch upload: expected an int32 [{L}] tensor for a model of {self.n} (got {blob.dtype} "
                             f"{tuple(blob.shape)} for {n})")
        return blob.contiguous().view(torch.float32).view(self.rows, self.cols)

    # ---- aggregation -------------------------------------------------------------------------
    def _recover(self, base, table):
        """``(base + the k largest estimates of table, their idx)`` on ``base``'s device."""
        dev = base.device
        est = ops.sketch_estimate(table, self._plan(dev), self.n)
        zeros = torch.zeros(self.n, dtype=torch.float32, device=dev)
        idx, val = ops.topk_delta(est, zeros, torch.zeros_like(zeros), self.k)  # (the scratch residual is discarded)
        one = torch.ones(1, dtype=torch.float32, device=dev)
        return ops.sparse_combine(base.contiguous(), idx[None].contiguous(), val[None].contiguous(), one), idx  # (1 v) / 1 = v

    def combine(self, base, ups, weights):
        """Add the tables onto ``E``, decode once, clear what was recovered: ``(base + top-k(estimate(E)), None)`` on
        ``base``'s device, in the order of ``ups``."""
        dev = base.device
        w = weights if isinstance(weights, torch.Tensor) else torch.tensor([float(x) for x in weights], dtype=torch.float32,
                                                                              device=dev)
        if self.basis.device != dev:
            self.basis = self.basis.to(dev)
        E = self.basis
        ops.sketch_accumulate_(E, torch.stack([u.reshape(-1) for u in ups]).contiguous(), w)
        new, idx = self._recover(base.detach(), E)
        ops.sketch_clear_(E, idx, self._plan(dev))
        return new, None

    def received(self, base, up):
        """``base`` plus the ``k`` largest estimates of one client's table (that client's model as far as its upload
        tells)."""
        return self._recover(base.detach(), up.contiguous())[0]

    # ---- the coordinator's snapshot ----------------------------------------------------------
    def state(self):
        return {self.STATE: self.basis.detach().cpu()}

    def load(self, st) -> None:
        saved = (st or {}).get(self.STATE)
        if saved is not None and tuple(saved.shape) == tuple(self.basis.shape):
            self.basis.copy_(saved.to(self.basis.device, torch.float32))
        else:
            obs.log(f"[server] the snapshot holds no sketch error table of {tuple(self.basis.shape)}: resuming with zeros")
