"""Elias-Fano coded index lists (``cfg.upload_index = "ef"``) for the star's top-k upload forms.

The three forms that send selected coordinates -- ``upload_topk`` alone, with ``upload_bits``, with ``upload_sign`` (STC)
-- put ``idx``, one int32 per coordinate, first in their blob; after the value-side compressors that word is most of
the upload (97 % of STC's).  ``topk_delta`` gives ``idx`` strictly ascending, and such a set has a succinct code whose
every bit has a known place (Elias 1974; Fano 1971; Vigna 2013): the low ``b = floor(log2(n / k))`` bits of every index
in a fixed-width array, the high parts in a unary bit vector, ``b + 1 + n / (k 2^b)`` bits an index -- 8.56 instead of 32
at ``upload_topk = 0.01`` -- and a size that depends on ``(n, k)`` alone, so blobs keep their fixed shape.

The code is lossless: :class:`IndexCoded` wraps one of the three codecs, replaces the ``k`` index words by the words of
:func:`ops.reference.ef_plan` in ``pack`` and puts them back in ``unpack``, and everything else -- selection, residuals,
validation of the decoded list, combines, snapshots -- is the wrapped codec's, bit for bit.  The arithmetic is
:func:`ops.ef_encode` / :func:`ops.ef_decode`: csrc/index_code.hip on device tensors (clients that combine among
themselves decode all rows in one batched call), the integer oracles on the host (the coordinator).
"""
from __future__ import annotations

import torch

from .. import ops
from ..ops import reference as ref
from . import comm
from .control import encode_tensor
from .upload import StarUpload, TopkUpload

INDEX_CODES = ("raw", "ef")


class IndexCoded(StarUpload):  # (its payload: the wrapped codec's)
    def __init__(self, inner: StarUpload):
        self.inner, self.sparse = inner, inner.sparse
        self.uses_residual = inner.uses_residual
        self.options = {**inner.options, "upload_index": "ef"}
        self.n = None  # coordinates of the flat buffer (bind): what ``pack`` codes against

    @staticmethod
    def check_cfg(cfg, driver: str) -> bool:
        """Whether ``cfg`` asks for the coded form; it is rejected where there is no index list to code."""
        v = cfg.upload_index
        if v not in INDEX_CODES:
            raise ValueError(f"upload_index={v}: expected raw or ef")
        if v == "raw":
            return False
        for key in ("upload_rotate", "upload_rank", "upload_sketch"):
            if getattr(cfg, key):
                raise ValueError(f"upload_index=ef cannot be combined with {key}={getattr(cfg, key)}: that upload "
                                 "carries no index list")
        if driver != "fedavg_star":
            raise ValueError(f"upload_index=ef is not available with mode={driver}: only the star clients upload a model "
                             "(use fedavg_star)")
        if not cfg.upload_topk:
            raise ValueError("upload_index=ef needs upload_topk > 0: only the top-k forms carry an index list to code")
        return True

    def bind(self, flat_params) -> "IndexCoded":
        self.inner.bind(flat_params)
        return self.plan_for(flat_params.flat.numel())

    def plan_for(self, n: int, device="cpu") -> "IndexCoded":
        self.n = int(n)
        return self

    def ef_words(self, n: int) -> int:
        """int32 words of the coded index list."""
        _, low_words, _, high_words = ref.ef_plan(n, self.sparse.k_for(n))
        return low_words + high_words

    def words_for(self, n: int) -> int:
        """int32 words of a packed upload."""
        return self.inner.words_for(n) - self.sparse.k_for(n) + self.ef_words(n)

    # ---- the wrapped codec's, as they are -------------------------------------------------------
    def compress(self, local, theta_g, residual, client, round_idx):
        return self.inner.compress(local, theta_g, residual, client, round_idx)

    def finite(self, up) -> bool:
        return self.inner.finite(up)

    def received(self, base, up):
        return self.inner.received(base, up)

    def combine(self, base, ups, weights):
        return self.inner.combine(base, ups, weights)

    # ---- the wire --------------------------------------------------------------------------------
    def pack(self, up) -> torch.Tensor:
        """One int32 1-D tensor: the Elias-Fano words of ``idx``, then the wrapped form's words after its ``idx``."""
        if self.n is None:
            raise RuntimeError("index-coded upload: bind(flat_params) has not been called for this model")
        raw, k = self.inner.pack(up).reshape(-1), up[0].numel()  # (idx comes first in all three forms)
        return torch.cat([ops.ef_encode(raw[:k].contiguous(), self.n), raw[k:]])

    def _decoded(self, blob, idx, count, n: int):
        """The wrapped codec's payload from one blob and what the decoder made of its index words, validated."""
        ew = self.ef_words(n)
        ref.ef_decoded_check(blob[:ew], idx, count, n, idx.numel())
        raw = torch.cat([idx, blob[ew:]])
        return self.inner.unpack(raw.view(2, -1) if isinstance(self.inner, TopkUpload) else raw, n)

    def unpack(self, blob: torch.Tensor, n: int):
        """The payload of a packed upload: the index words decoded and checked
        (:func:`ops.reference.ef_decoded_check`), then the wrapped codec's ``unpack``, which validates the list as it
        does a raw one; ``ValueError`` names what is wrong."""
        L = self.words_for(n)
        if blob.dtype != torch.int32 or blob.dim() != 1 or blob.numel() != L:
            raise ValueError(f"index-coded upload: expected an int32 [{L}] tensor (got {blob.dtype} {tuple(blob.shape)})")
        idx, count = ops.ef_decode(blob[:self.ef_words(n)].reshape(1, -1), n, self.sparse.k_for(n))
        return self._decoded(blob, idx[0], count[0], n)

    def combine_among(self, payload, weight: float, ctx, base: torch.Tensor, timeout_s: float):
        """As :meth:`StarUpload.combine_among`; on the device the clients' index words are decoded in one batched call."""
        if not base.is_cuda:
            return super().combine_among(payload, weight, ctx, base, timeout_s)
        n = base.numel()
        blob = self.pack(payload)
        word = torch.tensor([weight], dtype=torch.float32, device=blob.device).view(torch.int32)
        both = comm.allgather_stack(torch.cat([blob, word]), ctx.data_group, ctx.num_clients)
        idx, count = ops.ef_decode(both[:, :self.ef_words(n)].contiguous(), n, self.sparse.k_for(n))
        ups = []
        for c in range(ctx.num_clients):
            try:
                ups.append(self._decoded(both[c, :-1], idx[c], count[c], n))
            except ValueError as e:
                raise RuntimeError(f"client {c}: {e}")
        return self.combine(base, ups, both[:, -1].contiguous().view(torch.float32))

    def meta(self, up, blob: bytes = None) -> dict:
        return self.inner.meta(up, encode_tensor(self.pack(up)) if blob is None else blob)
