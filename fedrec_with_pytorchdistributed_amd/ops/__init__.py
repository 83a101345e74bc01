"""Fused ops of the engine.

Device tensors run the hand-written HIP/CDNA4 kernels of ``csrc/`` (``torch.ops.fedrec``);
host tensors run the torch-eager oracle in :mod:`.reference` (the CPU/gloo plumbing
configuration and the numerics reference of the tests).  On a device tensor a missing
extension is an error -- there is no silent eager fallback.

Kernel map:

====================  ===========================  ===========================================
op                    reference site               kernel (csrc/)
====================  ===========================  ===========================================
embed_ln              HF embeddings (K01)          embed_ln.hip: gather + pos add + LayerNorm
linear                q/k/v/out/lin1/lin2, heads   gemm_bf16.hip: MFMA 16x16x32 bf16, fused
                      (K02, K05, K06, K07)         bias / GELU / tanh / residual epilogues
layer_norm            sa/output LN (K04)           layernorm.hip: one wave per row
title_attention       HF attention (K03)           title_attn.hip: MFMA QK^T / PV, T pad 64
title_plan + *_packed frozen-backbone forward      title_attn.hip: pad tokens get Q only (no K/V)
additive_pool_*       attention.py:14-26 (K06/12)  additive_pool.hip: score, eps-softmax, pool
user_attention_*      attention.py:32-82 (K11)     user_attn.hip: 20 heads x d_k 20
score_ce              model.py:121-126 (K13)       score_ce.hip: sigmoid-CE fwd+bwd fused
segment_sum_rows      client.py:26-48,87-89        news_grad.hip: deterministic segment sum
                      (K16, K17)                   + LDP clip + Philox Gaussian noise
adam_flat             model.py:89,93 (K20)         adam.hip: one pass over the flat buffer
dedup / sample_batch  dataset.py:69-86 (K18)       batch.hip: on-device sampling + unique
topk_scores           (beyond the reference)       topk_scores.hip: fp32 MFMA U V^T fused with an
                                                   ordered per-user top-k (no [B, N] matrix)
rank_impressions      (beyond the reference)       rank_impressions.hip: an impression's whole
                                                   negative list gathered, scored and compared
                                                   with its positive; 4 integers per impression
mmr_rerank            (beyond the reference)       mmr_rerank.hip: a pool's rows gathered once, its
                                                   P x P cosines on fp32 MFMA in registers, the
                                                   greedy MMR picks and the list's ILD on the CU
trimmed_mean          (beyond the reference)       robust_agg.hip: W <= 32 clients' values of a
                                                   coordinate sorted in registers (compile-time
                                                   network), trimmed mean / median + dropped counts
topk_delta /          (beyond the reference)       sparse_delta.hip: exact magnitude top-k of one long
sparse_combine                                     row by radix select (no sort, no host sync) with
                                                   the error-feedback residual; W sparse lists
                                                   scattered onto a base through LDS tiles
quantize_delta /      (beyond the reference)       quant_delta.hip: stochastic int8 / int4 codes with one
dequant_combine                                    fp32 scale per 256 coordinates and the error-feedback
                                                   residual, 16 coordinates per lane in registers; W
                                                   quantised deltas dequantised onto a base
====================  ===========================  ===========================================
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import native
from . import reference as ref

_ACT = {"none": 0, "gelu": 1, "tanh": 2}


def _dev(t: torch.Tensor) -> bool:
    return t.is_cuda


# ---------------------------------------------------------------------------------------
def embed_ln(tokens, word, pos, ln_w, ln_b, eps: float, dtype=torch.float32):
    if _dev(word):
        if word.dtype != torch.bfloat16:
            native.no_kernel("embed_ln", word)
        return native.require_for(word).embed_ln(tokens.contiguous(), word, pos, ln_w, ln_b, float(eps))
    return ref.embed_ln(tokens, word, pos, ln_w, ln_b, eps).to(dtype)


def linear(x, w, b=None, act: str = "none", residual=None, out_dtype=None):
    """``act(x @ w^T + b) + residual``; bf16 device inputs run the MFMA GEMM."""
    if _dev(x):
        if x.dtype != torch.bfloat16:
            native.no_kernel("linear", x)
        return native.require_for(x).linear(x.contiguous(), w, b, _ACT[act], residual)
    y = ref.linear(x, w, b, act, residual)
    return y.to(out_dtype or x.dtype)


def layer_norm(x, w, b, eps: float, dtype=None, residual=None):
    """``LN(x [+ residual]) * w + b`` (the residual add is fused into the LN kernel)."""
    if _dev(x):
        if x.dtype != torch.bfloat16:
            native.no_kernel("layer_norm", x)
        return native.require_for(x).layer_norm(x, w, b, float(eps), residual)
    h = x if residual is None else x.float() + residual.float()
    return ref.layer_norm(h, w, b, eps).to(dtype or x.dtype)


def title_attention(qkv, mask, n_heads: int, drop=None):
    """``drop = (p, seed, offset)``: train-mode dropout on the attention probabilities."""
    if _dev(qkv):
        if qkv.dtype != torch.bfloat16:
            native.no_kernel("title_attention", qkv)
        if drop is not None:
            p, seed, off = drop
            return native.require_for(qkv).title_attention_drop(qkv, mask.contiguous(), int(n_heads), float(p),
                                                                int(seed), int(off))
        return native.require_for(qkv).title_attention(qkv, mask.contiguous(), int(n_heads))
    return ref.title_attention(qkv, mask, n_heads, drop).to(qkv.dtype)


def title_attention_bwd(qkv, dout, mask, n_heads: int, drop=None):
    lib = native.require_for(qkv)
    if drop is not None:
        p, seed, off = drop
        return lib.title_attention_bwd_drop(qkv, dout.contiguous(), mask.contiguous(), int(n_heads), float(p),
                                            int(seed), int(off))
    return lib.title_attention_bwd(qkv, dout.contiguous(), mask.contiguous(), int(n_heads))


def dropout_add(h, res, p: float, seed: int, offset: int):
    """``res + h o Z`` (``res`` may be None): Z = keep / (1 - p) from the element-indexed
    Philox mask (csrc/dropout.hip).  Its own backward: ``dh = dout o Z``."""
    if _dev(h):
        if h.dtype != torch.bfloat16:
            native.no_kernel("dropout_add", h)
        r = None if res is None else res.contiguous()
        return native.require_for(h).dropout_add(h.contiguous(), r, float(p), int(seed), int(offset))
    return ref.dropout_add(h, res, p, seed, offset).to(h.dtype)


# ---- packed title rows (frozen backbone forward, csrc/title_attn.hip) -----------------------
def title_plan(mask):
    """``mask [n, T]`` -> ``(rowmap [n,T], src [n*T], kv_start [n], kv_len [n], qstart [n], n_kv [1])``:
    the packed row order (key/value rows first, then query-only rows) and its inverse."""
    if _dev(mask):
        return tuple(native.require_for(mask).title_plan(mask.contiguous()))
    return ref.title_plan(mask)


def embed_ln_rows(tokens, src, word, pos, ln_w, ln_b, eps: float):
    """Embedding + LN of packed row r = flat token ``src[r]`` of ``tokens [n, T]``."""
    return native.require_for(word).embed_ln_rows(tokens.contiguous(), src, word, pos, ln_w, ln_b, float(eps))


def linear_split(x, w, b, full_rows, n_partial: int):
    """``x @ w^T + b`` with rows ``>= full_rows[0]`` computed on the first ``n_partial``
    output columns only (the rest of those rows is left unwritten)."""
    return native.require_for(x).linear_split(x.contiguous(), w, b, full_rows, int(n_partial))


def title_attention_packed(qkv, rowmap, kv_start, kv_len, qstart, n_heads: int):
    return native.require_for(qkv).title_attention_packed(qkv, rowmap, kv_start, kv_len, qstart, int(n_heads))


def layer_norm_scatter(x, w, b, eps: float, residual, dst, out=None):
    """``LN(x + residual)`` with row r stored at output row ``dst[r]`` (of ``out`` when given)."""
    return native.require_for(x).layer_norm_scatter(x, w, b, float(eps), residual, dst, out)


def additive_pool_fwd(x, e, w2, b2, keep=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> ``(pooled fp32 [n,D], alpha fp32 [n,T])``; ``keep [n,T]`` int (nonzero = pooled):
    the mask_padding position mask."""
    if _dev(x):
        return tuple(native.require_for(x).additive_pool_fwd(x.contiguous(), e.contiguous(),
                                                             w2.reshape(-1).float().contiguous(),
                                                             b2.reshape(-1).float().contiguous(), _mask32(keep)))
    return ref.additive_pool_fwd(x, e, w2, b2, keep=keep)


def _mask32(keep):
    return None if keep is None else keep.to(torch.int32).contiguous()


def additive_pool_bwd(x, e, alpha, w2, g, want_dx: bool, want_colsum: bool = False):
    """-> ``(dx_direct|None, dpre, dw2, db2)`` with ``dpre = da w2 (1 - e^2)`` (tanh folded);
    ``want_colsum`` appends ``dpre`` summed over all tokens (the first linear's bias
    gradient) when the kernel produced it for free, else None."""
    if _dev(x):
        dx, dpre, dw2, db2, dsum = native.require_for(x).additive_pool_bwd(
            x.contiguous(), e.contiguous(), alpha.contiguous(), w2.reshape(-1).float().contiguous(),
            g.float().contiguous(), bool(want_dx))
        out = (dx if want_dx else None), dpre, dw2, db2
        return out + ((dsum if dsum.numel() else None),) if want_colsum else out
    dx, de, dw2, db2 = ref.additive_pool_bwd(x, e, alpha, w2, g)
    dpre = de * (1.0 - e.float() ** 2)
    out = (dx if want_dx else None), dpre, dw2, db2
    return out + (None,) if want_colsum else out


def user_attention_fwd(qkv, heads: int, head_dim: int, keep=None, ctx_b=None):
    """-> ``(ctx [B,H,h*d], saved)``; ``saved`` is whatever the backward needs.  ``keep [B,H]``
    int (nonzero = attend): the mask_padding key mask.  ``ctx_b`` (bf16, like ctx, device
    only): also written with ctx rounded to bf16 (a GEMM operand)."""
    if _dev(qkv):
        return tuple(native.require_for(qkv).user_attention_fwd(qkv.contiguous(), heads, head_dim, _mask32(keep),
                                                                ctx_b))
    out = ref.user_attention_fwd(qkv, heads, head_dim, keep=keep)
    if ctx_b is not None:
        ctx_b.copy_(out[0].reshape(ctx_b.shape))
    return out


def user_qkv_attention_fwd(xd, W, bias, B: int, heads: int, head_dim: int, keep=None, ctx_b=None):
    """Q|K|V projection + attention forward in one launch (device only, H <= 64): ``xd [B*H, Din]``
    bf16, ``W [3*heads*head_dim, Din]`` bf16, ``bias`` fp32 -> ``(ctx [B,H,D], saved, qkv [B,H,3D])``
    -- the values of ``small_gemm(xd, W, +bias)`` followed by :func:`user_attention_fwd`."""
    return tuple(native.require_for(xd).user_qkv_attention_fwd(xd, W, bias, int(B), heads, head_dim, _mask32(keep),
                                                               ctx_b))


def user_attention_bwd_dctx(qkv, saved, dctx, dpre, w1t, heads: int, head_dim: int, keep=None):
    """Attention backward with the additive pool's input-gradient GEMM fused in (device only,
    H <= 64): the attention's dctx is ``dctx + dpre @ w1t.T`` (``dctx`` read, not written; ``dpre
    [B*H, Qd]`` and ``w1t [D, Qd]`` bf16) -> ``dqkv`` bf16 [B, H, 3D]."""
    return native.require_for(qkv).user_attention_bwd_dctx(qkv.contiguous(), saved, dctx.contiguous(), dpre, w1t,
                                                           heads, head_dim, _mask32(keep))


def user_attention_bwd(qkv, saved, dctx, heads: int, head_dim: int, keep=None, bf16_out: bool = False):
    """-> ``dqkv`` like qkv (bf16 with ``bf16_out``: the gradient GEMMs' operand)."""
    if _dev(qkv):
        return native.require_for(qkv).user_attention_bwd(qkv.contiguous(), saved, dctx.contiguous(),
                                                          heads, head_dim, _mask32(keep), bool(bf16_out))
    d = ref.user_attention_bwd(qkv, saved, dctx, heads, head_dim)  # the saved weights hold the mask
    return d.to(torch.bfloat16) if bf16_out else d


def score_ce(cand, user, act: str = "sigmoid"):
    """-> ``(loss [], scores [B,C], dcand [B,C,D], duser [B,D])`` (grads of the mean loss)."""
    if _dev(cand):
        return tuple(native.require_for(cand).score_ce(cand.float().contiguous(), user.float().contiguous(),
                                                       1 if act == "sigmoid" else 0))
    return ref.score_ce_fwd_bwd(cand, user, act)


def score_ce_rows(table, ci, user, act: str, dcand_out):
    """:func:`score_ce` with candidate ``(b, c)`` = row ``ci[b C + c]`` of ``table [U, D]`` and its
    gradient written into ``dcand_out [B C, D]`` -> ``(loss, scores, duser)``."""
    B = user.shape[0]
    if _dev(table):
        loss, scores, _, du = native.require_for(table).score_ce(table, user.contiguous(), 1 if act == "sigmoid" else 0,
                                                                 ci, dcand_out)
        return loss, scores, du
    loss, scores, dcand, du = ref.score_ce_fwd_bwd(table.index_select(0, ci.long()).view(B, -1, table.shape[1]), user,
                                                   act)
    dcand_out.copy_(dcand.reshape(dcand_out.shape))
    return loss, scores, du


def topk_scores(user, table, k: int, exclude=None, min_id: int = 0):
    """Catalog top-k -> ``(scores [B, k] fp32, ids [B, k] int32)``: the ``k`` best rows of ``table
    [N, D]`` for each row of ``user [B, D]`` by raw dot product (fp32 operands and accumulation),
    ordered by (score descending, id ascending).  Row ``n`` is eligible iff ``n >= min_id``, ``n`` is
    not in ``exclude[b, :]`` (int [B, E]; entries < 0 or >= N and duplicates are ignored) and its
    score is not NaN; slots past the eligible count hold ``(-inf, -1)``.  The device kernel never
    writes the ``[B, N]`` scores and is bitwise independent of its grid (csrc/topk_scores.hip)."""
    if _dev(user):
        ex = None if exclude is None else exclude.to(torch.int32).contiguous()
        return tuple(native.require_for(user).topk_scores(user, table, int(k), ex, int(min_id)))
    return ref.topk_scores(user, table, int(k), exclude, int(min_id))


def rank_impressions(user, table, pos, neg_ptr, negs, row0: int = 0):
    """Full-impression ranking -> ``counts [B, 4]`` int32 ``(n_gt, n_eq, n_neg, n_nan)``.  User ``b``
    (``user [B, D]`` fp32) is impression ``row0 + b`` of the corpus CSR ``pos [I]`` int32, ``neg_ptr
    [I + 1]`` int64, ``negs [M]`` int32 (the :class:`DeviceSampler`'s arrays, passed whole): ``n_gt``
    / ``n_eq`` count its negatives whose raw dot product with ``table [N, D]`` fp32 is greater than
    / equal to the positive's, ``n_neg`` is the list length, ``n_nan`` the candidates (positive
    included) with a NaN score.  The device kernel writes no score and no gathered row, sums every
    candidate in one fixed order (a negative with the positive's id ties bitwise) and is bitwise
    independent of ``B``, ``row0`` and its grid (csrc/rank_impressions.hip); ids are trusted to lie
    in ``[0, N)``.  :func:`eval.metrics.impression_metrics` turns the counts into AUC / MRR / nDCG."""
    if _dev(user):
        native.require_for(user)
        return torch.ops.fedrec_eval.rank_impressions(user, table, pos, neg_ptr, negs, int(row0))
    return ref.rank_impressions(user, table, pos, neg_ptr, negs, int(row0))


def mmr_rerank(table, ids, rel, k: int, lam: float):
    """Diversity re-rank of a candidate pool by Maximal Marginal Relevance -> ``(ids_out [B, k] int32,
    rel_out [B, k] fp32, ild [B] fp32)``.  ``ids [B, P]`` int32 are rows of ``table [N, D]`` fp32 (``< 0``:
    an empty slot -- what :func:`topk_scores` returns is a valid pool), ``rel [B, P]`` their relevance;
    ``1 <= k <= P <= 128``, ``0 <= lam <= 1``.  Greedily, ``k`` times: pick the not-yet-picked slot with
    the largest ``lam * rhat_j - (1 - lam) * max_{i picked} cos(row_i, row_j)``, ``rhat`` the pool's
    relevance scaled to [0, 1]; ties go to the lowest pool position, so ``lam = 1`` returns the pool's
    first ``k`` slots.  Outputs are in selection order (``rel_out``: the original ``rel``; ``(-1, -inf)``
    past the valid count); ``ild`` is the list's mean pairwise ``1 - cos``.  The device kernel keeps
    a user's whole cosine matrix in registers and is bitwise independent of the batch
    (csrc/mmr_rerank.hip); ids are trusted to lie in ``[0, N)``.  The exact contract:
    :func:`ops.reference.mmr_rerank`."""
    if _dev(table):
        native.require_for(table)
        return tuple(torch.ops.fedrec_rerank.mmr_rerank(table, ids.to(torch.int32).contiguous(), rel.contiguous(),
                                                         int(k), float(lam)))
    return ref.mmr_rerank(table, ids, rel, int(k), float(lam))


def trimmed_mean(stack, trim: int):
    """Coordinate-wise trimmed mean of ``W <= 32`` clients' vectors -> ``(out [n] fp32, dropped [W]
    int64)``: ``stack [W, n]`` fp32 contiguous, ``0 <= 2 trim < W``.  Per coordinate the ``trim`` lowest
    and ``trim`` highest values (ranked by a total order on the floats' bits, -0.0 < +0.0 < ... < +inf <
    NaN, ties to the lower client) are dropped and the rest averaged in rank order; ``trim = (W - 1)
    // 2`` is the median, ``trim = 0`` the plain mean in client order.  ``dropped[c]`` counts the
    coordinates where client ``c`` was cut.  The device kernel reads each value once, sorts in
    registers and writes ``n`` floats; both results are bitwise independent of its grid and of how a
    caller splits the coordinates into calls (csrc/robust_agg.hip).  The exact contract:
    :func:`ops.reference.trimmed_mean`."""
    if _dev(stack):
        native.require_for(stack)
        return tuple(torch.ops.fedrec_agg.trimmed_mean(stack, int(trim)))
    return ref.trimmed_mean(stack, int(trim))


def topk_delta(local, global_, residual, k: int):
    """Magnitude top-k of a round delta with error feedback -> ``(idx [k] int32 ascending, val [k]
    fp32)``; ``residual`` is updated in place.  ``local``, ``global_``, ``residual`` ``[n]`` fp32
    contiguous (a view such as ``x[1:]`` is fine), ``residual`` overlapping neither input, ``1 <= k <= n
    < 2^31``.  ``a = (local - global_) + residual``; the ``k`` coordinates with the largest ``bits(a) &
    0x7fffffff`` are sent (NaN above inf above every finite value, the lower index among equal keys),
    and ``residual`` becomes ``+0.0`` there and ``a`` elsewhere.  The device path is a radix select
    with no sort and no host synchronisation, bitwise independent of its grid
    (csrc/sparse_delta.hip).  The exact contract: :func:`ops.reference.topk_delta`."""
    if _dev(residual):
        native.require_for(residual)
        return tuple(torch.ops.fedrec_sparse.topk_delta(local, global_, residual, int(k)))
    return ref.topk_delta(local, global_, residual, int(k))


def sparse_combine(base, idx, val, weights):
    """``W`` sparse updates applied to ``base [n]`` fp32 -> ``out [n]``: ``out = base + (sum over c, in
    client order, of weights[c] * scatter(idx[c], val[c])) / sum(weights)``.  ``idx [W, k]`` int32 with
    every row strictly ascending in ``[0, n)`` (callers validate with
    :func:`ops.reference.sparse_upload_check`; the kernel stays in bounds whatever the content),
    ``val [W, k]`` fp32, ``weights [W]`` fp32.  Every product, sum and the division is rounded on its
    own, so the device kernel (csrc/sparse_delta.hip) and the host oracle hold the same bits.  The
    exact contract: :func:`ops.reference.sparse_combine`."""
    if _dev(base):
        native.require_for(base)
        return torch.ops.fedrec_sparse.combine(base, idx, val, weights)
    return ref.sparse_combine(base, idx, val, weights)


def quantize_delta(local, global_, residual, bits: int, seed: int, offset: int):
    """Stochastic block quantisation of a round delta with error feedback -> ``(codes uint8 [ceil(n bits /
    8)], scales fp32 [ceil(n / 256)])``; ``residual`` is updated in place.  ``local``, ``global_``,
    ``residual`` ``[n]`` fp32 contiguous (a view such as ``x[1:]`` is fine), ``residual`` overlapping neither
    input, ``1 <= n < 2^31``, ``bits`` 8 or 4.  ``a = (local - global_) + residual``; each block of 256
    coordinates gets the scale ``max|a| / Q`` (``Q = 2^(bits - 1) - 1``) and every coordinate the code
    ``clamp(floor(a / s) + up, -Q, Q)``, rounded up with probability ``frac(a / s)`` by the Philox stream
    ``(seed, offset)``; ``residual`` becomes ``a - code * s``.  A block with an inf or a NaN sends a NaN
    scale, zero codes and keeps a zero residual.  Bitwise independent of the grid
    (csrc/quant_delta.hip).  The exact contract: :func:`ops.reference.quantize_delta`."""
    if _dev(residual):
        native.require_for(residual)
        return tuple(torch.ops.fedrec_quant.quantize_delta(local, global_, residual, int(bits), int(seed), int(offset)))
    return ref.quantize_delta(local, global_, residual, int(bits), int(seed), int(offset))


def dequant_combine(base, codes, scales, weights, bits: int):
    """``W`` quantised updates applied to ``base [n]`` fp32 -> ``out [n]``: ``out = base + (sum over c, in
    client order, of weights[c] * (code[c] * scale[c])) / sum(weights)``.  ``codes [W, ceil(n bits / 8)]``
    uint8, ``scales [W, ceil(n / 256)]`` fp32 (callers validate with
    :func:`ops.reference.quant_upload_check`; the kernel stays in bounds whatever the content),
    ``weights [W]`` fp32.  Every product, sum and the division is rounded on its own, so the device kernel
    (csrc/quant_delta.hip) and the host oracle hold the same bits.  The exact contract:
    :func:`ops.reference.dequant_combine`."""
    if _dev(base):
        native.require_for(base)
        return torch.ops.fedrec_quant.dequant_combine(base, codes, scales, weights, int(bits))
    return ref.dequant_combine(base, codes, scales, weights, int(bits))


def dequantize(codes, scales, bits: int, n: int):
    """One upload's delta ``[n]`` fp32 from ``codes [ceil(n bits / 8)]`` and ``scales [ceil(n / 256)]``:
    :func:`dequant_combine` with ``W = 1``, a zero base and weight 1 (``-0.0`` reads as ``+0.0``)."""
    return dequant_combine(torch.zeros(int(n), dtype=torch.float32, device=codes.device), codes.reshape(1, -1),
                           scales.reshape(1, -1), torch.ones(1, dtype=torch.float32, device=codes.device), int(bits))


def segment_sum_rows(rows, inv, num_out: int, clip: float = 0.0, noise_std: float = 0.0,
                     seed: int = 0, offset: int = 0, generator=None, seg=None, zero_empty: bool = False,
                     dev_off=None):
    """Per-news gradient reduction ``out[inv[r]] += clip(rows[r]) + N(0, noise_std)``.

    ``seg = (perm, seg_ptr)`` (rows grouped by output id) enables the deterministic,
    atomic-free device kernel; it is produced by :func:`dedup`.  The device kernel expects
    the layout dedup produces: every output row has occurrences, except trailing padded rows
    (``zero_empty``, the step graphs' padded unique lists).  ``dev_off`` (device int64[1]):
    added to ``offset`` on the device, so a captured step graph draws fresh noise per replay.

    Device noise: element ``d`` of occurrence row ``r`` is one normal of Philox(``seed``, ``offset`` +
    ``dev_off``) in one of two counter layouts -- the same seed gives a different field in each.
    The fused float4 chunk pass (segsum variant 2, ``D % 4 == 0``, 16-byte aligned rows) uses counter
    ``(r << 16) | d // 4``, component ``d % 4``; every other case (variant 0 or 1, ``D % 4 != 0``, a
    misaligned view) runs the two-pass fallback with counter ``(r << 16) | (2 * (d % 64) + d // 256)``,
    component ``(d // 64) % 4`` (csrc/news_grad.hip; the oracle: tests/data_oracle.py).
    """
    if _dev(rows):
        if seg is None:
            perm, ptr = segments_from_inv(inv, num_out)
        else:
            perm, ptr = seg
        inv32 = inv.reshape(-1)
        inv32 = inv32 if inv32.dtype == torch.int32 else inv32.to(torch.int32)
        return native.require_for(rows).segment_sum_rows(rows.float().contiguous(), perm, ptr, int(num_out),
                                                         float(clip), float(noise_std), int(seed), int(offset),
                                                         inv32.contiguous(), bool(zero_empty), dev_off)
    if dev_off is not None:
        offset = int(offset) + int(dev_off.reshape(-1)[0])
    if noise_std > 0 and generator is None:
        generator = torch.Generator().manual_seed((int(seed) * 1_000_003 + int(offset)) & 0x7FFFFFFFFFFF)
    return ref.segment_sum_rows(rows, inv, num_out, clip, noise_std, generator)


def segments_from_inv(inv: torch.Tensor, num_out: int):
    inv = inv.reshape(-1).long()
    perm = torch.sort(inv, stable=True).indices.to(torch.int32)
    cnt = torch.bincount(inv, minlength=num_out)
    ptr = torch.zeros(num_out + 1, dtype=torch.int32, device=inv.device)
    ptr[1:] = torch.cumsum(cnt, 0).to(torch.int32)
    return perm, ptr


def adam_flat(p, g, m, v, step: int, lr: float, b1: float, b2: float, eps: float,
              grad_scale: float = 1.0, p_lowp: Optional[torch.Tensor] = None) -> None:
    """One fused Adam step over flat fp32 buffers (torch.optim.Adam semantics)."""
    if _dev(p):
        bc1 = 1.0 - b1 ** step
        bc2 = 1.0 - b2 ** step
        native.require_for(p).adam_flat(p, g, m, v, p_lowp, float(lr), float(b1), float(b2), float(eps),
                                        float(bc1), float(bc2), float(grad_scale))
        return
    ref.adam_step(p, g, m, v, step, lr, b1, b2, eps, grad_scale)
    if p_lowp is not None:
        p_lowp.copy_(p)


def dedup(ids: torch.Tensor, num_news: int):
    """Unique news ids of a batch -> ``(uniq [U], inv [R], perm [R], seg_ptr [U+1])``.

    ``uniq`` is sorted (deterministic), ``inv[r]`` maps each occurrence to its row of
    ``uniq``, ``perm``/``seg_ptr`` group occurrences by row for :func:`segment_sum_rows`.
    """
    flat = ids.reshape(-1)
    if _dev(flat):
        return tuple(native.require_for(flat).dedup(flat.to(torch.int32).contiguous(), int(num_news)))
    uniq, inv = torch.unique(flat.long(), sorted=True, return_inverse=True)
    perm, ptr = segments_from_inv(inv, uniq.numel())
    return uniq.to(torch.int32), inv.to(torch.int32), perm, ptr


# ---- small fp32 GEMMs on MFMA (csrc/small_gemm.hip) ------------------------------------------
class Gemm:
    """One GEMM of a :func:`small_gemm` launch: ``C = act(alpha * A(m,k) B(n,k) + bias) (+C)``.

    ``a_mode`` 0: A row-major [M, K] (``gather_on=1``: row m is ``A[gidx[m]]``); 1: A stored
    [K, M].  ``b_mode`` 0: B [N, K]; 1: B stored [K, N] (``gather_on=2``: row k is
    ``B[gidx[k]]``).  ``drop_on`` 1/2/3: Philox dropout (p, seed, offset) on A elements
    (m, k), on B elements (k, n), or on the output (m, n), element index ``row * drop_ld +
    col`` in the logical (gathered) matrix -- the mask of ``ops.dropout_add``."""

    __slots__ = ("A", "B", "C", "M", "N", "K", "lda", "ldb", "ldc", "a_mode", "b_mode", "act", "accumulate",
                 "alpha", "bias", "gidx", "gather_on", "pdrop", "drop_on", "drop_ld", "seed", "offset", "bseg", "kseg",
                 "asum")

    def __init__(self, A, B, C, M, N, K, lda, ldb, ldc, a_mode=0, b_mode=0, act=0, accumulate=False, alpha=1.0,
                 bias=None, gidx=None, gather_on=0, pdrop=0.0, drop_on=0, drop_ld=0, seed=0, offset=0,
                 bseg=(), kseg=0, asum=None):
        self.A, self.B, self.C = A, B, C
        self.M, self.N, self.K, self.lda, self.ldb, self.ldc = int(M), int(N), int(K), int(lda), int(ldb), int(ldc)
        self.a_mode, self.b_mode, self.act, self.accumulate = int(a_mode), int(b_mode), int(act), bool(accumulate)
        self.alpha, self.bias, self.gidx, self.gather_on = float(alpha), bias, gidx, int(gather_on)
        self.pdrop, self.drop_on, self.drop_ld = float(pdrop), int(drop_on), int(drop_ld)
        self.seed, self.offset = int(seed), int(offset)
        # K-segmented B (b_mode 1): rows [0, kseg) of B, [kseg, 2 kseg) of bseg[0], then bseg[1]
        self.bseg, self.kseg = tuple(bseg), int(kseg)
        # a_mode 1 only: asum[m] = sum_k A(m, k) in fp32 from the raw A values the GEMM stages
        # (a weight gradient's bias gradient dY^T 1 in the same launch)
        self.asum = asum


def gather_dropout(v: torch.Tensor, idx: torch.Tensor, p: float, seed: int, offset: int, dev_off=None,
                   bf16_out: bool = False) -> torch.Tensor:
    """``v[idx] * Z``: rows of ``v`` gathered and dropped out with the counter mask of element
    ``m * K + k`` (offset + ``*dev_off``) -- the mask ``small_gemm``'s dropout loads use.  fp32,
    or bf16 (``bf16_out``: the fp32 product rounded once, as a bf16-operand GEMM would)."""
    if _dev(v):
        return native.require_for(v).gather_dropout(v.contiguous(), idx.to(torch.int32).contiguous(), float(p),
                                                    int(seed), int(offset), dev_off, bool(bf16_out))
    x = v.index_select(0, idx.long())
    if p > 0:
        off = int(offset) + (int(dev_off.item()) if dev_off is not None else 0)
        idx_e = torch.arange(x.numel(), device=x.device, dtype=torch.int64)
        x = x * ref.dropout_scale(idx_e, p, int(seed), off).view_as(x).to(x.dtype)
    return x.to(torch.bfloat16) if bf16_out else x


def small_gemm(*gs: Gemm, dev_off=None, tile: int = 0) -> None:
    """Run up to 6 independent GEMMs in one launch (device only).  ``dev_off``: an int64[1]
    device counter added to every dropout offset (HIP-graph replays draw fresh masks).
    Operands A / B may be fp32 or bf16 (C fp32).  ``tile``: 0 = the launcher's choice, 1..4 =
    64x64 / 128x64 / 64x128 / 128x128, 5 = 64x64 without the LDS-DMA ring of the bf16 x bf16
    k-contiguous launches (benchmarks / tests)."""
    ints, floats, seeds = [], [], []
    for g in gs:
        ints += [g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.a_mode, g.b_mode, g.act, int(g.accumulate), g.drop_ld,
                 g.drop_on, g.gather_on, g.kseg]
        floats += [g.alpha, g.pdrop]
        seeds += [g.seed, g.offset]
    native.require_for(gs[0].A).small_gemm([g.A for g in gs], [g.gidx for g in gs], [g.B for g in gs],
                                           [g.bias for g in gs], [g.C for g in gs], ints, floats, seeds, dev_off,
                                           [t for g in gs for t in g.bseg], int(tile), [g.asum for g in gs])


def small_gemm_ref(g: Gemm) -> torch.Tensor:
    """fp32 torch emulation of one :class:`Gemm` (operands rounded to bf16 like the kernel)
    -> the new ``C`` [M, N] (tests)."""
    def rows(t, n_rows, n_cols, ld, gidx=None):  # strided view semantics of the kernel (base + r * ld + c)
        flat = torch.as_strided(t, (t.untyped_storage().nbytes() // t.element_size() - t.storage_offset(),), (1,),
                                t.storage_offset())
        idx = gidx.long()[:n_rows] if gidx is not None else torch.arange(n_rows, device=t.device)
        return flat[(idx[:, None] * ld + torch.arange(n_cols, device=t.device)[None, :]).reshape(-1)].view(
            n_rows, n_cols).float()

    def drop(x):  # logical element (r, c) -> index r * drop_ld + c
        idx = (torch.arange(x.shape[0], device=x.device)[:, None] * g.drop_ld
               + torch.arange(x.shape[1], device=x.device)[None, :]).cpu()
        return x * ref.dropout_scale(idx, g.pdrop, g.seed, g.offset).to(x.device)

    A = rows(g.A, g.M, g.K, g.lda, g.gidx if g.gather_on == 1 else None) if g.a_mode == 0 else rows(g.A, g.K, g.M, g.lda).t()
    if g.drop_on == 1:
        A = drop(A)
    if g.b_mode == 0:
        Bm = rows(g.B, g.N, g.K, g.ldb)  # [N, K]
    elif g.kseg:
        Bm = torch.cat([rows(t, min(g.kseg, g.K - i * g.kseg), g.N, g.ldb)
                        for i, t in enumerate((g.B, *g.bseg)) if i * g.kseg < g.K]).t()
    else:
        Bk = rows(g.B, g.K, g.N, g.ldb, g.gidx if g.gather_on == 2 else None)  # [K, N]
        if g.drop_on == 2:
            Bk = drop(Bk)
        Bm = Bk.t()
    A = A.to(torch.bfloat16).float()
    Bm = Bm.to(torch.bfloat16).float()
    out = g.alpha * (A @ Bm.t())
    if g.bias is not None:
        out = out + g.bias.float()[:g.N]
    if g.act == 1:
        out = torch.tanh(out)
    if g.drop_on == 3:
        out = drop(out)
    if g.accumulate:
        out = out + rows(g.C, g.M, g.N, g.ldc)
    return out


def colsum_f32(pairs, accumulate: bool = False) -> None:
    """``out[:N] (+)= X[:M, :N].sum(0)`` for each ``(X, out, M, N, ld)`` (one deterministic launch)."""
    ints = []
    for X, out, M, N, ld in pairs:
        ints += [int(M), int(N), int(ld), int(accumulate)]
    native.require_for(pairs[0][0]).colsum_f32([p[0] for p in pairs], [p[1] for p in pairs], ints)
