"""Torch-eager oracle for every fused op (fp32).  This is both the CPU execution path
(BASELINE config 1: CPU/gloo plumbing) and the numerics reference that each HIP kernel is
tested against.

Math is traced to the reference:

* DistilBERT block: HF post-LN block; attention scores ``q k^T / sqrt(d)`` with key padding
  filled with ``finfo.min`` (so an all-zero mask -- news row 0 -- gives a *uniform*
  softmax, E1/K03), GELU(erf) FFN, LayerNorm eps 1e-12.
* Additive attention (``attention.py:14-26``): ``alpha = exp(a) / (sum exp(a) + 1e-8)``
  with ``a = w2 . tanh(W1 x + b1) + b2``; no mask (Q7).
* Scaled dot-product attention (``attention.py:37-45``): ``A = exp(S) / (rowsum + 1e-8)``,
  no max subtraction (Q8), no mask.
* Score (``model.py:121-126``): ``CE(sigmoid(<cand, u>), label=0)``, mean over the batch.

The eps-normalised softmaxes are evaluated in the algebraically identical stable form
``exp(s - m) / (sum exp(s - m) + eps * exp(-m))`` (identical in exact arithmetic; the
literal form overflows for scores > 88).  ``literal=True`` selects the reference's form.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

EPS_SOFTMAX = 1e-8


def _f(t: torch.Tensor) -> torch.Tensor:
    """Compute dtype of the oracle: fp32, or fp64 when the caller is in fp64 (tests)."""
    return t if t.dtype == torch.float64 else t.float()


# ---------------------------------------------------------------------------------------
# eps-softmax helpers
# ---------------------------------------------------------------------------------------
def eps_softmax(s: torch.Tensor, dim: int, eps: float = EPS_SOFTMAX, literal: bool = False,
                keep: torch.Tensor | None = None) -> torch.Tensor:
    """``exp(s) / (sum exp(s) + eps)`` in the stable form.  ``keep`` (bool, broadcastable to
    ``s``): masked entries get weight exactly 0; a slice with every entry masked is all 0
    (max taken as 0) -- the kernels' mask_padding semantics."""
    if keep is not None:
        s = s.masked_fill(~keep, float("-inf"))
        m = s.amax(dim, keepdim=True)
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        e = torch.exp(s - m)
        return e / (e.sum(dim, keepdim=True) + eps * torch.exp(-m))
    if literal:
        e = torch.exp(s)
        return e / (e.sum(dim, keepdim=True) + eps)
    m = s.amax(dim, keepdim=True).clamp_min(-1e30)
    e = torch.exp(s - m)
    return e / (e.sum(dim, keepdim=True) + eps * torch.exp(-m))


def eps_softmax_backward(p: torch.Tensor, dp: torch.Tensor, dim: int) -> torch.Tensor:
    """``d s`` for ``p = eps_softmax(s)``: the eps term only rescales, so the Jacobian keeps
    the softmax form ``p (dp - sum p dp)``."""
    return p * (dp - (p * dp).sum(dim, keepdim=True))


# ---------------------------------------------------------------------------------------
# counter-based RNG (bit-exact twin of csrc/common.h Philox / drop_scale)
# ---------------------------------------------------------------------------------------
_U32 = 0xFFFFFFFF


def philox4x32(seed: int, offset: int, ctr: torch.Tensor) -> torch.Tensor:
    """Philox-4x32-10 (Salmon et al. 2011) with the kernels' layout: counter words
    (ctr lo, ctr hi, offset lo, offset hi), key (seed lo, seed hi).  ``ctr`` int64 -> ``[..., 4]``
    int64 holding uint32 values.  int64 products wrap mod 2^64, which keeps the low 64 bits of
    the 32x32 product exact -- all mul-hi / mul-lo need."""
    ctr = ctr.to(torch.int64)
    c0, c1 = ctr & _U32, (ctr >> 32) & _U32
    c2 = torch.full_like(ctr, int(offset) & _U32)
    c3 = torch.full_like(ctr, (int(offset) >> 32) & _U32)
    k0, k1 = int(seed) & _U32, (int(seed) >> 32) & _U32
    for _ in range(10):
        p0 = c0 * 0xD2511F53
        p1 = c2 * 0xCD9E8D57
        c0, c1, c2, c3 = ((p1 >> 32) & _U32) ^ c1 ^ k0, p1 & _U32, ((p0 >> 32) & _U32) ^ c3 ^ k1, p0 & _U32
        k0 = (k0 + 0x9E3779B9) & _U32
        k1 = (k1 + 0xBB67AE85) & _U32
    return torch.stack([c0, c1, c2, c3], -1)


def _keep_scale(words: torch.Tensor, p: float) -> torch.Tensor:
    """uint32 words (int64) -> dropout multipliers: keep / (1 - p), keep iff unit(x) > p."""
    u = ((words >> 8) + 1).to(torch.float32) * (1.0 / 16777216.0)
    pf = torch.tensor(p, dtype=torch.float32)
    inv_keep = torch.tensor(1.0, dtype=torch.float32) / (1.0 - pf)
    return torch.where(u > pf, inv_keep, torch.zeros((), dtype=torch.float32))


def dropout_scale(index: torch.Tensor, p: float, seed: int, offset: int) -> torch.Tensor:
    """Dropout multiplier of element ``index`` (int64): ``keep / (1 - p)`` with keep iff
    ``unit(x) > p`` where x = component ``index & 3`` of Philox counter ``index >> 2``."""
    x = philox4x32(seed, offset, index >> 2).gather(-1, (index & 3).unsqueeze(-1)).squeeze(-1)
    return _keep_scale(x, p)


def dropout_add(h: torch.Tensor, res: Optional[torch.Tensor], p: float, seed: int, offset: int) -> torch.Tensor:
    """``res + h o Z`` with Z the element-indexed mask of ``csrc/dropout.hip`` (one Philox
    call per 4 consecutive elements, as the kernel)."""
    n = h.numel()
    words = philox4x32(seed, offset, torch.arange((n + 3) // 4, device=h.device)).reshape(-1)[:n]
    z = _keep_scale(words, p).view(h.shape).to(_f(h).dtype)
    out = _f(h) * z
    return out if res is None else out + _f(res)


def attention_dropout_scale(n: int, n_heads: int, T: int, p: float, seed: int, offset: int) -> torch.Tensor:
    """``[n, h, T, T]`` multipliers of the attention probabilities: element (title, head, t, s)
    is mask index ``((title * h + head) * 64 + t) * 64 + s`` (title_attn.hip, T <= 64), i.e.
    Philox counter ``(pair * 64 + t) * 16 + s // 4``, word ``s % 4``."""
    g = (T + 3) // 4
    pair = torch.arange(n * n_heads, dtype=torch.int64).view(-1, 1, 1)
    t = torch.arange(T, dtype=torch.int64).view(1, T, 1)
    q = torch.arange(g, dtype=torch.int64).view(1, 1, g)
    words = philox4x32(seed, offset, (pair * 64 + t) * 16 + q).reshape(n * n_heads, T, 4 * g)[..., :T]
    return _keep_scale(words, p).view(n, n_heads, T, T)


# ---------------------------------------------------------------------------------------
# text backbone (DistilBERT-shaped) pieces
# ---------------------------------------------------------------------------------------
def embed_ln(tokens: torch.Tensor, word: torch.Tensor, pos: torch.Tensor, ln_w: torch.Tensor,
             ln_b: torch.Tensor, eps: float) -> torch.Tensor:
    """``LN(word[tok] + pos[0..T-1])`` -> ``[n*T, D]`` (HF Embeddings, eval mode)."""
    n, T = tokens.shape
    # F.embedding(padding_idx=0) like HF's nn.Embedding: the pad row gets no gradient
    x = F.embedding(tokens.long(), word, padding_idx=0) + pos[:T].unsqueeze(0)
    x = F.layer_norm(_f(x), (word.shape[1],), _f(ln_w), _f(ln_b), eps)
    return x.reshape(n * T, -1)


def linear(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], act: str = "none",
           residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    y = _f(x) @ _f(w).t()
    if b is not None:
        y = y + _f(b)
    if act == "gelu":
        y = F.gelu(y)  # erf form (HF "gelu")
    elif act == "tanh":
        y = torch.tanh(y)
    elif act != "none":
        raise ValueError(act)
    if residual is not None:
        y = y + _f(residual)
    return y


def layer_norm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float) -> torch.Tensor:
    return F.layer_norm(_f(x), (x.shape[-1],), _f(w), _f(b), eps)


def title_attention(qkv: torch.Tensor, mask: torch.Tensor, n_heads: int, drop=None) -> torch.Tensor:
    """HF DistilBERT eager attention.  ``qkv`` ``[n*T, 3D]`` (q | k | v), ``mask`` ``[n, T]``;
    ``drop = (p, seed, offset)``: train-mode dropout on the probabilities (HF
    ``nn.functional.dropout(attn_weights)``) with the kernels' Philox mask."""
    n, T = mask.shape
    D = qkv.shape[1] // 3
    dh = D // n_heads
    q, k, v = _f(qkv).view(n, T, 3, n_heads, dh).permute(2, 0, 3, 1, 4)
    q = q / math.sqrt(dh)
    s = q @ k.transpose(-1, -2)  # [n, h, T, T]
    keep = (mask != 0).view(n, 1, 1, T)
    s = s.masked_fill(~keep, torch.finfo(torch.float32).min)
    p = torch.softmax(s, dim=-1)
    if drop is not None:
        p = p * attention_dropout_scale(n, n_heads, T, *drop).to(p.device, p.dtype)
    ctx = p @ v  # [n, h, T, dh]
    return ctx.permute(0, 2, 1, 3).reshape(n * T, D)


def backbone_forward(tokens: torch.Tensor, mask: torch.Tensor, params: dict, n_layers: int,
                     n_heads: int, eps: float) -> torch.Tensor:
    """Whole frozen backbone in eval mode -> last hidden state ``[n*T, D]`` (fp32)."""
    x = embed_ln(tokens, params["word"], params["pos"], params["emb_ln_w"], params["emb_ln_b"], eps)
    for i in range(n_layers):
        L = params["layers"][i]
        qkv = linear(x, L["wqkv"], L["bqkv"])
        ctx = title_attention(qkv, mask, n_heads)
        h = linear(ctx, L["wo"], L["bo"], residual=x)
        x = layer_norm(h, L["ln1_w"], L["ln1_b"], eps)
        f = linear(x, L["w1"], L["b1"], act="gelu")
        h = linear(f, L["w2"], L["b2"], residual=x)
        x = layer_norm(h, L["ln2_w"], L["ln2_b"], eps)
    return x


# ---------------------------------------------------------------------------------------
# additive attention pooling (text head and user encoder)
# ---------------------------------------------------------------------------------------
def additive_pool_fwd(x: torch.Tensor, e: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
                      literal: bool = False, keep: torch.Tensor | None = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``x [n,T,D]``, ``e = tanh(W1 x + b1) [n,T,Q]`` -> ``(pooled [n,D], alpha [n,T])``;
    ``keep [n,T]`` (nonzero = pooled) masks positions (mask_padding)."""
    a = _f(e) @ _f(w2).reshape(-1) + _f(b2).reshape(())
    alpha = eps_softmax(a, dim=1, literal=literal, keep=None if keep is None else keep != 0)
    pooled = torch.einsum("nt,ntd->nd", alpha, _f(x))
    return pooled, alpha


def additive_pool_bwd(x: torch.Tensor, e: torch.Tensor, alpha: torch.Tensor, w2: torch.Tensor,
                      g: torch.Tensor):
    """Backward of :func:`additive_pool_fwd` -> ``(dx_direct [n,T,D], de [n,T,Q], dw2 [Q], db2 [])``.

    ``dx_direct`` is the ``alpha_t g`` term only; the ``W1^T dpre`` term is added by the
    caller (``dpre = de * (1 - e^2)``: ``e`` is a tanh output).
    """
    xf, ef, g = _f(x), _f(e), _f(g)
    dalpha = torch.einsum("ntd,nd->nt", xf, g)
    da = eps_softmax_backward(alpha, dalpha, dim=1)
    dx = alpha.unsqueeze(-1) * g.unsqueeze(1)
    de = da.unsqueeze(-1) * _f(w2).reshape(1, 1, -1)
    dw2 = torch.einsum("nt,ntq->q", da, ef)
    db2 = da.sum()
    return dx, de, dw2, db2


# ---------------------------------------------------------------------------------------
# user-side multi-head attention (attention.py:32-82)
# ---------------------------------------------------------------------------------------
def user_attention_fwd(qkv: torch.Tensor, n_heads: int, head_dim: int,
                       literal: bool = False, keep: torch.Tensor | None = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``qkv [B,H,3*h*d]`` -> ``(ctx [B,H,h*d], A [B,h,H,H])``; ``keep [B,H]`` (nonzero =
    attend) masks keys (mask_padding, attention.py:76-78)."""
    B, H, _ = qkv.shape
    q, k, v = _f(qkv).view(B, H, 3, n_heads, head_dim).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / math.sqrt(head_dim)
    A = eps_softmax(s, dim=-1, literal=literal, keep=None if keep is None else (keep != 0).view(B, 1, 1, H))
    ctx = (A @ v).permute(0, 2, 1, 3).reshape(B, H, n_heads * head_dim)
    return ctx, A


def user_attention_bwd(qkv: torch.Tensor, A: torch.Tensor, dctx: torch.Tensor, n_heads: int,
                       head_dim: int) -> torch.Tensor:
    B, H, _ = qkv.shape
    q, k, v = _f(qkv).view(B, H, 3, n_heads, head_dim).permute(2, 0, 3, 1, 4)
    dc = _f(dctx).view(B, H, n_heads, head_dim).permute(0, 2, 1, 3)
    dA = dc @ v.transpose(-1, -2)
    dv = A.transpose(-1, -2) @ dc
    dS = eps_softmax_backward(A, dA, dim=-1) / math.sqrt(head_dim)
    dq = dS @ k
    dk = dS.transpose(-1, -2) @ q
    d = torch.stack([dq, dk, dv], 0)  # [3,B,h,H,d]
    return d.permute(1, 3, 0, 2, 4).reshape(B, H, 3 * n_heads * head_dim)


# ---------------------------------------------------------------------------------------
# scoring + loss (model.py:121-126)
# ---------------------------------------------------------------------------------------
def score_ce_fwd_bwd(cand: torch.Tensor, user: torch.Tensor, act: str = "sigmoid",
                     label: int = 0):
    """Returns ``(loss, scores [B,C], dcand [B,C,D], duser [B,D])`` for a mean CE over the
    batch with target column ``label`` (always 0 in the reference, ``dataset.py:85``)."""
    c, u = _f(cand), _f(user)
    z = torch.einsum("bcd,bd->bc", c, u)
    s = torch.sigmoid(z) if act == "sigmoid" else z
    B = s.shape[0]
    lse = torch.logsumexp(s, dim=1)
    loss = (lse - s[:, label]).mean()
    ds = torch.softmax(s, dim=1)
    ds[:, label] -= 1.0
    ds = ds / B
    dz = ds * s * (1.0 - s) if act == "sigmoid" else ds
    dcand = dz.unsqueeze(-1) * u.unsqueeze(1)
    duser = torch.einsum("bc,bcd->bd", dz, c)
    return loss, s, dcand, duser


# ---------------------------------------------------------------------------------------
# per-news gradient reduction (+ LDP) : client.py:26-48, 87-89; model.py:105-109
# ---------------------------------------------------------------------------------------
def segment_sum_rows(rows: torch.Tensor, inv: torch.Tensor, num_out: int,
                     clip: float = 0.0, noise_std: float = 0.0,
                     generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """``out[inv[r]] += clip_r(rows[r]) + N(0, noise_std)`` -> ``[num_out, D]`` (fp32; fp64 for fp64 rows)."""
    g = _f(rows)
    if clip > 0:
        nrm = g.norm(dim=1, keepdim=True)
        g = g * torch.clamp(clip / (nrm + 1e-12), max=1.0)
    if noise_std > 0:
        g = g + torch.randn(g.shape, generator=generator, device=g.device).to(g.dtype) * noise_std
    out = torch.zeros(num_out, g.shape[1], dtype=g.dtype, device=g.device)
    out.index_add_(0, inv.long(), g)
    return out


# ---------------------------------------------------------------------------------------
# Adam (torch defaults: no weight decay, no amsgrad; bias correction)
# ---------------------------------------------------------------------------------------
def adam_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: int,
              lr: float, b1: float, b2: float, eps: float, grad_scale: float = 1.0) -> None:
    gs = g * grad_scale
    m.mul_(b1).add_(gs, alpha=1 - b1)
    v.mul_(b2).addcmul_(gs, gs, value=1 - b2)
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
    p.addcdiv_(m, denom, value=-lr / bc1)


def title_plan(mask: torch.Tensor):
    """Oracle of the title_count/title_rows kernels: kv rows (mask 1, or every row of an all-masked title)
    first, title-major in position order, then the query-only rows; ``kv_len < 0`` marks an
    all-masked title; ``qstart`` = each title's first query-only row."""
    m = mask.to(torch.int64) != 0
    n, T = m.shape
    allm = ~m.any(1)
    kv = m | allm[:, None]
    cnt = kv.sum(1)
    kv_start = torch.cumsum(cnt, 0) - cnt
    R = int(cnt.sum())
    rank_kv = torch.cumsum(kv.long(), 1) - kv.long()
    rank_q = torch.cumsum((~kv).long(), 1) - (~kv).long()
    q_start = R + torch.arange(n) * T - kv_start
    rowmap = torch.where(kv, kv_start[:, None] + rank_kv, q_start[:, None] + rank_q)
    src = torch.empty(n * T, dtype=torch.int64)
    src[rowmap.reshape(-1)] = torch.arange(n * T)
    kv_len = torch.where(allm, -T * torch.ones_like(cnt), cnt)
    qstart = q_start
    i32 = torch.int32
    return (rowmap.to(i32), src.to(i32), kv_start.to(i32), kv_len.to(i32), qstart.to(i32),
            torch.tensor([R], dtype=i32))


# ---------------------------------------------------------------------------------------
# Catalog top-k (oracle of csrc/topk_scores.hip)
# ---------------------------------------------------------------------------------------
def topk_scores(user: torch.Tensor, table: torch.Tensor, k: int, exclude: Optional[torch.Tensor] = None,
                min_id: int = 0, chunk: int = 256):
    """``s[b, n] = user[b] . table[n]`` in the dtype given -> ``(scores [B, k], ids [B, k] int32)``:
    the ``k`` best rows of each user by (score descending, id ascending) among the eligible rows
    -- ``n >= min_id``, ``n`` not in ``exclude[b, :]`` (entries < 0 or >= N and duplicates are
    ignored), ``s[b, n]`` not NaN.  Slots past the eligible count hold ``(-inf, -1)``.  Users run
    in chunks, so at most a ``[chunk, N]`` block of scores exists at a time.  The order comes from
    two stable sorts (score descending over the ascending ids, then eligible rows first), never
    from ``torch.topk``'s tie order."""
    B, N = user.shape[0], table.shape[0]
    k = int(k)
    scores = torch.full((B, k), float("-inf"), dtype=user.dtype)
    ids = torch.full((B, k), -1, dtype=torch.int32)
    kk = min(k, N)
    row_ok = torch.arange(N) >= int(min_id)
    for s in range(0, B, chunk):
        sc = user[s:s + chunk] @ table.t()
        c = sc.shape[0]
        elig = row_ok[None, :] & ~torch.isnan(sc)
        if exclude is not None and exclude.shape[1] > 0:
            ex = exclude[s:s + chunk].long()
            hit = torch.zeros(c, N + 1, dtype=torch.bool)
            hit.scatter_(1, torch.where((ex >= 0) & (ex < N), ex, torch.full_like(ex, N)), True)
            elig &= ~hit[:, :N]
        key = torch.where(elig, sc, torch.full_like(sc, float("-inf")))
        order = torch.sort(key, dim=1, descending=True, stable=True).indices
        # eligible rows first (an eligible score may itself be -inf); stable: keeps the order above
        front = torch.sort((~elig).gather(1, order).to(torch.int8), dim=1, stable=True).indices
        top = order.gather(1, front)[:, :kk]
        ok = elig.gather(1, top)
        scores[s:s + c, :kk] = torch.where(ok, sc.gather(1, top), torch.full_like(sc[:, :kk], float("-inf")))
        ids[s:s + c, :kk] = torch.where(ok, top, torch.full_like(top, -1)).to(torch.int32)
    return scores, ids


# ---------------------------------------------------------------------------------------
# Full-impression ranking (oracle of csrc/rank_impressions.hip)
# ---------------------------------------------------------------------------------------
def rank_impressions(user: torch.Tensor, table: torch.Tensor, pos: torch.Tensor, neg_ptr: torch.Tensor,
                     negs: torch.Tensor, row0: int = 0, chunk: int = 1 << 16) -> torch.Tensor:
    """User ``b`` is impression ``row0 + b`` of the corpus CSR (``pos [I]``, ``neg_ptr [I + 1]``,
    ``negs [M]``) -> ``counts [B, 4]`` int32 ``(n_gt, n_eq, n_neg, n_nan)``: the negatives whose score
    ``user[b] . table[n]`` (in the dtype given) is greater than / equal to the positive's, the list
    length, and the candidates -- positive included -- whose score is NaN (NaN compares false: in
    neither count).  Every score, the positive's too, is the same row-wise ``(u * v).sum(-1)``, so a
    negative with the positive's id ties bitwise.  At most ``chunk`` gathered rows exist at a time."""
    B, row0 = user.shape[0], int(row0)
    I = pos.numel()
    if neg_ptr.numel() != I + 1 or row0 < 0 or row0 + B > I:
        raise ValueError(f"rank_impressions: neg_ptr [I + 1], 0 <= row0, row0 + B <= I (row0 {row0}, B {B}, I {I})")
    ptr = neg_ptr[row0:row0 + B + 1].long()
    lens = ptr[1:] - ptr[:-1]
    sp = (user * table.index_select(0, pos[row0:row0 + B].long())).sum(-1)
    seg = torch.repeat_interleave(torch.arange(B), lens)
    ids = negs[int(ptr[0]):int(ptr[-1])].long()
    cmp = torch.zeros(3, B, dtype=torch.int64)  # gt, eq, nan
    for s in range(0, ids.numel(), chunk):
        sg = seg[s:s + chunk]
        sc = (user.index_select(0, sg) * table.index_select(0, ids[s:s + chunk])).sum(-1)
        p = sp.index_select(0, sg)
        for r, m in enumerate((sc > p, sc == p, torch.isnan(sc))):
            cmp[r].index_add_(0, sg, m.to(torch.int64))
    cmp[2] += torch.isnan(sp).to(torch.int64)
    return torch.stack([cmp[0], cmp[1], lens, cmp[2]], 1).to(torch.int32)


# ---------------------------------------------------------------------------------------
# Diversity re-rank (oracle of csrc/mmr_rerank.hip)
# ---------------------------------------------------------------------------------------
def mmr_rerank(table: torch.Tensor, ids: torch.Tensor, rel: torch.Tensor, k: int, lam: float,
               chunk_elems: int = 1 << 24):
    """Maximal Marginal Relevance over a candidate pool, in ``table``'s dtype -> ``(ids_out [B, k]
    int32, rel_out [B, k], ild [B])``.  Slot ``j`` of ``ids [B, P]`` is valid iff ``ids[b, j] >= 0``;
    ``rhat = (rel - min) / (max - min)`` over the valid slots (1 when ``max == min``); ``c_ij`` is the
    cosine of table rows ``ids_i`` and ``ids_j`` (``g_ij / (sqrt(g_ii) * sqrt(g_jj))``, 0 unless both
    norms are finite and positive and ``g_ij`` is finite).  Step ``t`` picks the not-yet-picked valid
    slot with the largest ``m_j = lam * rhat_j - (1 - lam) * max_{i picked} c_ij`` (``lam * rhat_j`` at
    ``t = 0``; a NaN ``m_j`` counts as ``-inf``; ties go to the lowest position).  Outputs are in
    selection order, ``rel_out`` the picks' original ``rel``, ``(-1, -inf)`` past the valid count;
    ``ild`` is the mean of ``1 - c_ij`` over the unordered pairs of picks (0 below two picks).  The
    Gram is a row-wise ``(x_i * x_j).sum(-1)`` -- one summation order for every pair, so duplicate
    rows tie bit for bit -- built for a few users at a time (``chunk_elems`` products at most)."""
    B, P = ids.shape
    D = table.shape[1]
    k, dt = int(k), table.dtype
    if not (1 <= k <= P) or not (0.0 <= float(lam) <= 1.0):
        raise ValueError(f"mmr_rerank: 1 <= k <= P and 0 <= lam <= 1 (got k {k}, P {P}, lam {lam})")
    valid = ids >= 0
    relc = rel.to(dt)
    inf = torch.full_like(relc, float("inf"))
    mn = torch.where(valid, relc, inf).amin(1, keepdim=True)
    mx = torch.where(valid, relc, -inf).amax(1, keepdim=True)
    rhat = torch.where(mx == mn, torch.ones_like(relc), (relc - mn) / (mx - mn))
    c = torch.empty(B, P, P, dtype=dt)
    step = max(1, int(chunk_elems) // (P * P * D))
    for s in range(0, B, step):
        x = table.index_select(0, ids[s:s + step].clamp(min=0).reshape(-1).long()).view(-1, P, D)
        g = (x[:, :, None, :] * x[:, None, :, :]).sum(-1)
        d = g.diagonal(dim1=1, dim2=2)
        ok = torch.isfinite(d) & (d > 0)
        r = torch.sqrt(torch.where(ok, d, torch.ones_like(d)))
        okk = ok[:, :, None] & ok[:, None, :] & torch.isfinite(g)
        c[s:s + step] = torch.where(okk, g / (r[:, :, None] * r[:, None, :]), torch.zeros_like(g))
    lam_t = torch.tensor(float(lam), dtype=dt)
    oml = torch.ones((), dtype=dt) - lam_t
    ids_out = torch.full((B, k), -1, dtype=torch.int32)
    rel_out = torch.full((B, k), float("-inf"), dtype=rel.dtype)
    alive = valid.clone()
    picked = torch.zeros_like(valid)
    ms = torch.zeros(B, P, dtype=dt)
    ar, pos = torch.arange(B), torch.arange(P)[None, :]
    for t in range(k):
        m = lam_t * rhat - oml * ms if t > 0 else lam_t * rhat
        m = torch.where(torch.isnan(m), torch.full_like(m, float("-inf")), m)
        best = torch.where(alive, m, torch.full_like(m, float("-inf"))).amax(1, keepdim=True)
        sel = torch.where(alive & (m == best), pos, torch.full_like(pos, P)).amin(1)
        has = sel < P
        sel = sel.clamp(max=P - 1)
        ids_out[:, t] = torch.where(has, ids[ar, sel].to(torch.int32), ids_out[:, t])
        rel_out[:, t] = torch.where(has, rel[ar, sel], rel_out[:, t])
        hit = has[:, None] & (pos == sel[:, None])
        alive &= ~hit
        picked |= hit
        csel = c[ar, :, sel]
        ms = torch.where(has[:, None], torch.maximum(ms, csel) if t > 0 else csel, ms)
    n_p = picked.sum(1)
    pair = picked[:, :, None] & picked[:, None, :] & torch.ones(P, P, dtype=torch.bool).triu(1)[None]
    tot = torch.where(pair, 1 - c, torch.zeros_like(c)).sum((1, 2))
    npair = (n_p * (n_p - 1) // 2).to(dt)
    ild = torch.where(n_p >= 2, tot / npair.clamp(min=1), torch.zeros_like(tot))
    return ids_out, rel_out, ild


# ---------------------------------------------------------------------------------------
# Byzantine-robust aggregation (oracle of csrc/robust_agg.hip)
# ---------------------------------------------------------------------------------------
def trimmed_mean_check(stack: torch.Tensor, trim: int) -> None:
    """The argument checks of ``fedrec_agg::trimmed_mean``, with its messages."""
    op = "fedrec_agg::trimmed_mean"
    if stack.dtype != torch.float32:
        raise RuntimeError(f"{op}: stack must be fp32")
    if stack.dim() != 2:
        raise RuntimeError(f"{op}: stack [W, n] (got {stack.dim()} dims)")
    if not stack.is_contiguous():
        raise RuntimeError(f"{op}: stack must be contiguous")
    W, n = stack.shape
    if not (1 <= W <= 32 and n >= 1):
        raise RuntimeError(f"{op}: 1 <= W <= 32, n >= 1 (got W {W}, n {n})")
    if not (0 <= 2 * trim < W):
        raise RuntimeError(f"{op}: 0 <= 2 * trim < W (got trim {trim}, W {W})")


def order_keys(x: torch.Tensor) -> torch.Tensor:
    """The monotone uint32 image of fp32 ``x`` (as int64): NaN -> 0xFFFFFFFF, sign bit set ->
    ``~bits``, else ``bits | 0x80000000``; so -inf < ... < -0.0 < +0.0 < ... < +inf < NaN."""
    b = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    k = torch.where(b >= 0x80000000, 0xFFFFFFFF - b, b | 0x80000000)
    return torch.where(torch.isnan(x), torch.full_like(k, 0xFFFFFFFF), k)


def trimmed_mean(stack: torch.Tensor, trim: int, acc_dtype: Optional[torch.dtype] = None, chunk: int = 1 << 20):
    """Coordinate-wise trimmed mean of ``stack [W, n]`` fp32 (1 <= W <= 32, 0 <= 2 trim < W) ->
    ``(out [n], dropped [W] int64)``.

    ``trim > 0``: a coordinate's W values are ranked by ``(order_keys(x), client index)`` -- a total
    order (ties go to the lower client; not ``torch.sort`` on floats, which does not tell -0.0 from
    +0.0).  ``out`` is the sum of ranks ``trim .. W - trim - 1`` in ascending rank order, added left to
    right from the first kept value, then one division by ``W - 2 trim``; a NaN or inf among the kept
    ranks propagates.  ``dropped[c]`` counts the coordinates where client ``c`` ranked among the
    ``trim`` lowest or ``trim`` highest (they sum to ``2 trim n``).  ``trim = (W - 1) // 2`` is the
    median.  ``trim = 0``: nothing is ranked; ``out`` is the sum in CLIENT order over ``W`` -- the
    plain mean bit for bit -- and ``dropped`` is zero.

    Sums and the division run in ``acc_dtype`` (default fp32, the device kernel's arithmetic; fp64
    gives the tests' reference).  At most ``chunk`` columns are ranked at a time."""
    trim = int(trim)
    trimmed_mean_check(stack, trim)
    W, n = stack.shape
    dt = acc_dtype or torch.float32
    m = W - 2 * trim
    out = torch.empty(n, dtype=dt)
    dropped = torch.zeros(W, dtype=torch.int64)
    div = torch.full((1,), float(m), dtype=dt)
    client = torch.arange(W, dtype=torch.int64)[:, None]
    for s in range(0, n, chunk):
        x = stack[:, s:s + chunk]
        if trim == 0:
            v = x.to(dt)
        else:
            idx = torch.sort(order_keys(x) * 32 + client, dim=0).values & 31
            v = torch.gather(x, 0, idx).to(dt)[trim:W - trim]
            cut = torch.cat([idx[:trim], idx[W - trim:]]).reshape(-1)
            dropped += torch.bincount(cut, minlength=W)
        acc = v[0].clone()
        for r in range(1, m):
            acc = acc + v[r]
        out[s:s + chunk] = acc / div.expand_as(acc)
    return out, dropped


# ---------------------------------------------------------------------------------------
# Multi-Krum aggregation (oracle of csrc/krum.hip)
# ---------------------------------------------------------------------------------------
def _krum_stack_check(stack: torch.Tensor, op: str) -> None:
    if stack.dtype != torch.float32:
        raise RuntimeError(f"{op}: stack must be fp32")
    if stack.dim() != 2:
        raise RuntimeError(f"{op}: stack [W, n] (got {stack.dim()} dims)")
    if not stack.is_contiguous():
        raise RuntimeError(f"{op}: stack must be contiguous")
    W, n = stack.shape
    if not (1 <= W <= 32 and n >= 1):
        raise RuntimeError(f"{op}: 1 <= W <= 32, n >= 1 (got W {W}, n {n})")


def krum_gram_check(stack: torch.Tensor, center: torch.Tensor, max_blocks: int = 0) -> None:
    """The argument checks of ``fedrec_krum::centered_gram``, with its messages."""
    op = "fedrec_krum::centered_gram"
    _krum_stack_check(stack, op)
    n = stack.shape[1]
    if center.dtype != torch.float32:
        raise RuntimeError(f"{op}: center must be fp32")
    if not (center.dim() == 1 and center.numel() == n):
        raise RuntimeError(f"{op}: center [n] (got {center.numel()} elements, n {n})")
    if not center.is_contiguous():
        raise RuntimeError(f"{op}: center must be contiguous")
    if not (0 <= max_blocks < 2 ** 31):
        raise RuntimeError(f"{op}: max_blocks >= 0 (got {max_blocks})")
    if stack.device != center.device:
        raise RuntimeError(f"{op}: stack and center must be on one device")


def krum_select_check(G: torch.Tensor, f: int, m: int) -> None:
    """The argument checks of ``fedrec_krum::select``, with its messages."""
    op = "fedrec_krum::select"
    if G.dtype != torch.float64:
        raise RuntimeError(f"{op}: G must be fp64")
    if not (G.dim() == 2 and G.shape[0] == G.shape[1]):
        raise RuntimeError(f"{op}: G [W, W]")
    if not G.is_contiguous():
        raise RuntimeError(f"{op}: G must be contiguous")
    W = G.shape[0]
    if not (1 <= W <= 32):
        raise RuntimeError(f"{op}: 1 <= W <= 32 (got W {W})")
    if not (f >= 0 and W >= 2 * f + 3):
        raise RuntimeError(f"{op}: f >= 0 and W >= 2 f + 3 (got f {f}, W {W})")
    if not (1 <= m <= W - f):
        raise RuntimeError(f"{op}: 1 <= m <= W - f (got m {m}, W {W}, f {f})")


def krum_mean_check(stack: torch.Tensor, selected: torch.Tensor) -> None:
    """The argument checks of ``fedrec_krum::selected_mean``, with its messages."""
    op = "fedrec_krum::selected_mean"
    _krum_stack_check(stack, op)
    W = stack.shape[0]
    if selected.dtype != torch.int32:
        raise RuntimeError(f"{op}: selected must be int32")
    if not (selected.dim() == 1 and selected.numel() == W):
        raise RuntimeError(f"{op}: selected [W] (got {selected.numel()} elements, W {W})")
    if not selected.is_contiguous():
        raise RuntimeError(f"{op}: selected must be contiguous")
    if stack.device != selected.device:
        raise RuntimeError(f"{op}: stack and selected must be on one device")


def krum_gram(stack: torch.Tensor, center: torch.Tensor, max_blocks: int = 0, chunk: int = 1 << 20) -> torch.Tensor:
    """``G = Y Y^T`` fp64 ``[W, W]`` of the centred rows ``Y = stack - center``: the subtraction is one
    fp32 operation per element (as the device kernel's), products and sums run in fp64.  Distances
    ``G_ii + G_jj - 2 G_ij`` do not depend on ``center``; taking it near the rows (the coordinate-wise
    median) keeps them from cancelling.  At most ``chunk`` columns are centred at a time."""
    krum_gram_check(stack, center, int(max_blocks))
    W, n = stack.shape
    G = torch.zeros(W, W, dtype=torch.float64)
    for s in range(0, n, chunk):
        y = (stack[:, s:s + chunk] - center[s:s + chunk]).double()
        G += y @ y.t()
    return G


def krum_select(G: torch.Tensor, f: int, m: int):
    """Krum scores (Blanchard et al. 2017) from a Gram matrix -> ``(selected [W] int32, scores [W] fp32)``.
    ``d_cj = max((G_cc + G_jj) - 2 G_cj, 0)`` in fp64, rounded to fp32, ``+inf`` where the fp64 value is
    not finite; ``score_c`` is the sum of the ``W - f - 2`` smallest ``d_cj`` over ``j != c``, added in
    ascending order in fp32 (a non-finite distance, hence score, ranks highest); the ``m`` clients with
    the lowest ``(score, client index)`` get ``selected = 1``.  ``f >= 0``, ``W >= 2 f + 3``, ``1 <= m <= W -
    f``; ``m = 1`` is plain Krum."""
    f, m = int(f), int(m)
    krum_select_check(G, f, m)
    W = G.shape[0]
    g = G.diagonal()
    t = (g[:, None] + g[None, :]) - 2.0 * G
    inf = torch.full((), float("inf"), dtype=torch.float32)
    d = torch.where(torch.isfinite(t), t.clamp_min(0.0).float(), inf)
    off = ~torch.eye(W, dtype=torch.bool)
    v = torch.sort(d[off].view(W, W - 1), dim=1).values
    scores = v[:, 0].clone()
    for r in range(1, W - f - 2):
        scores = scores + v[:, r]
    order = torch.sort(scores, stable=True).indices[:m]  # stable: ties go to the lower client
    selected = torch.zeros(W, dtype=torch.int32)
    selected[order] = 1
    return selected, scores


def krum_mean(stack: torch.Tensor, selected: torch.Tensor) -> torch.Tensor:
    """The mean of the rows with ``selected != 0``: added in CLIENT order in fp32, left to right from the
    first selected row, then one division by their count (NaN when there is none)."""
    krum_mean_check(stack, selected)
    rows = torch.nonzero(selected).reshape(-1).tolist()
    acc = stack[rows[0]].clone() if rows else torch.zeros(stack.shape[1])
    for c in rows[1:]:
        acc = acc + stack[c]
    return acc / torch.full((1,), float(len(rows)), dtype=torch.float32).expand_as(acc)


# ---------------------------------------------------------------------------------------
# Geometric-median aggregation on the Gram matrix (oracle of csrc/geomed.hip)
# ---------------------------------------------------------------------------------------
GM_ITERS = 32  # Weiszfeld rounds, fixed: the device kernel and this oracle run one recurrence


def geomed_weights_check(G: torch.Tensor) -> None:
    """The argument checks of ``fedrec_geomed::weights``, with its messages."""
    op = "fedrec_geomed::weights"
    if G.dtype != torch.float64:
        raise RuntimeError(f"{op}: G must be fp64")
    if not (G.dim() == 2 and G.shape[0] == G.shape[1]):
        raise RuntimeError(f"{op}: G [W, W]")
    if not G.is_contiguous():
        raise RuntimeError(f"{op}: G must be contiguous")
    if not (1 <= G.shape[0] <= 32):
        raise RuntimeError(f"{op}: 1 <= W <= 32 (got W {G.shape[0]})")


def geomed_combine_check(stack: torch.Tensor, a: torch.Tensor) -> None:
    """The argument checks of ``fedrec_geomed::combine``, with its messages."""
    op = "fedrec_geomed::combine"
    _krum_stack_check(stack, op)
    W = stack.shape[0]
    if a.dtype != torch.float64:
        raise RuntimeError(f"{op}: a must be fp64")
    if not (a.dim() == 1 and a.numel() == W):
        raise RuntimeError(f"{op}: a [W] (got {a.numel()} elements, W {W})")
    if not a.is_contiguous():
        raise RuntimeError(f"{op}: a must be contiguous")
    if stack.device != a.device:
        raise RuntimeError(f"{op}: stack and a must be on one device")


def geomed_weights(G: torch.Tensor, descending: bool = False):
    """Weiszfeld's iteration for the geometric median of ``W`` rows, run on their centred Gram matrix
    ``G [W, W]`` fp64 -> ``(a [W] fp64, dist [W] fp32)``: the aggregate is ``sum_c a_c x_c`` and ``dist_c`` is
    client ``c``'s distance to it.  With ``z = center + sum_c a_c y_c``, ``||x_i - z||^2 = G_ii - 2 (G a)_i +
    a^T G a``: no pass over the stack per round.

    Client ``c`` is valid iff ``G_cc`` is finite; an invalid one gets ``a_c = 0`` and ``dist_c = +inf`` (no
    valid client: every ``a_c`` is NaN).  ``nu2 = 1e-12 m + 1e-300`` smooths the weights, ``m`` the lower median
    of the valid ``G_cc``.  From ``a`` uniform over the valid clients, exactly ``GM_ITERS`` rounds in fp64, each
    product and sum rounded on its own: ``g_c = sum_j G_cj a_j`` over the valid ``j`` in ascending order (the
    columns of invalid clients count as zeros), ``q = sum_c a_c g_c`` over the valid ``c`` ascending, ``d2_c =
    max((G_cc - 2 g_c) + q, 0)``, ``w_c = 1 / sqrt(d2_c + nu2)``, ``a = w / sum_c w_c`` (ascending).
    ``dist_c = fp32(sqrt(d2_c))`` of the last round.  ``descending`` runs the three sums from the highest
    client down: the rounding probe of the tests."""
    geomed_weights_check(G)
    W = G.shape[0]
    diag = G.diagonal().clone()
    valid = torch.isfinite(diag)
    nv = int(valid.sum())
    if nv == 0:
        return torch.full((W,), float("nan"), dtype=torch.float64), torch.full((W,), float("inf"))
    nu2 = 1e-12 * float(torch.sort(diag[valid]).values[(nv - 1) // 2]) + 1e-300
    zero = torch.zeros((), dtype=torch.float64)
    Gm = torch.where(valid[None, :], G, zero)
    a = torch.where(valid, torch.ones(W, dtype=torch.float64) / float(nv), zero)
    order = range(W - 1, -1, -1) if descending else range(W)

    def total(v):  # python floats are IEEE doubles
        s, v = 0.0, v.tolist()
        for c in order:
            s = s + v[c]
        return s

    for _ in range(GM_ITERS):
        g = torch.zeros(W, dtype=torch.float64)
        for j in order:
            g = g + Gm[:, j] * a[j]
        q = total(torch.where(valid, a * g, zero))
        d2 = ((diag - 2.0 * g) + q).clamp_min(0.0)
        w = torch.where(valid, 1.0 / torch.sqrt(d2 + nu2), zero)
        a = w / total(w)
    return a, torch.where(valid, torch.sqrt(d2).float(), torch.full((W,), float("inf")))


def geomed_combine(stack: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
    """``out = sum_c a32_c x_c`` with ``a32 = fp32(a)``, over the clients with ``a32_c != 0`` in CLIENT order:
    the first product initialises the sum, every product and every sum is rounded on its own in fp32.  A row
    of weight zero is never read (a NaN or inf client under weight 0 cannot reach ``out``); a NaN weight makes
    ``out`` NaN everywhere; all-zero weights leave zeros."""
    geomed_combine_check(stack, a)
    a32 = a.float()
    rows = torch.nonzero(a32 != 0).reshape(-1).tolist()
    acc = stack[rows[0]] * a32[rows[0]] if rows else torch.zeros(stack.shape[1])
    for c in rows[1:]:
        acc = acc + stack[c] * a32[c]
    return acc


# ---------------------------------------------------------------------------------------
# Client-level DP on a round delta: clip + noise (oracle of csrc/dp_clip.hip)
# ---------------------------------------------------------------------------------------
DP_L = 1024  # coordinates per chunk of the squared norm
DP_SLOTS = 64  # partial sums of the finishing pass


def _dp_pair_check(local: torch.Tensor, base: torch.Tensor, op: str) -> int:
    if local.dtype != torch.float32 or base.dtype != torch.float32:
        raise RuntimeError(f"{op}: local and base must be fp32")
    if not (local.dim() == 1 and base.dim() == 1):
        raise RuntimeError(f"{op}: local [n] and base [n] (got {local.dim()} and {base.dim()} dims)")
    if not (local.is_contiguous() and base.is_contiguous()):
        raise RuntimeError(f"{op}: local and base must be contiguous")
    n = local.numel()
    if base.numel() != n:
        raise RuntimeError(f"{op}: local and base must have one length (got {n}, {base.numel()})")
    if n < 1:
        raise RuntimeError(f"{op}: n >= 1 (got n {n})")
    if local.device != base.device:
        raise RuntimeError(f"{op}: local and base must be on one device")
    return n


def dp_state_fields(state: torch.Tensor):
    """``(sq fp64, s fp32, clipped int32)`` of a 16-byte privatisation state (one host read)."""
    st = state.detach().cpu().contiguous()
    return float(st.view(torch.float64)[0]), float(st.view(torch.float32)[2]), int(st[3])


def dp_delta_sqnorm(local: torch.Tensor, base: torch.Tensor, max_blocks: int = 0, block: int = 1 << 20) -> torch.Tensor:
    """``|| local - base ||^2`` in fp64 in the device kernel's order -> the state, int32 ``[4]``: bytes 0..7
    ``sq`` (fp64), 8..11 the clip scale ``s`` (fp32) and 12..15 ``clipped`` (int32), both zero until
    :func:`dp_clip_noise` fills them in.

    ``d_k = local_k - base_k`` is one fp32 subtraction; its square is exact in fp64.  Chunk ``p`` covers ``[1024
    p, 1024 (p + 1))``; lane ``l`` of 64 adds the 16 squares of the chunk's coordinate quads ``l, l + 64, l + 128, l +
    192`` in ascending coordinate order from +0.0; the lane sums meet in an xor butterfly 32, 16, 8, 4, 2, 1;
    slot ``t`` of 64 adds the chunk sums ``p = t, t + 64, ...`` ascending, then the slots add in order.  Coordinates
    at and past ``n`` are zeros.  The order depends on ``n`` alone (``max_blocks`` caps the device grid and changes
    nothing; ``block``, a multiple of 65,536, bounds this function's memory)."""
    op = "fedrec_dp::delta_sqnorm"
    n = _dp_pair_check(local, base, op)
    if not (0 <= int(max_blocks) < 2 ** 31):
        raise RuntimeError(f"{op}: max_blocks >= 0 (got {max_blocks})")
    lanes = torch.arange(64)
    slots = torch.zeros(DP_SLOTS, dtype=torch.float64)
    for s0 in range(0, n, block):  # whole groups of 64 chunks: the slot order is kept across blocks
        d = (local[s0:s0 + block] - base[s0:s0 + block]).double()
        P = -(-d.numel() // DP_L)
        sq = torch.zeros(P * DP_L, dtype=torch.float64)
        sq[:d.numel()] = d * d
        sq = sq.view(P, 4, 64, 4).permute(0, 2, 1, 3).reshape(P, 64, 16)
        v = torch.zeros(P, 64, dtype=torch.float64)
        for i in range(16):
            v = v + sq[:, :, i]
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[:, lanes ^ o]
        part = torch.zeros(-(-P // DP_SLOTS) * DP_SLOTS, dtype=torch.float64)  # x + 0.0 is x for a sum of squares
        part[:P] = v[:, 0]
        for row in part.view(-1, DP_SLOTS):
            slots = slots + row
    tot = 0.0 + float(slots[0])
    for t in slots[1:].tolist():  # python floats are IEEE doubles
        tot = tot + t
    state = torch.zeros(4, dtype=torch.int32)
    state.view(torch.float64)[0] = tot
    return state


def dp_normals(n: int, seed: int, offset: int) -> torch.Tensor:
    """The fp32 standard normals of coordinates ``0 .. n - 1`` as ``common.h`` ``box_muller`` forms them: Philox
    counter ``k >> 2`` under ``(seed, offset)``, component ``k & 3``; words (x, y) make components 0 and 1, (z, w)
    2 and 3.  torch's ``log`` / ``sin`` / ``cos`` are not the device's ``logf`` / ``__sincosf``: the bits differ."""
    w = philox4x32(seed, offset, torch.arange((n + 3) // 4))
    u = ((w >> 8) + 1).to(torch.float32) * (1.0 / 16777216.0)
    u1, u2 = u[:, 0::2], u[:, 1::2]
    r = torch.sqrt(-2.0 * torch.log(u1))
    ang = torch.tensor(6.283185307179586, dtype=torch.float32) * u2
    return torch.stack([r * torch.cos(ang), r * torch.sin(ang)], -1).reshape(-1)[:n]


def dp_clip_noise(local: torch.Tensor, base: torch.Tensor, state: torch.Tensor, clip: float, std: float, seed: int,
                  offset: int) -> torch.Tensor:
    """The round delta clipped to L2 norm ``clip`` on top of ``base``, plus Gaussian noise of scale ``std``;
    ``state`` (of :func:`dp_delta_sqnorm` for the same pair) gains ``s`` and ``clipped`` in place.

    ``s = fp32(min(1, clip / sqrt(sq)))``, root and division in IEEE fp64; ``s = 1`` where ``sq`` is 0 or not
    finite.  ``p = local`` where ``s == 1`` (bit for bit), else ``base + s * (local - base)`` with every fp32
    operation rounded on its own.  ``out = p`` when ``std == 0``, else ``p + fp32(std) * z`` with ``z`` of
    :func:`dp_normals`.  ``clipped = (s < 1)``.  ``sq``, ``s``, ``clipped`` and ``p`` are bitwise the device's; the
    noise is not (see :func:`dp_normals`), and need not be: every client draws its own."""
    op = "fedrec_dp::clip_noise"
    n = _dp_pair_check(local, base, op)
    if not (state.dtype == torch.int32 and state.dim() == 1 and state.numel() == 4 and state.is_contiguous()):
        raise RuntimeError(f"{op}: state must be the int32 [4] of delta_sqnorm")
    clip, std = float(clip), float(std)
    if not clip > 0.0:
        raise RuntimeError(f"{op}: clip > 0 (got {clip})")
    std32 = torch.tensor(std, dtype=torch.float32)
    if not (std >= 0.0 and bool(torch.isfinite(std32))):
        raise RuntimeError(f"{op}: 0 <= std < inf (got {std})")
    if local.device != state.device:
        raise RuntimeError(f"{op}: local, base and state must be on one device")
    sq = float(state.view(torch.float64)[0])
    s = torch.ones((), dtype=torch.float32)
    if 0.0 < sq < math.inf:
        r = clip / math.sqrt(sq)
        if r < 1.0:
            s = torch.tensor(r, dtype=torch.float64).float()  # one rounding
    clipped = bool(s < 1)
    state.view(torch.float32)[2] = s
    state[3] = int(clipped)
    p = base + s * (local - base) if clipped else local.clone()
    return p + std32 * dp_normals(n, seed, offset) if std > 0.0 else p


# ---------------------------------------------------------------------------------------
# Top-k sparsified uploads with error feedback (oracle of csrc/sparse_delta.hip)
# ---------------------------------------------------------------------------------------
def _overlaps(a: torch.Tensor, b: torch.Tensor) -> bool:
    pa, pb = a.data_ptr(), b.data_ptr()
    return pa < pb + b.numel() * b.element_size() and pb < pa + a.numel() * a.element_size()


def _check_vec(t: torch.Tensor, op: str, name: str) -> None:
    if t.dtype != torch.float32:
        raise RuntimeError(f"{op}: {name} must be fp32")
    if t.dim() != 1:
        raise RuntimeError(f"{op}: {name} [n] (got {t.dim()} dims)")
    if not t.is_contiguous():
        raise RuntimeError(f"{op}: {name} must be contiguous")


def topk_delta_check(local: torch.Tensor, global_: torch.Tensor, residual: torch.Tensor, k: int) -> None:
    """The argument checks of ``fedrec_sparse::topk_delta``, with its messages."""
    op = "fedrec_sparse::topk_delta"
    _check_vec(local, op, "local")
    _check_vec(global_, op, "global")
    _check_vec(residual, op, "residual")
    n = local.numel()
    if not (global_.numel() == n and residual.numel() == n):
        raise RuntimeError(f"{op}: local, global and residual must have one length (got {n}, {global_.numel()}, "
                           f"{residual.numel()})")
    if not (1 <= n < 2 ** 31):
        raise RuntimeError(f"{op}: 1 <= n < 2^31 (got n {n})")
    if not (1 <= k <= n):
        raise RuntimeError(f"{op}: 1 <= k <= n (got k {k}, n {n})")
    if not (local.device == residual.device and global_.device == residual.device):
        raise RuntimeError(f"{op}: local, global and residual must be on one device")
    if _overlaps(residual, local) or _overlaps(residual, global_):
        raise RuntimeError(f"{op}: residual must not overlap local or global")


def magnitude_keys(a: torch.Tensor) -> torch.Tensor:
    """``bits(a) & 0x7fffffff`` of fp32 ``a`` as int32 (never negative, so it compares as the uint32
    does): +-0 lowest, inf above every finite value, every NaN above inf, ``+x`` and ``-x`` tie."""
    return a.contiguous().view(torch.int32) & 0x7FFFFFFF


def topk_delta(local: torch.Tensor, global_: torch.Tensor, residual: torch.Tensor, k: int):
    """Magnitude top-k with error feedback -> ``(idx [k] int32, val [k] fp32)``; ``residual`` is
    updated in place.

    ``a = (local - global_) + residual`` (one fp32 subtraction, one fp32 addition).  The selected set
    is the first ``k`` entries of a STABLE descending sort of ``magnitude_keys(a)``: the k largest
    magnitudes, NaN above inf above every finite value, the lower index among equal keys.  ``idx`` is
    that set in strictly ascending order, ``val = a[idx]`` (the bits of ``a``, a NaN's payload
    included), and afterwards ``residual`` is ``+0.0`` at ``idx`` and ``a`` elsewhere: what is not sent
    now is added to the next round's delta."""
    k = int(k)
    topk_delta_check(local, global_, residual, k)
    a = (local - global_) + residual
    order = torch.sort(magnitude_keys(a), descending=True, stable=True).indices[:k]
    idx = torch.sort(order).values
    val = a[idx].clone()
    residual.copy_(a)
    residual[idx] = 0.0
    return idx.to(torch.int32), val


def sparse_combine_check(base: torch.Tensor, idx: torch.Tensor, val: torch.Tensor, weights: torch.Tensor) -> None:
    """The argument checks of ``fedrec_sparse::combine``, with its messages."""
    op = "fedrec_sparse::combine"
    _check_vec(base, op, "base")
    if idx.dtype != torch.int32:
        raise RuntimeError(f"{op}: idx must be int32")
    if val.dtype != torch.float32:
        raise RuntimeError(f"{op}: val must be fp32")
    if not (idx.dim() == 2 and val.dim() == 2 and idx.shape == val.shape):
        raise RuntimeError(f"{op}: idx and val [W, k] of one shape")
    if not (idx.is_contiguous() and val.is_contiguous()):
        raise RuntimeError(f"{op}: idx and val must be contiguous")
    _check_vec(weights, op, "weights")
    n, (W, k) = base.numel(), idx.shape
    if not (1 <= n < 2 ** 31):
        raise RuntimeError(f"{op}: 1 <= n < 2^31 (got n {n})")
    if not (1 <= W <= 65536 and weights.numel() == W):
        raise RuntimeError(f"{op}: 1 <= W <= 65536 and weights [W] (got W {W}, weights {weights.numel()})")
    if not (1 <= k <= n):
        raise RuntimeError(f"{op}: 1 <= k <= n (got k {k}, n {n})")
    if not (idx.device == base.device and val.device == base.device and weights.device == base.device):
        raise RuntimeError(f"{op}: base, idx, val and weights must be on one device")


def sparse_combine(base: torch.Tensor, idx: torch.Tensor, val: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
    """``W`` sparse lists scattered onto ``base [n]`` -> ``out [n]`` fp32.  ``idx [W, k]`` int32, each row
    strictly ascending in ``[0, n)`` (the caller's check: :func:`sparse_upload_check`), ``val [W, k]``,
    ``weights [W]``.  ``acc`` starts at ``+0.0``; for ``c = 0 .. W - 1`` in that order ``acc[idx[c]] +=
    weights[c] * val[c]`` (the product and the sum rounded separately); ``wsum`` is the sequential fp32
    sum of the weights from ``+0.0``; ``out = base + acc / wsum`` at every coordinate."""
    sparse_combine_check(base, idx, val, weights)
    acc = torch.zeros_like(base)
    ws = torch.zeros((), dtype=torch.float32)
    for c in range(idx.shape[0]):
        ix = idx[c].long()
        acc[ix] = acc[ix] + weights[c] * val[c]
        ws = ws + weights[c]
    return base + acc / ws


def sparse_upload_check(idx: torch.Tensor, val: torch.Tensor, n: int, k: int) -> None:
    """A sparse upload as :func:`topk_delta` makes it: ``idx`` int32 ``[k]`` strictly ascending within
    ``[0, n)``, ``val`` fp32 ``[k]``.  Raises ``ValueError`` naming the first violation."""
    if idx.dtype != torch.int32:
        raise ValueError(f"sparse upload: idx must be int32 (got {idx.dtype})")
    if val.dtype != torch.float32:
        raise ValueError(f"sparse upload: val must be fp32 (got {val.dtype})")
    if idx.dim() != 1 or idx.numel() != k:
        raise ValueError(f"sparse upload: idx must have length {k} (got shape {tuple(idx.shape)})")
    if val.dim() != 1 or val.numel() != k:
        raise ValueError(f"sparse upload: val must have length {k} (got shape {tuple(val.shape)})")
    i = idx.long()
    bad = ((i < 0) | (i >= n)).nonzero()
    if bad.numel():
        j = int(bad[0])
        raise ValueError(f"sparse upload: idx[{j}] = {int(i[j])} is outside [0, {n})")
    bad = (i[1:] <= i[:-1]).nonzero()
    if bad.numel():
        j = int(bad[0]) + 1
        raise ValueError(f"sparse upload: idx is not strictly ascending at {j} ({int(i[j - 1])} then {int(i[j])})")


# ---------------------------------------------------------------------------------------
# Block-quantized uploads with error feedback (oracle of csrc/quant_delta.hip)
# ---------------------------------------------------------------------------------------
QUANT_GROUP = 256  # coordinates per scale block


def quant_levels(bits: int) -> int:
    """``Q = 2^(bits - 1) - 1``: codes run over ``[-Q, Q]`` (127 at 8 bits, 7 at 4)."""
    return (1 << (int(bits) - 1)) - 1


def quant_sizes(n: int, bits: int) -> Tuple[int, int]:
    """``(bytes of codes, scale blocks)`` of ``n`` coordinates."""
    return (int(n) * int(bits) + 7) // 8, (int(n) + QUANT_GROUP - 1) // QUANT_GROUP


def _canonical_nan() -> torch.Tensor:
    return torch.tensor([0x7FC00000], dtype=torch.int32).view(torch.float32)[0]


def quantize_delta_check(local: torch.Tensor, global_: torch.Tensor, residual: torch.Tensor, bits: int) -> None:
    """The argument checks of ``fedrec_quant::quantize_delta``, with its messages."""
    op = "fedrec_quant::quantize_delta"
    _check_vec(local, op, "local")
    _check_vec(global_, op, "global")
    _check_vec(residual, op, "residual")
    n = local.numel()
    if not (global_.numel() == n and residual.numel() == n):
        raise RuntimeError(f"{op}: local, global and residual must have one length (got {n}, {global_.numel()}, "
                           f"{residual.numel()})")
    if not (1 <= n < 2 ** 31):
        raise RuntimeError(f"{op}: 1 <= n < 2^31 (got n {n})")
    if bits not in (8, 4):
        raise RuntimeError(f"{op}: bits must be 8 or 4 (got {bits})")
    if not (local.device == residual.device and global_.device == residual.device):
        raise RuntimeError(f"{op}: local, global and residual must be on one device")
    if _overlaps(residual, local) or _overlaps(residual, global_):
        raise RuntimeError(f"{op}: residual must not overlap local or global")


def pack_codes(q: torch.Tensor, bits: int) -> torch.Tensor:
    """Integer codes ``q [n]`` -> uint8 ``[ceil(n bits / 8)]``: at 8 bits byte ``i`` is ``q[i]`` as
    two's-complement int8; at 4 bits byte ``j`` holds coordinate ``2 j`` in its low nibble and ``2 j + 1``
    in its high nibble, each 4-bit two's complement, the padding nibble of an odd ``n`` zero."""
    q = q.to(torch.int64)
    if bits == 8:
        return (q & 0xFF).to(torch.uint8)
    nib = q & 0xF
    if nib.numel() & 1:
        nib = torch.cat([nib, nib.new_zeros(1)])
    return (nib[0::2] | (nib[1::2] << 4)).to(torch.uint8)


def unpack_codes(codes: torch.Tensor, bits: int, n: int) -> torch.Tensor:
    """The inverse of :func:`pack_codes` over the last dimension -> int64 ``[..., n]``; every byte decodes
    (``0x80`` is -128, the nibble ``0x8`` is -8)."""
    c = codes.to(torch.int64)
    if bits == 8:
        return (((c & 0xFF) ^ 0x80) - 0x80)[..., :n]
    nib = torch.stack([c & 0xF, (c >> 4) & 0xF], -1).reshape(*c.shape[:-1], -1)
    return ((nib ^ 0x8) - 0x8)[..., :n]


def quantize_delta(local: torch.Tensor, global_: torch.Tensor, residual: torch.Tensor, bits: int, seed: int,
                   offset: int):
    """Stochastic block quantisation with error feedback -> ``(codes uint8 [ceil(n bits / 8)], scales fp32
    [ceil(n / 256)])``; ``residual`` is updated in place.

    ``a = (local - global_) + residual`` (one fp32 subtraction, one fp32 addition).  Per block of 256
    coordinates ``amax`` is the float whose bits are ``max(bits(a) & 0x7fffffff)``.  A block with an inf
    or a NaN gets the canonical NaN as its scale, zero codes and a ``+0.0`` residual.  Otherwise ``s =
    amax / Q`` (``Q = 2^(bits - 1) - 1``); ``s < 2^-126`` makes a zero block (scale ``+0.0``, zero codes,
    ``residual = a``).  On a live block ``x = a / s``, ``f = floor(x)``, ``p = x - f``; the code rounds up
    iff ``float(word >> 8) < p * 2^24`` with ``word`` component ``i & 3`` of ``philox4x32(seed, offset,
    i >> 2)``; ``q = clamp(f + up, -Q, Q)`` (``fl(amax / fl(amax / Q))`` can exceed ``Q``); ``residual =
    a - float(q) * s``, product and difference rounded separately.  Codes are packed as
    :func:`pack_codes` does."""
    bits = int(bits)
    quantize_delta_check(local, global_, residual, bits)
    n, G, Q = local.numel(), QUANT_GROUP, quant_levels(bits)
    nb = (n + G - 1) // G
    a = (local - global_) + residual
    keys = F.pad(magnitude_keys(a), (0, nb * G - n)).view(nb, G)
    amax_key = keys.max(1).values
    amax = amax_key.view(torch.float32)
    nonfinite = amax_key >= 0x7F800000
    s = amax / torch.full_like(amax, float(Q))
    live = ~nonfinite & (s >= 2.0 ** -126)
    zero = torch.zeros((), dtype=torch.float32)
    scales = torch.where(nonfinite, _canonical_nan(), torch.where(live, s, zero))
    el = lambda t: t.repeat_interleave(G)[:n]  # noqa: E731  (per block -> per coordinate)
    s_e, live_e = el(torch.where(live, s, torch.ones_like(s))), el(live)
    x = a / s_e
    f = torch.floor(x)
    p = x - f
    word = philox4x32(seed, offset, torch.arange((n + 3) // 4)).reshape(-1)[:n]
    up = (word >> 8).to(torch.float32) < p * 16777216.0
    q = torch.clamp(f + up.to(torch.float32), -float(Q), float(Q))
    d = q * s_e
    r = a - d
    residual.copy_(torch.where(live_e, r, torch.where(el(nonfinite), zero, a)))
    qi = torch.where(live_e, q, zero).to(torch.int64)
    return pack_codes(qi, bits), scales


def dequant_combine_check(base: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, weights: torch.Tensor,
                          bits: int) -> None:
    """The argument checks of ``fedrec_quant::dequant_combine``, with its messages."""
    op = "fedrec_quant::dequant_combine"
    _check_vec(base, op, "base")
    if codes.dtype != torch.uint8:
        raise RuntimeError(f"{op}: codes must be uint8")
    if scales.dtype != torch.float32:
        raise RuntimeError(f"{op}: scales must be fp32")
    if not (codes.dim() == 2 and scales.dim() == 2):
        raise RuntimeError(f"{op}: codes [W, nbytes] and scales [W, nb]")
    if not (codes.is_contiguous() and scales.is_contiguous()):
        raise RuntimeError(f"{op}: codes and scales must be contiguous")
    _check_vec(weights, op, "weights")
    n, W = base.numel(), codes.shape[0]
    if not (1 <= n < 2 ** 31):
        raise RuntimeError(f"{op}: 1 <= n < 2^31 (got n {n})")
    if bits not in (8, 4):
        raise RuntimeError(f"{op}: bits must be 8 or 4 (got {bits})")
    if not (1 <= W <= 65536 and weights.numel() == W and scales.shape[0] == W):
        raise RuntimeError(f"{op}: 1 <= W <= 65536, scales [W, nb] and weights [W] (got W {W}, scales "
                           f"{scales.shape[0]}, weights {weights.numel()})")
    nbytes, nb = quant_sizes(n, bits)
    if not (codes.shape[1] == nbytes and scales.shape[1] == nb):
        raise RuntimeError(f"{op}: n {n} at {bits} bits takes codes [W, {nbytes}] and scales [W, {nb}] (got "
                           f"{codes.shape[1]}, {scales.shape[1]})")
    if not (codes.device == base.device and scales.device == base.device and weights.device == base.device):
        raise RuntimeError(f"{op}: base, codes, scales and weights must be on one device")


def dequant_combine(base: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, weights: torch.Tensor,
                    bits: int) -> torch.Tensor:
    """``W`` quantised deltas applied to ``base [n]`` -> ``out [n]`` fp32.  ``codes [W, ceil(n bits / 8)]``
    uint8, ``scales [W, ceil(n / 256)]`` fp32, ``weights [W]``.  ``acc`` starts at ``+0.0``; for ``c = 0 ..
    W - 1`` in that order ``acc[i] += weights[c] * (float(q[c, i]) * scales[c, i / 256])`` (three
    separately rounded operations); ``wsum`` is the sequential fp32 sum of the weights from ``+0.0``;
    ``out = base + acc / wsum``.  Codes are taken as they decode (-128 and -8 included); rejecting a bad
    upload is the caller's check (:func:`quant_upload_check`)."""
    bits = int(bits)
    dequant_combine_check(base, codes, scales, weights, bits)
    n = base.numel()
    acc = torch.zeros_like(base)
    ws = torch.zeros((), dtype=torch.float32)
    for c in range(codes.shape[0]):
        q = unpack_codes(codes[c], bits, n).to(torch.float32)
        acc = acc + weights[c] * (q * scales[c].repeat_interleave(QUANT_GROUP)[:n])
        ws = ws + weights[c]
    return base + acc / ws


def dequantize(codes: torch.Tensor, scales: torch.Tensor, bits: int, n: int) -> torch.Tensor:
    """One upload's delta ``d [n]``: :func:`dequant_combine` with ``W = 1``, a zero base and weight 1
    (``-0.0`` reads as ``+0.0``)."""
    return dequant_combine(torch.zeros(int(n), dtype=torch.float32, device=codes.device), codes.reshape(1, -1),
                           scales.reshape(1, -1), torch.ones(1, dtype=torch.float32, device=codes.device), bits)


def quant_upload_check(codes: torch.Tensor, scales: torch.Tensor, n: int, bits: int) -> None:
    """A quantised upload as :func:`quantize_delta` makes it: ``codes`` uint8 ``[ceil(n bits / 8)]``,
    ``scales`` fp32 ``[ceil(n / 256)]``, every scale finite and not below ``+0.0`` (``-0.0`` is below it).
    Raises ``ValueError`` naming the first violation."""
    nbytes, nb = quant_sizes(n, bits)
    if codes.dtype != torch.uint8:
        raise ValueError(f"quantized upload: codes must be uint8 (got {codes.dtype})")
    if scales.dtype != torch.float32:
        raise ValueError(f"quantized upload: scales must be fp32 (got {scales.dtype})")
    if codes.dim() != 1 or codes.numel() != nbytes:
        raise ValueError(f"quantized upload: codes must have length {nbytes} (got shape {tuple(codes.shape)})")
    if scales.dim() != 1 or scales.numel() != nb:
        raise ValueError(f"quantized upload: scales must have length {nb} (got shape {tuple(scales.shape)})")
    sb = scales.contiguous().view(torch.int32)
    bad = ((sb < 0) | (sb >= 0x7F800000)).nonzero()
    if bad.numel():
        j = int(bad[0])
        raise ValueError(f"quantized upload: scales[{j}] = {float(scales[j])} is not a finite value >= +0.0")


# ---------------------------------------------------------------------------------------
# Randomized-Hadamard rotation in front of the block quantiser (oracle of csrc/rotate_delta.hip)
# ---------------------------------------------------------------------------------------
ROTATE_L = 4096  # coordinates per chunk: 2^12, twelve butterfly stages
ROTATE_STREAM = 1 << 62  # the Philox offset of the signs: no (client << 32) | round of the quantiser's stream


def rotate_pad(n: int) -> int:
    """``n_pad``: ``n`` rounded up to whole chunks."""
    return -(-int(n) // ROTATE_L) * ROTATE_L


def rotate_signs(n_pad: int, seed: int) -> torch.Tensor:
    """``d [n_pad]`` fp32, ``-1.0`` where bit 31 of component ``i & 3`` of ``philox4x32(seed, 2^62, i >> 2)`` is set,
    else ``1.0``: the same on every client and in every round."""
    words = philox4x32(seed, ROTATE_STREAM, torch.arange(n_pad // 4)).reshape(-1)
    return torch.where((words >> 31) == 1, -1.0, 1.0).to(torch.float32)


def rotate(x: torch.Tensor, seed: int, inverse: bool = False, n: Optional[int] = None) -> torch.Tensor:
    """``R x`` per chunk of 4096 coordinates, ``R = 2^-6 H D`` (``H`` the Sylvester Hadamard matrix, ``D`` the signs of
    :func:`rotate_signs`).  Forward: ``x [n]`` -> ``[n_pad]``, the last chunk padded with ``+0.0``; ``t = d x`` (exact),
    then stages ``s = 0 .. 11`` in that order, every pair ``(p, p | 2^s)`` with bit ``s`` of ``p`` clear ``(u, v) -> (u +
    v, u - v)``, one fp32 rounding each, then one multiplication by ``2^-6``.  Inverse: ``x [n_pad]`` -> ``[n]`` (``n``:
    all of it when None): the same stages and scale, then the signs."""
    _check_vec(x, "fedrec_rotate::rotate", "x")
    m = x.numel()
    if inverse and (m == 0 or m % ROTATE_L or rotate_pad(m if n is None else n) != m):
        raise RuntimeError(f"fedrec_rotate::rotate: the inverse takes the whole chunks of 4096 that n pads to (got {m} for n {n})")
    n_pad = rotate_pad(m)
    d = rotate_signs(n_pad, seed).to(x.device)
    t = F.pad(x, (0, n_pad - m))
    if not inverse:
        t = d * t
    for s in range(12):
        v = t.view(-1, 2, 1 << s)
        a, b = v[:, 0], v[:, 1]
        t = torch.stack([a + b, a - b], 1).reshape(-1)
    t = t * 2.0 ** -6
    return (d * t)[:m if n is None else int(n)] if inverse else t


def rotate_quantize(local: torch.Tensor, global_: torch.Tensor, residual_rot: torch.Tensor, bits: int, seed: int,
                    offset: int):
    """:func:`quantize_delta` of ``z = rotate(local - global_)`` (one fp32 subtraction) against a zero vector ->
    ``(codes uint8 [n_pad bits / 8], scales fp32 [n_pad / 256])``; ``residual_rot [n_pad]``, the error feedback in the
    rotated domain, is updated in place.  An inf or a NaN reaches the 16 scale blocks of its chunk."""
    z = rotate((local - global_).contiguous(), seed)
    return quantize_delta(z, torch.zeros_like(z), residual_rot, bits, seed, offset)


def rotate_combine(base: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, weights: torch.Tensor, bits: int,
                   seed: int) -> torch.Tensor:
    """``W`` rotated uploads applied to ``base [n]`` -> ``out [n]``: per rotated coordinate ``acc`` and ``wsum`` as
    :func:`dequant_combine` forms them over ``n_pad`` coordinates, ``m = acc / wsum``, ``out = base + rotate(m,
    inverse)[:n]``: averaged in the rotated domain, rotated back once."""
    bits, n = int(bits), base.numel()
    n_pad = rotate_pad(n)
    dequant_combine_check(torch.zeros(n_pad, device=base.device), codes, scales, weights, bits)
    _check_vec(base, "fedrec_rotate::combine", "base")
    acc = torch.zeros(n_pad, dtype=torch.float32, device=base.device)
    ws = torch.zeros((), dtype=torch.float32)
    for c in range(codes.shape[0]):
        q = unpack_codes(codes[c], bits, n_pad).to(torch.float32)
        acc = acc + weights[c] * (q * scales[c].repeat_interleave(QUANT_GROUP))
        ws = ws + weights[c]
    return base + rotate(acc / ws, seed, inverse=True, n=n)


# ---------------------------------------------------------------------------------------
# 1-bit scaled-sign uploads with error feedback (oracle of csrc/sign_delta.hip and the rotate_sign_* kernels)
# ---------------------------------------------------------------------------------------
def _sign_quantize_check(op: str, local: torch.Tensor, global_: torch.Tensor, residual: torch.Tensor, rotated: bool) -> int:
    """The argument checks of ``fedrec_sign::quantize`` / ``rotate_quantize``, with their messages -> the coordinates coded."""
    rname = "residual_rot" if rotated else "residual"
    _check_vec(local, op, "local")
    _check_vec(global_, op, "global")
    _check_vec(residual, op, rname)
    n = local.numel()
    if global_.numel() != n:
        raise RuntimeError(f"{op}: local and global must have one length (got {n}, {global_.numel()})")
    m = _sign_coded(op, n, rotated)
    if residual.numel() != m:
        raise RuntimeError(f"{op}: {rname} must have {m} coordinates for n {n} (got {residual.numel()})")
    if not (local.device == residual.device and global_.device == residual.device):
        raise RuntimeError(f"{op}: local, global and {rname} must be on one device")
    if _overlaps(residual, local) or _overlaps(residual, global_):
        raise RuntimeError(f"{op}: {rname} must not overlap local or global")
    return m


def _sign_coded(op: str, n: int, rotated: bool) -> int:
    if not rotated:
        if not (1 <= n < 2 ** 31):
            raise RuntimeError(f"{op}: 1 <= n < 2^31 (got n {n})")
        return n
    if not (1 <= n <= 2 ** 31 - ROTATE_L):
        raise RuntimeError(f"{op}: 1 <= n <= 2^31 - 4096 (got n {n})")
    return rotate_pad(n)


def _sign_combine_check(op: str, base: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, weights: torch.Tensor,
                        rotated: bool) -> int:
    """The argument checks of ``fedrec_sign::combine`` / ``rotate_combine``, with their messages -> the coordinates coded."""
    _check_vec(base, op, "base")
    if codes.dtype != torch.uint8:
        raise RuntimeError(f"{op}: codes must be uint8")
    if scales.dtype != torch.float32:
        raise RuntimeError(f"{op}: scales must be fp32")
    if not (codes.dim() == 2 and scales.dim() == 2):
        raise RuntimeError(f"{op}: codes [W, nbytes] and scales [W, nb]")
    if not (codes.is_contiguous() and scales.is_contiguous()):
        raise RuntimeError(f"{op}: codes and scales must be contiguous")
    _check_vec(weights, op, "weights")
    n, W = base.numel(), codes.shape[0]
    m = _sign_coded(op, n, rotated)
    if not (1 <= W <= 65536 and weights.numel() == W and scales.shape[0] == W):
        raise RuntimeError(f"{op}: 1 <= W <= 65536, scales [W, nb] and weights [W] (got W {W}, scales {scales.shape[0]}, "
                           f"weights {weights.numel()})")
    nbytes, nb = quant_sizes(m, 1)
    if not (codes.shape[1] == nbytes and scales.shape[1] == nb):
        raise RuntimeError(f"{op}: n {n} takes codes [W, {nbytes}] and scales [W, {nb}] (got {codes.shape[1]}, "
                           f"{scales.shape[1]})")
    if not (codes.device == base.device and scales.device == base.device and weights.device == base.device):
        raise RuntimeError(f"{op}: base, codes, scales and weights must be on one device")
    return m


def _sign_code(a: torch.Tensor, residual: torch.Tensor):
    """The coder of :func:`sign_quantize` on ``a [n]``; ``residual [n]`` takes what is kept."""
    n, G = a.numel(), QUANT_GROUP
    nbytes, nb = quant_sizes(n, 1)
    mag = F.pad(a.abs(), (0, nb * G - n)).view(nb, 16, 16)  # block, run, coordinate of the run
    p = torch.zeros(nb, 16, dtype=torch.float32)
    for e in range(16):  # each run in ascending order from +0.0
        p = p + mag[:, :, e]
    j = torch.arange(16)
    for o in (1, 2, 4, 8):  # p_j + p_(j ^ o): the same bits in all 16
        p = p + p[:, j ^ o]
    p = p[:, 0]
    count = torch.clamp(n - G * torch.arange(nb), max=G).to(torch.float32)
    s = p / count
    nonfinite = (p.view(torch.int32) & 0x7FFFFFFF) >= 0x7F800000
    live = ~nonfinite & (s >= 2.0 ** -126)
    zero = torch.zeros((), dtype=torch.float32)
    scales = torch.where(nonfinite, _canonical_nan(), torch.where(live, s, zero))
    el = lambda t: t.repeat_interleave(G)[:n]  # noqa: E731  (per block -> per coordinate)
    live_e = el(live)
    r = a - torch.copysign(el(s), a)
    residual.copy_(torch.where(live_e, r, torch.where(el(nonfinite), zero, a)))
    bit = F.pad(((a.view(torch.int32) < 0) & live_e).to(torch.int64), (0, 8 * nbytes - n)).view(nbytes, 8)
    return (bit << torch.arange(8)).sum(1).to(torch.uint8), scales


def sign_quantize(local: torch.Tensor, global_: torch.Tensor, residual: torch.Tensor):
    """Scaled-sign coding with error feedback -> ``(codes uint8 [ceil(n / 8)], scales fp32 [ceil(n / 256)])``;
    ``residual`` is updated in place.  Deterministic: no Philox, no seed.

    ``a = (local - global_) + residual`` (one fp32 subtraction, one fp32 addition).  Per block of 256 coordinates ``p``
    is the sum of ``|a|`` (``+0.0`` past ``n``) in a fixed order: 16 runs of 16 consecutive coordinates, each summed
    from ``+0.0`` in ascending order, then four butterfly steps ``p_j = p_j + p_(j ^ o)``, ``o = 1, 2, 4, 8``, over the
    run sums.  ``s = p / float(min(256, n - b0))``, one division: the block's mean magnitude.  ``bits(p) & 0x7fffffff >=
    0x7f800000`` (an inf, a NaN, an overflowing sum): the canonical NaN as the scale, zero codes, a ``+0.0`` residual.
    Else ``s < 2^-126``: a zero block (scale ``+0.0``, zero codes, ``residual = a``).  Else bit ``i & 7`` of byte ``i >>
    3`` is the sign bit of ``a[i]`` (``-0.0`` codes 1) and ``residual[i] = a[i] - copysign(s, a[i])``.  Padding bits
    are zero."""
    _sign_quantize_check("fedrec_sign::quantize", local, global_, residual, False)
    return _sign_code((local - global_) + residual, residual)


def unpack_signs(codes: torch.Tensor, n: int) -> torch.Tensor:
    """Bit ``i & 7`` of byte ``i >> 3`` over the last dimension -> bool ``[..., n]``."""
    c = codes.to(torch.int64)
    return (((c[..., None] >> torch.arange(8, device=codes.device)) & 1) == 1).reshape(*c.shape[:-1], -1)[..., :n]


def _sign_mean(codes: torch.Tensor, scales: torch.Tensor, weights: torch.Tensor, m: int) -> torch.Tensor:
    """``acc / wsum`` of :func:`sign_combine` over ``m`` coded coordinates."""
    acc = torch.zeros(m, dtype=torch.float32, device=codes.device)
    ws = torch.zeros((), dtype=torch.float32)
    for c in range(codes.shape[0]):
        t = (weights[c] * scales[c]).repeat_interleave(QUANT_GROUP)[:m]
        acc = acc + torch.where(unpack_signs(codes[c], m), -t, t)
        ws = ws + weights[c]
    return acc / ws


def sign_combine(base: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
    """``W`` sign uploads applied to ``base [n]`` -> ``out [n]`` fp32.  ``codes [W, ceil(n / 8)]`` uint8, ``scales [W,
    ceil(n / 256)]`` fp32, ``weights [W]``.  ``acc`` starts at ``+0.0``; for ``c = 0 .. W - 1`` in that order ``t =
    weights[c] * scales[c, i / 256]`` (one rounding) and ``acc[i] += -t if bit else t``; ``wsum`` is the sequential fp32
    sum of the weights from ``+0.0``; ``out = base + acc / wsum``.  Rejecting a bad upload is the caller's check
    (:func:`quant_upload_check` with ``bits = 1``)."""
    n = _sign_combine_check("fedrec_sign::combine", base, codes, scales, weights, False)
    return base + _sign_mean(codes, scales, weights, n)


def sign_dequantize(codes: torch.Tensor, scales: torch.Tensor, n: int) -> torch.Tensor:
    """One upload's delta ``d [n]``: :func:`sign_combine` with ``W = 1``, a zero base and weight 1."""
    return sign_combine(torch.zeros(int(n), dtype=torch.float32, device=codes.device), codes.reshape(1, -1),
                        scales.reshape(1, -1), torch.ones(1, dtype=torch.float32, device=codes.device))


def rotate_sign_quantize(local: torch.Tensor, global_: torch.Tensor, residual_rot: torch.Tensor, seed: int):
    """:func:`sign_quantize`'s coder on ``a = rotate(local - global_) + residual_rot`` (one fp32 subtraction, one fp32
    addition) over ``n_pad`` coordinates, every block full -> ``(codes uint8 [n_pad / 8], scales fp32 [n_pad / 256])``;
    ``residual_rot [n_pad]`` is updated in place.  An inf or a NaN reaches the 16 scale blocks of its chunk."""
    _sign_quantize_check("fedrec_sign::rotate_quantize", local, global_, residual_rot, True)
    return _sign_code(rotate((local - global_).contiguous(), seed) + residual_rot, residual_rot)


def rotate_sign_combine(base: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, weights: torch.Tensor,
                        seed: int) -> torch.Tensor:
    """``W`` rotated sign uploads applied to ``base [n]`` -> ``out [n]``: ``m = acc / wsum`` as :func:`sign_combine`
    forms it over ``n_pad`` rotated coordinates, ``out = base + rotate(m, inverse)[:n]``."""
    n_pad = _sign_combine_check("fedrec_sign::rotate_combine", base, codes, scales, weights, True)
    return base + rotate(_sign_mean(codes, scales, weights, n_pad), seed, inverse=True, n=base.numel())


# ---------------------------------------------------------------------------------------
# Elias-Fano coding of the top-k forms' index list (oracle of csrc/index_code.hip)
# ---------------------------------------------------------------------------------------
def ef_plan(n: int, k: int) -> Tuple[int, int, int, int]:
    """``(b, low_words, high_bits, high_words)`` of ``k`` strictly ascending positions in ``[0, n)``, ``1 <= k <= n <
    2^31``.  ``b`` is the largest integer with ``(k << b) <= n`` (0 when ``k > n / 2``).  The low section holds ``k``
    fields of ``b`` bits, ``idx_i & (2^b - 1)``, field ``i`` at bit ``i b``, LSB first in little-endian uint32 words:
    ``low_words = ceil(k b / 32)``.  The high section is a bit vector of ``high_bits = k + ((n - 1) >> b) + 1`` bits
    (``high_words = ceil(high_bits / 32)``) with bit ``(idx_i >> b) + i`` set for every ``i``.  The blob is the low
    words, then the high words, as int32; every padding bit is zero.  ``b + 1 + n / (k 2^b)`` bits per index."""
    n, k = int(n), int(k)
    if not 1 <= k <= n < 2 ** 31:
        raise ValueError(f"Elias-Fano index: 1 <= k <= n < 2^31 (got k {k}, n {n})")
    b = 0
    while (k << (b + 1)) <= n:
        b += 1
    high_bits = k + ((n - 1) >> b) + 1
    return b, (k * b + 31) // 32, high_bits, (high_bits + 31) // 32


def _ef_bits(words: torch.Tensor) -> torch.Tensor:
    """The bits of int32 words, LSB first, as int64 0 / 1 ``[32 len]``."""
    return (((words.long() & _U32)[:, None] >> torch.arange(32, device=words.device)) & 1).reshape(-1)


def _ef_words(bits: torch.Tensor, nwords: int) -> torch.Tensor:
    """``bits`` (int64 0 / 1, LSB first), zero-padded to ``nwords`` int32 words."""
    pad = torch.zeros(32 * nwords, dtype=torch.int64, device=bits.device)
    pad[:bits.numel()] = bits
    return _wrap_i32((pad.view(nwords, 32) << torch.arange(32, device=bits.device)).sum(1))


def ef_encode(idx: torch.Tensor, n: int) -> torch.Tensor:
    """``idx`` int32 ``[k]``, strictly ascending in ``[0, n)`` as :func:`topk_delta` gives it (the caller's contract)
    -> the blob of :func:`ef_plan`, int32 ``[low_words + high_words]``."""
    if idx.dtype != torch.int32 or idx.dim() != 1:
        raise RuntimeError(f"fedrec_index::encode: idx must be int32 [k] (got {idx.dtype} {tuple(idx.shape)})")
    k = idx.numel()
    b, low_words, high_bits, high_words = ef_plan(n, k)
    i = idx.long()
    low = (((i & ((1 << b) - 1))[:, None] >> torch.arange(b, device=idx.device)) & 1).reshape(-1)
    high = torch.zeros(high_bits, dtype=torch.int64, device=idx.device)
    high[(i >> b) + torch.arange(k, device=idx.device)] = 1
    return torch.cat([_ef_words(low, low_words), _ef_words(high, high_words)])


def _ef_padding_check(words: torch.Tensor, n: int, k: int) -> None:
    """The bits of a blob that no code sets: at or past ``high_bits`` of the high section, past ``k b`` of the low."""
    b, low_words, high_bits, high_words = ef_plan(n, k)
    if high_bits % 32 and (int(words[-1]) & _U32) >> (high_bits % 32):
        raise ValueError(f"Elias-Fano index: a bit is set at or past the {high_bits} bits of the high section")
    if k * b % 32 and (int(words[low_words - 1]) & _U32) >> (k * b % 32):
        raise ValueError("Elias-Fano index: the padding bits after the low fields are not zero")


def ef_decoded_check(words: torch.Tensor, idx: torch.Tensor, count, n: int, k: int) -> None:
    """What a decoder's output for one blob must satisfy before it is taken for a code (the device decoder writes
    whatever the words spell and leaves the verdict to this check; :func:`ef_decode` runs it on its own result):
    ``count``, the set bits of the high section, is ``k``; no padding bit is set; every decoded index is in ``[0, n)``
    (the device writes -1 otherwise).  Ascending and distinct follow from the format.  Raises ``ValueError``."""
    if int(count) != k:
        raise ValueError(f"Elias-Fano index: the high section holds {int(count)} set bits, expected k = {k}")
    _ef_padding_check(words, n, k)
    bad = ((idx < 0) | (idx >= n)).nonzero()
    if bad.numel():
        raise ValueError(f"Elias-Fano index: the index decoded at rank {int(bad[0])} is outside [0, {n})")


def ef_decode(words: torch.Tensor, n: int, k: int) -> torch.Tensor:
    """One blob of :func:`ef_plan` -> ``idx`` int32 ``[k]``.  The set bit of rank ``i`` at position ``p`` of the high
    section gives ``high = p - i``, field ``i`` of the low section ``low``, ``idx_i = (high << b) | low``.  Raises
    ``ValueError`` for words that :func:`ef_encode` cannot have made: another popcount than ``k``, a set bit at or past
    ``high_bits``, a non-zero padding bit, a decoded index ``>= n``."""
    b, low_words, high_bits, high_words = ef_plan(n, k)
    if words.dtype != torch.int32 or words.dim() != 1 or words.numel() != low_words + high_words:
        raise ValueError(f"Elias-Fano index: expected an int32 [{low_words + high_words}] tensor (got {words.dtype} "
                         f"{tuple(words.shape)})")
    pos = _ef_bits(words[low_words:]).nonzero().flatten()
    idx = torch.full((k,), -1, dtype=torch.int64, device=words.device)
    if pos.numel() == k:
        low = (_ef_bits(words[:low_words])[:k * b].view(k, b) << torch.arange(b, device=words.device)).sum(1)
        idx = ((pos - torch.arange(k, device=words.device)) << b) | low
    ef_decoded_check(words, idx, pos.numel(), n, k)
    return idx.to(torch.int32)


# ---------------------------------------------------------------------------------------
# Low-rank (PowerSGD) uploads with error feedback (oracle of csrc/lowrank_delta.hip)
# ---------------------------------------------------------------------------------------
LOWRANK_RANKS = (1, 2, 4, 8)


class LowRankPlan:
    """Which coordinates of a padded flat buffer travel as rank-``R`` factors and which dense: a pure function of
    the layout and ``R``, so a client and the coordinator derive the same one.

    ``layout``: ``(offset, shape)`` of every parameter, offsets ascending, inside ``[0, n)``.  A parameter is a
    matrix of the plan when it is 2-D, ``min(rows, cols) >= 16`` and ``R (rows + cols) <= rows cols / 2``; every
    other coordinate of ``[0, n)`` (biases, vectors, the alignment padding) is "rest".  The payload is fp32 ``[L]``:
    per matrix ``P^ [rows, R]`` at ``fac`` and ``Q' [cols, R]`` at ``fac + rows R`` (the factors fill ``[0, F)``),
    then the rest segments' values.  ``mats`` int32 ``[M, 4]``: flat offset, rows, cols, ``fac``; ``rest`` int32
    ``[S, 3]``: flat start, length, payload offset.  The tile tables are the kernels' (csrc/lowrank_delta.hip):
    ``tiles_p [*, 2]`` 16 rows of a matrix; ``tiles_b [*, 3]`` 64 columns x a chunk of 256 rows and ``tiles_f [*,
    4]`` a column group's chunks; ``tiles_e [*, 3]`` 32 x 256 of a matrix or 1024 elements of a rest segment."""

    def __init__(self, layout, n: int, rank: int):
        if rank not in LOWRANK_RANKS:
            raise ValueError(f"upload_rank={rank}: expected one of {LOWRANK_RANKS}")
        R, n = int(rank), int(n)
        if not 1 <= n < 2 ** 31:
            raise ValueError(f"low-rank plan: 1 <= n < 2^31 (got n {n})")
        mats, rest, fac, end = [], [], 0, 0
        for off, shape in layout:
            off, numel = int(off), int(math.prod(shape))
            if off < end or off + numel > n:
                raise ValueError(f"low-rank plan: parameter at {off} of {numel} elements overlaps its neighbour or ends past {n}")
            if len(shape) == 2 and min(shape) >= 16 and 2 * R * (shape[0] + shape[1]) <= shape[0] * shape[1]:
                if off > end:
                    rest.append([end, off - end])
                mats.append([off, int(shape[0]), int(shape[1]), fac])
                fac += R * (shape[0] + shape[1])
                end = off + numel
        if n > end:
            rest.append([end, n - end])
        if not mats:
            raise ValueError(f"low-rank plan: no parameter of the layout is a matrix to factor at rank {R}")
        self.rank, self.n, self.F = R, n, fac
        pay = fac
        for seg in rest:
            seg.append(pay)
            pay += seg[1]
        self.L = pay
        tp, tb, tf, te = [], [], [], []
        for m, (off, rows, cols, _) in enumerate(mats):
            tp += [[m, r0] for r0 in range(0, rows, 16)]
            nch = -(-rows // 256)
            for c0 in range(0, cols, 64):
                tf.append([m, c0, len(tb), nch])
                tb += [[m, c0, ch] for ch in range(nch)]
            te += [[m, r0, c0] for r0 in range(0, rows, 32) for c0 in range(0, cols, 256)]
        for s, (_, ln, _) in enumerate(rest):
            te += [[-1 - s, e0, 0] for e0 in range(0, ln, 1024)]
        i32 = lambda rows, w: torch.tensor(rows, dtype=torch.int32).reshape(-1, w)  # noqa: E731
        self.tables = {"mats": i32(mats, 4), "rest": i32(rest, 3), "tiles_p": i32(tp, 2), "tiles_b": i32(tb, 3),
                       "tiles_f": i32(tf, 4), "tiles_e": i32(te, 3)}
        self.mats, self.rest = [tuple(r) for r in mats], [tuple(r) for r in rest]
        self._on = {}

    def on(self, device) -> dict:
        """The tables on ``device`` (copied once)."""
        device = torch.device(device)
        if device not in self._on:
            self._on[device] = {k: t.to(device) for k, t in self.tables.items()}
        return self._on[device]

    def factors(self, payload: torch.Tensor, m: int):
        """Views ``(P^ [rows, R], Q' [cols, R])`` of matrix ``m`` in a payload (or a basis)."""
        _, rows, cols, fac = self.mats[m]
        R = self.rank
        return payload[fac:fac + rows * R].view(rows, R), payload[fac + rows * R:fac + (rows + cols) * R].view(cols, R)

    def initial_basis(self, seed: int) -> torch.Tensor:
        """The round-1 basis ``[F]`` on the host: ``Q`` of matrix ``m`` standard normal from a generator seeded by
        ``(seed, m)``, at the place of ``Q'``; zeros at the place of ``P^``."""
        basis = torch.zeros(self.F, dtype=torch.float32)
        for m in range(len(self.mats)):
            g = torch.Generator().manual_seed((int(seed) * 1_000_003 + m) & 0x7FFFFFFFFFFF)
            q = self.factors(basis, m)[1]
            q.copy_(torch.randn(q.shape, generator=g, dtype=torch.float32))
        return basis


def _lowrank_check(plan: LowRankPlan, op: str, payload: torch.Tensor, *flats: torch.Tensor) -> None:
    for t in flats:
        _check_vec(t, op, "a flat tensor")
        if t.numel() != plan.n:
            raise RuntimeError(f"{op}: local, global, residual and base must have the plan's {plan.n} elements (got {t.numel()})")
    if payload.dim() != 1 or payload.numel() < plan.F:
        raise RuntimeError(f"{op}: the payload must be 1-D with at least the plan's {plan.F} factor elements")


def _lowrank_a(local, global_, residual, off: int, rows: int, cols: int) -> torch.Tensor:
    s = slice(off, off + rows * cols)
    return ((local[s] - global_[s]) + residual[s]).view(rows, cols)


def lowrank_project(local, global_, residual, basis, payload, plan: LowRankPlan) -> torch.Tensor:
    """``P = a Q`` of every matrix of the plan into ``payload`` (at the place of ``P^``), ``a = (local - global_) +
    residual`` in fp32 and ``Q`` from ``basis`` (the payload's factor layout).  A tolerance contract: the order of
    a dot product's sum is the implementation's."""
    _lowrank_check(plan, "lowrank_project", payload, local, global_, residual)
    for m, (off, rows, cols, _) in enumerate(plan.mats):
        plan.factors(payload, m)[0].copy_(_lowrank_a(local, global_, residual, off, rows, cols) @ plan.factors(basis, m)[1])
    return payload


def lowrank_orth(payload, plan: LowRankPlan) -> torch.Tensor:
    """``P^ = orth(P)`` in place, per matrix: modified Gram-Schmidt over the ``R`` columns in order.  Column ``c``
    is projected against columns ``0 .. c - 1`` in order, twice (re-orthogonalisation): ``v -= <p_b, v> p_b`` with
    the dot product and the update in fp64, the column rounded to the payload's type after every update.  With
    ``n0`` and ``n1`` the column's squared norms (fp64) before and after, ``n1 == 0`` or ``n1 <= 2^-40 n0`` makes it
    a zero column, else it is divided by ``sqrt(n1)`` in fp64 and rounded.  A payload of fp64 keeps every value
    in fp64: the same algorithm as its own high-precision oracle."""
    if payload.dim() != 1 or payload.numel() < plan.F:
        raise RuntimeError(f"lowrank_orth: the payload must be 1-D with at least the plan's {plan.F} factor elements")
    for m in range(len(plan.mats)):
        P = plan.factors(payload, m)[0]
        for c in range(plan.rank):
            v = P[:, c].double()
            n0 = (v * v).sum()
            for _ in range(2):
                for b in range(c):
                    pb = P[:, b].double()
                    v = (v - (pb * v).sum() * pb).to(P.dtype).double()
            n1 = (v * v).sum()
            zero = bool(n1 == 0) or bool(n1 <= 2.0 ** -40 * n0)
            P[:, c] = torch.zeros_like(P[:, c]) if zero else (v / torch.sqrt(n1)).to(P.dtype)
    return payload


def lowrank_backproject(local, global_, residual, payload, plan: LowRankPlan) -> torch.Tensor:
    """``Q' = a^T P^`` of every matrix into ``payload`` (at the place of ``Q'``).  A tolerance contract."""
    _lowrank_check(plan, "lowrank_backproject", payload, local, global_, residual)
    for m, (off, rows, cols, _) in enumerate(plan.mats):
        P, Q = plan.factors(payload, m)
        Q.copy_(_lowrank_a(local, global_, residual, off, rows, cols).t() @ P)
    return payload


def lowrank_decode(payload, plan: LowRankPlan, m: int) -> torch.Tensor:
    """``d [rows, cols]`` of matrix ``m``: ``d_ij = P^_i0 Q'_j0``, then ``+ P^_it Q'_jt`` for ``t = 1 .. R - 1`` in
    order, every product and every sum rounded on its own (no FMA)."""
    P, Q = plan.factors(payload, m)
    d = P[:, 0:1] * Q[:, 0][None, :]
    for t in range(1, plan.rank):
        d = d + P[:, t:t + 1] * Q[:, t][None, :]
    return d


def lowrank_residual(local, global_, residual, payload, plan: LowRankPlan) -> torch.Tensor:
    """The end of a client's round, ``residual`` and ``payload`` in place: on a matrix ``residual = a -
    decode(payload)`` (:func:`lowrank_decode`; one fp32 subtraction); on the rest ``payload = a`` and ``residual =
    +0.0``.  A bitwise contract."""
    _lowrank_check(plan, "lowrank_residual", payload, local, global_, residual)
    if payload.numel() != plan.L:
        raise RuntimeError(f"lowrank_residual: the payload must have the plan's {plan.L} elements (got {payload.numel()})")
    for m, (off, rows, cols, _) in enumerate(plan.mats):
        a = _lowrank_a(local, global_, residual, off, rows, cols)
        residual[off:off + rows * cols] = (a - lowrank_decode(payload, plan, m)).reshape(-1)
    for start, ln, pay in plan.rest:
        s = slice(start, start + ln)
        payload[pay:pay + ln] = (local[s] - global_[s]) + residual[s]
        residual[s] = 0.0
    return payload


def lowrank_combine(base, stack, weights, plan: LowRankPlan) -> torch.Tensor:
    """``W`` low-rank uploads ``stack [W, L]`` applied to ``base [n]`` -> ``out [n]`` fp32: ``acc`` starts at
    ``+0.0``; for ``c = 0 .. W - 1`` in that order ``acc += weights[c] * d_c`` (product and sum rounded on their
    own) with ``d_c`` the decoded matrix (:func:`lowrank_decode`) or the dense rest value; ``wsum`` is the
    sequential fp32 sum of the weights from ``+0.0``; ``out = base + acc / wsum``.  A bitwise contract."""
    _lowrank_check(plan, "lowrank_combine", stack[0] if stack.dim() == 2 and stack.shape[0] else stack, base)
    if stack.dim() != 2 or stack.shape[1] != plan.L or weights.numel() != stack.shape[0]:
        raise RuntimeError(f"lowrank_combine: stack [W, {plan.L}] and weights [W] (got {tuple(stack.shape)}, {weights.numel()})")
    out = base.clone()
    ws = torch.zeros((), dtype=torch.float32)
    for c in range(stack.shape[0]):
        ws = ws + weights[c]
    for m, (off, rows, cols, _) in enumerate(plan.mats):
        acc = torch.zeros(rows, cols, dtype=torch.float32)
        for c in range(stack.shape[0]):
            acc = acc + weights[c] * lowrank_decode(stack[c], plan, m)
        s = slice(off, off + rows * cols)
        out[s] = base[s] + (acc / ws).reshape(-1)
    for start, ln, pay in plan.rest:
        acc = torch.zeros(ln, dtype=torch.float32)
        for c in range(stack.shape[0]):
            acc = acc + weights[c] * stack[c, pay:pay + ln]
        s = slice(start, start + ln)
        out[s] = base[s] + acc / ws
    return out


# ---------------------------------------------------------------------------------------
# Count-sketch (FetchSGD) uploads (oracle of csrc/sketch_delta.hip)
# ---------------------------------------------------------------------------------------
SKETCH_T = 1024  # the tile: coordinates of one (block, tile) pair share their hash words
SKETCH_ROWS = (1, 3, 5)
SKETCH_STREAM = 0x736B657463680001  # the Philox offset of the hash words ("sketch", version 1)


def _wrap_i32(x: torch.Tensor) -> torch.Tensor:
    """uint32 values held in int64 -> the int32 with the same bits."""
    return (((x & _U32) + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)


def fmix32(h: torch.Tensor) -> torch.Tensor:
    """The murmur3 finaliser on uint32 values held in int64."""
    h = h & _U32
    h = ((h ^ (h >> 16)) * 0x85EBCA6B) & _U32
    h = ((h ^ (h >> 13)) * 0xC2B2AE35) & _U32
    return h ^ (h >> 16)


def sketch_cols_for(k: int) -> int:
    """The smallest power of two ``>= max(1024, 4 k)``."""
    return 1 << max(10, (4 * int(k) - 1).bit_length())


def sketch_plan(n: int, cols: int, seed: int) -> torch.Tensor:
    """The hash of a count sketch of ``n`` coordinates with ``cols`` buckets per row, as its words: int32 ``[nb, 8,
    4]``, ``nb = ceil(n / cols)``.  A pure function of ``(n, cols, seed)``.

    Coordinate ``i`` is ``(q, p_hi, p_lo) = (i / C, (i % C) / T, i % T)`` with ``T = 1024``, and row ``r`` sends it
    to bucket ``j_hi T + j_lo``: ``j_hi = (p_hi + rot_q) & (C / T - 1)`` (one tile rotation per block, shared by the
    rows), ``j_lo = (p_lo m + o) & (T - 1)`` with ``m`` odd, and gives it the sign ``-1`` iff bit 31 of
    ``fmix32(uint32(i) ^ sx)`` is set.  Slot ``r < 5`` of block ``q`` holds ``(m, o, sx, minv)`` of row ``r`` --
    ``philox4x32(seed, SKETCH_STREAM, 8 q + r)``'s words 0, 1, 2 (``m = word 0 | 1``, ``o = word 1 & (T - 1)``) and
    ``minv``, the inverse of ``m`` modulo 2^32: ``p_lo = ((j_lo - o) minv) & (T - 1)``; slot 7 holds ``rot_q`` (word 0
    of counter ``8 q + 7``) and zeros.  Inside a block every row is a bijection onto the row's buckets, so a bucket
    takes exactly one coordinate of every block and a kernel can gather them in block order."""
    n, C = int(n), int(cols)
    if C < SKETCH_T or C & (C - 1):
        raise ValueError(f"sketch plan: cols must be a power of two >= {SKETCH_T} (got {C})")
    if not 1 <= n < 2 ** 31:
        raise ValueError(f"sketch plan: 1 <= n < 2^31 (got n {n})")
    nb = -(-n // C)
    w = philox4x32(int(seed), SKETCH_STREAM, torch.arange(nb * 8, dtype=torch.int64)).view(nb, 8, 4)
    m = w[:, :, 0] | 1
    minv = m.clone()  # Newton: five steps double 3 correct bits to 96 >= 32
    for _ in range(5):
        minv = (minv * ((2 - m * minv) & _U32)) & _U32
    plan = torch.stack([m, w[:, :, 1] & (SKETCH_T - 1), w[:, :, 2], minv], -1)
    plan[:, 5:] = 0
    plan[:, 7, 0] = w[:, 7, 0]
    return _wrap_i32(plan)


def sketch_hash(plan: torch.Tensor, i: torch.Tensor, rows: int, cols: int):
    """Coordinates ``i`` (int64, inside the plan's blocks) -> ``(bucket [rows, len] int64, negative [rows, len]
    bool)`` by the forward hash of :func:`sketch_plan`."""
    T, C = SKETCH_T, int(cols)
    w = plan.to(torch.int64) & _U32
    q, p_hi, p_lo = i // C, (i % C) // T, i % T
    j_hi = (p_hi + w[q, 7, 0]) & (C // T - 1)
    j, neg = [], []
    for r in range(int(rows)):
        j.append(j_hi * T + ((p_lo * w[q, r, 0] + w[q, r, 1]) & (T - 1)))
        neg.append(fmix32(i ^ w[q, r, 2]) >> 31 != 0)
    return torch.stack(j), torch.stack(neg)


def _flip(v: torch.Tensor, neg: torch.Tensor) -> torch.Tensor:
    """``v`` with its sign bit flipped where ``neg`` (exact for every value, a NaN included)."""
    b = v.contiguous().view(torch.int32)
    return torch.where(neg, b ^ -2 ** 31, b).view(torch.float32)


def _sketch_check(op: str, plan: torch.Tensor, n: int, rows: int, cols: int) -> None:
    if rows not in SKETCH_ROWS:
        raise RuntimeError(f"{op}: rows must be 1, 3 or 5 (got {rows})")
    if cols < SKETCH_T or cols & (cols - 1):
        raise RuntimeError(f"{op}: cols must be a power of two >= {SKETCH_T} (got {cols})")
    if not 1 <= n < 2 ** 31:
        raise RuntimeError(f"{op}: 1 <= n < 2^31 (got n {n})")
    if plan.dtype != torch.int32 or tuple(plan.shape) != (-(-n // cols), 8, 4) or not plan.is_contiguous():
        raise RuntimeError(f"{op}: plan must be a contiguous int32 [{-(-n // cols)}, 8, 4] tensor (got {plan.dtype} "
                           f"{tuple(plan.shape)})")


def sketch_delta(local: torch.Tensor, global_: torch.Tensor, plan: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    """The count sketch ``S [rows, cols]`` fp32 of a round delta.  ``a = local - global_`` (one fp32 subtraction);
    every bucket starts at ``+0.0`` and takes, for the blocks ``q = 0, 1, ..`` in that order, ``+a_i`` or ``-a_i`` of
    its coordinate ``i`` of block ``q`` (one fp32 addition per block; a coordinate ``i >= n`` adds nothing).  A
    function of ``(n, rows, cols, seed)`` and the inputs alone.  A non-finite ``a_i`` lands in its ``rows`` buckets."""
    op = "fedrec_sketch::delta"
    _check_vec(local, op, "local")
    _check_vec(global_, op, "global")
    n, R, C = local.numel(), int(rows), int(cols)
    if global_.numel() != n:
        raise RuntimeError(f"{op}: local and global must have one length (got {n}, {global_.numel()})")
    _sketch_check(op, plan, n, R, C)
    a = local - global_
    S = torch.zeros(R, C, dtype=torch.float32)
    for q in range(plan.shape[0]):
        i = torch.arange(q * C, min(n, (q + 1) * C), dtype=torch.int64)
        j, neg = sketch_hash(plan, i, R, C)
        for r in range(R):
            S[r, j[r]] = S[r, j[r]] + _flip(a[i], neg[r])
    return S


def order_values(k: torch.Tensor) -> torch.Tensor:
    """The inverse of :func:`order_keys`; the NaN key 0xFFFFFFFF comes back as the NaN 0x7FFFFFFF."""
    b = torch.where(k >= 0x80000000, k ^ 0x80000000, _U32 - k)
    return _wrap_i32(b).view(torch.float32)


def sketch_estimate(table: torch.Tensor, plan: torch.Tensor, n: int) -> torch.Tensor:
    """``est [n]`` fp32 of a sketch ``table [rows, cols]``: ``est_i`` is the median over the rows of ``sign_r(i)
    table[r, h_r(i)]`` under :func:`order_keys` (``-0.0 < +0.0``, every NaN one key above ``+inf``): the middle of
    the ``rows`` keys, turned back into its float.  Exact; no tie can show."""
    op = "fedrec_sketch::estimate"
    if table.dtype != torch.float32 or table.dim() != 2 or not table.is_contiguous():
        raise RuntimeError(f"{op}: table must be a contiguous fp32 [rows, cols] tensor")
    R, C = table.shape
    _sketch_check(op, plan, int(n), R, C)
    i = torch.arange(int(n), dtype=torch.int64)
    j, neg = sketch_hash(plan, i, R, C)
    keys = torch.stack([order_keys(_flip(table[r, j[r]], neg[r])) for r in range(R)])
    return order_values(torch.sort(keys, 0).values[R // 2])


def sketch_accumulate_(table: torch.Tensor, stack: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
    """In place ``table += (sum over c, in client order, of weights[c] * stack[c]) / sum(weights)``, every element of
    ``table`` against the same element of ``stack [W, table.numel()]``, ``1 <= W <= 32``; the products, the sums
    from ``+0.0``, the division and the final addition each rounded on their own (as :func:`dequant_combine`)."""
    op = "fedrec_sketch::accumulate_"
    if table.dtype != torch.float32 or not table.is_contiguous():
        raise RuntimeError(f"{op}: table must be contiguous fp32")
    if stack.dtype != torch.float32 or stack.dim() != 2 or not stack.is_contiguous() or stack.shape[1] != table.numel():
        raise RuntimeError(f"{op}: stack must be a contiguous fp32 [W, {table.numel()}] tensor (got {tuple(stack.shape)})")
    _check_vec(weights, op, "weights")
    W = stack.shape[0]
    if not (1 <= W <= 32 and weights.numel() == W):
        raise RuntimeError(f"{op}: 1 <= W <= 32 and weights [W] (got W {W}, weights {weights.numel()})")
    acc = torch.zeros(table.numel(), dtype=torch.float32)
    ws = torch.zeros((), dtype=torch.float32)
    for c in range(W):
        acc = acc + weights[c] * stack[c]
        ws = ws + weights[c]
    table.copy_((table.reshape(-1) + acc / ws).view_as(table))
    return table


def sketch_clear_(table: torch.Tensor, idx: torch.Tensor, plan: torch.Tensor) -> torch.Tensor:
    """In place ``table[r, h_r(i)] = +0.0`` for every ``i`` of ``idx`` (int32, inside the plan's blocks; an index
    outside them is skipped) and every row: idempotent, so members that share a bucket need no order."""
    op = "fedrec_sketch::clear_"
    if table.dtype != torch.float32 or table.dim() != 2 or not table.is_contiguous():
        raise RuntimeError(f"{op}: table must be a contiguous fp32 [rows, cols] tensor")
    if idx.dtype != torch.int32 or idx.dim() != 1:
        raise RuntimeError(f"{op}: idx must be int32 [k]")
    R, C = table.shape
    _sketch_check(op, plan, plan.shape[0] * C if plan.dim() == 3 and plan.shape[0] else 0, R, C)
    i = idx.to(torch.int64)
    i = i[(i >= 0) & (i < plan.shape[0] * C)]
    j, _ = sketch_hash(plan, i, R, C)
    for r in range(R):
        table[r, j[r]] = 0.0
    return table
