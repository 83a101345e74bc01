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
