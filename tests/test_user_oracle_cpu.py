"""The user-tower oracle (``tests/user_oracle.py``) checked without a GPU:

* its explicit fp64 intermediates equal fp64 autograd through ``ops.reference`` to 1e-12;
* a rounding model of each kernel family -- torch on the CPU in fp32 with the kernels' order of
  operations (stabilised eps-softmax, P recomputed from the saved stats, chunked online softmax
  for H > 64, bf16 rounding where the kernel rounds) -- stays inside the bound on every shared
  input set of the GPU tests (the worst ratio per family is printed);
* mutants of the model -- the mistakes the bound is there to catch -- each push at least one
  group's ratio above 1 on those same inputs."""
import functools
import math

import pytest
import torch

import user_oracle as uo
from fedrec_with_pytorchdistributed_amd.ops import reference as ref

DK = uo.DK
SC = torch.tensor(1.0 / math.sqrt(DK), dtype=torch.float32)
EPSF = torch.tensor(1e-8, dtype=torch.float32)
NINF = -math.inf


def bf(x):
    return x.to(torch.bfloat16).float()


def report(family, worst):
    print("user-oracle model ratio %-22s %.3f" % (family, worst))


# ------------------------------------------------------------------------------ rounding models
def model_attn(qkv, keep, NH, dctx=None, mut="", bf16_out=False):
    """-> (ctx, stats [B, NH, H, 2], ctx_b, dqkv | None) in the kernels' order of operations."""
    B, H, _ = qkv.shape
    q, k, v = qkv.view(B, H, 3, NH, DK).permute(2, 0, 3, 1, 4)
    kp = torch.ones(B, 1, 1, H, dtype=torch.bool) if keep is None else (keep != 0).view(B, 1, 1, H)
    kpf = torch.ones_like(kp) if mut == "fwd_mask" else kp  # mutant: a masked key keeps its weight
    long = H > 64
    S = (q @ k.transpose(-1, -2)) * SC
    Sm = S.masked_fill(~kpf, NINF)
    if not long:
        m = Sm.amax(-1, keepdim=True)
        m = torch.where(m == NINF, torch.zeros_like(m), m)
        p = torch.exp(Sm - m)
        L = p.sum(-1, keepdim=True)
        acc = p @ v
    else:  # online softmax over 64-key chunks
        m = torch.full((B, NH, H, 1), NINF)
        L = torch.zeros(B, NH, H, 1)
        acc = torch.zeros(B, NH, H, DK)
        for s0 in range(0, H, 64):
            Sc = Sm[..., s0:s0 + 64]
            mc = torch.maximum(m, Sc.amax(-1, keepdim=True))
            alpha = torch.where(mc == NINF, torch.zeros_like(mc), torch.exp(m - mc))
            p = torch.where(Sc == NINF, torch.zeros_like(Sc), torch.exp(Sc - mc))
            L = (L if mut == "long_alpha" else L * alpha) + p.sum(-1, keepdim=True)  # mutant: l not rescaled
            acc = acc * alpha + p @ v[:, :, s0:s0 + 64]
            m = mc
        m = torch.where(m == NINF, torch.zeros_like(m), m)
    et = {"no_eps": torch.zeros_like(m), "eps_unscaled": EPSF.expand_as(m)}.get(mut, EPSF * torch.exp(-m))
    l = L + et
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    ctx4 = acc * inv
    if mut == "head_tile" and not long:  # mutant: the first 16-row query tile from the neighbouring head
        ctx4 = ctx4.clone()
        ctx4[:, :, :16] = torch.roll(acc * inv, 1, dims=1)[:, :, :16]
    inv_s = torch.where(L > 0, 1.0 / L, torch.zeros_like(L)) if mut == "inv_no_eps" else inv  # mutant: saved 1 / l
    ctx = ctx4.permute(0, 2, 1, 3).reshape(B, H, NH * DK)
    stats = torch.cat([m, inv_s], -1)
    if dctx is None:
        return ctx, stats, bf(ctx), None
    g = dctx.view(B, H, NH, DK).permute(0, 2, 1, 3)
    Pun = torch.exp(S - m) * inv_s  # recomputed from the saved stats
    P = torch.where(kp, Pun, torch.zeros_like(Pun))
    dA = g @ v.transpose(-1, -2)
    Dt = ((Pun if mut == "D_masked" else P) * dA).sum(-1, keepdim=True)  # mutant: D_t over masked keys too
    dS = P * (dA - Dt) * SC
    Pk = Pun if mut == "bwd_mask" else P  # mutant: a masked key gets dK / dV
    dSk = Pk * (dA - Dt) * SC
    if mut == "bf16_twice" and bf16_out:  # mutant: the dS / P operands rounded as well as the outputs
        dS, dSk, Pk = bf(dS), bf(dSk), bf(Pk)
    if long:
        dQ = SC * (((P * dA) @ k) - Dt * (P @ k))
    else:
        dQ = dS @ k
    parts = [dQ, dSk.transpose(-1, -2) @ q, Pk.transpose(-1, -2) @ g]
    dqkv = torch.cat([x.permute(0, 2, 1, 3).reshape(B, H, NH * DK) for x in parts], 2)
    return ctx, stats, bf(ctx), (bf(dqkv) if bf16_out else dqkv)


def model_pool_fwd(x, e, w2, b2, keep):
    a = e @ w2 + b2
    if keep is not None:
        a = a.masked_fill(keep == 0, NINF)
    m = a.amax(-1, keepdim=True)
    m = torch.where(m == NINF, torch.zeros_like(m), m)
    p = torch.exp(a - m)
    alpha = p * (1.0 / (p.sum(-1, keepdim=True) + EPSF * torch.exp(-m)))
    return torch.einsum("nt,ntd->nd", alpha, x), alpha


def model_pool_bwd(x, e, alpha, w2, g, mut=""):
    dal = torch.einsum("ntd,nd->nt", x, g)
    sd = (alpha * dal).sum(-1, keepdim=True)
    da = alpha * (dal if mut == "da_no_sum" else dal - sd)  # mutant: no - sum alpha dalpha
    dw = da.unsqueeze(-1) * w2
    dpre = dw if mut == "dpre_no_tanh" else dw * (1.0 - e * e)  # mutant: no (1 - e^2)
    return dict(da=da, dx=alpha.unsqueeze(-1) * g.unsqueeze(1), dpre=dpre, dpre_b=bf(dpre),
                dw2=torch.einsum("nt,ntq->q", da, e), db2=da.sum().reshape(1))


def model_score(cand, u, act, mut=""):
    B, C, _ = cand.shape
    z = torch.einsum("bcd,bd->bc", cand, u)
    s = 1.0 / (1.0 + torch.exp(-z)) if act == "sigmoid" else z
    mx = s.amax(-1, keepdim=True)
    ex = torch.exp(s - mx)
    se = ex.sum(-1, keepdim=True)
    lab = 1 if mut == "label1" else 0  # mutant: the label in column 1
    hot = torch.zeros(B, C)
    hot[:, lab] = 1.0
    scale = 1.0 if mut == "no_invB" else 1.0 / B  # mutant: no 1 / B
    ds = (ex / se - hot) * scale
    dz = ds * s * (1.0 - s) if act == "sigmoid" else ds
    lossb = ((mx + torch.log(se)).squeeze(-1) - s[:, lab]) * scale
    dzu = torch.roll(dz, 1, dims=1) if mut == "wrong_dz" else dz  # mutant: duser with a neighbour's dz
    return lossb.sum(), s, dz.unsqueeze(-1) * u.unsqueeze(1), torch.einsum("bc,bcd->bd", dzu, cand)


# ------------------------------------------------------------------------------ shared cases
@functools.lru_cache(maxsize=16)
def attn_case(H, NH, regime, masked, keep_x=False):
    qkv, keep, dctx = uo.attn_inputs(H, NH, regime, masked)
    return qkv, keep, dctx, uo.AttnOracle(qkv, keep, NH, dctx, keep_x)


def attn_ratios(orc, out, bf16_out=False):
    ctx, stats, ctx_b, dqkv = out
    w = {"ctx": orc.check_ctx(ctx), "ctx_b": orc.check_ctx(ctx_b, bf16=True), "stats": orc.check_stats(stats)}
    w.update(orc.check_bwd(dqkv, bf16=bf16_out))
    return max(w.values())


ATTN_ALL = [c + (mk,) for c in uo.attn_cases() for mk in (False, True)]


def _fails(f) -> bool:
    try:
        f()
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------ autograd
def close(a, b, scale=None):
    s = float((b if scale is None else scale).abs().max())
    assert float((a - b).abs().max()) <= 1e-12 * s + 1e-300, (float((a - b).abs().max()), s)


@pytest.mark.parametrize("H,NH,regime,masked", [(17, 3, "randn", True), (50, 3, "eps", True), (64, 3, "ovf", False),
                                               (76, 3, "eps", True), (129, 3, "q4", True), (33, 20, "eps", False)])
def test_attention_explicit_equals_autograd(H, NH, regime, masked):
    qkv, keep, dctx, orc = attn_case(H, NH, regime, masked, True)
    x = qkv.double().requires_grad_(True)
    ctx, A = ref.user_attention_fwd(x, NH, DK, keep=keep)
    ctx.backward(dctx.double())
    close(orc.ctx, ctx.detach())
    close(orc.x["A"], A.detach())
    close(orc.dqkv, x.grad)
    close(orc.dqkv, ref.user_attention_bwd(qkv.double(), A.detach(), dctx.double(), NH, DK))


@pytest.mark.parametrize("T,D,Q,masked", [(17, 400, 200, True), (50, 256, 4, True), (64, 512, 256, False),
                                          (76, 400, 200, True)])
def test_pool_explicit_equals_autograd(T, D, Q, masked):
    x, e, w2, b2, keep, g = uo.pool_inputs(T, D, Q, masked)
    po = uo.PoolOracle(x, e, w2, b2, keep)
    xs = [t.double().requires_grad_(True) for t in (x, e, w2, b2)]
    pooled, alpha = ref.additive_pool_fwd(*xs, keep=keep)
    pooled.backward(g.double())
    bw = po.backward(g)
    close(po.pooled, pooled.detach())
    close(po.alpha, alpha.detach())
    close(bw["dx"][0], xs[0].grad)
    close(bw["dpre"][0], xs[1].grad * (1 - e.double() ** 2))
    close(bw["da"][0].unsqueeze(-1) * w2.double(), xs[1].grad)
    close(bw["dw2"][0], xs[2].grad)
    # sum_t da_t cancels to (1 - sum alpha) sum alpha dalpha: relative to the terms, not to the sum
    close(bw["db2"][0], xs[3].grad.reshape(1), scale=bw["da"][0].abs().sum())


@pytest.mark.parametrize("act", ["sigmoid", "identity"])
@pytest.mark.parametrize("B,C,D,kind", [(5, 5, 400, "small"), (33, 16, 64, "wide"), (5, 2, 256, "sat"), (1, 1, 64, "small")])
def test_score_explicit_equals_autograd(B, C, D, kind, act):
    cand, u = uo.score_inputs(B, C, D, kind)
    so = uo.ScoreOracle(cand, u, act)
    c64, u64 = cand.double().requires_grad_(True), u.double().requires_grad_(True)
    loss, s, dc, du = ref.score_ce_fwd_bwd(c64, u64, act)
    loss.backward()
    close(so.loss, loss.detach().reshape(1))
    close(so.scores, s.detach())
    # at |z| = 30 the reference's own fp64 ``1 - s`` has three digits: relative to |ds| |user|, which it rounds
    mag_c = (so.x["dz"].abs() + so.x["p"] / B * 1e-3).unsqueeze(-1) * u64.detach().abs().unsqueeze(1)
    for mine, theirs in ((so.dcand, c64.grad), (so.dcand, dc.detach())):
        close(mine, theirs, scale=mag_c * (1e3 if (act == "sigmoid" and kind != "small") else 1.0))
    mag_u = torch.einsum("bc,bcd->bd", so.x["p"] / B, cand.double().abs())
    for mine, theirs in ((so.duser, u64.grad), (so.duser, du.detach())):
        close(mine, theirs, scale=mag_u)


# -------------------------------------------------------------------------- the models pass
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("H", uo.H_SHORT + uo.H_LONG)
def test_attention_model_inside_bound(H, masked):
    worst = 0.0
    for (h, NH, regime) in uo.attn_cases():
        if h != H:
            continue
        qkv, keep, dctx, orc = attn_case(H, NH, regime, masked)
        worst = max(worst, attn_ratios(orc, model_attn(qkv, keep, NH, dctx)))
        if H <= 64:
            worst = max(worst, attn_ratios(orc, model_attn(qkv, keep, NH, dctx, bf16_out=True), bf16_out=True))
    report("attention H=%d%s" % (H, " masked" if masked else ""), worst)


def pool_ratios(po, g, pooled, alpha, out, ta=None, tg=None, skip=()):
    bw = po.backward(g, alpha=alpha if ta is None else None, ta=ta, tg=tg)
    w = [uo.check(pooled, po.pooled, po.tol_pooled, "pooled"), uo.check(alpha, po.alpha, po.tol_alpha, "alpha")]
    for name in ("da", "dx", "dpre", "dpre_b", "dw2", "db2"):
        if name not in skip:
            w.append(uo.check(out[name], bw[name][0], bw[name][1], name))
    return max(w)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("T,D,Q", uo.POOL_SHAPES + uo.POOL_LONG)
def test_pool_model_inside_bound(T, D, Q, masked):
    x, e, w2, b2, keep, g = uo.pool_inputs(T, D, Q, masked)
    po = uo.PoolOracle(x, e, w2, b2, keep)
    pooled, alpha = model_pool_fwd(x, e, w2, b2, keep)
    report("pool T=%d D=%d Q=%d" % (T, D, Q), pool_ratios(po, g, pooled, alpha, model_pool_bwd(x, e, alpha, w2, g)))
    if masked:  # an all-masked sequence: everything exactly 0
        assert not bool(po.alpha[1].any()) and not bool(po.pooled[1].any())


SCORE_CASES = [(B, C, D, kind, act) for B in uo.SCORE_B for C in uo.SCORE_C for D in uo.SCORE_D
               for kind, act in uo.SCORE_REGIMES]


def test_score_model_inside_bound():
    worst = 0.0
    for B, C, D, kind, act in SCORE_CASES:
        cand, u = uo.score_inputs(B, C, D, kind)
        worst = max(worst, uo.ScoreOracle(cand, u, act).check(*model_score(cand, u, act), what=str((B, C, D, kind, act))))
    report("score_ce", worst)


def test_score_rows_model_inside_bound():
    worst = 0.0
    for B in uo.ROWS_B:
        for C, D in uo.ROWS_CD:
            for kind, act in uo.SCORE_REGIMES:
                table, ci, u = uo.rows_inputs(B, C, D, kind)
                cand = table[ci.long()].view(B, C, D)
                so = uo.ScoreOracle(cand, u, act)
                worst = max(worst, so.check(*model_score(cand, u, act), what=str((B, C, D, kind, act))))
    report("score_ce_rows", worst)


def test_tail_model_inside_composed_bound():
    worst = 0.0
    for B, T, D, Q, C, act, masked, want_bwd in uo.TAIL_CASES:
        x, e, w2, b2, keep, table, ci = uo.tail_inputs(B, T, D, Q, C, masked)
        po, so, bw = uo.tail_oracle(x, e, w2, b2, keep, table, ci, act)
        pooled, alpha = model_pool_fwd(x, e, w2, b2, keep)
        cand = table[ci.long()].view(B, C, D)
        loss, s, dc, du = model_score(cand, pooled, act)
        worst = max(worst, so.check(loss, s, dc, du, "tail"))
        out = model_pool_bwd(x, e, alpha, w2, du)
        worst = max(worst, pool_ratios(po, so.duser, pooled, alpha, out, ta=po.tol_alpha, tg=so.tol_duser,
                                       skip=("dw2", "db2")))
    report("fused tail", worst)


# ------------------------------------------------------------------------------- the mutants
ATTN_MUTANTS = ["no_eps", "eps_unscaled", "fwd_mask", "bwd_mask", "D_masked", "inv_no_eps", "head_tile", "long_alpha",
                "bf16_twice"]


@pytest.mark.parametrize("mut", ATTN_MUTANTS)
def test_attention_mutant_exceeds_bound(mut):
    """Each mutant is above 1 for some (impression, head) of some shared case; the cases most
    likely to show it come first."""
    eps_first = mut in ("no_eps", "eps_unscaled", "inv_no_eps")
    cases = sorted(ATTN_ALL, key=lambda c: ((c[2] not in ("eps", "ovf")) if eps_first else (not c[3]), c[0], c[1]))
    for H, NH, regime, masked in cases:
        if (mut == "long_alpha" and H <= 64) or (mut in ("head_tile", "bf16_twice") and H > 64):
            continue  # a mutant of the other form
        if mut in ("fwd_mask", "bwd_mask", "D_masked") and not masked:
            continue
        qkv, keep, dctx, orc = attn_case(H, NH, regime, masked)
        bfo = mut == "bf16_twice"
        if _fails(lambda: attn_ratios(orc, model_attn(qkv, keep, NH, dctx, mut=mut, bf16_out=bfo), bf16_out=bfo)):
            print("mutant %s caught at H=%d NH=%d %s masked=%s" % (mut, H, NH, regime, masked))
            return
    raise AssertionError("mutant %s stays inside the bound on every shared case" % mut)


@pytest.mark.parametrize("mut", ["da_no_sum", "dpre_no_tanh"])
def test_pool_mutant_exceeds_bound(mut):
    for T, D, Q in uo.POOL_SHAPES + uo.POOL_LONG:
        x, e, w2, b2, keep, g = uo.pool_inputs(T, D, Q, True)
        po = uo.PoolOracle(x, e, w2, b2, keep)
        pooled, alpha = model_pool_fwd(x, e, w2, b2, keep)
        if _fails(lambda: pool_ratios(po, g, pooled, alpha, model_pool_bwd(x, e, alpha, w2, g, mut))):
            print("mutant %s caught at T=%d D=%d Q=%d" % (mut, T, D, Q))
            return
    raise AssertionError("mutant %s stays inside the bound on every shared case" % mut)


@pytest.mark.parametrize("mut", ["label1", "no_invB", "wrong_dz"])
def test_score_mutant_exceeds_bound(mut):
    for B, C, D, kind, act in SCORE_CASES:
        if (C if mut != "no_invB" else B) == 1:
            continue  # the mutant is the identity there
        cand, u = uo.score_inputs(B, C, D, kind)
        so = uo.ScoreOracle(cand, u, act)
        if _fails(lambda: so.check(*model_score(cand, u, act, mut), what=mut)):
            print("mutant %s caught at B=%d C=%d D=%d %s %s" % (mut, B, C, D, kind, act))
            return
    raise AssertionError("mutant %s stays inside the bound on every shared case" % mut)
