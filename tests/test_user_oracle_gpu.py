"""Every user-tower kernel form against the fp64 oracle and its per-element bound
(``tests/user_oracle.py``): the user attention forward and backward (the fp32 matrix-core forms at
H <= 64 with their bf16 outputs, the long forms up to H = 2048, the forms with the Q|K|V projection
and the pool's dctx GEMM fused in), the additive pool's fp32 user forms, ``score_ce`` in both
variants and its table-row form, and the fused tail ``user_pool_score``.  Attention is judged per
(impression, head), pool and score per impression.  Every call is made twice and must be
bit-identical and finite.  The inputs are the shared builders of ``user_oracle`` (the mask zoo, the
eps-dominated and overflowing score regimes, saturated sigmoids, repeated table rows);
``tests/test_user_oracle_cpu.py`` runs a rounding model and its mutants over the same sets.  Each
test prints its worst ratio (``-rP`` shows them)."""
import ctypes

import pytest
import torch

import user_oracle as uo
from gemm_oracle import U as GEMM_U
from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import native

pytestmark = pytest.mark.gpu

DK = uo.DK
BF = torch.bfloat16


def report(form, worst):
    print("attn-oracle ratio %-34s %.3f" % (form, worst))


def _twice(f):
    """Call twice: bit-identical and finite.  -> the first result (a tensor or a tuple)."""
    a, b = f(), f()
    ta = a if isinstance(a, (tuple, list)) else (a,)
    tb = b if isinstance(b, (tuple, list)) else (b,)
    for x, y in zip(ta, tb):
        assert torch.equal(x, y), "a second call differs"
        assert bool(torch.isfinite(x.float()).all()), "a non-finite value"
    return a


def _to(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


def _zero(t) -> bool:
    return not bool(t.any())


# ================================================================================== attention
def attn_fwd(qkv, keep, NH, with_b):
    cb = torch.full(qkv.shape[:2] + (NH * DK,), float("nan"), device=qkv.device, dtype=BF) if with_b else None
    ctx, stats = ops.user_attention_fwd(qkv, NH, DK, keep, cb)
    return (ctx, stats, cb) if with_b else (ctx, stats)


@pytest.mark.parametrize("H,NH,regime", uo.attn_cases())
def test_attention_forward_and_backward(dev, H, NH, regime):
    """``user_attention_fwd`` (ctx, the saved stats, ctx_b at H <= 64) and ``user_attention_bwd``
    (fp32, and ``bf16_out`` at H <= 64; dQ, dK, dV judged separately), without a mask and with the
    mask zoo; the gradients of masked keys and of an all-masked impression are exactly 0."""
    short = H <= 64
    for masked in (False, True):
        qkv_c, keep_c, dctx_c = uo.attn_inputs(H, NH, regime, masked)
        orc = uo.AttnOracle(qkv_c, keep_c, NH, dctx_c)
        qkv, keep, dctx = _to(dev, qkv_c, keep_c, dctx_c)
        tag = "H=%d%s" % (H, " masked" if masked else "")
        out = _twice(lambda: attn_fwd(qkv, keep, NH, short))
        report("user fwd ctx " + tag, orc.check_ctx(out[0], tag + " ctx"))
        report("user fwd stats " + tag, orc.check_stats(out[1], tag + " stats"))
        if short:
            report("user fwd ctx_b " + tag, orc.check_ctx(out[2], tag + " ctx_b", bf16=True))
        forms = [(False, "bwd fp32")] + ([(True, "bwd bf16")] if short else [])
        for bf16_out, name in forms:
            d = _twice(lambda: ops.user_attention_bwd(qkv, out[1], dctx, NH, DK, keep, bf16_out))
            assert d.dtype == (BF if bf16_out else torch.float32)
            for part, r in orc.check_bwd(d, "%s %s" % (tag, name), bf16=bf16_out).items():
                report("user %s %s %s" % (name, part, tag), r)
            if masked:
                D = NH * DK
                rows = orc.masked_rows().to(dev)
                assert _zero(d[..., D:][rows]), "a masked key has a dK / dV"
                if orc.B > 1:
                    assert not bool(keep_c[1].any())
                    assert _zero(d[1]) and _zero(out[0][1]), "an all-masked impression has a gradient / a ctx"


def _fused_inputs(H, NH, Din, masked):
    g = torch.Generator().manual_seed(9176 + 131 * H + Din)
    keep = uo.zoo_mask(H, g) if masked else None
    B = 5
    xd = torch.randn(B * H, Din, generator=g).to(BF)
    W = (torch.randn(3 * NH * DK, Din, generator=g) / Din ** 0.5).to(BF)
    bias = torch.randn(3 * NH * DK, generator=g)
    return B, xd, W, bias, keep


@pytest.mark.parametrize("Din,NH", [(8, 3), (400, 20)])
@pytest.mark.parametrize("H", uo.H_FUSED)
def test_qkv_attention_fused(dev, H, Din, NH):
    """``user_qkv_attention_fwd``: the written qkv against the fp64 GEMM of the bf16 operands (the
    K-term fp32-accumulate bound of ``gemm_oracle``: (K + 2) U S); ctx, stats and ctx_b against the
    attention oracle evaluated on that written qkv."""
    for masked in (False, True):
        B, xd_c, W_c, bias_c, keep_c = _fused_inputs(H, NH, Din, masked)
        xd, W, bias, keep = _to(dev, xd_c, W_c, bias_c, keep_c)
        D = NH * DK

        def run():
            cb = torch.full((B, H, D), float("nan"), device=dev, dtype=BF)
            return ops.user_qkv_attention_fwd(xd, W, bias, B, NH, DK, keep, cb) + (cb,)

        ctx, stats, qkv, cb = _twice(run)
        want = xd_c.double() @ W_c.double().t() + bias_c.double()
        S = xd_c.double().abs() @ W_c.double().abs().t() + bias_c.double().abs()
        tag = "H=%d Din=%d%s" % (H, Din, " masked" if masked else "")
        w = uo.check(qkv.view(B * H, 3 * D), want, (Din + 2) * GEMM_U * S + uo.TINY, tag + " qkv")
        report("user qkv-fused qkv " + tag, w)
        orc = uo.AttnOracle(qkv.cpu(), keep_c, NH)
        report("user qkv-fused ctx, stats " + tag,
               max(orc.check_ctx(ctx, tag + " ctx"), orc.check_stats(stats, tag + " stats")))
        report("user qkv-fused ctx_b " + tag, orc.check_ctx(cb, tag + " ctx_b", bf16=True))


@pytest.mark.parametrize("Qd,NH", [(8, 3), (200, 20)])
@pytest.mark.parametrize("H", uo.H_FUSED)
def test_attention_bwd_dctx_fused(dev, H, Qd, NH):
    """``user_attention_bwd_dctx`` is bit-equal to the two-launch sequence (the dctx GEMM, then the
    bf16 backward), and that result is on the oracle with dctx the fp32 sum the GEMM produced."""
    for masked in (False, True):
        qkv_c, keep_c, dctx_c = uo.attn_inputs(H, NH, "randn", masked)
        B, D = qkv_c.shape[0], NH * DK
        g = torch.Generator().manual_seed(4409 + H + Qd)
        dpre_c = torch.randn(B * H, Qd, generator=g).to(BF)
        w1t_c = (torch.randn(D, Qd, generator=g) / Qd ** 0.5).to(BF)
        qkv, keep, dctx, dpre, w1t = _to(dev, qkv_c, keep_c, dctx_c, dpre_c, w1t_c)
        _, stats = ops.user_attention_fwd(qkv, NH, DK, keep)
        got = _twice(lambda: ops.user_attention_bwd_dctx(qkv, stats, dctx, dpre, w1t, NH, DK, keep))
        assert torch.equal(dctx.cpu(), dctx_c), "dctx_direct was written"
        d2 = dctx.clone()
        ops.small_gemm(ops.Gemm(dpre, w1t, d2.view(B * H, D), B * H, D, Qd, Qd, Qd, D, accumulate=True), tile=1004)
        want = ops.user_attention_bwd(qkv, stats, d2, NH, DK, keep, True)
        assert torch.equal(got, want)
        tag = "H=%d Qd=%d%s" % (H, Qd, " masked" if masked else "")
        orc = uo.AttnOracle(qkv_c, keep_c, NH, d2.cpu())
        report("user bwd-dctx " + tag, max(orc.check_bwd(got, tag, bf16=True).values()))


def test_attention_rejections(dev):
    """Shapes outside the kernels' domain: the op raises, or the launcher returns its code, before
    anything is launched (the buffers are real, whatever the launcher did with them)."""
    with pytest.raises(RuntimeError):
        ops.user_attention_fwd(torch.zeros(1, 2049, 3 * DK, device=dev), 1, DK)
    with pytest.raises(RuntimeError):
        ops.user_attention_fwd(torch.zeros(1, 4, 3 * 2 * 16, device=dev), 2, 16)
    with pytest.raises(RuntimeError):
        ops.user_attention_bwd(torch.zeros(1, 4, 3 * 2 * 16, device=dev), torch.zeros(1, 2, 4, 2, device=dev),
                               torch.zeros(1, 4, 32, device=dev), 2, 16)
    # ctx_b / bf16_out with H = 65: the launchers refuse (code 2); the ops convert the fp32 result
    H, NH = 65, 1
    so = ctypes.CDLL(str(native.SO_PATH))
    P, I = ctypes.c_void_p, ctypes.c_int
    so.fr_user_attn_fwd.argtypes = [P, P, P, I, I, I, I, P, P, P]
    so.fr_user_attn_bwd.argtypes = [P, P, P, P, I, I, I, I, P, P, I]
    so.fr_user_attn_fwd.restype = so.fr_user_attn_bwd.restype = I
    qkv = torch.randn(1, H, 3 * DK, device=dev)
    ctx = torch.full((1, H, DK), 7.0, device=dev)
    stats = torch.full((1, NH, H, 2), 7.0, device=dev)
    cb = torch.full((1, H, DK), 7.0, device=dev, dtype=BF)
    dq = torch.full((1, H, 3 * DK), 7.0, device=dev, dtype=BF)
    torch.cuda.synchronize()
    q_, c_, s_ = qkv.data_ptr(), ctx.data_ptr(), stats.data_ptr()
    assert so.fr_user_attn_fwd(q_, c_, s_, 1, H, NH, DK, None, None, cb.data_ptr()) == 2
    assert so.fr_user_attn_bwd(q_, s_, c_, dq.data_ptr(), 1, H, NH, DK, None, None, 1) == 2
    assert so.fr_user_attn_fwd(q_, c_, s_, 1, 2049, NH, DK, None, None, None) == 1
    assert so.fr_user_attn_fwd(q_, c_, s_, 1, H, NH, 16, None, None, None) == 1
    torch.cuda.synchronize()
    for t in (ctx, stats, cb, dq):
        assert bool((t == 7.0).all()), "a refused call wrote an output"
    c2, st2 = ops.user_attention_fwd(qkv, NH, DK, None, cb)
    assert torch.equal(cb, c2.to(BF))
    assert torch.equal(ops.user_attention_bwd(qkv, st2, c2, NH, DK, None, True),
                       ops.user_attention_bwd(qkv, st2, c2, NH, DK).to(BF))


# ====================================================================================== pools
def _pool_checks(dev, T, D, Q, masked, da_form):
    x_c, e_c, w2_c, b2_c, keep_c, g_c = uo.pool_inputs(T, D, Q, masked)
    po = uo.PoolOracle(x_c, e_c, w2_c, b2_c, keep_c)
    x, e, w2, b2, keep, g = _to(dev, x_c, e_c, w2_c, b2_c, keep_c, g_c)
    tag = "T=%d D=%d Q=%d%s" % (T, D, Q, " masked" if masked else "")
    pooled, alpha = _twice(lambda: ops.additive_pool_fwd(x, e, w2, b2, keep))
    w = max(uo.check(pooled, po.pooled, po.tol_pooled, tag + " pooled"),
            uo.check(alpha, po.alpha, po.tol_alpha, tag + " alpha"))
    report("user pool fwd " + tag, w)
    bw = po.backward(g_c, alpha=alpha.cpu())  # the backward reads the alpha the forward wrote
    dx, dpre, dw2, db2 = _twice(lambda: ops.additive_pool_bwd(x, e, alpha, w2, g, True))
    outs = dict(dx=dx, dpre=dpre, dw2=dw2, db2=db2)
    zero = [dx, dpre]
    if da_form:
        dx2, dpre2, da8, dpre_b = _twice(lambda: native.lib().upool_bwd_da(x, e, alpha, w2, g, True))
        outs.update(dx_da=dx2, dpre_da=dpre2, da=da8[:, 0].view(-1, T), dpre_b=dpre_b)
        assert _zero(da8[:, 1:]), "da8 columns 1.. are not zero"
        zero += [dx2, dpre2, da8.view(-1, T, 8), dpre_b]
    w = {k: uo.check(v, *bw[k.replace("_da", "")], "%s %s" % (tag, k), lead=0 if k in ("dw2", "db2") else 1)
         for k, v in outs.items()}
    if da_form:
        report("user pool bwd dpre_b " + tag, w.pop("dpre_b"))
    report("user pool bwd " + tag, max(w.values()))
    if masked:  # sequence 1 is all masked: everything exactly 0
        assert not bool(keep_c[1].any())
        assert _zero(alpha[1]) and _zero(pooled[1]), "an all-masked sequence pools to non-zero"
        for t in zero:
            assert _zero(t[1]), "an all-masked sequence has a gradient"


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("T,D,Q", uo.POOL_SHAPES)
def test_user_pool_short_forms(dev, T, D, Q, masked):
    """``upool_fwd`` / ``upool_bwd`` (US = 4 blocks per sequence) and ``upool_bwd_da``."""
    _pool_checks(dev, T, D, Q, masked, True)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("T,D,Q", uo.POOL_LONG)
def test_user_pool_generic_form(dev, T, D, Q, masked):
    _pool_checks(dev, T, D, Q, masked, False)


# ================================================================================= score + CE
@pytest.mark.parametrize("D", uo.SCORE_D)
@pytest.mark.parametrize("B", uo.SCORE_B)
def test_score_ce_both_variants(dev, B, D):
    lib = native.lib()
    worst = 0.0
    for C in uo.SCORE_C:
        for kind, act in uo.SCORE_REGIMES:
            cand_c, u_c = uo.score_inputs(B, C, D, kind)
            so = uo.ScoreOracle(cand_c, u_c, act)
            cand, u = _to(dev, cand_c, u_c)
            for variant in (1, 0):
                lib.score_set_variant(variant)
                try:  # process-global: restored even when the call fails
                    out = _twice(lambda: ops.score_ce(cand, u, act))
                finally:
                    lib.score_set_variant(1)
                worst = max(worst, so.check(*out, what="variant %d B=%d C=%d D=%d %s %s" % (variant, B, C, D, kind, act)))
    report("score_ce B=%d D=%d" % (B, D), worst)


@pytest.mark.parametrize("B", uo.ROWS_B)
def test_score_ce_rows(dev, B):
    """The table-row form, its batch loss summed by the last block (130 > one 64-lane pass); the
    second call gives the identical loss: the ticket was re-armed."""
    worst = 0.0
    for C, D in uo.ROWS_CD:
        for kind, act in uo.SCORE_REGIMES:
            table_c, ci_c, u_c = uo.rows_inputs(B, C, D, kind)
            so = uo.ScoreOracle(table_c[ci_c.long()].view(B, C, D), u_c, act)
            table, ci, u = _to(dev, table_c, ci_c, u_c)

            def run():
                dc = torch.full((B * C, D), float("nan"), device=dev)
                loss, scores, du = ops.score_ce_rows(table, ci, u, act, dc)
                return loss, scores, dc, du

            worst = max(worst, so.check(*_twice(run), what="rows B=%d C=%d D=%d %s %s" % (B, C, D, kind, act)))
    report("score_ce_rows B=%d" % B, worst)


def test_score_ce_rejects_17_candidates(dev):
    with pytest.raises(RuntimeError):
        ops.score_ce(torch.zeros(2, 17, 64, device=dev), torch.zeros(2, 64, device=dev), "sigmoid")


# ============================================================================ the fused tail
@pytest.mark.parametrize("B,T,D,Q,C,act,masked,want_bwd", uo.TAIL_CASES)
def test_user_pool_score(dev, B, T, D, Q, C, act, masked, want_bwd):
    """``user_pool_score`` against the composed oracle (pool -> score + CE -> pool backward for
    du), and the three-launch path the engine falls back to against the same oracle (so the two
    agree within the two bounds)."""
    cpu = uo.tail_inputs(B, T, D, Q, C, masked)
    po, so, bw = uo.tail_oracle(*cpu, act, want_bwd)
    x, e, w2, b2, keep, table, ci = _to(dev, *cpu)
    sig = 1 if act == "sigmoid" else 0

    def fused():
        dc = torch.full((B * C, D), float("nan"), device=dev)
        return tuple(native.lib().user_pool_score(x, e, w2, b2, keep, table, ci, sig, dc, want_bwd)) + (dc,)

    def three():
        u, alpha = ops.additive_pool_fwd(x, e, w2, b2, keep)
        dc = torch.full((B * C, D), float("nan"), device=dev)
        loss, scores, du = ops.score_ce_rows(table, ci, u, act, dc)
        if not want_bwd:
            return loss, scores, None, None, None, None, dc
        dctx, dpre, da8, dpre_b = native.lib().upool_bwd_da(x, e, alpha, w2, du, True)
        return loss, scores, dctx, dpre, dpre_b, da8, dc

    tag = "B=%d T=%d D=%d Q=%d C=%d %s%s%s" % (B, T, D, Q, C, act, " masked" if masked else "", "" if want_bwd else " fwd")
    for name, out in (("fused", _twice(fused)), ("3-launch", three())):
        loss, scores, dctx, dpre, dpre_b, da8, dc = out
        assert loss.numel() == 1, "the fused form refused a shape of its domain"
        w = [uo.check(loss.reshape(1), so.loss, so.tol_loss, tag + " loss", lead=1),
             uo.check(scores, so.scores, so.tol_scores, tag + " scores"),
             uo.check(dc, so.dcand, so.tol_dcand, tag + " dcand")]
        if want_bwd:
            w += [uo.check(dctx, *bw["dx"], tag + " dctx"), uo.check(dpre, *bw["dpre"], tag + " dpre"),
                  uo.check(dpre_b, *bw["dpre_b"], tag + " dpre_b"),
                  uo.check(da8[:, 0].view(B, T), *bw["da"], tag + " da8")]
            assert _zero(da8[:, 1:]), "da8 columns 1.. are not zero"
        else:
            assert out[2] is None or out[2].numel() == 0
        report("user tail %s %s" % (name, tag), max(w))


@pytest.mark.parametrize("T,D,C", [(65, 400, 5), (17, 252, 5), (17, 516, 5), (17, 400, 17)])
def test_user_pool_score_not_this_form(dev, T, D, C):
    """Outside the fused form's domain the op returns an empty loss and launches nothing."""
    B, Q = 2, 200
    g = torch.Generator().manual_seed(T + D + C)
    x, e = torch.randn(B, T, D, generator=g).to(dev), torch.tanh(torch.randn(B, T, Q, generator=g)).to(dev)
    w2, b2 = torch.randn(Q, generator=g).to(dev), torch.zeros(1, device=dev)
    table = torch.randn(8, D, generator=g).to(dev)
    ci = torch.randint(0, 8, (B * C,), generator=g).to(torch.int32).to(dev)
    dc = torch.full((B * C, D), 7.0, device=dev)
    out = native.lib().user_pool_score(x, e, w2, b2, None, table, ci, 1, dc, True)
    torch.cuda.synchronize()
    assert out[0].numel() == 0
    assert bool((dc == 7.0).all()), "a refused call wrote dcand_out"
