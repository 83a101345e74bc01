"""The additive pool's bf16 kernels -- the 16-byte vectorised ``pool_fwd16`` / ``pool_bwd16`` (T <= 128)
and the generic ``pool_fwd_kernel<bf16>`` / ``pool_bwd_kernel<bf16>``, the only bf16 path that writes
``dx`` -- against the fp64 oracle and its per-element bounds (``tests/text_pool_oracle.py``), at every
lane map the shapes select, without a mask and with the mask zoo.  Every call is made twice and must
be bit-identical and finite; ``dsum`` is held to the column sums of the ``dpre`` the kernel wrote;
which kernel ran is pinned through ``dsum``'s presence.  ``tests/test_text_pool_oracle_cpu.py`` runs a
rounding model and its mutants over the same inputs.  Each test prints its worst ratios (``-rP``)."""
import pytest
import torch

import text_pool_oracle as tp
import user_oracle as uo
from fedrec_with_pytorchdistributed_amd import ops

pytestmark = pytest.mark.gpu


def report(form, worst):
    print("text-pool ratio %-34s %.3f" % (form, worst))


def _twice(f):
    """Call twice: bit-identical and finite.  -> the first result (None entries kept)."""
    a, b = f(), f()
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x, y), "a second call differs"
            assert bool(torch.isfinite(x.float()).all()), "a non-finite value"
    return a


def _zero(t) -> bool:
    return not bool(t.any())


def _case(dev, T, D, Q, masked, worst):
    vec = tp.vec_ok(T, D, Q)
    x_c, e_c, w2_c, b2_c, keep_c, g_c = tp.inputs(T, D, Q, masked)
    po = tp.oracle(T, D, Q, masked)
    x, e, w2, b2, keep, g = [None if t is None else t.to(dev) for t in (x_c, e_c, w2_c, b2_c, keep_c, g_c)]
    assert x.dtype == tp.BF and e.dtype == tp.BF
    tag = "T=%d D=%d Q=%d%s" % (T, D, Q, " masked" if masked else "")

    def note(name, r):
        worst[name] = max(worst.get(name, 0.0), r)

    pooled, alpha = _twice(lambda: ops.additive_pool_fwd(x, e, w2, b2, keep))
    assert pooled.dtype == torch.float32 and alpha.dtype == torch.float32
    note("pooled", uo.check(pooled, po.pooled, po.tol_pooled, tag + " pooled"))
    note("alpha", uo.check(alpha, po.alpha, po.tol_alpha, tag + " alpha"))
    bw = po.backward(g_c, alpha=alpha.cpu())  # the backward reads the alpha the forward wrote
    runs = {}
    for want_dx in (False, True):
        dx, dpre, dw2, db2, dsum = _twice(lambda: ops.additive_pool_bwd(x, e, alpha, w2, g, want_dx, want_colsum=True))
        runs[want_dx] = (dpre, dw2)
        path = "%s want_dx=%s" % (tag, want_dx)
        # the vectorised kernel, and only it, gives dsum; it does not write dx
        assert (dsum is not None) == (vec and not want_dx), path + ": dsum from the wrong kernel"
        assert (dx is not None) == want_dx and dpre.dtype == tp.BF and dpre.shape == e.shape
        if want_dx:
            assert dx.dtype == torch.float32 and dx.shape == x.shape
            note("dx", uo.check(dx, *bw["dx"], path + " dx"))
        note("dpre", uo.check(dpre, *bw["dpre_b"], path + " dpre"))
        note("dw2", uo.check(dw2, *bw["dw2"], path + " dw2", lead=0))
        note("db2", uo.check(db2, *bw["db2"], path + " db2", lead=0))
        if dsum is not None:
            assert dsum.shape == (Q,)
            note("dsum", uo.check(dsum, *tp.dsum_ref(dpre), path + " dsum", lead=0))
        if masked:  # sequence 1 is all masked: everything exactly 0
            assert not bool(keep_c[1].any())
            assert _zero(alpha[1]) and _zero(pooled[1]), tag + ": an all-masked sequence pools to non-zero"
            assert _zero(dpre[1]) and (dx is None or _zero(dx[1])), path + ": an all-masked sequence has a gradient"
    if vec:  # the two kernels on one input: each within its own bound of the oracle
        for (a, b), name in zip(zip(runs[False], runs[True]), ("dpre_b", "dw2")):
            want, tol = bw[name]
            uo.check(a, b.detach().double().cpu().reshape(want.shape), 2 * tol.expand_as(want),
                     tag + " %s vectorised vs generic" % name, lead=0)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("form", list(tp.FORMS))
def test_bf16_pool_forms(dev, form, masked):
    """Forward, and backward with and without ``dx`` (vectorised shapes: the generic backward must take
    the ``want_dx`` call and write ``dx``), per element."""
    worst = {}
    for T, D, Q in tp.FORMS[form]:
        _case(dev, T, D, Q, masked, worst)
    for k, v in worst.items():
        report("%s%s %s" % (form, " masked" if masked else "", k), v)
    report("%s%s" % (form, " masked" if masked else ""), max(worst.values()))
    assert ("dsum" in worst) == (form == "vectorised")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_no_sequences(dev, dtype):
    """n = 0: nothing is launched; empty outputs, dw2 and db2 exactly zero (they were the column sums
    of an unwritten partial row), dsum zero or absent."""
    T, D, Q = 50, 768, 384
    x, e = torch.zeros(0, T, D, device=dev, dtype=dtype), torch.zeros(0, T, Q, device=dev, dtype=dtype)
    w2, b2 = torch.ones(Q, device=dev), torch.ones(1, device=dev)
    pooled, alpha = ops.additive_pool_fwd(x, e, w2, b2)
    assert pooled.shape == (0, D) and alpha.shape == (0, T)
    g = torch.zeros(0, D, device=dev)
    for want_dx in (False, True):
        torch.full((2 * Q + 1,), float("nan"), device=dev)  # freed at once: the block the op's partial row gets next
        dx, dpre, dw2, db2, dsum = ops.additive_pool_bwd(x, e, alpha, w2, g, want_dx, want_colsum=True)
        assert dpre.shape == (0, T, Q) and (dx is None or dx.shape == (0, T, D))
        assert dw2.shape == (Q,) and db2.numel() == 1 and _zero(dw2) and _zero(db2)
        assert dsum is None or (dsum.shape == (Q,) and _zero(dsum))


def test_too_long_a_sequence_raises(dev):
    """T = 2049 > MAXT_G: the launchers return 1 before any launch and the ops raise."""
    T, D, Q = 2049, 8, 8
    x, e = torch.zeros(2, T, D, device=dev, dtype=tp.BF), torch.zeros(2, T, Q, device=dev, dtype=tp.BF)
    w2, b2 = torch.zeros(Q, device=dev), torch.zeros(1, device=dev)
    with pytest.raises(RuntimeError, match=r"additive_pool_fwd: unsupported shape \(code 1\)"):
        ops.additive_pool_fwd(x, e, w2, b2)
    alpha, g = torch.zeros(2, T, device=dev), torch.zeros(2, D, device=dev)
    for want_dx in (False, True):
        with pytest.raises(RuntimeError, match=r"additive_pool_bwd: kernel launch rejected the arguments \(code 1\)"):
            ops.additive_pool_bwd(x, e, alpha, w2, g, want_dx)
    torch.cuda.synchronize()
