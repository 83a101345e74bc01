"""The bf16 text-pool oracle (``tests/text_pool_oracle.py``) checked without a GPU:

* a rounding model of the two bf16 forms -- ``model_pool_fwd`` / ``model_pool_bwd`` of
  ``tests/test_user_oracle_cpu.py`` on the bf16 operands, ``dpre`` rounded to bf16 to nearest even,
  ``dsum`` from the rounded values -- stays inside every bound at every shape of the GPU tests,
  masked and unmasked (the worst ratio per family is printed);
* mutants of the model -- the mistakes a norm-wise 1e-2 lets through -- exceed a bound at the shapes
  where the kernels could make them;
* the argument checks of ``fedrec::additive_pool_fwd`` / ``_bwd`` raise on host tensors, one message
  per rule, and run before the device check."""
import functools

import pytest
import torch

import test_user_oracle_cpu as tu
import text_pool_oracle as tp
import user_oracle as uo
from fedrec_with_pytorchdistributed_amd.ops import native

ALL_SHAPES = tp.VEC_SHAPES + tp.GENERIC_SHAPES
NINF = tu.NINF


def report(family, worst):
    print("text-pool model ratio %-34s %.3f" % (family, worst))


# ------------------------------------------------------------------------------ rounding model
def model_fwd(x, e, w2, b2, keep, mut=""):
    xf, ef = x.float(), e.float()
    if mut == "eps_unscaled":  # mutant: + 1e-8 without exp(-m)
        a = ef @ w2 + b2
        if keep is not None:
            a = a.masked_fill(keep == 0, NINF)
        m = a.amax(-1, keepdim=True)
        m = torch.where(m == NINF, torch.zeros_like(m), m)
        p = torch.exp(a - m)
        alpha = p * (1.0 / (p.sum(-1, keepdim=True) + tu.EPSF))
        return torch.einsum("nt,ntd->nd", alpha, xf), alpha
    pooled, alpha = tu.model_pool_fwd(xf, ef, w2, b2, keep)
    if mut == "odd_rows_dropped":  # mutant: pooled = part[0] alone, the even t (part[1] holds the odd ones)
        pooled = torch.einsum("nt,ntd->nd", alpha[:, 0::2], xf[:, 0::2])
    return pooled, alpha


def model_bwd(x, e, alpha, w2, g, mut=""):
    """-> the dict of ``tu.model_pool_bwd`` with ``dpre_b`` as the kernels store it and ``dsum``."""
    xf, ef = x.float(), e.float()
    if mut == "d_chunk1_dropped":  # mutant: dalpha without the second 64-lane chunk over D (columns >= 512)
        xf = xf.clone()
        xf[..., 512:] = 0
    out = tu.model_pool_bwd(xf, ef, alpha, w2, g, mut)  # (its dx reads alpha and g only)
    dpre = out["dpre"]
    if mut == "dpre_trunc":  # mutant: bf16 by truncation
        out["dpre_b"] = (dpre.view(torch.int32) & -65536).view(torch.float32).to(tp.BF)
    else:
        out["dpre_b"] = dpre.to(tp.BF)
    out["dsum"] = (dpre if mut == "dsum_unrounded" else out["dpre_b"].float()).sum((0, 1))  # mutant: fp32 values summed
    return out


@functools.lru_cache(maxsize=None)
def model_case(T, D, Q, masked, mut=""):
    x, e, w2, b2, keep, g = tp.inputs(T, D, Q, masked)
    pooled, alpha = model_fwd(x, e, w2, b2, keep, mut)
    return pooled, alpha, model_bwd(x, e, alpha, w2, g, mut)


def judge(T, D, Q, masked, mut=""):
    """-> {family: worst ratio}; raises AssertionError (``uo.check``) at the first family above 1."""
    po = tp.oracle(T, D, Q, masked)
    g = tp.inputs(T, D, Q, masked)[5]
    pooled, alpha, out = model_case(T, D, Q, masked, mut)
    bw = po.backward(g, alpha=alpha)  # the alpha the forward wrote, as the GPU tests do
    w = dict(pooled=uo.check(pooled, po.pooled, po.tol_pooled, "pooled"),
             alpha=uo.check(alpha, po.alpha, po.tol_alpha, "alpha"))
    for name in ("dx", "dpre_b", "dw2", "db2"):
        w[name] = uo.check(out[name], *bw[name], name, lead=0 if name in ("dw2", "db2") else 1)
    if tp.vec_ok(T, D, Q):
        w["dsum"] = uo.check(out["dsum"], *tp.dsum_ref(out["dpre_b"]), "dsum", lead=0)
    return w


def fails(T, D, Q, mut) -> bool:
    return tu._fails(lambda: judge(T, D, Q, False, mut))


# -------------------------------------------------------------------------- the model passes
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("form", list(tp.FORMS))
def test_model_inside_every_bound(form, masked):
    worst = {}
    for T, D, Q in tp.FORMS[form]:
        for k, v in judge(T, D, Q, masked).items():
            worst[k] = max(worst.get(k, 0.0), v)
        if masked:  # sequence 1 is all masked: exactly zero in the oracle
            po = tp.oracle(T, D, Q, True)
            assert not bool(po.alpha[1].any()) and not bool(po.pooled[1].any())
    for k, v in worst.items():
        report("%s%s %s" % (form, " masked" if masked else "", k), v)
    assert ("dsum" in worst) == (form == "vectorised")


def test_dsum_depth_is_read_from_the_kernel():
    """TG = 256 / (Q / 8) t-groups; ``T + 4 n + 3`` of dw2's bound is no less at any shape here."""
    assert [tp.dsum_depth(T, Q, 5) for T, _, Q in tp.VEC_SHAPES] == [10 + 5 + 5, 32 + 4 + 5, 3 + 8 + 5, 1 + 7 + 5, 1 + 8 + 5]
    for T, D, Q in tp.VEC_SHAPES:
        n = tp.inputs(T, D, Q, False)[0].shape[0]
        assert n >= 2 and tp.dsum_depth(T, Q, n) <= T + 4 * n + 3


# ------------------------------------------------------------------------------- the mutants
@pytest.mark.parametrize("T,D,Q", ALL_SHAPES)
def test_eps_unscaled_exceeds_the_bound_on_the_eps_sequence(T, D, Q):
    po = tp.oracle(T, D, Q, False)
    _, alpha, _ = model_case(T, D, Q, False, "eps_unscaled")
    r = uo.ratios(alpha, po.alpha, po.tol_alpha)
    assert float(r[-1]) > 1.0, "eps_unscaled stays inside tol_alpha on the eps sequence (ratio %.3g)" % float(r[-1])
    assert fails(T, D, Q, "eps_unscaled")


@pytest.mark.parametrize("mut", ["dpre_trunc", "odd_rows_dropped", "da_no_sum", "dpre_no_tanh"])
@pytest.mark.parametrize("T,D,Q", ALL_SHAPES)
def test_mutant_exceeds_a_bound_at_every_shape(T, D, Q, mut):
    if mut == "odd_rows_dropped" and T == 1:
        assert not fails(T, D, Q, mut)  # no odd row: the mutant is the identity there
        return
    assert fails(T, D, Q, mut), "mutant %s stays inside every bound at T=%d D=%d Q=%d" % (mut, T, D, Q)


@pytest.mark.parametrize("T,D,Q", tp.VEC_SHAPES)
def test_dsum_unrounded_exceeds_the_bound_at_every_vectorised_shape(T, D, Q):
    assert fails(T, D, Q, "dsum_unrounded")


@pytest.mark.parametrize("T,D,Q", ALL_SHAPES)
def test_d_chunk1_dropped_exceeds_a_bound_exactly_where_d_passes_512(T, D, Q):
    assert fails(T, D, Q, "d_chunk1_dropped") == (D > 512)


# ------------------------------------------------------------------------- the argument checks
def _host(T=3, D=16, Q=8, n=2, dtype=torch.bfloat16):
    return dict(x=torch.zeros(n, T, D, dtype=dtype), e=torch.zeros(n, T, Q, dtype=dtype), alpha=torch.zeros(n, T),
                w2=torch.zeros(Q), g=torch.zeros(n, D), b2=torch.zeros(1))


E_SHARE, E_W2, E_CONTIG = r"e must share x's \[n, T\]", "w2 must be contiguous fp32 of Q = 8 elements", "x and e must be contiguous"
E_ALPHA, E_G = r"alpha must be contiguous fp32 \[n, T\] = \[2, 3\]", r"g must be contiguous fp32 \[n, D\] = \[2, 16\]"
BAD = [("e_n", dict(e=torch.zeros(3, 3, 8, dtype=torch.bfloat16)), E_SHARE, True),
       ("e_T", dict(e=torch.zeros(2, 4, 8, dtype=torch.bfloat16)), E_SHARE, True),
       ("w2_short", dict(w2=torch.zeros(7)), E_W2, True),
       ("w2_long", dict(w2=torch.zeros(16)), E_W2, True),
       ("x_strided", dict(x=torch.zeros(2, 16, 3, dtype=torch.bfloat16).transpose(1, 2)), E_CONTIG, True),
       ("e_strided", dict(e=torch.zeros(2, 3, 16, dtype=torch.bfloat16)[:, :, ::2]), E_CONTIG, True),
       ("alpha_flat", dict(alpha=torch.zeros(6)), E_ALPHA, False),
       ("alpha_T", dict(alpha=torch.zeros(2, 4)), E_ALPHA, False),
       ("alpha_fp64", dict(alpha=torch.zeros(2, 3, dtype=torch.float64)), E_ALPHA, False),
       ("g_D", dict(g=torch.zeros(2, 8)), E_G, False),
       ("g_n", dict(g=torch.zeros(1, 16)), E_G, False),
       ("g_bf16", dict(g=torch.zeros(2, 16, dtype=torch.bfloat16)), E_G, False)]


def _calls(a, fwd=True):
    F = torch.ops.fedrec
    bwd = [lambda: F.additive_pool_bwd(a["x"], a["e"], a["alpha"], a["w2"], a["g"], dx) for dx in (False, True)]
    return ([lambda: F.additive_pool_fwd(a["x"], a["e"], a["w2"], a["b2"], None)] if fwd else []) + bwd


@pytest.mark.parametrize("name,change,msg,fwd", BAD, ids=[b[0] for b in BAD])
def test_argument_checks_raise_on_host_tensors_with_one_message(name, change, msg, fwd):
    """Mismatched sizes used to reach the kernels, which index x, e, w2, alpha and g by x's n, T, D
    and e's Q: an out-of-bounds read.  The checks run before the device check."""
    native.lib()
    a = dict(_host(), **change)
    errs = []
    for call in _calls(a, fwd):
        with pytest.raises(RuntimeError, match=msg) as e:
            call()
        errs.append(str(e.value).splitlines()[0].split(": ", 1)[1])
    assert len(set(errs)) == 1  # forward and backward word a rule alike


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_a_well_formed_host_tensor_fails_the_device_check(dtype):
    native.lib()
    for call in _calls(_host(dtype=dtype)):
        with pytest.raises(RuntimeError, match="must be device tensors"):
            call()
    with pytest.raises(RuntimeError, match="of one dtype, bf16 or fp32"):
        _calls(dict(_host(), e=torch.zeros(2, 3, 8)))[0]()
