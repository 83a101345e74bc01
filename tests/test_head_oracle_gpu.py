"""Every launch family of the fused text head (csrc/text_head.hip) on the per-element fp64 oracle of
tests/head_oracle.py: ``head_score``, ``head_pool``, ``head_pool_bwd`` / ``head_pool_bwd_g`` (da, db2p, the
g rewrite and its column partials), ``head_wgrad_g`` and the round-4 ``head_wgrad``.

A case passes when EVERY output element is within its counted bound (``ratio <= 1``); a failure names
the worst element's title slot, token, stage and fragment.  Each stage is judged on the exact
tensors its kernel received -- where those are a previous kernel's output, that kernel's actual
output.  The shapes are the smallest at which each mechanism can go wrong, sized from the launch
rules (the CU count is read from the device, as the launchers do): row counts around every row
tile, titles that straddle tile, stage and split seams, every template dispatch of the pools,
splits around the split count, the clamped splits, padded titles (nreal) and a table of 37 titles
read through ids with duplicates.  Run with ``-s`` for the worst ratio per family.
"""
import functools

import pytest
import torch

import head_oracle as ho
from fedrec_with_pytorchdistributed_amd.ops import native

pytestmark = pytest.mark.gpu

WORST = {}
COUNT = [0]


def _note(fam: str, ratio: float) -> None:
    WORST[fam] = max(WORST.get(fam, 0.0), ratio)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\n%d cases; worst observed / bound per family: %s" % (COUNT[0], {k: "%.4f" % v for k, v in sorted(WORST.items())}))


@functools.lru_cache(maxsize=None)
def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else ho.NOMINAL_CUS


def _nreal(r):
    return None if r is None else torch.tensor([r], dtype=torch.int32, device="cuda")


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


@functools.lru_cache(maxsize=2)
def _score_set(Un, T, D, Q, kind):
    """Inputs, gathered rows and score oracle of an input set, on the device (the last two are kept)."""
    d = ho.make_inputs(Un, T, D, Q, kind, device="cuda", gout=False)
    x = ho.gather(d["table"], d["ids"], T).reshape(-1, D)
    return d, ho.score_oracle(x, d["w1"], d["b1"], d["w2"], d["b2"])


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def _params(cases):
    return pytest.mark.parametrize("case", cases, ids=_ids(cases))


@_params(sorted(ho.score_cases(_cus()), key=lambda c: (c[:4], c[4])))
def test_score(dev, case):
    """e and the score a, every row of the real titles (rows of padded titles, m >= nreal T, are left
    unwritten by contract and not judged)."""
    Un, T, D, Q, kind, forced, nreal = case
    d, o = _score_set(Un, T, D, Q, kind)
    lib = native.lib()
    try:
        lib.head_score_set_rows(forced)
        e, a = lib.head_score(d["table"], d["ids"], T, d["w1"], d["b1"], d["w2"], d["b2"], True, _nreal(nreal))
        torch.cuda.synchronize()
    finally:
        lib.head_score_set_rows(0)
    assert e.shape == (Un * T, Q) and e.dtype == torch.bfloat16 and a.shape == (Un * T,) and a.dtype == torch.float32
    n = (Un if nreal is None else nreal) * T
    tile = ho.score_tile(Un * T, T, Q, _cus(), forced, nreal is not None)
    walk = Un * T > _cus() * 160
    _note("walk e" if walk else "score e", ho.check(e[:n], o["e"][:n], o["tol_e"][:n], "e %s" % (case,), T, tile))
    _note("walk a" if walk else "score a", ho.check(a[:n], o["a"][:n], o["tol_a"][:n], "a %s" % (case,), T, tile))
    COUNT[0] += 1


def _scores(d, T, nreal=None):
    """(e, a) of the set from head_score itself: what the later stages consume."""
    return native.lib().head_score(d["table"], d["ids"], T, d["w1"], d["b1"], d["w2"], d["b2"], True, _nreal(nreal))


@_params(ho.pool_cases())
def test_pool(dev, case):
    """alpha and pooled on the scores head_score wrote (the shifted sets: moved per title so that the
    1e-8 term carries half of the denominator, vanishes, or meets the overflow edge); all-masked and
    padded titles are exact zeros; pooled_b is the bf16 rounding of pooled."""
    Un, T, D, kind, masked, nreal = case
    d = ho.make_inputs(Un, T, D, 384, "plain" if kind == "shifted" else kind, masked, device="cuda")
    x = ho.gather(d["table"], d["ids"], T)
    keep = ho.title_keep(d["keep"], d["ids"])
    _, a = _scores(d, T)
    a = a.view(Un, T)
    if kind == "shifted":
        a = ho.shift_scores(a, keep)
    pooled, alpha, pb = native.lib().head_pool(d["table"], d["ids"], T, a.reshape(-1), d["tokens"], _nreal(nreal), True)
    torch.cuda.synchronize()
    assert pooled.shape == (Un, D) and alpha.shape == (Un, T) and pb.shape == (Un, D)
    R = Un if nreal is None else nreal
    o = ho.pool_oracle(x[:R], a[:R], keep[:R])
    _note("alpha", ho.check(alpha[:R], o["alpha"], o["tol_alpha"], "alpha %s" % (case,)))
    _note("pooled", ho.check(pooled[:R], o["pooled"], o["tol_pooled"], "pooled %s" % (case,)))
    assert torch.equal(_bits(pb), _bits(pooled.to(torch.bfloat16)))
    dead = ~keep[:R].any(1)
    if bool(dead.any()):
        assert float(alpha[:R][dead].abs().max()) == 0.0 and float(pooled[:R][dead].abs().max()) == 0.0
    if R < Un:
        assert float(alpha[R:].abs().max()) == 0.0 and float(pooled[R:].abs().max()) == 0.0
        assert float(pb[R:].float().abs().max()) == 0.0
    COUNT[0] += 1


@_params(ho.pool_bwd_cases())
def test_pool_backward_and_g_rewrite(dev, case):
    """da / db2p of both launches (bitwise equal to each other) on the alpha head_pool wrote; the G path's
    g = bf16(da (1 - e^2)) from its own da and the e head_score wrote, cs[0] = sum da e and cs[1] = the
    sum of the stored g; padded titles: zeros, their e rows untouched."""
    Un, T, D, kind, nreal = case
    d = ho.make_inputs(Un, T, D, 384, kind, device="cuda")
    lib = native.lib()
    nr = _nreal(nreal)
    e, a = _scores(d, T, nreal)
    _, alpha, _ = lib.head_pool(d["table"], d["ids"], T, a, None, nr, False)
    da, db2p = lib.head_pool_bwd(d["table"], d["ids"], T, alpha, d["gout"], nr)
    eg = e.clone()
    da_g, db2p_g, cs = lib.head_pool_bwd_g(d["table"], d["ids"], T, alpha, d["gout"], eg, nr)
    torch.cuda.synchronize()
    assert torch.equal(_bits(da_g), _bits(da)) and torch.equal(_bits(db2p_g), _bits(db2p))
    R = Un if nreal is None else nreal
    n = R * T
    x = ho.gather(d["table"], d["ids"], T)
    o = ho.pool_bwd_oracle(x[:R], alpha[:R], d["gout"][:R])
    _note("da", ho.check(da[:n], o["da"], o["tol_da"], "da %s" % (case,)))
    _note("db2p", ho.check(db2p[:R], o["db2p"], o["tol_db2p"], "db2p %s" % (case,)))
    og = ho.g_oracle(da[:n], e[:n], T)
    _note("g", ho.check(eg[:n], og["g"], og["tol_g"], "g %s" % (case,), T))
    _note("cs", ho.check(cs[0, :R], og["cs0"], og["tol_cs0"], "cs[0] %s" % (case,)))
    _note("cs", ho.check(cs[1, :R], *ho.cs1_oracle(eg[:n], T), "cs[1] %s" % (case,)))
    if R < Un:
        assert float(da[n:].abs().max()) == 0.0 and float(db2p[R:Un].abs().max()) == 0.0
        assert float(cs[:, R:].abs().max()) == 0.0 and torch.equal(_bits(eg[n:]), _bits(e[n:]))
    COUNT[0] += 1


def _grads(fam, got, o, case):
    for name, t in zip(("dW1", "db1", "dw2", "db2"), got):
        assert t.dtype == torch.float32
        _note("%s %s" % (fam, name), ho.check(t, o[name], o["tol_" + name], "%s %s %s" % (fam, name, case)))
    COUNT[0] += 1


@_params(ho.wgrad_g_cases(_cus()))
def test_wgrad_g(dev, case):
    """head_wgrad_g on G / cs / db2p drawn directly (nonzero in the rows of padded titles, which must add
    nothing): title counts around the split count, titles shorter and longer than the 32-row stage,
    the clamped split (tps = MAX_SPLIT_TITLES - 2); nreal = 0: every gradient exactly zero."""
    Un, T, D, nreal = case
    d = ho.make_wgrad_g_inputs(Un, T, D, nreal, device="cuda")
    got = native.lib().head_wgrad_g(d["table"], d["ids"], T, d["G"], d["cs"], d["w2"], d["db2p"], _nreal(nreal))
    torch.cuda.synchronize()
    S, tps = ho.wgrad_g_split(Un, D, _cus())
    x = ho.gather(d["table"], d["ids"], T).reshape(Un * T, D)
    o = ho.wgrad_g_oracle(x, d["G"], d["cs"], d["w2"], d["db2p"], T, Un if nreal is None else nreal, S, tps)
    _grads("wgrad_g cap" if tps == ho.MAX_SPLIT_TITLES - 2 else "wgrad_g", got, o, case)
    if nreal == 0:
        assert all(float(t.abs().max()) == 0.0 for t in got)


@_params(ho.wgrad_cases(_cus()))
def test_wgrad_round4(dev, case):
    """The round-4 head_wgrad (g formed in its LDS pipeline) on e / da / db2p drawn directly: one split, row
    counts that are no multiple of the stage, seams inside titles, the ``mchunk > cap`` clamp, nreal."""
    Un, T, D, Q, nreal = case
    d = ho.make_wgrad_inputs(Un, T, D, Q, nreal, device="cuda")
    got = native.lib().head_wgrad(d["table"], d["ids"], T, d["e"], d["da"], d["w2"], d["db2p"], _nreal(nreal))
    torch.cuda.synchronize()
    S, mchunk = ho.wgrad_split(Un * T, T, D, Q, _cus())
    x = ho.gather(d["table"], d["ids"], T).reshape(Un * T, D)
    o = ho.wgrad_oracle(x, d["e"], d["da"], d["w2"], d["db2p"], T, Un if nreal is None else nreal, S, mchunk)
    _grads("wgrad clamp" if S > _cus() else "wgrad", got, o, case)
    if nreal == 0:
        assert all(float(t.abs().max()) == 0.0 for t in got)
