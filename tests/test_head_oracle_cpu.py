"""The text-head oracle (tests/head_oracle.py) is right and sharp -- no GPU.

* anchor: its fp64 functions, chained, are torch autograd of the plain module math (the ``_oracle``
  of tests/test_text_head_gpu.py lifted to fp64): the forward and all four gradients to 1e-12;
* the recorded ``__expf`` error is what the fp32 transcription measures;
* a torch model of the kernels' roundings (fp32 with bf16 e and g, ``tanh_fast_f32``, the
  transcribed ``__expf``, fp32 sums in a shuffled order, per-split partials) stays inside every
  bound on every input set of tests/test_head_oracle_gpu.py (at NOMINAL_CUS);
* twelve mutants (a)-(l), (k) in both its forms -- each a named one-line change to the model --
  leave the bound of the family they break, two of them while passing the whole-tensor norms the
  suite judged this family by.

Run with ``-s`` for the worst ratio per family.
"""
import math

import pytest
import torch

import head_oracle as ho

BF = torch.bfloat16
CUS = ho.NOMINAL_CUS
WORST = {}


def _note(fam, ratio):
    WORST[fam] = max(WORST.get(fam, 0.0), ratio)
    return ratio


def _f(c):
    return torch.tensor(c, dtype=torch.float32)


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(20240229)  # the shuffles of ssum: the same orders in every run


def ssum(v, dim, gen=None):
    """An fp32 sum along ``dim`` in a shuffled order."""
    perm = torch.randperm(v.shape[dim], generator=gen)
    return v.index_select(dim, perm).sum(dim)


# ------------------------------------------------------------------------------------ the model
def model_score(x, w1, b1, w2, b2, mut=None, frag=None):
    """``(e bf16 [M, Q], a fp32 [M])`` of head_score2_kernel for the rows ``x`` bf16 [M, D]."""
    acc = x.float() @ w1.float().t()
    if mut == "b":  # one 64-wide k-tile missing from one 16 x 16 fragment of pre
        r0, q0, k0 = frag or ((x.shape[0] // 2) // 16 * 16, 32, 64)
        acc[r0:r0 + 16, q0:q0 + 16] -= x[r0:r0 + 16, k0:k0 + 64].float() @ w1[q0:q0 + 16, k0:k0 + 64].float().t()
    v = ho.tanh_fast_f32(acc + b1)
    e = v.to(BF)
    src = e.float() if mut == "a" else v  # (a): the score from the bf16-rounded e
    a = ssum(src * w2.reshape(1, -1), 1) + b2.reshape(())
    return e, a


def model_pool(x, a, keep=None, mut=None):
    """``(alpha fp32 [Un, T], pooled fp32 [Un, D])`` of head_pool2_kernel."""
    Un, T, D = x.shape
    a = a.view(Un, T)
    kp = torch.ones(Un, T, dtype=torch.bool) if keep is None else keep.clone()
    if mut == "d":  # a masked token keeps its weight
        kp[:, T // 2] = True
    am = a.masked_fill(~kp, -math.inf)
    m = am.amax(1, keepdim=True)
    m = torch.where(m > -math.inf, m, torch.zeros_like(m))
    p = torch.where(kp, ho.expf_f32(a - m), torch.zeros_like(a))
    eps = _f(1e-8) * (torch.ones_like(m) if mut == "c" else ho.expf_f32(-m))  # (c): without the e^-m factor
    inv = _f(1.0) / (ssum(p, 1).view(-1, 1) + eps)
    alpha = p * inv
    w = alpha
    if mut == "e" and T > 64:  # tokens t >= 64 take the weight of t - 64
        w = torch.cat([alpha[:, :64], alpha[:, : T - 64]], 1)
    pooled = ssum(w.unsqueeze(-1) * x.float(), 1)
    return alpha, pooled


def model_pool_bwd(x, alpha, g, mut=None):
    """``(da fp32 [Un, T], db2p fp32 [Un])`` of head_pool_bwd2 / 3."""
    dal = ssum(g.unsqueeze(1) * x.float(), 2)
    sm = ssum(alpha * dal, 1).view(-1, 1)
    da = alpha * dal if mut == "f" else alpha * (dal - sm)  # (f): the sum alpha dalpha term omitted
    return da, ssum(da, 1)


def model_g(da, e, T, mut=None):
    """``(g bf16 [M, Q], cs fp32 [2, titles, Q])`` of the rewrite in head_pool_bwd3."""
    f = e.float()
    dav = da.reshape(-1, 1)
    g = (dav * ((_f(1.0) - f) if mut == "g" else (_f(1.0) - f * f))).to(BF)  # (g): (1 - e) for (1 - e^2)
    Q = e.shape[1]
    cs0 = ssum((dav * f).view(-1, T, Q), 1)
    cs1 = ssum(g.float().view(-1, T, Q), 1)
    return g, torch.stack([cs0, cs1])


def _split_rows(mb, me, s, target, mut, seam):
    """The rows a split sums: (h) drops its part-filled last stage, (i) counts the ``seam`` rows in front of it twice."""
    if s == target and mut == "h":
        me = mb + (me - mb) // ho.WTM * ho.WTM
    if s == target and mut == "i":
        mb = max(0, mb - seam)
    return mb, me


def model_wgrad_g(x, G, cs, w2, db2p, T, R, S, tps, mut=None):
    """``dict(dW1, db1, dw2, db2)`` of head_wgrad_g_kernel + head_reduce_kernel: R real titles re-split over
    the S splits of ``tps`` whole titles, 32-row stages, the partials summed in fp32."""
    Un = x.shape[0] // T
    Ur, tp = ho.wgrad_g_resplit(Un, Un if mut == "j" else R, S, tps)  # (j): the padded titles contribute
    spans = [(min(Ur, s * tp), min(Ur, min(Ur, s * tp) + tp)) for s in range(S)]
    part = [s for s, (lo, hi) in enumerate(spans) if (hi - lo) * T % ho.WTM and lo > 0]
    target = part[len(part) // 2] if part else -1
    P, c0, c1 = [], [], []
    for s, (lo, hi) in enumerate(spans):
        mb, me = _split_rows(lo * T, hi * T, s, target, mut, T)
        P.append(G[mb:me].float().t() @ x[mb:me].float())
        c0.append(ssum(cs[0, lo:hi], 0))
        c1.append(ssum(cs[1, lo:hi], 0))
    w2 = w2.reshape(-1)
    db1 = ssum(torch.stack(c1), 0)
    return dict(dW1=ssum(torch.stack(P), 0) * w2.view(-1, 1), db1=db1 if mut == "k1" else db1 * w2,  # (k1): db1 omits w2
                dw2=ssum(torch.stack(c0), 0), db2=ssum(db2p.reshape(-1)[:Un], 0).reshape(1)), target


def model_wgrad(x, e, da, w2, db2p, T, R, S, mchunk, mut=None):
    """``dict(dW1, db1, dw2, db2)`` of head_wgrad_kernel + head_reduce_kernel: g formed per stage in bf16,
    the real rows re-split over S splits of ``mchunk`` rows (the seams fall inside titles)."""
    M = x.shape[0]
    Un = M // T
    Mr, mc = ho.wgrad_resplit(M, T, Un if mut == "j" else R, S, mchunk)
    spans = [(min(Mr, s * mc), min(Mr, s * mc + mc)) for s in range(S)]
    part = [s for s, (lo, hi) in enumerate(spans) if (hi - lo) % ho.WTM and lo > 0]
    target = part[len(part) // 2] if part else -1
    f = e.float()
    dav = da.reshape(-1, 1)
    g = (dav * (_f(1.0) - f * f)).to(BF).float()
    t = (dav * f).to(BF).float() if mut == "k2" else dav * f  # (k2): dw2 from bf16-rounded terms
    P, c0, c1 = [], [], []
    for s, (lo, hi) in enumerate(spans):
        mb, me = _split_rows(lo, hi, s, target, mut, ho.WTM)
        P.append(g[mb:me].t() @ x[mb:me].float())
        c0.append(ssum(t[mb:me], 0))
        c1.append(ssum(g[mb:me], 0))
    w2 = w2.reshape(-1)
    return dict(dW1=ssum(torch.stack(P), 0) * w2.view(-1, 1), db1=ssum(torch.stack(c1), 0) * w2,
                dw2=ssum(torch.stack(c0), 0), db2=ssum(db2p.reshape(-1)[:Un], 0).reshape(1)), target


def rel_err(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / (b.norm() + 1e-20))


# ------------------------------------------------------------------------------------ anchor
@pytest.mark.parametrize("T,masked", [(50, False), (50, True), (128, True)])
def test_oracle_chain_is_torch_autograd_in_fp64(T, masked):
    Un, D, Q = 21, 256, 384
    d = ho.make_inputs(Un, T, D, Q, "plain", masked, seed=3)
    x = ho.gather(d["table"], d["ids"], T)
    keep = ho.title_keep(d["keep"], d["ids"])
    params = [d["w1"].double().requires_grad_(True)] + [d[k].double().requires_grad_(True) for k in ("b1", "w2", "b2")]
    w1, b1, w2, b2 = params
    xd = x.double()
    e = torch.tanh(xd @ w1.t() + b1)
    a = e @ w2 + b2
    p = torch.exp(a) * keep
    alpha = p / (p.sum(1, keepdim=True) + 1e-8)
    pooled = torch.einsum("ut,utd->ud", alpha, xd)
    gw = torch.autograd.grad(pooled, params, d["gout"].double())

    def close(got, want):
        assert float((got.reshape(want.shape) - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))

    sc = ho.score_oracle(x.reshape(-1, D), d["w1"], d["b1"], d["w2"], d["b2"])
    close(sc["e"], e.detach().reshape(-1, Q))
    close(sc["a"], a.detach().reshape(-1))
    po = ho.pool_oracle(x, sc["a"], keep)
    close(po["alpha"], alpha.detach())
    close(po["pooled"], pooled.detach())
    pb = ho.pool_bwd_oracle(x, po["alpha"], d["gout"])
    go_ = ho.g_oracle(pb["da"], sc["e"], T)
    cs1, _ = ho.cs1_oracle(go_["g"], T)
    cs = torch.stack([go_["cs0"], cs1])
    for o in (ho.wgrad_g_oracle(x.reshape(-1, D), go_["g"], cs, d["w2"], pb["db2p"], T, Un, 1, Un),
              ho.wgrad_oracle(x.reshape(-1, D), sc["e"], pb["da"], d["w2"], pb["db2p"], T, Un, 1, Un * T)):
        for name, want in zip(("dW1", "db1", "dw2", "db2"), gw):
            close(o[name], want)
            assert bool((o["tol_" + name] > 0).all()) and bool(torch.isfinite(o["tol_" + name]).all())
    for o, names in ((sc, ("e", "a")), (po, ("alpha", "pooled")), (pb, ("da", "db2p")), (go_, ("g", "cs0"))):
        for n in names:
            assert bool((o["tol_" + n] > 0).all()) and bool(torch.isfinite(o["tol_" + n]).all())
    if masked:  # the all-masked title: exact zeros
        z = (~keep.any(1)).nonzero().reshape(-1)
        assert z.numel() > 0 and float(po["alpha"][z].abs().max()) == 0.0 and float(po["pooled"][z].abs().max()) == 0.0


def test_recorded_expf_eps_is_what_the_transcription_measures():
    got = ho.measure_expf_eps()
    print("__expf relative error over max(1, |x|), measured: %.4g" % got)
    rec = ho.EPS_MEASURED["expf"]
    assert 0.9 * rec <= got <= 1.05 * rec, (got, rec)
    assert ho.EPS["expf"] == ho.ACT_MARGIN * rec and ho.EPS["tanh_fast"] == ho.go.EPS["tanh_fast"]
    # the edges: e^-m overflows past 88.72 (the kernel's alpha = 0 there); below 2^-126 the values are inside TINY
    assert float(ho.expf_f32(_f(88.0))) < math.inf and float(ho.expf_f32(_f(89.0))) == math.inf
    assert math.exp(-88.72) / 1e-8 < ho.TINY and float(ho.expf_f32(_f(-104.0))) == 0.0


def test_shifted_scores_do_what_they_claim():
    """The eps titles: sum alpha strictly between 0.2 and 0.9 (the eps term carries about half of the
    denominator); high: the eps term vanishes; low: alpha about 0, below the absolute floor."""
    for T, masked in ((50, False), (128, True), (1, False)):
        d = ho.make_inputs(40, T, 256, 384, "plain", masked)
        x = ho.gather(d["table"], d["ids"], T)
        keep = ho.title_keep(d["keep"], d["ids"])
        _, a = model_score(x.reshape(-1, 256), d["w1"], d["b1"], d["w2"], d["b2"])
        sa = ho.shift_scores(a.view(40, T), keep)
        po = ho.pool_oracle(x, sa, keep)
        tot = po["alpha"].sum(1)
        live = keep.any(1)
        cls = torch.arange(40) % 4
        assert int((live & (cls == 0)).sum()) >= 5
        s0 = tot[live & (cls == 0)]
        assert bool((s0 > 0.2).all()) and bool((s0 < 0.9).all()), s0
        top = sa.masked_fill(~keep, -math.inf).amax(1)[live & (cls == 0)]  # sum exp(a) = 1e-8: the largest score near -20
        assert bool(((top >= math.log(1e-8 / T) - 1e-3) & (top <= math.log(1e-8) + 1e-3)).all()), top
        assert bool((tot[live & (cls == 1)] > 1 - 1e-12).all())
        assert bool((po["alpha"][cls == 2] < ho.TINY).all())
        assert float(tot[~live].abs().max() if bool((~live).any()) else 0.0) == 0.0


# ------------------------------------------------------------------------------------ the model stays inside
def _uniq(cases, key):
    seen, out = set(), []
    for c in cases:
        if key(c) not in seen:
            seen.add(key(c))
            out.append(c)
    return out


def _rows_subset(M, n=400):
    return None if M <= 2 * n else torch.cat([torch.arange(n), torch.arange(M - n, M)])


def test_rounding_model_stays_inside_the_score_bounds():
    sets = _uniq(ho.score_cases(CUS), lambda c: c[:5])
    for Un, T, D, Q, kind, _, _ in sets:
        d = ho.make_inputs(Un, T, D, Q, kind, gout=False)
        x = ho.gather(d["table"], d["ids"], T).reshape(-1, D)
        idx = _rows_subset(x.shape[0])  # the walk: a row's roundings do not depend on the row count
        x = x if idx is None else x[idx]
        o = ho.score_oracle(x, d["w1"], d["b1"], d["w2"], d["b2"])
        e, a = model_score(x, d["w1"], d["b1"], d["w2"], d["b2"])
        what = "model score %s" % ((Un, T, D, Q, kind),)
        _note("score e", ho.check(e, o["e"], o["tol_e"], what + " e", T))
        _note("score a", ho.check(a, o["a"], o["tol_a"], what + " a", T))
    print("score input sets: %d; worst model ratio: e %.3f, a %.4f" % (len(sets), WORST["score e"], WORST["score a"]))
    assert WORST["score e"] > 0.8  # the bound on e is the bf16 rounding, not a multiple of it


def _pool_inputs(Un, T, D, kind, masked):
    d = ho.make_inputs(Un, T, D, 384, "plain" if kind == "shifted" else kind, masked)
    x = ho.gather(d["table"], d["ids"], T)
    keep = ho.title_keep(d["keep"], d["ids"])
    e, a = model_score(x.reshape(-1, D), d["w1"], d["b1"], d["w2"], d["b2"])
    a = a.view(Un, T)
    if kind == "shifted":
        a = ho.shift_scores(a, keep)
    return d, x, keep, e, a


def test_rounding_model_stays_inside_the_pool_bounds():
    sets = _uniq(ho.pool_cases(), lambda c: c[:5])
    for Un, T, D, kind, masked, _ in sets:
        d, x, keep, _, a = _pool_inputs(Un, T, D, kind, masked)
        o = ho.pool_oracle(x, a, keep)
        alpha, pooled = model_pool(x, a, keep)
        what = "model pool %s" % ((Un, T, D, kind, masked),)
        _note("alpha", ho.check(alpha, o["alpha"], o["tol_alpha"], what + " alpha"))
        _note("pooled", ho.check(pooled, o["pooled"], o["tol_pooled"], what + " pooled"))
        dead = ~keep.any(1)
        if bool(dead.any()):
            assert float(alpha[dead].abs().max()) == 0.0 and float(pooled[dead].abs().max()) == 0.0
    print("pool input sets: %d; worst model ratio: alpha %.3f, pooled %.3f" % (len(sets), WORST["alpha"], WORST["pooled"]))


def test_rounding_model_stays_inside_the_pool_backward_bounds():
    sets = _uniq(ho.pool_bwd_cases(), lambda c: c[:4])
    for Un, T, D, kind, _ in sets:
        d, x, keep, e, a = _pool_inputs(Un, T, D, kind, False)
        alpha, _ = model_pool(x, a, None)
        o = ho.pool_bwd_oracle(x, alpha, d["gout"])
        da, db2p = model_pool_bwd(x, alpha, d["gout"])
        what = "model pool_bwd %s" % ((Un, T, D, kind),)
        _note("da", ho.check(da, o["da"], o["tol_da"], what + " da"))
        _note("db2p", ho.check(db2p, o["db2p"], o["tol_db2p"], what + " db2p"))
        og = ho.g_oracle(da.reshape(-1), e, T)
        g, cs = model_g(da, e, T)
        _note("g", ho.check(g, og["g"], og["tol_g"], what + " g", T))
        _note("cs", ho.check(cs[0], og["cs0"], og["tol_cs0"], what + " cs0"))
        _note("cs", ho.check(cs[1], *ho.cs1_oracle(g, T), what + " cs1"))
    print("pool backward input sets: %d; worst model ratio: %s"
          % (len(sets), {k: "%.4f" % WORST[k] for k in ("da", "db2p", "g", "cs")}))


KS, QS = 32, 16  # the column / row slice of dW1 the model and the oracle run on for the large sets


def _check_grads(fam, m, o, what):
    for n in ("dW1", "db1", "dw2", "db2"):
        _note("%s %s" % (fam, n), ho.check(m[n], o[n], o["tol_" + n], "%s %s" % (what, n)))


def test_rounding_model_stays_inside_the_wgrad_g_bounds():
    sets = _uniq(ho.wgrad_g_cases(CUS), lambda c: c)
    for Un, T, D, nreal in sets:
        d = ho.make_wgrad_g_inputs(Un, T, D, nreal)
        big = Un * T > 20000
        tab = d["table"][:, :KS].contiguous() if big else d["table"]  # (an element's roundings do not depend on the other columns)
        x = ho.gather(tab, d["ids"], T).reshape(Un * T, -1)
        S, tps = ho.wgrad_g_split(Un, D, CUS)
        R = Un if nreal is None else nreal
        o = ho.wgrad_g_oracle(x, d["G"], d["cs"], d["w2"], d["db2p"], T, R, S, tps)
        m, _ = model_wgrad_g(x, d["G"], d["cs"], d["w2"], d["db2p"], T, R, S, tps)
        _check_grads("wgrad_g", m, o, "model wgrad_g %s" % ((Un, T, D, nreal),))
        if nreal == 0:
            assert all(float(m[n].abs().max()) == 0.0 for n in ("dW1", "db1", "dw2", "db2"))
        if tps == ho.MAX_SPLIT_TITLES - 2:
            _note("wgrad_g cap", max(ho.worst_ratio(m[n], o[n], o["tol_" + n]) for n in ("dW1", "db1", "dw2")))
    assert "wgrad_g cap" in WORST
    print("wgrad_g input sets: %d; worst model ratio: %s"
          % (len(sets), {k: "%.4f" % v for k, v in sorted(WORST.items()) if k.startswith("wgrad_g")}))


def test_rounding_model_stays_inside_the_wgrad_bounds():
    sets = _uniq(ho.wgrad_cases(CUS), lambda c: c)
    clamped = 0
    for Un, T, D, Q, nreal in sets:
        d = ho.make_wgrad_inputs(Un, T, D, Q, nreal)
        big = Un * T > 20000
        tab = d["table"][:, :KS].contiguous() if big else d["table"]
        x = ho.gather(tab, d["ids"], T).reshape(Un * T, -1)
        e, w2 = (d["e"][:, :QS].contiguous(), d["w2"][:QS]) if big else (d["e"], d["w2"])
        S, mchunk = ho.wgrad_split(Un * T, T, D, Q, CUS)
        clamped += S > CUS
        R = Un if nreal is None else nreal
        o = ho.wgrad_oracle(x, e, d["da"], w2, d["db2p"], T, R, S, mchunk)
        m, _ = model_wgrad(x, e, d["da"], w2, d["db2p"], T, R, S, mchunk)
        _check_grads("wgrad", m, o, "model wgrad %s" % ((Un, T, D, Q, nreal),))
        if nreal == 0:
            assert all(float(m[n].abs().max()) == 0.0 for n in ("dW1", "db1", "dw2", "db2"))
    assert clamped == 2  # the T = 1 and T = 3 clamp cases do clamp
    print("wgrad input sets: %d; worst model ratio: %s"
          % (len(sets), {k: "%.4f" % v for k, v in sorted(WORST.items()) if k.startswith("wgrad ")}))


# ------------------------------------------------------------------------------------ mutants
MUTANTS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if MUTANTS:
        print("\nmutant ratios: %s" % {k: "%.4g" % v for k, v in sorted(MUTANTS.items())})


def _mutant(name, ratio, clean):
    MUTANTS[name] = ratio
    assert clean <= 1.0, (name, "the unmutated model", clean)
    assert ratio > 1.0, (name, ratio)


def test_score_mutants_leave_the_bound():
    Un, T, D, Q = 9, 50, 768, 384
    d = ho.make_inputs(Un, T, D, Q)
    x = ho.gather(d["table"], d["ids"], T).reshape(-1, D)
    args = (d["w1"], d["b1"], d["w2"], d["b2"])
    o = ho.score_oracle(x, *args)
    e, a = model_score(x, *args)
    clean = max(ho.worst_ratio(e, o["e"], o["tol_e"]), ho.worst_ratio(a, o["a"], o["tol_a"]))
    da_ = ho.make_inputs(Un, T, 256, Q, "aligned")  # the smallest accumulation term, the roundings of row 0 aligned
    xa = ho.gather(da_["table"], da_["ids"], T).reshape(-1, 256)
    aargs = (da_["w1"], da_["b1"], da_["w2"], da_["b2"])
    oa = ho.score_oracle(xa, *aargs)
    ea, a0 = model_score(xa, *aargs)
    ea2, aa = model_score(xa, *aargs, mut="a")
    assert torch.equal(ea, ea2)
    # (with random signs the same change stays inside: the accumulation term of the bound hides it)
    MUTANTS["(a) on the plain set, random signs (stays inside)"] = ho.worst_ratio(model_score(x, *args, mut="a")[1], o["a"], o["tol_a"])
    _mutant("(a) score from the bf16 e: a", ho.worst_ratio(aa, oa["a"], oa["tol_a"]),
            max(clean, ho.worst_ratio(a0, oa["a"], oa["tol_a"]), ho.worst_ratio(ea, oa["e"], oa["tol_e"])))
    eb, ab = model_score(x, *args, mut="b")
    _mutant("(b) lost k-tile of one fragment: e", ho.worst_ratio(eb, o["e"], o["tol_e"]), clean)
    _mutant("(b) lost k-tile of one fragment: a", ho.worst_ratio(ab, o["a"], o["tol_a"]), clean)
    xl = ho.gather(d["table"], torch.roll(d["ids"], -1), T).reshape(-1, D)  # (l): rows gathered from ids[u + 1]
    el, al = model_score(xl, *args)
    _mutant("(l) row from ids[u + 1]: e", ho.worst_ratio(el, o["e"], o["tol_e"]), clean)
    _mutant("(l) row from ids[u + 1]: a", ho.worst_ratio(al, o["a"], o["tol_a"]), clean)


def test_pool_mutants_leave_the_bound():
    for mut, name, (Un, T, D, kind, masked), fams in (
            ("c", "(c) 1e-8 without e^-m", (40, 50, 768, "shifted", False), ("alpha", "pooled")),
            ("d", "(d) a masked token keeps its weight", (40, 50, 768, "plain", True), ("alpha", "pooled")),
            ("e", "(e) t >= 64 takes the weight of t - 64", (40, 128, 768, "plain", True), ("pooled",))):
        d, x, keep, _, a = _pool_inputs(Un, T, D, kind, masked)
        o = ho.pool_oracle(x, a, keep)
        res = dict(zip(("alpha", "pooled"), model_pool(x, a, keep)))
        clean = max(ho.worst_ratio(res[n], o[n], o["tol_" + n]) for n in ("alpha", "pooled"))
        mres = dict(zip(("alpha", "pooled"), model_pool(x, a, keep, mut=mut)))
        for n in fams:
            _mutant("%s: %s" % (name, n), ho.worst_ratio(mres[n], o[n], o["tol_" + n]), clean)


def test_pool_backward_mutants_leave_the_bound():
    Un, T, D = 24, 50, 768
    d, x, keep, e, a = _pool_inputs(Un, T, D, "plain", False)
    alpha, _ = model_pool(x, a, None)
    o = ho.pool_bwd_oracle(x, alpha, d["gout"])
    da, db2p = model_pool_bwd(x, alpha, d["gout"])
    clean = max(ho.worst_ratio(da, o["da"], o["tol_da"]), ho.worst_ratio(db2p, o["db2p"], o["tol_db2p"]))
    daf, dbf = model_pool_bwd(x, alpha, d["gout"], mut="f")
    _mutant("(f) da without sum alpha dalpha: da", ho.worst_ratio(daf, o["da"], o["tol_da"]), clean)
    _mutant("(f) da without sum alpha dalpha: db2p", ho.worst_ratio(dbf, o["db2p"], o["tol_db2p"]), clean)
    og = ho.g_oracle(da.reshape(-1), e, T)
    g, cs = model_g(da, e, T)
    clean = max(ho.worst_ratio(g, og["g"], og["tol_g"]), ho.worst_ratio(cs[0], og["cs0"], og["tol_cs0"]))
    gg, _ = model_g(da, e, T, mut="g")
    _mutant("(g) (1 - e) for (1 - e^2): g", ho.worst_ratio(gg, og["g"], og["tol_g"]), clean)
    # the one-ulp allowance of tests/test_text_head_gpu.py stays; this bound is inside it
    assert bool((og["tol_g"] <= og["g"].abs() * 2.0 ** -7 + ho.TINY).all())


def _wgrad_g_set(Un, T, D, nreal):
    d = ho.make_wgrad_g_inputs(Un, T, D, nreal)
    x = ho.gather(d["table"], d["ids"], T).reshape(Un * T, -1)
    S, tps = ho.wgrad_g_split(Un, D, CUS)
    return d, x, S, tps


def test_wgrad_g_mutants_leave_the_bound():
    Un, T, D, nreal = 2 * (CUS // 6) + 40, 50, 768, 2 * (CUS // 6) + 3
    d, x, S, tps = _wgrad_g_set(Un, T, D, nreal)
    args = (x, d["G"], d["cs"], d["w2"], d["db2p"], T, nreal, S, tps)
    o = ho.wgrad_g_oracle(*args)
    m, target = model_wgrad_g(*args)
    assert target > 0  # a split with a part-filled last stage exists
    clean = max(ho.worst_ratio(m[n], o[n], o["tol_" + n]) for n in ("dW1", "db1", "dw2", "db2"))
    for mut, name, fams in (("h", "(h) part-filled last stage dropped", ("dW1",)),
                            ("i", "(i) seam title counted twice", ("dW1",)),
                            ("j", "(j) padded titles contribute", ("dW1", "db1", "dw2")),
                            ("k1", "(k) db1 without w2", ("db1",))):
        mm, _ = model_wgrad_g(*args, mut=mut)
        for n in fams:
            _mutant("%s: wgrad_g %s" % (name, n), ho.worst_ratio(mm[n], o[n], o["tol_" + n]), clean)


def test_wgrad_mutants_leave_the_bound():
    Un, T, D, Q, nreal = 120, 50, 256, 128, 83
    d = ho.make_wgrad_inputs(Un, T, D, Q, nreal)
    x = ho.gather(d["table"], d["ids"], T).reshape(Un * T, -1)
    S, mchunk = ho.wgrad_split(Un * T, T, D, Q, CUS)
    args = (x, d["e"], d["da"], d["w2"], d["db2p"], T, nreal, S, mchunk)
    o = ho.wgrad_oracle(*args)
    m, target = model_wgrad(*args)
    assert target > 0
    clean = max(ho.worst_ratio(m[n], o[n], o["tol_" + n]) for n in ("dW1", "db1", "dw2", "db2"))
    for mut, name, fams in (("h", "(h) part-filled last stage dropped", ("dW1", "dw2")),
                            ("i", "(i) seam stage counted twice", ("dW1", "dw2")),
                            ("j", "(j) padded titles contribute", ("dW1", "db1", "dw2")),
                            ("k2", "(k) dw2 from bf16-rounded terms", ("dw2",))):
        mm, _ = model_wgrad(*args, mut=mut)
        for n in fams:
            _mutant("%s: wgrad %s" % (name, n), ho.worst_ratio(mm[n], o[n], o["tol_" + n]), clean)


# ------------------------------------------------------------------------------------ what the norms miss
def test_norm_tolerances_miss_what_the_oracle_catches():
    """At the shape of tests/test_text_head_gpu.py (1577 titles of 50 tokens, D = 768, Q = 384): mutant
    (b) moves ``pooled`` by less than its ``_rel < 2e-3`` and mutant (h) moves dW1 by less than its
    ``_rel < 3e-2``; the oracle sees (b) at 364 bounds on e and (h) -- 12 rows of 78,850 -- at 3.0 on dW1,
    where the per-split count of the bound is what makes the difference (the count over the whole
    sum would put it at 0.07)."""
    Un, T, D, Q = 1577, 50, 768, 384
    d = ho.make_inputs(Un, T, D, Q, gout=False)
    args = (d["w1"], d["b1"], d["w2"], d["b2"])
    tx = d["table"].view(-1, T, D)  # the distinct titles: the model once per table title
    _, a_t = model_score(tx.reshape(-1, D), *args)
    _, pooled_t = model_pool(tx, a_t.view(-1, T))
    ref = pooled_t[d["ids"].long()]  # [Un, D]: the clean fp32 pooled rows
    x = ho.gather(d["table"], d["ids"], T).reshape(-1, D)
    r0 = (Un * T // 2) // 16 * 16  # the mutated fragment's rows, as model_score picks them
    us = sorted({r0 // T, (r0 + 15) // T})
    rows = torch.cat([torch.arange(u * T, (u + 1) * T) for u in us])
    xs = x[rows]
    ce, ca = model_score(xs, *args)
    em, am = model_score(xs, *args, mut="b", frag=(r0 - us[0] * T, 32, 64))
    _, pooled_m = model_pool(xs.view(len(us), T, D), am.view(len(us), T))
    mut = ref.clone()
    mut[us] = pooled_m
    norm_b = rel_err(mut, ref)
    o = ho.score_oracle(xs, *args)
    ratio_e = ho.worst_ratio(em, o["e"], o["tol_e"])
    ratio_a = ho.worst_ratio(am, o["a"], o["tol_a"])
    assert ho.worst_ratio(ce, o["e"], o["tol_e"]) <= 1.0 and ho.worst_ratio(ca, o["a"], o["tol_a"]) <= 1.0
    print("(b) at 1577 x 50: pooled _rel %.3g (< 2e-3 passes); oracle ratio e %.4g, a %.4g" % (norm_b, ratio_e, ratio_a))
    assert norm_b < 2e-3 and ratio_e > 1.0 and ratio_a > 1.0
    # (h) on the G path's weight gradient
    dg, xg, S, tps = _wgrad_g_set(Un, T, D, None)
    gargs = (xg, dg["G"], dg["cs"], dg["w2"], dg["db2p"], T, Un, S, tps)
    clean, target = model_wgrad_g(*gargs)
    mh, _ = model_wgrad_g(*gargs, mut="h")
    norm_h = rel_err(mh["dW1"], clean["dW1"])
    og = ho.wgrad_g_oracle(xg[:, :KS].contiguous(), dg["G"], dg["cs"], dg["w2"], dg["db2p"], T, Un, S, tps)
    ratio_h = ho.worst_ratio(mh["dW1"][:, :KS], og["dW1"], og["tol_dW1"])
    assert ho.worst_ratio(clean["dW1"][:, :KS], og["dW1"], og["tol_dW1"]) <= 1.0
    print("(h) at 1577 x 50: dW1 _rel %.3g (< 3e-2 passes); oracle ratio %.4g" % (norm_h, ratio_h))
    assert target > 0 and 0 < norm_h < 3e-2 and ratio_h > 1.0
    MUTANTS["(b) at 1577 x 50, pooled _rel"] = norm_b
    MUTANTS["(b) at 1577 x 50, oracle e"] = ratio_e
    MUTANTS["(h) at 1577 x 50, dW1 _rel"] = norm_h
    MUTANTS["(h) at 1577 x 50, oracle dW1"] = ratio_h
