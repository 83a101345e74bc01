"""The LayerNorm / gradient-reduction oracle (``tests/norm_oracle.py``) checked without a GPU:

* its explicit fp64 intermediates equal fp64 autograd through ``ops.reference`` /
  ``F.layer_norm`` / ``F.gelu`` to 1e-12;
* a rounding model of each kernel -- torch on the CPU in fp32 in the kernel's order of operations
  (two-pass statistics summed per lane and then by the butterfly, dw / db per lane stride, then
  over the 4 waves, then over the blocks; the chunked two-pass column sums; embedding rows summed
  in occurrence order; Abramowitz-Stegun erf; bf16 rounding where the kernel rounds) -- stays
  inside the bound on every shared input set of the GPU tests (the worst ratio per family is
  printed; ``-rP`` shows them);
* mutants of the model -- the mistakes the bound is there to catch -- each push some ratio above
  1 on those same inputs;
* the approximation constants of the GELU forms are measured again and hold the record."""
import math

import pytest
import torch
import torch.nn.functional as F

import gemm_oracle as go
import norm_oracle as no
from fedrec_with_pytorchdistributed_amd.ops import reference as ref

BF = torch.bfloat16
CUS = no.NOMINAL_CUS
EPSF = torch.tensor(no.LN_EPS, dtype=torch.float32)


def bf(x):
    return x.to(BF).float()


def report(family, worst):
    print("norm-oracle model ratio %-28s %.3f" % (family, worst))


# ------------------------------------------------------------------------------ rounding models
def lane_sum(t, lanes: int, width: int):
    """[rows, D] fp32 -> [rows, 1]: lane l owns ``width`` consecutive elements of every 256-element
    chunk and adds them in order (masked elements add 0), then the xor butterfly over the lanes."""
    rows, D = t.shape
    per = lanes * width
    nc = (D + per - 1) // per
    tp = F.pad(t, (0, nc * per - D)).view(rows, nc, lanes, width)
    s = torch.zeros(rows, lanes)
    for c in range(nc):
        for k in range(width):
            s = s + tp[:, c, :, k]
    o = lanes // 2
    while o >= 1:
        s = s[:, :o] + s[:, o:2 * o]
        o //= 2
    return s


def model_stats(v, wide_form: bool, mut=""):
    D = v.shape[1]
    lanes, width = (32, 8) if wide_form else (64, 4)
    Df = torch.tensor(float(D))
    inv = torch.tensor(1.0) / Df

    def mean_of(t):
        s = lane_sum(t, lanes, width)
        return s * inv if wide_form else s / Df

    mean = mean_of(v)
    d = v - mean
    if mut == "onepass":  # mutant: E[v^2] - mean^2
        var = mean_of(v * v) - mean * mean
    elif mut == "unbiased":  # mutant: D - 1
        var = lane_sum(d * d, lanes, width) / (Df - 1.0)
    else:
        var = mean_of(d * d)
    if mut == "eps_outside":  # mutant: eps outside the sqrt
        rstd = 1.0 / (torch.sqrt(var) + EPSF)
    else:
        rstd = 1.0 / torch.sqrt(var + EPSF)
    return d, rstd


def model_ln(x, w, b, r=None, wide: int = 0, mut=""):
    """-> bf16 [rows, D], the forward kernels' arithmetic (ln_kernel, ln16_kernel, ln16p_kernel)."""
    v = x.float()
    if r is not None:
        v = v + r.float()
        if mut == "res_bf16":  # mutant: the residual sum rounded to bf16 before the statistics
            v = bf(v)
    d, rstd = model_stats(v, wide >= 1 and x.shape[1] % 256 == 0, mut)
    return (d * rstd * w + b).to(BF)


def model_embed(tok, word, pos, w, b, T, src=None, wide=0, mut=""):
    s = torch.arange(tok.numel()) if src is None else src.long()
    t = (s // T) % pos.shape[0] if mut == "pos_div" else s % T  # mutant: row // T
    return model_ln(word[tok.reshape(-1).long()[s]], w, b, pos[t], wide)


def model_store(y, dst, guard: int, rpb: int, mut=""):
    """The output buffer of a scattered store: ``guard`` rows past the end, all filled with the
    sentinel; the mutant also stores the first clamped tail row (computed from row rows - 1)."""
    rows = y.shape[0]
    buf = torch.full((rows + guard, y.shape[1]), no.SENTINEL, dtype=BF)
    buf[torch.arange(rows) if dst is None else dst.long()] = y
    if mut == "tail_store" and rows % rpb != 0:
        buf[rows] = y[rows - 1]
    return buf


def block_sum(t):
    """[rows, D] fp32 -> [D]: ln_bwd_kernel's dw / db / dxs: per lane over the rows of its stride,
    the 4 waves in LDS order, the blocks one atomic after the other."""
    rows, D = t.shape
    blocks = min((rows + 3) // 4, 1024)
    stride = blocks * 4
    k = (rows + stride - 1) // stride
    tp = F.pad(t, (0, 0, 0, k * stride - rows)).view(k, blocks, 4, D)
    acc = torch.zeros(blocks, 4, D)
    for i in range(k):
        acc = acc + tp[i]
    blk = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    out = torch.zeros(D)
    for bi in range(blocks):
        out = out + blk[bi]
    return out


def model_ln_bwd(x, w, dy, drop=None, mut=""):
    """-> dict(dx bf16, dw, db, dxs | (dxz bf16, cs))."""
    v = x.float()
    d, rstd = model_stats(v, False)
    xh = d * rstd
    dyf = dy.float()
    g = dyf * w
    Df = torch.tensor(float(x.shape[1]))
    mg = lane_sum(g, 64, 4) / Df
    mgx = lane_sum(g * xh, 64, 4) / Df
    t = g - mg if mut == "no_xhat_term" else g - mg - xh * mgx  # mutant: no xhat mean(g xhat)
    dx32 = rstd * t
    dx = dx32.to(BF)
    out = dict(dx=dx, dw=block_sum(dyf * (v if mut == "dw_x" else xh)), db=block_sum(dyf))  # mutant: dy x
    if drop is None:
        out["dxs"] = block_sum(dx32 if mut == "dxs_fp32" else dx.float())  # mutant: the fp32 dx summed
    else:
        p, seed, off = drop
        out["dxz"] = ref.dropout_add(dx, None, p, seed, off).to(BF)
        out["cs"] = block_sum(out["dxz"].float())
    return out


def model_colsum(x, budget: int, unroll: int, mut=""):
    """The chunked two-pass column sums (colsum_partial_kernel / gelu_bwd_colsum_partial_kernel and
    colsum_final_kernel) of the rows of x (for the fused GELU backward: the dz it wrote)."""
    M, N = x.shape
    chunks = no.cs_chunks(M, N, budget)
    rows_per = (M + chunks - 1) // chunks
    xf = x.float()
    partial = torch.zeros(chunks, N)
    for ch in range(chunks):
        r0 = ch * rows_per
        r1 = min(M, r0 + rows_per)
        if mut == "drop_tail":  # mutant: the last (rows of the chunk) % 4 rows dropped
            r1 = r0 + max(r1 - r0, 0) // 4 * 4
        wave = []
        for wv in range(4):
            acc = torch.zeros(N)
            r = r0 + wv
            if unroll == 16:
                while r + 12 < r1:
                    acc = acc + ((xf[r] + xf[r + 4]) + (xf[r + 8] + xf[r + 12]))
                    r += 16
            else:
                while r + 4 < r1:
                    acc = acc + (xf[r] + xf[r + 4])
                    r += 8
            while r < r1:
                acc = acc + xf[r]
                r += 4
            wave.append(acc)
        partial[ch] = ((wave[0] + wave[1]) + wave[2]) + wave[3]
    tot = torch.zeros(N)
    for wv in range(16):
        s = torch.zeros(N)
        for k in range(wv, chunks, 16):
            s = s + partial[k]
        tot = tot + s
    return tot


def model_embed_grad(dx, tok, V, mut=""):
    srt, perm = torch.sort(tok.long(), stable=True)
    xf = dx.float()
    out = torch.zeros(V, dx.shape[1])
    R = tok.numel()
    b = 0
    while b < R:
        t = int(srt[b])
        e = b
        while e < R and int(srt[e]) == t:
            e += 1
        if t != 0 or mut == "pad":  # mutant: the pad token summed
            rows = xf[perm[b:e]]
            L = e - b
            if mut == "cut64" and L > no.EG_HEAVY:  # mutant: a heavy segment cut at EG_HEAVY rows
                rows, L = rows[:no.EG_HEAVY], no.EG_HEAVY
            if L <= no.EG_HEAVY:
                acc = torch.zeros(dx.shape[1])
                for i in range(L):
                    acc = acc + rows[i]
            else:  # 16 waves stride the rows, then a fixed-order combine
                acc = torch.zeros(dx.shape[1])
                for wv in range(16):
                    s = torch.zeros(dx.shape[1])
                    for i in range(wv, L, 16):
                        s = s + rows[i]
                    acc = acc + s
            out[t] = acc
        b = e
    return out


def model_gelu_fwd(z, mut=""):
    x = z.float()
    if mut == "tanh":  # mutant: the tanh approximation
        return F.gelu(x, approximate="tanh").to(BF)
    return go.gelu_scalar_f32(x).to(BF)


def model_gelu_bwd(z, dh, form, mut=""):
    x = z.float()
    if mut == "tanh":
        xg = x.clone().requires_grad_(True)
        F.gelu(xg, approximate="tanh").sum().backward()
        gp = xg.grad
    else:
        gp = no.gelu_grad_stream_f32(x) if form == "stream" else go.gelu_grad_scalar_f32(x)
    return (dh.float() * gp).to(BF)


# -------------------------------------------------------------------------- the judged families
def fwd_ratios(mut=""):
    """Worst ratio per (wide, residual) over every forward shape; the ln16p walk at wide 4."""
    out = {}
    for wide in (0, 1, 4):  # the rounding model has two forms: generic and half-wave (wide >= 1)
        shapes = no.fwd_shapes(wide) + ([(rows, 256) for rows in no.walk_rows(CUS)] if wide == 4 else [])
        for rows, D in shapes:
            x, r, w, b, _ = no.ln_inputs(rows, D)
            for res in (None, r):
                o = no.ln_oracle(x, w, b, res)
                k = "ln fwd wide=%d%s" % (wide, " +res" if res is not None else "")
                out[k] = max(out.get(k, 0.0), no.ratio(model_ln(x, w, b, res, wide, mut), o["y"], o["tol"]))
    return out


def regime_ratios(mut=""):
    """Worst forward ratio per input regime, over every shape, both model forms, with and without r."""
    out = {}
    for wide in (0, 1):
        for rows, D in no.fwd_shapes(wide):
            x, r, w, b, kinds = no.ln_inputs(rows, D)
            for res in (None, r):
                o = no.ln_oracle(x, w, b, res)
                per_row = go.elem_ratio(model_ln(x, w, b, res, wide, mut), o["y"], o["tol"]).amax(1)
                for k, v in zip(kinds, per_row.tolist()):
                    out[k] = max(out.get(k, 0.0), v)
    return out


def scatter_ratios(mut=""):
    w_ = 0.0
    for rph, rpb in ((1, 8), (2, 16), (4, 32)):
        for rows, D in ((rows, D) for D in no.SCATTER_D for rows in no.FWD_ROWS):
            x, r, w, b, dst = no.scatter_inputs(rows, D)
            for res in (None, r):
                o = no.ln_oracle(x, w, b, res)
                buf = model_store(model_ln(x, w, b, res, 1), dst, 8, rpb, mut)
                w_ = max(w_, no.scatter_ratio(buf, o["y"], o["tol"], dst))
    return {"ln scatter": w_}


def embed_ratios(mut=""):
    out = {}
    for wide in (0, 1):
        for n, T, D in no.embed_shapes(wide):
            tok, word, pos, w, b, src = no.embed_inputs(n, T, D)
            for s in (None, src) if D % 256 == 0 else (None,):
                o = no.embed_oracle(tok, word, pos, w, b, T, s)
                k = "embed_ln%s wide=%d" % ("_rows" if s is not None else "", wide)
                y = model_embed(tok, word, pos, w, b, T, s, wide, mut)
                out[k] = max(out.get(k, 0.0), no.ratio(y, o["y"], o["tol"]))
    return out


def bwd_ratios(mut="", cases=None):
    out = {}

    def put(k, v):
        out[k] = max(out.get(k, 0.0), v)

    for rows, D, wc in (cases or no.bwd_cases()):
        x, w, dy, _ = no.ln_bwd_inputs(rows, D, wc)
        o = no.ln_bwd_oracle(x, w, dy)
        m = model_ln_bwd(x, w, dy, None, mut)
        put("ln bwd dx", no.ratio(m["dx"], o["dx"], o["tol_dx"]))
        put("ln bwd dw", no.ratio(m["dw"], o["dw"], o["tol_dw"]))
        put("ln bwd db", no.ratio(m["db"], o["db"], o["tol_db"]))
        put("ln bwd dxs", no.ratio(m["dxs"], *no.written_colsum(m["dx"])))
        for p in no.DROP_P:
            md = model_ln_bwd(x, w, dy, (p, no.DROP_SEED, no.DROP_OFFSET), mut)
            put("ln bwd drop cs", no.ratio(md["cs"], *no.written_colsum(md["dxz"])))
    return out


def gelu_ratios(mut=""):
    out = {"gelu fwd": 0.0, "gelu bwd": 0.0}
    for n in no.GELU_N + (no.GELU_N_STRIDE,):
        z, dh = no.gelu_inputs(n)
        out["gelu fwd"] = max(out["gelu fwd"], no.ratio(model_gelu_fwd(z, mut), *no.gelu_fwd_oracle(z)))
        out["gelu bwd"] = max(out["gelu bwd"], no.ratio(model_gelu_bwd(z, dh, "stream", mut),
                                                        *no.gelu_bwd_oracle(z, dh, "stream")))
    return out


def colsum_ratios(mut=""):
    w_ = 0.0
    for M, N, sliced in no.colsum_cases():
        x = no.colsum_inputs(M, N, sliced)
        x = x[:, N:2 * N] if sliced else x
        w_ = max(w_, no.ratio(model_colsum(x, 1024, 16, mut), *no.colsum_oracle(x)))
    return {"colsum": w_}


def gelu_colsum_ratios(mut=""):
    out = {"gelu_bwd_colsum dz": 0.0, "gelu_bwd_colsum cs": 0.0}
    for M, N in no.gelu_colsum_cases():
        df, z = no.gelu_colsum_inputs(M, N)
        dz = model_gelu_bwd(z, df, "colsum", "tanh" if mut == "tanh" else "")
        out["gelu_bwd_colsum dz"] = max(out["gelu_bwd_colsum dz"], no.ratio(dz, *no.gelu_bwd_oracle(z, df, "colsum")))
        cs = model_colsum(dz, 2048, 8, mut)
        out["gelu_bwd_colsum cs"] = max(out["gelu_bwd_colsum cs"], no.ratio(cs, *no.written_colsum(dz)))
    return out


def embed_grad_ratios(mut=""):
    w_ = 0.0
    for name, *_ in no.EG_CASES:
        dx, tok, V = no.embed_grad_inputs(name)
        w_ = max(w_, no.ratio(model_embed_grad(dx, tok, V, mut), *no.embed_grad_oracle(dx, tok, V)))
    return {"embed_grad": w_}


# ------------------------------------------------------------------------------------- tests
def test_oracle_intermediates_match_fp64_autograd():
    x, r, w, b, _ = no.ln_inputs(33, 36)
    for res in (None, r):
        o = no.ln_oracle(x, w, b, res)
        v = x.double() if res is None else x.double() + res.double()
        want = ref.layer_norm(v, w.double(), b.double(), no.LN_EPS)
        assert float((o["y"] - want).abs().max() / want.abs().max()) < 1e-12
    # backward: a well-conditioned set (no tiny-variance / zero rows: rstd = 1e6 amplifies the last bit)
    g = torch.Generator().manual_seed(5)
    xb = (torch.randn(9, 36, generator=g) * 2 + 0.5).to(BF)
    dyb = torch.randn(9, 36, generator=g).to(BF)
    wb, _ = no.affine(36, g)
    o = no.ln_bwd_oracle(xb, wb, dyb)
    xd = xb.double().requires_grad_(True)
    wd = wb.double().requires_grad_(True)
    bd = torch.zeros(36, dtype=torch.float64, requires_grad=True)
    F.layer_norm(xd, (36,), wd, bd, no.LN_EPS).backward(dyb.double())
    for got, want in ((o["dx"], xd.grad), (o["dw"], wd.grad), (o["db"], bd.grad)):
        assert float((got - want).abs().max() / want.abs().max()) < 1e-12
    # the all-zero row: dx = rstd (g - mean g), y = b
    z = torch.zeros(1, 36, dtype=BF)
    oz = no.ln_bwd_oracle(z, wb, dyb[:1])
    gg = dyb[:1].double() * wb.double()
    assert torch.allclose(oz["dx"], (gg - gg.mean()) / math.sqrt(no.LN_EPS), rtol=1e-12, atol=0.0)
    _, _, w0, b0, _ = no.ln_inputs(1, 36)
    assert torch.equal(no.ln_oracle(z, w0, b0)["y"], b0.double().expand(1, 36))
    # embedding: ops.reference in fp64
    tok, word, pos, w, b, src = no.embed_inputs(3, 5, 36)
    want = ref.embed_ln(tok.long(), word.double(), pos.double(), w.double(), b.double(), no.LN_EPS)
    o = no.embed_oracle(tok, word, pos, w, b, 5)
    assert float((o["y"] - want).abs().max()) < 1e-12 * float(want.abs().max())
    o = no.embed_oracle(tok, word, pos, w, b, 5, src)
    assert float((o["y"] - want[src.long()]).abs().max()) < 1e-12 * float(want.abs().max())
    # GELU: F.gelu and its autograd in fp64
    zz = torch.linspace(-6, 6, 481, dtype=torch.float64).requires_grad_(True)
    F.gelu(zz).sum().backward()
    assert float((go.gelu_exact(zz.detach()) - F.gelu(zz.detach())).abs().max()) < 1e-12
    assert float((go.gelu_grad_exact(zz.detach()) - zz.grad).abs().max()) < 1e-12
    # embed_grad: autograd of F.embedding(padding_idx=0)
    dx, tok, V = no.embed_grad_inputs("end1-256")
    tab = torch.zeros(V, 256, dtype=torch.float64, requires_grad=True)
    F.embedding(tok.long(), tab, padding_idx=0).backward(dx.double())
    assert float((no.embed_grad_oracle(dx, tok, V)[0] - tab.grad).abs().max()) < 1e-12


def test_input_sets_reach_the_paths_they_are_there_for():
    kinds = set()
    for rows in no.FWD_ROWS:
        kinds |= set(no.ln_inputs(rows, 768)[4])
    assert kinds == set(no.REGIMES)
    assert any("const" in no.ln_bwd_inputs(*c)[3] for c in no.bwd_cases())
    for rows in no.walk_rows(CUS):  # ln16p: a second and a third row per half-wave, a ragged end
        assert rows > 64 * CUS and rows % 8 != 0
    assert no.walk_rows(CUS)[1] > 128 * CUS
    for rows in no.BWD_WALK_ROWS:  # ln_bwd: 1024 blocks x 4 waves
        assert rows > 4096 and rows % 4 != 0
    for name, D, lengths, pad in no.EG_CASES:
        assert {no.EG_HEAVY, no.EG_HEAVY + 1} <= set(lengths)
    assert sum(L > no.EG_HEAVY for L in no.EG_CASES[-1][2]) > 256  # the heavy kernel's 256-block grid strides
    assert {c[2][-1] for c in no.EG_CASES} >= {1, 64, 65, 1000}  # what ends at R
    assert no.GELU_N_STRIDE // 4 > 4096 * 256
    for N in no.CS_N:  # one empty chunk, one tail-only chunk, full chunks with two unrolled trips
        for budget, unroll in ((1024, 16), (2048, 8)):
            M = no.cs_mixed_M(N, budget, unroll)
            chunks = no.cs_chunks(M, N, budget)
            rp = (M + chunks - 1) // chunks
            sizes = [max(min(M, (c + 1) * rp) - c * rp, 0) for c in range(chunks)]
            assert 0 in sizes and any(0 < s <= unroll - 4 for s in sizes)
            assert rp > 2 * unroll and rp % 4 != 0 and sizes[0] == rp


def test_gelu_constants_hold_the_record():
    got = no.measure_stream_eps()["gelu_grad_stream"]
    rec = no.EPS_MEASURED_STREAM["gelu_grad_stream"]
    assert got <= rec <= 1.02 * got, (got, rec)
    x = go.act_grid()[::257]
    # gelu_grad_s of train_grad.hip is the recorded scalar form, operation for operation
    f = go._f
    z = x * f(go._RSQRT2)
    az = z.abs()
    t = torch.reciprocal(f(1.0) + f(0.3275911) * az)
    erfv = torch.copysign(f(1.0) - go._poly(t, go._P) * torch.exp(-az * az), z)
    own = f(0.5) * (f(1.0) + erfv) + x * f(go._RSQRT2PI) * torch.exp(f(-0.5) * x * x)
    assert torch.equal(own, go.gelu_grad_scalar_f32(x))
    m = go.measure_activation_eps()
    for k in ("gelu_scalar", "gelu_grad_scalar"):
        assert m[k] <= go.EPS_MEASURED[k] <= 1.02 * m[k], (k, m[k])


FAMILIES = [fwd_ratios, scatter_ratios, embed_ratios, bwd_ratios, gelu_ratios, colsum_ratios, gelu_colsum_ratios,
            embed_grad_ratios]


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.__name__)
def test_rounding_model_is_inside_the_bound(family):
    for k, v in family().items():
        report(k, v)
        assert v < 1.0, (k, v)


SMALL_BWD = [c for c in no.bwd_cases() if c[0] <= 1000]
MUTANTS = [
    ("onepass", fwd_ratios), ("unbiased", fwd_ratios), ("eps_outside", fwd_ratios), ("res_bf16", fwd_ratios),
    ("pos_div", embed_ratios), ("tail_store", scatter_ratios),
    ("no_xhat_term", lambda m: bwd_ratios(m, SMALL_BWD)), ("dw_x", lambda m: bwd_ratios(m, SMALL_BWD)),
    ("dxs_fp32", lambda m: bwd_ratios(m, SMALL_BWD)),
    ("drop_tail", colsum_ratios), ("drop_tail", gelu_colsum_ratios), ("pad", embed_grad_ratios),
    ("cut64", embed_grad_ratios), ("tanh", gelu_ratios), ("tanh", gelu_colsum_ratios),
]


@pytest.mark.parametrize("mut,family", MUTANTS, ids=["%s-%d" % (m, i) for i, (m, _) in enumerate(MUTANTS)])
def test_mutants_leave_the_bound(mut, family):
    r = family(mut)
    worst = max(r.values())
    print("norm-oracle mutant %-14s worst ratio %.3g" % (mut, worst))
    assert worst > 1.0, (mut, r)
    if mut == "onepass":  # it is the large-mean rows that fail, and only they
        per = regime_ratios(mut)
        assert per["bigmean"] > 1.0 and all(v < 1.0 for k, v in per.items() if k != "bigmean"), per
    if mut == "eps_outside":  # visible on the tiny-variance rows
        assert regime_ratios(mut)["tinyvar"] > 1.0
