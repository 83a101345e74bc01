"""Every kernel form of csrc/layernorm.hip and csrc/train_grad.hip against the fp64 oracle and its
per-element bound (``tests/norm_oracle.py``): the LayerNorm forward in all five ``ln_set_wide``
forms with its residual, embedding, packed-row and scattered-store variants, the LayerNorm
backward (plain, with the fused column sums, with the fused dropout backward), the streaming
GELU forward and backward, ``colsum``, ``gelu_bwd_colsum`` and ``embed_grad``.  Every call is made
twice and every output must be finite; everything but the float-atomic sums of ``ln_bwd`` (dw, db,
dxs) must be bit-identical across the two calls.  The inputs are the shared builders of
``norm_oracle`` (unit Gaussian, large-mean, outlier-column, tiny-variance, all-zero and constant
rows; w with zeros and negative entries); ``tests/test_norm_oracle_cpu.py`` runs a rounding model
and its mutants over the same sets.  The reference is never another kernel form.  Each test
prints its worst ratio (``-rP`` shows them)."""
import functools

import pytest
import torch

import norm_oracle as no
from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import native

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EPS = no.LN_EPS


def report(form, worst):
    print("norm-oracle ratio %-44s %.3f" % (form, worst))


def _finite(*ts):
    for t in ts:
        assert bool(torch.isfinite(t.float()).all()), "a non-finite value"


def _twice(f):
    """Call twice: bit-identical and finite.  -> the first result (a tensor or a tuple)."""
    a, b = f(), f()
    ta = a if isinstance(a, (tuple, list)) else (a,)
    tb = b if isinstance(b, (tuple, list)) else (b,)
    for x, y in zip(ta, tb):
        assert torch.equal(x, y), "a second call differs"
        _finite(x)
    return a


def _to(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


def _with_wide(wide, f):
    """``ln_set_wide`` is process-global: restored to the default (4) even when the call fails."""
    lib = native.lib()
    lib.ln_set_wide(wide)
    try:
        return f()
    finally:
        lib.ln_set_wide(4)


def _cus(dev) -> int:
    return torch.cuda.get_device_properties(dev).multi_processor_count


# One oracle per input set, shared by the five forms and left unchanged.
@functools.lru_cache(maxsize=None)
def fwd_oracle(rows, D, res):
    x, r, w, b, _ = no.ln_inputs(rows, D)
    o = no.ln_oracle(x, w, b, r if res else None)
    return o["y"], o["tol"]


@functools.lru_cache(maxsize=None)
def scatter_oracle(rows, D, res):
    x, r, w, b, _ = no.scatter_inputs(rows, D)
    o = no.ln_oracle(x, w, b, r if res else None)
    return o["y"], o["tol"]


@functools.lru_cache(maxsize=None)
def embed_oracle(n, T, D, rows_form):
    tok, word, pos, w, b, src = no.embed_inputs(n, T, D)
    o = no.embed_oracle(tok, word, pos, w, b, T, src if rows_form else None)
    return o["y"], o["tol"]


# =========================================================================== LayerNorm forward
@pytest.mark.parametrize("wide", [0, 1, 2, 3, 4])
def test_layer_norm_forward(dev, wide):
    """wide 0: ln_kernel at every D, D % 256 != 0 (the ``i < D`` masking) included.  wide 1 / 2 / 3:
    ln16_kernel with 1 / 2 / 4 rows per half-wave; the row counts are the tails of its 8-, 16- and
    32-row blocks (a clamped tail row is computed from row rows - 1 and not stored).  wide 4:
    ln16p_kernel.  D = 400 at wide >= 1 falls through to ln_kernel.  An all-zero row must come out
    as exactly bf16(b)."""
    lib = native.lib()
    worst = {False: 0.0, True: 0.0}
    for rows, D in no.fwd_shapes(wide):
        x_c, r_c, w_c, b_c, kinds = no.ln_inputs(rows, D)
        x, r, w, b = _to(dev, x_c, r_c, w_c, b_c)
        zero = torch.tensor([k == "zero" for k in kinds])
        for res in (False, True):
            y = _with_wide(wide, lambda: _twice(lambda: lib.layer_norm(x, w, b, EPS, r if res else None)))
            tag = "wide=%d rows=%d D=%d%s" % (wide, rows, D, " +res" if res else "")
            worst[res] = max(worst[res], no.check(y, *fwd_oracle(rows, D, res), tag))
            if bool(zero.any()):
                assert torch.equal(y.cpu()[zero], b_c.to(BF).expand(int(zero.sum()), D)), tag + ": zero row != bf16(b)"
    report("ln fwd wide=%d" % wide, worst[False])
    report("ln fwd wide=%d +res" % wide, worst[True])


def test_layer_norm_persistent_walk(dev):
    """ln16p_kernel's row loop (the default forward, wide = 4) at D = 256: with rows = 64 CUs + 11
    some half-waves take a second row -- the prefetch, the ax = nx hand-over, the clamped last
    prefetch and the nrow >= rows exit -- and with 128 CUs + 3 a third; both ends are ragged."""
    lib = native.lib()
    for rows in no.walk_rows(_cus(dev)):
        x_c, r_c, w_c, b_c, _ = no.ln_inputs(rows, 256)
        x, r, w, b = _to(dev, x_c, r_c, w_c, b_c)
        for res in (False, True):
            y = _with_wide(4, lambda: _twice(lambda: lib.layer_norm(x, w, b, EPS, r if res else None)))
            tag = "ln16p walk rows=%d%s" % (rows, " +res" if res else "")
            report(tag, no.check(y, *fwd_oracle(rows, 256, res), tag))


@pytest.mark.parametrize("wide", [0, 1, 2, 3, 4])
def test_layer_norm_scatter(dev, wide):
    """``layer_norm_scatter`` with ``out=`` a buffer filled with a sentinel, 8 guard rows past its end:
    dst is a partial permutation (two pairs of identical input rows share a destination), so two
    destination rows, and the guard rows -- where a stored clamped tail row of the RPH > 1 forms
    would land -- must keep the sentinel.  wide 0 and 1 are the same one-row form."""
    worst = 0.0
    for D in no.SCATTER_D:
        for rows in no.FWD_ROWS:
            x_c, r_c, w_c, b_c, dst_c = no.scatter_inputs(rows, D)
            x, r, w, b, dst = _to(dev, x_c, r_c, w_c, b_c, dst_c)
            for res in (False, True):
                def run():
                    buf = torch.full((rows + 8, D), no.SENTINEL, device=dev, dtype=BF)
                    ops.layer_norm_scatter(x, w, b, EPS, r if res else None, dst, buf[:rows])
                    return buf

                buf = _with_wide(wide, lambda: _twice(run))
                ref, tol = scatter_oracle(rows, D, res)
                ratio = no.scatter_ratio(buf, ref, tol, dst_c)
                tag = "scatter wide=%d rows=%d D=%d%s" % (wide, rows, D, " +res" if res else "")
                assert ratio <= 1.0, "%s: ratio %g (inf: a row that no dst names was written)" % (tag, ratio)
                worst = max(worst, ratio)
    report("ln scatter wide=%d" % wide, worst)


@pytest.mark.parametrize("wide", [0, 1, 2, 3, 4])
def test_embed_ln_forms(dev, wide):
    """``embed_ln`` and (D % 256 == 0) ``embed_ln_rows`` against the fp64 LN(word[tok] + pos[t]): the
    position index row % T, the src gather, repeated tokens, token 0, the last vocabulary row,
    position T - 1.  The embedding forms have no persistent kernel: wide 4 runs the one-row form."""
    worst = {False: 0.0, True: 0.0}
    for n, T, D in no.embed_shapes(wide):
        tok, word, pos, w, b, src = _to(dev, *no.embed_inputs(n, T, D))
        tag = "wide=%d n=%d T=%d D=%d" % (wide, n, T, D)
        y = _with_wide(wide, lambda: _twice(lambda: ops.embed_ln(tok, word, pos, w, b, EPS)))
        worst[False] = max(worst[False], no.check(y, *embed_oracle(n, T, D, False), "embed_ln " + tag))
        if D % 256 == 0:
            y = _with_wide(wide, lambda: _twice(lambda: ops.embed_ln_rows(tok, src, word, pos, w, b, EPS)))
            worst[True] = max(worst[True], no.check(y, *embed_oracle(n, T, D, True), "embed_ln_rows " + tag))
    report("embed_ln wide=%d" % wide, worst[False])
    report("embed_ln_rows wide=%d" % wide, worst[True])


# ========================================================================== LayerNorm backward
def _bwd_sums(dw, db, dxs, written, o, tag, worst):
    """dw, db against the oracle; the fused column sums against the tensor the kernel wrote."""
    _finite(dw, db)
    worst["dw"] = max(worst["dw"], no.check(dw, o["dw"], o["tol_dw"], tag + " dw"))
    worst["db"] = max(worst["db"], no.check(db, o["db"], o["tol_db"], tag + " db"))
    if dxs is not None:
        _finite(dxs)
        worst["dxs"] = max(worst["dxs"], no.check(dxs, *no.written_colsum(written), tag + " dxs"))


@pytest.mark.parametrize("rows,D,with_const", no.bwd_cases())
def test_layer_norm_backward(dev, rows, D, with_const):
    """``layer_norm_bwd``, ``_colsum`` and ``_drop``.  D = 36 and 400: the ``i < D`` masking (masked lanes
    read row 0 and discard it).  rows = 4096 + 5 and 2 * 4096 + 1 at D = 256: the 1024-block grid
    strides, a wave takes a second and a third row -- the row-ahead prefetch with its last-trip
    guard, and pw / pb / px accumulated over more than one row per lane.  dx and dxz are
    deterministic; dw, db and the column sums go through float atomics across blocks: both calls
    are held to the bound, bit-identity is asked where the grid is one block (rows <= 4)."""
    lib = native.lib()
    x_c, w_c, dy_c, kinds = no.ln_bwd_inputs(rows, D, with_const)
    o = no.ln_bwd_oracle(x_c, w_c, dy_c)
    x, w, dy = _to(dev, x_c, w_c, dy_c)
    tag = "rows=%d D=%d%s" % (rows, D, " const" if with_const else "")
    worst = dict(dx=0.0, dw=0.0, db=0.0, dxs=0.0)
    forms = [("plain", lambda: tuple(lib.layer_norm_bwd(x, w, dy, EPS)) + (None,)),
             ("colsum", lambda: tuple(lib.layer_norm_bwd_colsum(x, w, dy, EPS)))]
    dx0 = None
    for name, f in forms:
        a, b = f(), f()
        assert torch.equal(a[0], b[0]), name + ": dx differs between two calls"
        _finite(a[0])
        worst["dx"] = max(worst["dx"], no.check(a[0], o["dx"], o["tol_dx"], "%s %s dx" % (tag, name)))
        dx0 = a[0] if dx0 is None else dx0
        assert torch.equal(a[0], dx0), "the forms disagree on dx"
        for c in (a, b):
            _bwd_sums(c[1], c[2], c[3], c[0], o, "%s %s" % (tag, name), worst)
        if rows <= 4:
            for u, v in zip(a[1:], b[1:]):
                assert u is None or torch.equal(u, v), name + ": one block, yet a sum differs"
    for p in no.DROP_P:
        f = lambda: lib.layer_norm_bwd_drop(x, w, dy, EPS, p, no.DROP_SEED, no.DROP_OFFSET)
        a, b = f(), f()
        name = "drop p=%g" % p
        assert torch.equal(a[0], dx0) and torch.equal(b[0], dx0), name + ": dx differs from the plain form"
        assert torch.equal(a[1], b[1]), name + ": dxz differs between two calls"
        _finite(a[1])
        assert torch.equal(a[1], ops.dropout_add(dx0, None, p, no.DROP_SEED, no.DROP_OFFSET)), name + ": dxz"
        for c in (a, b):
            _bwd_sums(c[2], c[3], c[4], c[1], o, "%s %s" % (tag, name), worst)
        if rows <= 4:
            for u, v in zip(a[2:], b[2:]):
                assert torch.equal(u, v), name + ": one block, yet a sum differs"
        compared = dx0 != 0
        kept = int(((a[1] != 0) & compared).sum())
        lo, hi = no.drop_kept_limits(int(compared.sum()), p)
        assert lo <= kept <= hi, "%s %s: kept %d of %d, outside [%.1f, %.1f]" % (tag, name, kept, int(compared.sum()), lo, hi)
    for k, v in worst.items():
        report("ln bwd %s %s" % (k, tag), v)


# ======================================================================================= GELU
@pytest.mark.parametrize("n", no.GELU_N + (no.GELU_N_STRIDE,))
def test_gelu_stream(dev, n):
    """``gelu`` forward and backward over the saturating / tail grid.  n = 4 (4096 * 256 + 37): more
    4-element groups than the 4096-block grid has threads -- the grid-stride loop, with a ragged
    last trip."""
    lib = native.lib()
    z_c, dh_c = no.gelu_inputs(n)
    z, dh = _to(dev, z_c, dh_c)
    h = _twice(lambda: lib.gelu(z, None))
    dz = _twice(lambda: lib.gelu(z, dh))
    report("gelu fwd n=%d" % n, no.check(h, *no.gelu_fwd_oracle(z_c), "gelu fwd n=%d" % n))
    report("gelu bwd n=%d" % n, no.check(dz, *no.gelu_bwd_oracle(z_c, dh_c, "stream"), "gelu bwd n=%d" % n))


# ========================================================================== column reductions
# The launchers' chunk rule (train_grad.hip), copied: cb = ceil(N / 512); chunks = 1024 / cb (colsum)
# or 2048 / cb (gelu_bwd_colsum), clamped to [16, 256], then to at most M; a chunk is
# ceil(M / chunks) rows and the 4 waves of a block stride over them, 16 (colsum) or 8 (gelu) rows per
# unrolled trip, then one row per tail trip.  no.cs_mixed_M picks, per N, an M at which full chunks
# make two unrolled trips and a ragged tail, one chunk of 5 / 3 rows runs the tail loop only, and
# one chunk is empty (tests/test_norm_oracle_cpu.py checks that it does).  M = 1, 3, 17: fewer rows
# than chunks (M = 17 at 16 < chunks: one row per chunk).
@pytest.mark.parametrize("M,N,sliced", no.colsum_cases())
def test_colsum(dev, M, N, sliced):
    x_c = no.colsum_inputs(M, N, sliced)
    x = x_c.to(dev)
    if sliced:  # the middle third of [M, 3 N]: ld = 3 N
        x_c, x = x_c[:, N:2 * N], x[:, N:2 * N]
    got = _twice(lambda: native.lib().colsum(x))
    tag = "colsum M=%d N=%d%s" % (M, N, " ld=3N" if sliced else "")
    report(tag, no.check(got, *no.colsum_oracle(x_c), tag))


@pytest.mark.parametrize("M,N", no.gelu_colsum_cases())
def test_gelu_bwd_colsum(dev, M, N):
    df_c, z_c = no.gelu_colsum_inputs(M, N)
    df, z = _to(dev, df_c, z_c)
    dz, cs = _twice(lambda: tuple(native.lib().gelu_bwd_colsum(df, z)))
    tag = "gelu_bwd_colsum M=%d N=%d" % (M, N)
    report(tag + " dz", no.check(dz, *no.gelu_bwd_oracle(z_c, df_c, "colsum"), tag + " dz"))
    report(tag + " cs", no.check(cs, *no.written_colsum(dz), tag + " cs"))


# ================================================================================= embed_grad
@pytest.mark.parametrize("name", [c[0] for c in no.EG_CASES])
def test_embed_grad(dev, name):
    """Segments of 1, 63, 64, 65, 66 and 1000 rows around EG_HEAVY = 64 (64: the light kernel's last
    length; 65: the heavy kernel's first), the last one ending at R with each of 1, 64, 65 and 1000
    rows; D = 256 and 512 (nc < 3 in the heavy kernel); 261 heavy tokens: the heavy kernel's
    256-block grid strides.  The pad row 0 and every absent token must be exactly zero in the
    output as it stands."""
    dx_c, tok_c, V = no.embed_grad_inputs(name)
    srt, perm = torch.sort(tok_c, stable=True)
    dx, srt, perm = _to(dev, dx_c, srt.to(torch.int32), perm.to(torch.int32))
    got = _twice(lambda: native.lib().embed_grad(dx, srt, perm, V))
    ref, tol = no.embed_grad_oracle(dx_c, tok_c, V)
    report("embed_grad " + name, no.check(got, ref, tol, "embed_grad " + name))
    absent = torch.ones(V, dtype=torch.bool)
    absent[tok_c.long()] = False
    absent[0] = True
    assert int(absent.sum()) > 2 and not bool(got.cpu()[absent].any()), "the pad row or an absent token is not zero"
