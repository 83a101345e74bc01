"""Every launch form of csrc/small_gemm.hip (generic, register queue, 128-row / -column tiles,
mixed dtypes, the LDS-DMA ring at 2 / 3 / 4 stages, register-direct, ``splitk_reduce``), ``colsum_f32``,
``gather_dropout`` and the weight-gradient GEMM of csrc/gemm_wgrad.hip on the per-element fp64 oracle
of tests/sgemm_oracle.py.

A case passes when EVERY output element is within its counted bound (``ratio <= 1``) and nothing
outside ``C[:M, :N]`` was written: each launch runs into sentinel-filled buffers with ``ldc = N + 3`` and
``N + 4``, two guard rows, an aligned and a 1-float-offset base, twice, and the two runs must agree
bit for bit.  Which form a case reaches is read from ``sgemm_oracle.dispatch``, the transcription of
the launcher's conditions, and asserted against the form the case names.  Shapes are the smallest
that reach a path (the case lists and their reasons are in the oracle module).  Run with ``-s`` for
the worst ratio per form.
"""
import functools

import pytest
import torch

import sgemm_oracle as so
from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import Gemm, native

pytestmark = pytest.mark.gpu

WORST = {}
C_VARIANTS = ((3, 0), (4, 0), (3, 1), (4, 1))  # (ldc - N, floats the base is off 16-byte alignment)
DEV_OFF = 5


def _note(form: str, ratio: float) -> None:
    WORST[form] = max(WORST.get(form, 0.0), ratio)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nworst observed / bound per form: %s" % {k: "%.3f" % v for k, v in sorted(WORST.items())})


@functools.lru_cache(maxsize=None)
def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _run_case(case, dev) -> None:
    name, specs, tile, form, *rest = case
    extra = rest[0] if rest else {}
    built = [so.build(s).to(dev) for s in specs]
    use_off = any(s.drop_on and s.seed % 2 == 1 for s in specs)
    dev_off = torch.tensor([DEV_OFF], device=dev, dtype=torch.int64) if use_off else None
    oracles = None
    for (pad, boff) in C_VARIANTS:
        runs = []
        for _ in range(2):
            bufs, gs = [], []
            for b in built:
                s = b.spec
                flat, C = so.padded_c(s.M, s.N, s.N + pad, 2, boff, b.prior, dev)
                a_s = torch.full((s.M + 2,), float("nan"), device=dev) if s.asum else None
                bufs.append((flat, C, a_s))
                gs.append(b.gemm(C, s.N + pad, None if a_s is None else a_s[:s.M]))
            runs.append((bufs, gs))
        gs = runs[0][1]
        if oracles is None:  # once per case: the prior C is the same in every variant
            got_form, sk, blocks = so.dispatch(gs, tile)
            assert got_form == form, "%s: the launcher's conditions give %s, the case names %s" % (name, got_form, form)
            if "splits" in extra:
                assert [x[0] for x in sk] == extra["splits"], (name, sk)
            if "blocks" in extra:
                assert blocks == extra["blocks"], (name, blocks)
            off = DEV_OFF if use_off else 0
            oracles = [(so.small_gemm_oracle(g, sp, off), so.asum_oracle(g, sp) if g.asum is not None else None)
                       for g, (sp, _) in zip(gs, sk)]
        for _, g2 in runs:
            ops.small_gemm(*g2, dev_off=dev_off, tile=tile)
        for i, (b, g) in enumerate(zip(built, gs)):
            s = b.spec
            what = "%s desc %d ldc N + %d base + %d" % (name, i, pad, boff)
            (flat, C, a_s), (flat2, C2, a_s2) = runs[0][0][i], runs[1][0][i]
            so.check_padding(flat, C, s.M, s.N, g.ldc, what)
            assert torch.equal(_bits(flat), _bits(flat2)), "%s: not bitwise repeatable" % what
            got = so.c_view(C, s.M, s.N, g.ldc)
            (ref, tol), asum_o = oracles[i]
            if s.regime == "exact":
                want = so.exact_expected(s.M, s.N, s.K, s.bias, s.accumulate).to(dev)
                assert torch.equal(got, want), "%s: %s" % (what, so.describe(got, want.double(), tol))
            _note(form, so.check(got, ref, tol, what))
            if a_s is not None:
                assert bool(torch.isnan(a_s[s.M:]).all()), "%s: asum written past M" % what
                assert torch.equal(_bits(a_s[:s.M]), _bits(a_s2[:s.M])), "%s: asum not repeatable" % what
                _note(form + " asum", so.check(a_s[:s.M], asum_o[0], asum_o[1], what + " asum"))
                if s.regime == "exact":
                    assert torch.equal(a_s[:s.M], torch.ones(s.M, device=dev)), what


def _run_all(cases, dev) -> None:
    for c in cases:
        _run_case(c, dev)


@pytest.mark.parametrize("tile", list(so.LDS_FORMS) + so.RD_CODES)
def test_tile_edges(dev, tile):
    _run_all(so.edge_cases(tile), dev)


@pytest.mark.parametrize("tile", [1, 5, 2, 3, 4])
def test_dtype_quadrants_and_layouts(dev, tile):
    _run_all(so.quadrant_cases(tile), dev)


def test_generic_kernel(dev):
    _run_all(so.generic_cases(), dev)


@pytest.mark.parametrize("form", range(len(so.EPI_FORMS)), ids=["%d-%s-K%d" % (t, f, k) for t, f, _, k in so.EPI_FORMS])
def test_epilogues(dev, form):
    tile, _, _, K = so.EPI_FORMS[form]
    _run_all([c for c in so.epilogue_cases() if c[0].startswith("epilogue tile %d K %d " % (tile, K))], dev)


def test_split_k(dev):
    _run_all(so.split_cases(), dev)


def test_grouped_launches(dev):
    _run_all(so.grouped_cases(), dev)


def test_step_descriptors(dev):
    _run_all(so.all_step_cases(), dev)


def test_position_coded_integers(dev):
    _run_all(so.exact_cases(), dev)


def test_deferred_reduction(dev):
    """A launch of weight-gradient descs only leaves its split-K reduction pending under
    ``small_gemm_set_defer``; ``small_gemm_flush_pending`` runs it: C and asum bit-equal to the
    undeferred launch."""
    S = so.Spec
    specs = [S(72, 136, 800, a_mode=1, b_mode=1, a_bf16=False, lda_pad=0, asum=True),
             S(8, 72, 1200, a_mode=1, b_mode=1, lda_pad=0, asum=True, seed=1)]
    built = [so.build(s).to(dev) for s in specs]
    lib = native.lib()

    def fresh():
        bufs = [so.padded_c(s.M, s.N, s.N + 4, device=dev) + (torch.full((s.M,), float("nan"), device=dev),)
                for s in specs]
        return bufs, [b.gemm(C, b.spec.N + 4, a) for b, (_, C, a) in zip(built, bufs)]

    b0, g0 = fresh()
    assert [x[0] for x in so.dispatch(g0, 0)[1]] == [2, 3]
    ops.small_gemm(*g0)
    b1, g1 = fresh()
    assert not lib.small_gemm_flush_pending()
    lib.small_gemm_set_defer(True)
    try:
        ops.small_gemm(*g1)
        torch.cuda.synchronize()
        for (flat, C, a), s in zip(b1, specs):  # only partials so far: C and asum untouched
            so.check_padding(flat, C, 0, 0, s.N + 4, "deferred, before the flush")
            assert bool(torch.isnan(a).all())
        assert lib.small_gemm_flush_pending() is True  # pending was reported and has now run
        assert lib.small_gemm_flush_pending() is False
    finally:
        lib.small_gemm_set_defer(False)
        lib.small_gemm_flush_pending()
    for (f0, _, a0), (f1, _, a1) in zip(b0, b1):
        assert torch.equal(_bits(f0), _bits(f1)) and torch.equal(_bits(a0), _bits(a1))


def test_refusals_launch_nothing(dev):
    S = so.Spec
    b = so.build(S(64, 64, 72)).to(dev)
    bf = so.build(S(64, 64, 72, a_bf16=False, b_mode=1)).to(dev)
    flat, C = so.padded_c(64, 64, 64, device=dev)

    def refused(*gs, tile=0):
        with pytest.raises(RuntimeError):
            ops.small_gemm(*gs, tile=tile)
        torch.cuda.synchronize()
        so.check_padding(flat, C, 0, 0, 64, "refused launch")

    g = b.gemm(C, 64)
    refused(*([g] * 7))  # more than six descs
    blk = torch.zeros(72, 64, device=dev, dtype=torch.bfloat16)
    refused(Gemm(b.A, b.B, C, 64, 64, 72, b.lda, b.ldb, 64, kseg=36, bseg=(blk, blk)))  # kseg with b_mode 0
    refused(Gemm(b.A, b.B, C, 64, 64, 72, b.lda, b.ldb, 64, pdrop=0.2, drop_on=3, drop_ld=72))  # drop_ld % 16
    refused(Gemm(b.A, b.B, C, 64, 64, 72, b.lda, b.ldb, 64, pdrop=0.2, drop_on=1, drop_ld=80))  # drop_on 1, bf16 A
    refused(Gemm(b.A, b.B, C, 64, 64, 72, b.lda, b.ldb, 64, asum=torch.zeros(64, device=dev)))  # asum with a_mode 0
    refused(Gemm(b.A, b.B, C, 65, 64, 72, b.lda, b.ldb, 64))  # A too small
    refused(Gemm(b.A, b.B, C, 64, 65, 72, b.lda, b.ldb, 65))  # B too small
    refused(Gemm(bf.A, bf.B, C, 64, 64, 73, bf.lda, bf.ldb, 64, b_mode=1))  # B too small (K-major)
    small = torch.zeros(64 * 64 - 1, device=dev)
    refused(Gemm(b.A, b.B, small, 64, 64, 72, b.lda, b.ldb, 64))  # C too small
    assert so.dispatch([g], 1005)[0] == "refused"
    refused(g, tile=1005)  # register-direct with 5 k-steps in flight on an eligible launch
    ops.small_gemm(g, tile=1004)  # (the same launch with P = 4 runs)
    assert not torch.equal(C[:64], flat.new_full((64,), so.SENTINEL))


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_gather_dropout_bit_equal_to_cpu_path(dev, p):
    """The operand dropout of the oracle rests on the device forming the same fp32 product as the CPU
    path of ``ops.gather_dropout``: bit for bit, fp32 and bf16, with and without ``dev_off``."""
    gen = torch.Generator().manual_seed(3)
    for M in (1, 3, 130):
        for K in (4, 200, 400):
            n_src = M // 2 + 2
            v = torch.rand(n_src, K, generator=gen) * 2 - 1
            idx = so.make_gidx(M, n_src, gen)
            for off in (None, torch.tensor([7], dtype=torch.int64)):
                for bf in (False, True):
                    want = ops.gather_dropout(v, idx, p, 11, 3, off, bf)
                    got = ops.gather_dropout(v.to(dev), idx.to(dev), p, 11, 3, None if off is None else off.to(dev), bf)
                    assert got.dtype == want.dtype and torch.equal(_bits(got.cpu()), _bits(want)), (M, K, off, bf)


def test_tanhf_term(dev):
    """Re-measures the device ``tanhf`` through the kernel (an exact pre-activation, see the oracle
    module) and holds it to the recorded ``TANHF_MEASURED``; every form computes the same bits."""
    lo_, hi_, n = so.TANH_GRID
    x = torch.cat([torch.linspace(lo_, hi_, n, dtype=torch.float64).float(), torch.tensor(so.TANH_EDGES)])
    hi = x.to(torch.bfloat16)
    lo = x - hi.float()
    assert torch.equal(hi.float() + lo, x)  # the fp32 sum the epilogue forms is exactly x
    N = x.numel()
    A = torch.eye(8, dtype=torch.bfloat16, device=dev)
    B = hi.to(dev)[:, None].expand(N, 8).contiguous()
    bias = lo.to(dev)
    outs = []
    for tile in (6, 5, 1003, 0):  # (tile 0: 4,097 64 x 64 tiles -> the launcher picks 128 x 128)
        C = torch.zeros(8, N, device=dev)
        g = Gemm(A, B, C, 8, N, 8, 8, 8, N, bias=bias, act=1)
        assert so.dispatch([g], tile)[0] == {6: "ring2", 5: "regq", 1003: "rd03", 0: "tile4"}[tile]
        ops.small_gemm(g, tile=tile)
        outs.append(C)
        assert torch.equal(_bits(C), _bits(C[:1].expand(8, N)))
    assert all(torch.equal(_bits(outs[0]), _bits(o)) for o in outs[1:])
    want = torch.tanh(x.double().to(dev))
    err = (outs[0][0].double() - want).abs() / (so.U * want.abs().clamp(min=so.TANH_TINY))
    measured = float(err.max())
    print("\ntanhf: worst error %.4f U max(|y|, tiny) at x = %.9g (recorded %.4f, the bound uses %.1f x)"
          % (measured, float(x[int(err.argmax())]), so.TANHF_MEASURED, so.ACT_MARGIN))
    assert measured <= so.TANHF_MEASURED


def _colsum_pair(M, N, form, gen, dev):
    """(X view, out flat, out, ld): form 0 = the vector path when N % 4 == 0, 1 = a 1-float-offset view
    (scalar path), 2 = an odd ld (scalar path)."""
    ld = (N + 3) // 4 * 4 + 4 if form < 2 else N + 1 + N % 2
    off = 1 if form == 1 else 0
    buf = torch.full((off + M * ld + 4,), so.POISON)
    buf[off:off + M * ld].view(M, ld)[:, :N] = torch.rand(M, N, generator=gen) * 2 - 1
    flat = torch.full((N + 8,), so.SENTINEL, device=dev)
    return buf.to(dev)[off:], flat, flat[4:4 + N], ld


def _colsum_check(X, flat, out, M, N, ld, prior, what):
    ref, tol = so.colsum_oracle(X, M, N, ld, prior)
    s = torch.tensor(so.SENTINEL, device=flat.device)
    assert torch.equal(flat[:4], s.expand(4)) and torch.equal(flat[4 + N:], s.expand(4)), what + ": guard written"
    _note("colsum_f32", so.check(out, ref, tol, what))


@pytest.mark.parametrize("accumulate", [False, True])
def test_colsum_f32(dev, accumulate):
    gen = torch.Generator().manual_seed(5)
    for M in so.COLSUM_M:
        for N in so.COLSUM_N:
            for form in (0, 1, 2):
                X, flat, out, ld = _colsum_pair(M, N, form, gen, dev)
                prior = torch.randn(N, generator=gen).to(dev) if accumulate else None
                res = []
                for _ in range(2):
                    out.copy_(prior if accumulate else torch.full_like(out, float("nan")))
                    ops.colsum_f32([(X, out, M, N, ld)], accumulate=accumulate)
                    res.append(out.clone())
                assert torch.equal(_bits(res[0]), _bits(res[1]))
                _colsum_check(X, flat, out, M, N, ld, prior, "colsum M %d N %d form %d" % (M, N, form))


def test_colsum_f32_grouped(dev):
    """One launch mixing descs that are final after pass 1 (one row chunk) with many-chunk descs."""
    gen = torch.Generator().manual_seed(6)
    shapes = [(100, 260, 0), (513, 33, 2), (1, 1203, 2), (129, 256, 0), (128, 64, 1), (300, 1, 2)]
    items = [(M, N) + _colsum_pair(M, N, form, gen, dev) for M, N, form in shapes]
    ops.colsum_f32([(X, out, M, N, ld) for M, N, X, flat, out, ld in items])
    for M, N, X, flat, out, ld in items:
        _colsum_check(X, flat, out, M, N, ld, None, "grouped colsum M %d N %d" % (M, N))


def _wgrad_case(M, N, K, regime="", seed=0):
    dev = torch.device("cuda", 0)
    dy, x = (t.to(dev) for t in so.wgrad_inputs(M, N, K, regime, seed))
    plan = so.wgrad_plan(M, N, K, _cus())
    out = native.lib().wgrad(dy, x)
    assert out.dtype == torch.float32 and out.shape == (N, K)
    assert torch.equal(_bits(out), _bits(native.lib().wgrad(dy, x))), "wgrad not bitwise repeatable"
    ref, tol = so.wgrad_oracle(dy, x, plan["S"])
    what = "wgrad %dx%dx%d %s (S %d, %d rows in the last split)" % (M, N, K, regime, plan["S"], plan["last_rows"])
    if regime == "exact":
        assert torch.equal(out.double(), ref), what
    _note("wgrad S = 1" if plan["S"] == 1 else "wgrad S > 1", so.check(out, ref, tol, what))
    return plan


def test_wgrad_single_split_stage_counts(dev):
    """M = 1 .. 129: one to five 32-row stages of a single split -- the two-stage prologue part-filled,
    exactly filled, and the three-stage ring wrapping -- with one tile, a full tile and a partial
    second tile in N and K."""
    for M in so.WGRAD_M_SMALL:
        for N, K in so.WGRAD_NK:
            plan = _wgrad_case(M, N, K)
            assert plan["S"] == 1 and plan["scratch"] == 0 and plan["steps"] == -(-M // 32)


def test_wgrad_split_reduce(dev):
    seen = set()
    for N, K in ((264, 520), (8, 8), (256, 264)):
        for M in so.WGRAD_M_SPLIT + [so.shortest_last_split_m(N, K, _cus())]:
            plan = _wgrad_case(M, N, K)
            assert plan["scratch"] == (0 if plan["S"] == 1 else plan["S"] * N * K)
            seen.add(plan["S"] > 1)
    assert True in seen, "no case reached the partials + reduce path at %d CUs" % _cus()


@pytest.mark.parametrize("regime", ["col30", "zero", "exact"])
def test_wgrad_regimes(dev, regime):
    for M, N, K in ((97, 264, 248), (1025, 248, 264), (33, 8, 520)):
        _wgrad_case(M, N, K, regime)


def test_wgrad_zero_rows_and_refusal(dev):
    z = native.lib().wgrad(torch.zeros(0, 264, device=dev, dtype=torch.bfloat16),
                           torch.zeros(0, 8, device=dev, dtype=torch.bfloat16))
    assert z.shape == (264, 8) and int(torch.count_nonzero(z)) == 0
    dy, x = (t.to(dev) for t in so.wgrad_inputs(33, 12, 8))
    with pytest.raises(RuntimeError):
        native.lib().wgrad(dy, x)  # N % 8 != 0
    with pytest.raises(RuntimeError):
        native.lib().wgrad(x, dy)  # K % 8 != 0
