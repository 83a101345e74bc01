"""csrc/batch.hip (``dedup``, ``sample_batch``, ``multi_copy``) against exact integer twins, and every
segment-sum form of csrc/news_grad.hip -- plain, clipped, noised, both noise counter layouts --
against the fp64 oracle and its per-element bound (``tests/data_oracle.py``).  Every call is made
twice and must be bit-identical and finite.  The segments of the layout cases sit on the
16-position chunk grid on purpose and their occurrences are scattered through the rows;
``tests/test_data_oracle_cpu.py`` runs fp32 models and planted defects over the same cases.  The
reference is never another kernel form.  Each test prints its worst ratio (``-rP`` shows them)."""
import functools

import numpy as np
import pytest
import torch

import data_oracle as do
from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import native

pytestmark = pytest.mark.gpu

SEED, OFFSET = 11, 3
WIDTHS4 = (4, 36, 256, 260, 400, 512)  # float4 forms: D / 4 on both sides of 64
WIDTHS1 = (1, 63, 65, 398, 511)  # the scalar chunk form
MISALIGNED = "36 misaligned"  # a contiguous [R, 36] view 4 bytes off a 16-byte boundary: the fallback
ALL_FORMS = ((0, 3), (1, 3), (2, 0), (2, 1), (2, 2), (2, 3))  # (segsum variant, ldp_block bits)
SCALAR_FORMS = ((0, 3), (1, 3), (2, 3))


def report(what, worst):
    print("data-oracle ratio %-58s %.3f" % (what, worst))


def _twice(f):
    """Call twice: bit-identical and finite.  -> the first result (a tensor or a tuple)."""
    a, b = f(), f()
    ta = a if isinstance(a, (tuple, list)) else (a,)
    tb = b if isinstance(b, (tuple, list)) else (b,)
    assert len(ta) == len(tb)
    for x, y in zip(ta, tb):
        assert torch.equal(x, y), "a second call differs"
        assert bool(torch.isfinite(x.float()).all()), "a non-finite value"
    return a


def _i32(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(dev)


def _with_form(form, f):
    """The segsum switches are process-global: restored to the defaults even when the call fails."""
    lib = native.lib()
    lib.segsum_set_variant(form[0])
    lib.segsum_set_ldp_block(form[1])
    try:
        return f()
    finally:
        lib.segsum_set_variant(2)
        lib.segsum_set_ldp_block(3)


# =========================================================================== (a) dedup
def _check_dedup(dev, ids, num_news, what):
    t = _i32(dev, ids)
    got = _twice(lambda: ops.dedup(t, num_news))
    for name, g, w in zip(("uniq", "inv", "perm", "seg_ptr"), got, do.dedup_oracle(ids)):
        assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy().astype(np.int64), w), (what, name)


@pytest.mark.parametrize("R", [1, 2, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8191, 8192])
def test_dedup_exact(dev, R):
    """Register slots E = 1, 2, 4, 8; narrow keys up to num_news = 2^19 (id 2^19 - 1 at the last
    occurrence: the largest real key beside the pad key), wide keys from 2^19 + 1 (at R = 8192: the
    LDS form); flags on the thread-run and wave-run edges of the scan."""
    n = 0
    for num_news in (500, 1 << 19, (1 << 19) + 1, 3 << 20, 0):
        for pat in do.DEDUP_PATTERNS:
            if pat == "wide_max" and num_news != 0:
                continue
            _check_dedup(dev, do.dedup_ids(pat, R, num_news), num_news, (pat, R, num_news))
            n += 1
    print("data-oracle dedup R=%d: %d id lists exact" % (R, n))


def test_dedup_sort_path_exact(dev):
    """R = 8193: the sort path of the binding, the same contract."""
    for num_news in (500, 1 << 19, 0):
        for pat in ("equal", "descending", "random", "thread_runs", "top_last"):
            _check_dedup(dev, do.dedup_ids(pat, 8193, num_news), num_news, (pat, num_news))


# =========================================================================== (b) sample_batch
N_ROWS = 4200


@functools.lru_cache(maxsize=None)
def _csr(H):
    return do.sampler_csr(N_ROWS, H)


@pytest.mark.parametrize("H", [1, 50, 64, 65, 130])
@pytest.mark.parametrize("npratio", [1, 4, 16])
def test_sample_batch_exact(dev, npratio, H):
    pos, neg_ptr, negs, his_ptr, his = _csr(H)
    d = [torch.from_numpy(a).to(dev) for a in (pos, neg_ptr, negs, his_ptr, his)]
    lib = native.lib()
    n = 0
    for B in (1, 3, 4, 33):
        rows = (N_ROWS - 1 - np.arange(B) * 131) % N_ROWS  # ids on both sides of 4096, every count of the CSR
        if B > 1:
            rows[-1] = rows[0]  # a repeated row draws the same negatives
        rt = _i32(dev, rows)
        for seed, offset in ((0, 0), ((1 << 31) - 1, 1), ((1 << 40) + 7, (1 << 33) + 5)):
            for truncate in (True, False):
                for valid in (False, True):
                    cand, hist = _twice(lambda: lib.sample_batch(rt, d[0], d[1], d[2], d[3], d[4], npratio, H, truncate,
                                                                 seed, offset, valid))
                    wc, wh = do.sample_oracle(rows, pos, neg_ptr, negs, his_ptr, his, npratio, H, truncate, seed,
                                              offset, valid)
                    what = (B, seed, offset, truncate, valid)
                    assert cand.shape == (B, npratio + 1) and hist.shape == (B, H)
                    assert np.array_equal(cand.cpu().numpy(), wc), what
                    assert np.array_equal(hist.cpu().numpy(), wh), what
                    # the two halves of one buffer: the dedup reads [cand | his] without a copy
                    assert cand.untyped_storage().data_ptr() == hist.untyped_storage().data_ptr()
                    assert cand.storage_offset() == 0 and hist.storage_offset() == B * (npratio + 1)
                    assert cand.is_contiguous() and hist.is_contiguous()
                    n += 1
    print("data-oracle sample_batch npratio=%d H=%d: %d batches exact" % (npratio, H, n))


# =========================================================================== (c) multi_copy
SENTINEL = 0x5A5A5A5A


def _multi_copy_case(dev, n_dsts, n_srcs, fills, dtypes, slack=5):
    """Destinations are views inside one backing buffer with ``slack`` words after each; the
    backing words outside them must keep the sentinel."""
    rng = np.random.default_rng(len(n_dsts) * 1000 + sum(n_dsts))
    srcs = [rng.integers(-2 ** 31, 2 ** 31, size=ns).astype(np.int32) if dt == np.int32
            else rng.standard_normal(ns).astype(np.float32) for ns, dt in zip(n_srcs, dtypes)]
    want = do.multi_copy_oracle(srcs, n_dsts, fills)
    tdt = {np.int32: torch.int32, np.float32: torch.float32}
    backs = [torch.full((nd + 2 * slack,), SENTINEL, dtype=torch.int32, device=dev).view(tdt[dt])
             for nd, dt in zip(n_dsts, dtypes)]
    dsts = [b[slack:slack + nd] for b, nd in zip(backs, n_dsts)]
    st = [torch.from_numpy(s).to(dev) for s in srcs]

    def run():
        native.lib().multi_copy(st, dsts, list(fills))
        return tuple(b.view(torch.int32).clone() for b in backs)

    got = _twice(run)
    for g, w, nd in zip(got, want, n_dsts):
        g = g.cpu().numpy()
        assert np.array_equal(g[slack:slack + nd], w.view(np.int32)), "destination words"
        assert (g[:slack] == SENTINEL).all() and (g[slack + nd:] == SENTINEL).all(), "words outside a destination"


@pytest.mark.parametrize("dtype", [np.int32, np.float32])
@pytest.mark.parametrize("n", [1, 8])
def test_multi_copy_exact(dev, n, dtype):
    n_dsts = [1, 7, 256, 257, 1000, 3, 64, 4097][:n] if n > 1 else [301]
    fills = [7, -1, 1 << 30, -(1 << 31), 3521, -12345, 1, 99][:n]
    for mode in ("none", "one", "all", "mixed"):
        n_srcs = [{"none": 0, "one": 1, "all": nd, "mixed": (nd * (i + 1)) // 9}[mode] for i, nd in enumerate(n_dsts)]
        _multi_copy_case(dev, n_dsts, n_srcs, fills, [dtype] * n)
    if n == 8:  # both dtypes in one launch
        _multi_copy_case(dev, n_dsts, [nd // 2 for nd in n_dsts], fills, [np.int32, np.float32] * 4)


def test_multi_copy_grid_stride_wraps(dev):
    """More than 1024 blocks x 256 words in all: every thread takes a second trip."""
    n_dsts = [5, 300000, 17, 70001]
    assert sum(n_dsts) > 1024 * 256
    _multi_copy_case(dev, n_dsts, [5, 123457, 0, 70001], [-7, 11, -13, 17], [np.int32, np.float32, np.int32, np.int32])


# =========================================================================== (d) segment sums
def _dev_layout(dev, lay):
    return _i32(dev, lay.inv), _i32(dev, lay.perm), _i32(dev, lay.seg_ptr)


def _rows_on(dev, g, width):
    """``g`` on the device; the misaligned width as a contiguous view 4 bytes off 16-byte alignment."""
    t = torch.from_numpy(g)
    if width != MISALIGNED:
        out = t.to(dev)
        assert out.data_ptr() % 16 == 0
        return out
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev)
    buf[1:].copy_(t.reshape(-1).to(dev))
    out = buf[1:].view(t.shape)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


def _width_D(width):
    return 36 if width == MISALIGNED else width


def _forms(width):
    return ALL_FORMS if width in WIDTHS4 else SCALAR_FORMS


def _noise_layout(width, form):
    return "fused" if width in WIDTHS4 and form[0] == 2 else "rows"


def _segsum(rows, dl, U_pad, form, clip=0.0, std=0.0, seed=SEED, offset=OFFSET, dev_off=None):
    inv, perm, ptr = dl
    return _with_form(form, lambda: _twice(lambda: ops.segment_sum_rows(
        rows, inv, U_pad, clip=clip, noise_std=std, seed=seed, offset=offset, seg=(perm, ptr), zero_empty=True,
        dev_off=dev_off))).cpu().numpy()


@pytest.mark.parametrize("name", list(do.CASES))
def test_segment_sum_plain(dev, name):
    """Every width and form, 0 / 1 / 9 trailing empty segments: integer rows bit for bit, float rows
    inside the bound, one-occurrence segments their row exactly, empty segments exactly 0."""
    worst = {}
    for width in WIDTHS4 + WIDTHS1 + (MISALIGNED,):
        D = _width_D(width)
        lay0 = do.case_layout(name)
        gi, gf = do.int_rows(lay0.R, D), do.float_rows(lay0.R, D)
        ri, rf = _rows_on(dev, gi, width), _rows_on(dev, gf, width)
        for trailing in do.TRAILING:
            lay = do.case_layout(name, trailing)
            dl = _dev_layout(dev, lay)
            want_i = do.segsum_oracle(gi, lay.inv, lay.U_pad)
            want_f = do.segsum_oracle(gf, lay.inv, lay.U_pad)
            tol_f = do.segsum_tol(gf.astype(np.float64), np.zeros(gf.shape), lay.inv, lay.U_pad)
            ones = np.nonzero(np.diff(lay.seg_ptr) == 1)[0]
            for form in _forms(width):
                what = "%s D=%s +%d form %s" % (name, width, trailing, form)
                out = _segsum(ri, dl, lay.U_pad, form)
                assert out.shape == (lay.U_pad, D) and np.array_equal(out.astype(np.float64), want_i), what
                out = _segsum(rf, dl, lay.U_pad, form)
                w = do.check(out, want_f, tol_f, what)
                worst[form] = max(worst.get(form, 0.0), w)
                assert np.array_equal(out[ones], gf[lay.perm[lay.seg_ptr[ones]]]), what
                assert (out[lay.U:] == 0).all(), what
    for form, w in sorted(worst.items()):
        report("%s plain form %s" % (name, form), w)


MODES = (("clip 0.5", 0.5, 0.0), ("clip 2", 2.0, 0.0), ("noise", 0.0, 1.0), ("clip + noise", 0.5, 0.5))


@pytest.mark.parametrize("name", list(do.CASES))
def test_segment_sum_ldp(dev, name):
    """Clip only, noise only and both, every width and form, with and without the padded empty
    segments of the step graphs: each form against the oracle of the counter layout it uses.  The
    fused and the fallback forms draw different noise from the same seed."""
    worst = {}
    lay0 = do.case_layout(name)
    for width in WIDTHS4 + WIDTHS1 + (MISALIGNED,):
        D = _width_D(width)
        g = do.float_rows(lay0.R, D, 3, clip=0.5)
        rows = _rows_on(dev, g, width)
        layouts = sorted({_noise_layout(width, f) for f in _forms(width)})
        noise = {lo: do.ldp_noise_parts(lay0.R, D, SEED, OFFSET, lo) for lo in layouts}
        for mode, clip, std in MODES:
            orc = {lo: do.ldp_rows_oracle(g, clip, std, SEED, OFFSET, lo, noise=noise[lo]) for lo in layouts}
            for trailing in (0, 9):
                lay = do.case_layout(name, trailing)
                dl = _dev_layout(dev, lay)
                ref = {lo: (do.segsum_oracle(t, lay.inv, lay.U_pad), do.segsum_tol(t, e_t, lay.inv, lay.U_pad))
                       for lo, (t, e_t) in orc.items()}
                outs = {}
                for form in _forms(width):
                    lo = _noise_layout(width, form)
                    what = "%s D=%s +%d %s form %s (%s)" % (name, width, trailing, mode, form, lo)
                    out = _segsum(rows, dl, lay.U_pad, form, clip, std)
                    w = do.check(out, ref[lo][0], ref[lo][1], what)
                    key = (mode, form[0], lo) if form[0] != 2 else (mode, form, lo)
                    worst[key] = max(worst.get(key, 0.0), w)
                    assert (out[lay.U:] == 0).all(), what
                    outs[form] = out
                if std > 0 and len(layouts) == 2 and D >= 36:  # same seed, two layouts: two fields
                    assert (outs[(2, 3)][:lay.U] != outs[(1, 3)][:lay.U]).mean() > 0.9, (width, mode)
    for key, w in sorted(worst.items(), key=str):
        report("%s %s form %s (%s)" % (name, key[0], key[1], key[2]), w)


@pytest.mark.parametrize("layout,R,D", [("fused", 4096, 400), ("rows", 1024, 398)])
def test_noise_probe(dev, layout, R, D):
    """Rows 0, clip 0, std 1, one occurrence per segment: the output is the noise field itself.
    Measures the hardware sine / cosine term (``data_oracle.E_TRIG_MEASURED`` records it) and holds
    every element to the draw of its own counter under the tolerance in use, which must not exceed
    2^-12 whatever was measured."""
    rows = torch.zeros(R, D, device=dev)
    inv = torch.arange(R, device=dev, dtype=torch.int32)
    perm, ptr = ops.segments_from_inv(inv, R)
    out = _twice(lambda: ops.segment_sum_rows(rows, inv, R, clip=0.0, noise_std=1.0, seed=SEED, offset=OFFSET,
                                              seg=(perm, ptr))).cpu().numpy()
    z, rad = do.ldp_noise_parts(R, D, SEED, OFFSET, layout)
    key = "%s R=%d D=%d" % (layout, R, D)
    e = do.measure_e_trig(out, z, rad)
    print("data-oracle E_TRIG measured %-22s %.4g (recorded %.4g, in use %.4g, cap %.4g)"
          % (key, e, do.E_TRIG_MEASURED[key], do.E_TRIG, do.E_TRIG_CAP))
    assert do.E_TRIG == 4 * max(do.E_TRIG_MEASURED.values()) and do.E_TRIG <= do.E_TRIG_CAP
    report("noise probe %s" % key, do.check(out, z, do.noise_tol(z, rad), key))
    assert e <= do.E_TRIG_MEASURED[key] * 1.0000001, "the recorded E_TRIG_MEASURED is below this run's"
    other = do.ldp_noise(R, D, SEED, OFFSET, "rows" if layout == "fused" else "fused")
    assert (do.elem_ratio(out, other, do.noise_tol(z, rad)) > 1).mean() > 0.9  # not the other layout's field


@pytest.mark.parametrize("width", [400, 398])
def test_device_offset_adds_to_the_host_offset(dev, width):
    """``dev_off = [7]`` with ``offset = 5`` is ``offset = 12`` bit for bit and matches the oracle of
    offset 12; the same above 2^32 (counter word c3)."""
    lay = do.case_layout("crossing_70_chunks", 9)
    dl = _dev_layout(dev, lay)
    g = do.float_rows(lay.R, width, 5, clip=0.5)
    rows = _rows_on(dev, g, width)
    lo = _noise_layout(width, (2, 3))
    seven = torch.tensor([7], dtype=torch.int64, device=dev)
    for base in (0, 1 << 32):
        a = _segsum(rows, dl, lay.U_pad, (2, 3), 0.5, 0.5, offset=base + 5, dev_off=seven)
        b = _segsum(rows, dl, lay.U_pad, (2, 3), 0.5, 0.5, offset=base + 12)
        c = _segsum(rows, dl, lay.U_pad, (2, 3), 0.5, 0.5, offset=base + 5)
        assert np.array_equal(a, b) and not np.array_equal(a, c)
        t, e_t = do.ldp_rows_oracle(g, 0.5, 0.5, SEED, base + 12, lo)
        w = do.check(a, do.segsum_oracle(t, lay.inv, lay.U_pad), do.segsum_tol(t, e_t, lay.inv, lay.U_pad), lo)
        report("dev_off D=%d offset %d + 7 (%s)" % (width, base + 5, lo), w)
    big = torch.tensor([(1 << 32) + 7], dtype=torch.int64, device=dev)  # the device counter itself above 2^32
    a = _segsum(rows, dl, lay.U_pad, (2, 3), 0.5, 0.5, offset=5, dev_off=big)
    assert np.array_equal(a, b)


def test_wide_rows_are_refused(dev):
    """D = 516 is past the 512 columns a wave holds: an error, not a partial sum."""
    lay = do.case_layout("15_2_15")
    dl = _dev_layout(dev, lay)
    rows = torch.zeros(lay.R, 516, device=dev)
    for kw in ({}, {"clip": 0.5}, {"noise_std": 1.0}):
        with pytest.raises(RuntimeError):
            ops.segment_sum_rows(rows, dl[0], lay.U, seg=(dl[1], dl[2]), **kw)
    torch.cuda.synchronize()
