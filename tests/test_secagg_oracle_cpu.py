"""The oracle of tests/test_secagg_oracle_gpu.py checked on the CPU (``tests/secagg_oracle.py``):

* with no peers the twins equal the independent host formulations of ``parallel/secagg.py``
  (``hist_local``, ``hist_frac_bits``, ``quantize_ref``, ``dequantize_ref``);
* W oracle clients' histograms and payloads cancel to ``sum_k round(x_k 2^f)`` exactly, and no case
  input reaches the int32 wrap that the choice of f exists to exclude;
* the masks do what a mask must: nearly every word of an upload differs from ``Q(x)``, the bits are
  balanced, and the streams of two pairs, two rounds, two (step, bucket) rounds and the histogram
  and payload spaces share no more words than chance allows;
* each planted defect changes the twin's output on at least one named case of the GPU file (printed:
  ``-rP`` shows them), so the GPU comparison can see what it is there to see."""
import numpy as np
import pytest
import torch

import secagg_oracle as so
from fedrec_with_pytorchdistributed_amd.parallel import secagg

SMALL = 4099


# ================================================================================ independent checks
def test_hist_twin_without_peers_is_hist_local():
    n = 0
    for case in so.HIST_CASES:
        if case.npeers or case.n == 0 or case.n > SMALL:
            continue
        x = so.hist_input(case)
        want = secagg.hist_local(torch.from_numpy(x.copy()))
        assert np.array_equal(so.hist_want(case).astype(np.int64), want), case.name
        n += 1
    assert n > 100
    # the slot rule at every binade edge against the host's hist_slot
    for e in range(-149, 128):
        for v in (np.float32(2.0 ** e), np.nextafter(np.float32(2.0 ** e), np.float32(0)), np.float32(1.5 * 2.0 ** e)):
            h = so.hist_plain(np.array([0.0, -v], dtype=np.float32))
            assert int(np.nonzero(h)[0][0]) == secagg.hist_slot(float(v)) and h.sum() == 1, float(v)
    assert int(np.nonzero(so.hist_plain(np.array([so.FLT_MAX])))[0][0]) == 255
    assert int(np.nonzero(so.hist_plain(np.zeros(0, np.float32)))[0][0]) == 0  # the kernel's n = 0


def test_hist_scale_twin_is_hist_frac_bits():
    for W in so.EXACT_W + (6, 7, 16, 17, 1000, (1 << 23) - 1, (1 << 23) + 1):
        for name in so.EXACT_HISTS:
            H = so.exact_hist(name)
            assert so.hist_scale_twin(H, W) == secagg.hist_frac_bits(H, W), (W, name)
        for s in range(2, so.HB):
            H = np.zeros(so.HB, dtype=np.int32)
            H[s] = 1
            assert so.hist_scale_twin(H, W) == secagg.hist_frac_bits(H, W), (W, s)
    assert [so.ceil_log2(W) for W in (1, 2, 3, 4, 5, 8, 9, 64, 65, 1 << 23)] == [0, 1, 2, 2, 3, 3, 4, 6, 7, 23]
    # both clamps are reached by the hand-built histograms
    assert so.hist_scale_twin(so.exact_hist("f60_clamp"), 1)[0] == 60
    assert so.hist_scale_twin(so.exact_hist("f-120_clamp"), 1 << 23)[0] == -120
    assert so.hist_scale_twin(so.exact_hist("huge"), 1)[0] == -98  # the star upload's smallest f


def test_quantizers_without_peers_are_the_host_references():
    n = 0
    for case in so.MASK_CASES:
        if case.npeers or case.n > SMALL:
            continue
        x = so.mask_input(case)
        want = secagg.quantize_ref(torch.from_numpy(x.copy()), case.f, case.clip).numpy()
        assert np.array_equal(so.mask_want(case), want), case.name
        n += 1
    for case in so.EXACT_CASES:
        if case.npeers or case.n > SMALL:
            continue
        x, H = so.exact_input(case)
        f, _ = secagg.hist_frac_bits(H, case.W)
        v = torch.from_numpy(x.copy())
        v = torch.where(torch.isfinite(v), v, torch.zeros_like(v))
        want = torch.round(v.double() * 2.0 ** f).to(torch.int64).numpy()  # the host protocol's line
        assert np.array_equal(so.exact_want(case).astype(np.int64), want), case.name
        n += 1
    assert n > 300


def test_unmask_twins_are_dequantize_ref():
    for case in so.UNMASK_CASES:
        if case.n > SMALL:
            continue
        q = so.unmask_input(case.n)
        want = secagg.dequantize_ref(torch.from_numpy(q.copy()), case.f).numpy()
        assert np.array_equal(so.bits(so.unmask_twin(q, 2.0 ** -case.f)), so.bits(want)), case.name
    for case in so.UNMASK_EXACT_CASES:
        if case.n > SMALL:
            continue
        q, H = so.unmask_input(case.n), so.exact_hist(case.hist)
        f, bad = secagg.hist_frac_bits(H, case.W)
        got = so.unmask_exact_twin(q, H, case.W)
        if bad:
            assert np.isnan(got).all() and (so.bits(got) == so.NAN_BITS).all(), case.name
        else:
            with np.errstate(over="ignore"):
                want = (q.astype(np.float64) * 2.0 ** -f).astype(np.float32)  # one rounding here, two there:
            ok = np.abs(q.astype(np.int64)) <= 1 << 24  # equal where the conversion is exact
            assert np.array_equal(so.bits(got)[ok], so.bits(want)[ok]), case.name
            assert np.array_equal(so.bits(got), so.bits(secagg.dequantize_ref(torch.from_numpy(q.copy()), f).numpy()))
    # 2^120 q overflows to inf exactly from |q| = 2^8 on
    H = so.exact_hist("f-120_clamp")
    out = so.unmask_exact_twin(np.array([255, 256, -256, 2 ** 31 - 1], dtype=np.int32), H, 1 << 23)
    assert np.isfinite(out[0]) and out[1] == np.inf and out[2] == -np.inf and out[3] == np.inf


@pytest.mark.parametrize("W", so.CPU_FLEET_W)
def test_oracle_clients_cancel_to_the_plain_quantized_sum(W):
    for nonfinite in (False, True):
        xs = so.fleet_inputs(W, nonfinite=nonfinite)
        seeds = secagg.pair_seeds(W, 3) if W <= 9 else so.random_seeds(W)
        rnd = 7 * 4096 + 2
        hs, H, f, ups, total, out = so.fleet_exact(xs, seeds, rnd)
        plain = so.wrap_sum([so.hist_plain(x).view(np.int32) for x in xs])
        assert np.array_equal(H, plain) and f == 30 - so.ceil_log2(W) - 10
        want = so.plain_quantized_sum(xs, f)
        assert np.abs(want).max() <= 1 << 30  # the no-wrap condition
        assert np.array_equal(total.astype(np.int64), want)
        if nonfinite:
            assert np.isnan(out).all() and H[1] == 2
        else:
            assert np.array_equal(so.bits(out), so.bits(np.ldexp(want.astype(np.float64), -f).astype(np.float32)))
            for i in range(W if W > 1 else 0):  # masked: neither stage shows a client's own values
                assert (hs[i] != so.hist_plain(xs[i]).view(np.int32)).sum() >= so.HB - 1
                assert (ups[i] != so.quantize_exact(xs[i], f).view(np.int32)).sum() >= xs[i].size - 1


def test_clamped_oracle_clients_cancel():
    for W in so.CPU_FLEET_W:
        xs = so.fleet_inputs(W, salt=1)
        seeds = so.random_seeds(W, 1)
        ups = [so.mask_twin(xs[i], 2.0 ** 16, 1024.0, *so.peers_of(i, seeds[i]), 5) for i in range(W)]
        want = sum(so.quantize_clamped(x, 2.0 ** 16, 1024.0).view(np.int32).astype(np.int64) for x in xs)
        assert np.array_equal(so.wrap_sum(ups).astype(np.int64), want)


def test_no_case_input_can_wrap():
    """|Q(x)| <= 2^30 on every single-client case (the fleets: the test above).  At the f = -120 clamp
    W = 2^23 such clients could wrap (module docstring); one cannot."""
    for case in so.MASK_CASES:
        if case.n <= SMALL:
            q = so.quantize_clamped(so.mask_input(case), 2.0 ** case.f, case.clip).view(np.int32).astype(np.int64)
            assert np.abs(q).max() <= 1 << 30, case.name
    for case in so.EXACT_CASES:
        if case.n <= SMALL:
            x, H = so.exact_input(case)
            q = so.quantize_exact(x, so.hist_scale_twin(H, case.W)[0]).view(np.int32).astype(np.int64)
            assert np.abs(q).max() <= 1 << 30, case.name


# ================================================================================ the masks are masks
N_WORDS = 1 << 14


def _stream(seed, rnd, n=N_WORDS):
    return so.element_mask([seed], [1], rnd, n)


def _balanced(words):
    ones = int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())
    nbits = 32 * words.size
    return abs(ones - nbits / 2) <= 5 * np.sqrt(nbits) / 2


def test_uploads_differ_from_the_plaintext_and_are_balanced():
    """P(a mask word is 0) = 2^-32: more than one equal word among <= 4099 is a 1e-11 event."""
    n = 0
    for case in so.MASK_CASES:
        if case.npeers and case.n == SMALL:
            up, q = so.mask_want(case), so.quantize_clamped(so.mask_input(case), 2.0 ** case.f, case.clip)
            assert (up.view(np.uint32) == q).sum() <= 1 and _balanced(up), case.name
            n += 1
    for case in so.EXACT_CASES:
        if case.npeers and case.n == SMALL:
            x, H = so.exact_input(case)
            up, q = so.exact_want(case), so.quantize_exact(x, so.hist_scale_twin(H, case.W)[0])
            assert (up.view(np.uint32) == q).sum() <= 1 and _balanced(up), case.name
            n += 1
    for case in so.HIST_CASES:
        if case.npeers and case.n == SMALL:
            up = so.hist_want(case)
            assert (up == so.hist_plain(so.hist_input(case)).view(np.int32)).sum() <= 1 and _balanced(up), case.name
            n += 1
    assert n > 200


def test_streams_are_unrelated():
    """Two streams of 2^14 words agree at a position with probability 2^-32 each: at most one
    coincidence (P(two) ~ 7e-12), at the same positions and shifted by one word or one call."""
    s = so.random_seeds(3)
    pairs = {
        "two pairs": (_stream(s[0, 1], 3), _stream(s[0, 2], 3)),
        "two special seeds": (_stream(so.SPECIAL_SEEDS[0], 3), _stream(so.SPECIAL_SEEDS[2], 3)),
        "seeds differing in the high word only": (_stream(s[0, 1], 3), _stream(int(s[0, 1]) ^ (1 << 40), 3)),
        "two rounds": (_stream(s[0, 1], 3), _stream(s[0, 1], 4)),
        "rounds differing in the high word only": (_stream(s[0, 1], 5), _stream(s[0, 1], (1 << 32) + 5)),
        "two buckets of a step": (_stream(s[0, 1], 9 * 4096 + 0), _stream(s[0, 1], 9 * 4096 + 1)),
        "one bucket in two steps": (_stream(s[0, 1], 9 * 4096 + 1), _stream(s[0, 1], 10 * 4096 + 1)),
        "histogram and payload spaces": (_stream(s[0, 1], so.HIST_ROUND | 3), _stream(s[0, 1], 3)),
        "clamped and exact layouts": (so.net_mask([int(s[0, 1])], [1], 3, N_WORDS)[:, 0], _stream(s[0, 1], 3)),
    }
    for name, (a, b) in pairs.items():
        assert _balanced(a) and _balanced(b), name
        for shift in (0, 1, 4):
            assert int((a[shift:] == b[:a.size - shift]).sum()) <= 1, (name, shift)
    # the (step, bucket) rounds reducer.py forms stay distinct, and clear of the histogram space
    rounds = {step * 4096 + b for step in range(64) for b in range(64)}
    assert len(rounds) == 64 * 64 and max(rounds) < so.HIST_ROUND
    # a pair's two ends draw the same words with opposite signs
    a = so.element_mask([int(s[0, 1])], [1], 3, 1000) + so.element_mask([int(s[1, 0])], [-1], 3, 1000)
    assert not a.any()


# ================================================================================ planted defects
def _seen_by(defect):
    """Names of the (small) GPU cases whose expected output the defect changes."""
    seen = []
    for cases, want in ((so.MASK_CASES, so.mask_want), (so.HIST_CASES, so.hist_want), (so.EXACT_CASES, so.exact_want)):
        for case in cases:
            if case.n > SMALL or (case.npeers == 64 and len(seen) > 3):
                continue
            if not np.array_equal(want(case), want(case, defect)):
                seen.append(case.name)
    for case in so.UNMASK_EXACT_CASES:
        if case.n <= SMALL:
            q, H = so.unmask_input(case.n), so.exact_hist(case.hist)
            if not np.array_equal(so.bits(so.unmask_exact_twin(q, H, case.W)),
                                  so.bits(so.unmask_exact_twin(q, H, case.W, defect))):
                seen.append(case.name)
    return seen


@pytest.mark.parametrize("defect", so.DEFECTS)
def test_planted_defect_is_seen_by_a_named_gpu_case(defect):
    seen = _seen_by(defect)
    print("secagg-oracle defect %-22s seen by %4d cases, first: %s" % (defect, len(seen), seen[:1]))
    assert seen, defect
    kinds = {s.split()[0] for s in seen}
    expect = {
        "word_reversed": {"mask", "hist", "exact"}, "counter_is_element": {"hist", "exact"},
        "sign_flipped": {"mask", "hist", "exact"}, "seed_hi_dropped": {"mask", "hist", "exact"},
        "round_hi_dropped": {"mask", "hist", "exact"}, "trunc": {"mask", "exact"}, "half_away": {"mask", "exact"},
        "floor_log2": {"exact", "unmask_exact"}, "slot_pow2_off_by_one": {"hist"}, "nonfinite_kept": {"exact"},
        "tail_unmasked": {"exact"}, "zero_mask": {"mask", "hist", "exact"},
    }[defect]
    assert expect <= kinds, (defect, kinds)


def test_fleet_sees_the_defects_too():
    """The one-device fleets of the GPU file: a defect on one side of a pair breaks the cancellation."""
    xs, seeds = so.fleet_inputs(5), so.random_seeds(5)
    good = so.fleet_exact(xs, seeds, 3)
    for defect in ("sign_flipped", "word_reversed", "counter_is_element", "tail_unmasked", "floor_log2", "trunc"):
        bad = so.fleet_exact(xs, seeds, 3, defect)
        assert any(not np.array_equal(a, b) for a, b in zip(good[3], bad[3])), defect
