"""csrc/secagg.hip against the exact Philox twins of ``tests/secagg_oracle.py``: every word of every
upload equals ``Q(x)`` plus the pairwise Philox masks, every histogram its one-hot plus the masks of the
``2^62 | r`` space, every dequantised value the same fp32 bits -- no tolerance, no sampling.  The cases
(sizes on both sides of a block, a wave, a 4-element group and the first grid-stride trip; 0 / 1 / 3 / 64
peers of mixed signs; seeds and rounds with busy and empty high words; both clamps of f; ties, bounds,
non-finite coordinates) are the lists of the oracle module; ``tests/test_secagg_oracle_cpu.py`` checks the
twins against independent formulations and shows that each planted defect changes a named case.  Then W
clients through the kernels on one device, and ``ExactMasker.allreduce_`` as one device client among
W - 1 oracle clients."""
import numpy as np
import pytest
import torch

import secagg_oracle as so
from fedrec_with_pytorchdistributed_amd.ops import native
from fedrec_with_pytorchdistributed_amd.parallel import secagg

pytestmark = pytest.mark.gpu


def _peers(dev, seeds, signs):
    return (torch.tensor(list(seeds), dtype=torch.int64, device=dev),
            torch.tensor(list(signs), dtype=torch.int32, device=dev))


def _np(t):
    return t.detach().cpu().numpy()


class _Upload:
    """The last input moved to the device, kept while consecutive cases share it."""

    def __init__(self, dev):
        self.dev, self.key, self.t = dev, None, None

    def __call__(self, a):
        if self.key is not a:
            self.key, self.t = a, torch.from_numpy(np.array(a)).to(self.dev)
        return self.t


def _same_words(got, want, what):
    got = _np(got[0] if isinstance(got, (tuple, list)) else got)  # ``-> (Tensor)`` ops
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.nonzero(so.bits(got) != so.bits(want))[0]
    assert bad.size == 0, "%s: %d of %d words differ, first at %d: %#x != %#x" % (
        what, bad.size, want.size, bad[0], so.bits(got)[bad[0]], so.bits(want)[bad[0]])


# ================================================================================ mask / unmask
@pytest.mark.parametrize("n", so.MASK_SMALL_N + (so.MASK_BIG_N,))
def test_mask_is_q_plus_philox(dev, n):
    lib, up, k = native.lib(), _Upload(dev), 0
    for case in so.MASK_CASES:
        if case.n != n:
            continue
        sd, sg = _peers(dev, *so.peers(case.npeers))
        got = lib.secagg_mask(up(so.mask_input(case)), sd, sg, 2.0 ** case.f, case.clip, case.rnd)
        _same_words(got, so.mask_want(case), case.name)
        k += 1
    print("secagg-oracle mask n=%d: %d cases exact" % (n, k))
    assert k == (3 if n == so.MASK_BIG_N else 80)


@pytest.mark.parametrize("W", [1, 2, 4])
def test_mask_local_as_the_star_upload_calls_it(dev, W):
    """``mask_local(u, k, W, row, r, f, bound)``: the peers and signs it derives from a seed row, with
    ``clip`` the agreed bound 2^E and f from -98 to 60."""
    seeds = so.random_seeds(W, 2)
    for f, clip in so.MASK_GRIDS:
        for n in (257, 4099):
            x = so._mask_input(n, f, clip)
            for i in range(W):
                for rnd in (3, (1 << 32) + 5):
                    got = secagg.mask_local(torch.from_numpy(x.copy()).to(dev).view(1, n), i, W, seeds[i], rnd, f, clip)
                    want = so.mask_twin(x, 2.0 ** f, clip, *so.peers_of(i, seeds[i]), rnd)
                    _same_words(got.view(-1), want, ("mask_local", W, i, f, n, rnd))


def test_unmask_is_the_fp32_product(dev):
    lib, up = native.lib(), _Upload(dev)
    for case in so.UNMASK_CASES:
        q = so.unmask_input(case.n)
        _same_words(lib.secagg_unmask(up(q), 2.0 ** -case.f), so.unmask_twin(q, 2.0 ** -case.f), case.name)
        if case.f == 16:
            _same_words(secagg.unmask_sum(up(q)), so.unmask_twin(q, 2.0 ** -16), case.name + " unmask_sum")


# ================================================================================ hist
@pytest.mark.parametrize("n", so.HIST_N)
def test_hist_is_one_hot_plus_philox(dev, n):
    lib, up, k = native.lib(), _Upload(dev), 0
    for case in so.HIST_CASES:
        if case.n != n:
            continue
        sd, sg = _peers(dev, *so.peers(case.npeers, salt=1))
        got = lib.secagg_hist(up(so.hist_input(case)), sd, sg, case.rnd)
        _same_words(got, so.hist_want(case), case.name)
        k += 1
    print("secagg-oracle hist n=%d: %d cases exact" % (n, k))
    assert k >= 42


# ================================================================================ mask_exact / unmask_exact
@pytest.mark.parametrize("n", so.EXACT_SMALL_N + (so.EXACT_BIG_N,))
def test_mask_exact_is_q_plus_philox(dev, n):
    lib, up, k = native.lib(), _Upload(dev), 0
    for case in so.EXACT_CASES:
        if case.n != n:
            continue
        x, H = so.exact_input(case)
        sd, sg = _peers(dev, *so.peers(case.npeers, salt=2))
        got = lib.secagg_mask_exact(up(x), sd, sg, torch.from_numpy(H).to(dev), case.W, case.rnd)
        _same_words(got, so.exact_want(case), case.name)
        k += 1
    print("secagg-oracle mask_exact n=%d: %d cases exact" % (n, k))
    assert k >= 3


GUARD = 3  # elements on either side of ``out``: the view starts 12 bytes off a 16-byte boundary
SENTINEL = 0x7FA5A5A5  # a NaN pattern no result can hold


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 4099, so.EXACT_BIG_N])
def test_unmask_exact_fills_its_view_and_nothing_else(dev, n):
    lib, up, k = native.lib(), _Upload(dev), 0
    for case in so.UNMASK_EXACT_CASES:
        if case.n != n:
            continue
        q, H = so.unmask_input(n), so.exact_hist(case.hist)
        buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
        lib.secagg_unmask_exact_(up(q), torch.from_numpy(H).to(dev), case.W, buf[GUARD:GUARD + n])
        got = _np(buf.view(torch.int32))
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + n:] == SENTINEL).all(), case.name
        _same_words(buf[GUARD:GUARD + n], so.unmask_exact_twin(q, H, case.W), case.name)
        k += 1
    assert k >= 4


# ================================================================================ one device, W clients
@pytest.mark.parametrize("W", so.FLEET_W)
def test_w_clients_on_one_device_sum_exactly(dev, W):
    """hist -> SUM -> mask_exact -> SUM -> unmask_exact with every client's kernels on this device and
    the wrap-around adds in torch int32; then the clamped kernel the same way."""
    lib = native.lib()
    xs, seeds, rnd = so.fleet_inputs(W), so.random_seeds(W), 11 * 4096 + 3
    hs, H, f, ups, total, out = so.fleet_exact(xs, seeds, rnd)
    dx = [torch.from_numpy(x).to(dev) for x in xs]
    arr = []
    for i in range(W):
        _, sd, sg = secagg._peer_arrays(i, seeds[i])
        assert sd.numel() == min(W - 1, so.MAXP + 1)
        arr.append((sd.to(dev), sg.to(dev)))
    dh = [lib.secagg_hist(dx[i], *arr[i], so.HIST_ROUND | rnd) for i in range(W)]
    for i in range(W):
        _same_words(dh[i], hs[i], ("hist of client", i))
    dH = dh[0].clone()
    for t in dh[1:]:
        dH += t  # int32 wrap-around, as the SUM all-reduce
    _same_words(dH, so.wrap_sum([so.hist_plain(x).view(np.int32) for x in xs]), "summed histogram")
    dq = [lib.secagg_mask_exact(dx[i], *arr[i], dH, W, rnd) for i in range(W)]
    for i in range(W):
        _same_words(dq[i], ups[i], ("upload of client", i))
    dtot = dq[0].clone()
    for t in dq[1:]:
        dtot += t
    got = torch.empty(so.FLEET_N, device=dev)
    lib.secagg_unmask_exact_(dtot, dH, W, got)
    _same_words(got, out, "dequantised sum")
    want = np.ldexp(so.plain_quantized_sum(xs, f).astype(np.float64), -f).astype(np.float32)
    _same_words(got, want, "sum_k round(x_k 2^f) 2^-f")
    # the clamped kernels through their host wrappers
    dtot = None
    for i in range(W):
        m = secagg.mask_local(dx[i], i, W, seeds, 5)
        _same_words(m, so.mask_twin(xs[i], 2.0 ** 16, 1024.0, *so.peers_of(i, seeds[i]), 5), ("clamped upload", i))
        dtot = m.clone() if dtot is None else dtot + m
    plain = sum(so.quantize_clamped(x, 2.0 ** 16, 1024.0).view(np.int32).astype(np.int64) for x in xs)
    _same_words(secagg.unmask_sum(dtot), so.unmask_twin(plain.astype(np.int32), 2.0 ** -16), "clamped sum")


def test_more_peers_than_a_launch_holds_are_refused(dev):
    """MAXP + 1 = 65 peers (W = 66), and W < 1: the binding's error, nothing launched."""
    lib = native.lib()
    x = torch.ones(8, device=dev)
    sd, sg = _peers(dev, *so.peers(so.MAXP + 1))
    H = torch.from_numpy(so.exact_hist("natural")).to(dev)
    with pytest.raises(RuntimeError, match="secagg_mask: unsupported shape"):
        lib.secagg_mask(x, sd, sg, 65536.0, 1024.0, 3)
    with pytest.raises(RuntimeError, match="secagg_hist: unsupported shape"):
        lib.secagg_hist(x, sd, sg, 3)
    with pytest.raises(RuntimeError, match="secagg_mask_exact: unsupported shape"):
        lib.secagg_mask_exact(x, sd, sg, H, 66, 3)
    with pytest.raises(RuntimeError, match="secagg_mask_exact: unsupported shape"):
        lib.secagg_mask_exact(x, sd[:3], sg[:3], H, 0, 3)
    out = torch.full((8,), 7.0, device=dev)
    with pytest.raises(RuntimeError, match="secagg_unmask_exact_: unsupported shape"):
        lib.secagg_unmask_exact_(torch.ones(8, dtype=torch.int32, device=dev), H, 0, out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(RuntimeError):
        secagg.mask_local(x, 0, so.MAXP + 2, so.random_seeds(so.MAXP + 2), 3)
    # MAXP itself is accepted (W = 65 in the fleet test); here at the clamped kernel's smallest size
    sd, sg = _peers(dev, *so.peers(so.MAXP))
    got = lib.secagg_mask(x[:1], sd, sg, 65536.0, 1024.0, 3)
    _same_words(got, so.mask_twin(np.ones(1, np.float32), 65536.0, 1024.0, *so.peers(so.MAXP), 3), "MAXP peers")


# ================================================================================ ExactMasker among oracle clients
class _OracleClients:
    """Stands in for the IPC all-reduce: adds, wrap-around, what the W - 1 oracle clients upload --
    the histograms at the first call, the payloads at the second."""

    def __init__(self, dev, parts):
        self.parts, self.calls = [torch.from_numpy(np.array(p)).to(dev) for p in parts], 0

    def allreduce_(self, t):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == self.parts[self.calls].numel()
        t += self.parts[self.calls]
        self.calls += 1


MASKER_N = 4099
BLOCK = (82, 50)  # the "block" form: the left half of an [82, 100] buffer, which no 1-D view covers


def _masker_round(dev, W, me, rnd, form, nonfinite=False):
    n = BLOCK[0] * BLOCK[1] if form == "block" else MASKER_N
    xs = so.fleet_inputs(W, n, nonfinite=nonfinite, salt=W)
    assert not nonfinite or me != W - 1  # the non-finite coordinates belong to an oracle client
    if form == "bf16":
        xs[me] = torch.from_numpy(xs[me]).bfloat16().float().numpy()
    seeds = secagg.pair_seeds(W, 21) if W <= 9 else so.random_seeds(W, 3)
    hs, H, f, ups, total, out = so.fleet_exact(xs, seeds, rnd)
    others = [k for k in range(W) if k != me]
    ipc = _OracleClients(dev, [so.wrap_sum([hs[k] for k in others]), so.wrap_sum([ups[k] for k in others])]
                         if others else [np.zeros(so.HB, np.int32), np.zeros(n, np.int32)])
    masker = secagg.ExactMasker(me, W, seeds[me], dev)
    x = torch.from_numpy(xs[me].copy()).to(dev)
    base = None
    if form == "fp32":
        g = x.view(n)
    elif form == "bf16":
        g = x.bfloat16()
    else:  # part of a buffer whose other elements must keep their bits
        base = torch.full((2 * n,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
        g = base[::2] if form == "strided" else base.view(BLOCK[0], 2 * BLOCK[1])[:, :BLOCK[1]]
        g.copy_(x.view(g.shape))
        assert not g.is_contiguous()
    masker.allreduce_(g, rnd, None, ipc=ipc)
    assert ipc.calls == 2
    _same_words(masker.hist, so.wrap_sum([so.hist_plain(v).view(np.int32) for v in xs]), "summed histogram")
    assert masker.frac_bits() == f
    if form == "bf16":
        want = torch.from_numpy(out.copy()).bfloat16().view(torch.int16).numpy()
        assert np.array_equal(_np(g.view(torch.int16)), want), (W, me, form)
    else:
        _same_words(g.reshape(-1), out, (W, me, form))
    if form == "strided":
        assert bool((base.view(torch.int32)[1::2] == SENTINEL).all())
    if form == "block":
        assert bool((base.view(torch.int32).view(BLOCK[0], 2 * BLOCK[1])[:, BLOCK[1]:] == SENTINEL).all())
    if nonfinite:
        assert bool(torch.isnan(g).all())
    else:
        want = np.ldexp(so.plain_quantized_sum(xs, f).astype(np.float64), -f).astype(np.float32)
        assert np.array_equal(so.bits(out), so.bits(want))


@pytest.mark.parametrize("W,me", [(1, 0), (2, 1), (4, 0), (4, 2), (9, 8), (17, 5)])
def test_exact_masker_among_oracle_clients(dev, W, me):
    _masker_round(dev, W, me, 13 * 4096 + 1, "fp32")
    _masker_round(dev, W, me, (1 << 32) + 5, "fp32")


@pytest.mark.parametrize("form", ["bf16", "strided", "block"])
def test_exact_masker_converts_and_copies_back(dev, form):
    """A bf16 or non-contiguous gradient takes the ``float().contiguous()`` branch and its copy-back;
    a column block, which ``reshape(-1)`` can only copy, still receives the sum in place."""
    _masker_round(dev, 4, 1, 13 * 4096 + 2, form)
    _masker_round(dev, 3, 2, 7, form)


def test_exact_masker_with_a_non_finite_oracle_client(dev):
    _masker_round(dev, 4, 1, 13 * 4096 + 3, "fp32", nonfinite=True)
    _masker_round(dev, 4, 0, 13 * 4096 + 3, "strided", nonfinite=True)
