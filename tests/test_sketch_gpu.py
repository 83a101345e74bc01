"""The count-sketch kernels (csrc/sketch_delta.hip) against the host oracles of ops/reference.py, bit for bit: the
sketch and its estimate at one block, ragged blocks and 1, 2 and 4 tiles per row, on a misaligned view and with
non-finite inputs; the accumulate, the clear, and two whole rounds of the codec.  The oracle itself is held to an
fp64 sum per bucket: a bucket is ``nb`` fp32 additions, so it is within ``nb 2^-24 sum|a|`` of its exact sum."""
import pytest
import torch

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import reference as ref
from fedrec_with_pytorchdistributed_amd.parallel.sketch import SketchUpload

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _pair(n, seed, pad=0):
    """Host ``(local, theta)`` of ``n`` coordinates; ``pad``: views that start ``pad`` elements into their storage."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n + pad, generator=g)[pad:], torch.randn(n + pad, generator=g)[pad:]


def _both(local, theta, plan, R, C, dev):
    """(device S, host S) after asserting that the device estimate of the device S is the host's of the host's."""
    n = local.numel()
    want = ref.sketch_delta(local.contiguous(), theta.contiguous(), plan, R, C)
    pad = local.storage_offset()
    dl, dt = (torch.cat([t.new_zeros(pad), t]).to(dev)[pad:] for t in (local, theta))  # the same misalignment on the device
    got = ops.sketch_delta(dl, dt, plan.to(dev), R, C)
    est = ops.sketch_estimate(got, plan.to(dev), n)
    assert torch.equal(_bits(est), _bits(ref.sketch_estimate(want, plan, n))), n
    return got, want


@pytest.mark.parametrize("R", [1, 3, 5])
@pytest.mark.parametrize("C", [1024, 2048, 4096])
def test_delta_and_estimate_are_the_host_oracles_bit_for_bit(dev, C, R):
    for n in (1, 1023, 1025, C, C + 1, 3 * C - 5):
        plan = ref.sketch_plan(n, C, 11)
        got, want = _both(*_pair(n, n + R), plan, R, C, dev)
        assert torch.equal(_bits(got), _bits(want)), n


def test_a_view_off_the_16_byte_grid_gives_the_same_bits(dev):
    n, R, C = 3 * 2048 - 5, 5, 2048
    plan = ref.sketch_plan(n, C, 11)
    local, theta = _pair(n, 4, pad=1)
    got, want = _both(local, theta, plan, R, C, dev)
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(want), _bits(ref.sketch_delta(local.clone(), theta.clone(), plan, R, C)))


def test_an_inf_and_a_nan_stay_in_their_own_buckets(dev):
    n, R, C = 3 * 2048 - 5, 5, 2048
    plan = ref.sketch_plan(n, C, 11)
    local, theta = _pair(n, 5)
    local[7], local[C + 9] = float("inf"), float("nan")
    got, want = _both(local, theta, plan, R, C, dev)
    j, _ = ref.sketch_hash(plan, torch.tensor([7, C + 9]), R, C)
    rows = torch.arange(R)
    assert bool(torch.isinf(want[rows, j[:, 0]]).all()) and bool(torch.isnan(want[rows, j[:, 1]]).all())
    assert int((~torch.isfinite(want)).sum()) == len({(r, int(b)) for r in range(R) for b in j[r]})
    # IEEE 754 leaves the sign and payload of a NaN that an addition passes on to the implementation: NaN compares as NaN
    assert torch.equal(torch.isnan(got.cpu()), torch.isnan(want))
    assert torch.equal(_bits(got.cpu().nan_to_num(nan=0.0)), _bits(want.nan_to_num(nan=0.0)))


@pytest.mark.parametrize("W", [1, 3, 32])
def test_accumulate_is_the_host_oracle_bit_for_bit(dev, W):
    g = torch.Generator().manual_seed(W)
    E, stack = torch.randn(3, 1024, generator=g), torch.randn(W, 3 * 1024, generator=g)
    w = 0.37 * torch.arange(1, W + 1, dtype=torch.float32)
    got = ops.sketch_accumulate_(E.to(dev), stack.to(dev), w.to(dev))
    assert torch.equal(_bits(got), _bits(ref.sketch_accumulate_(E.clone(), stack, w)))


def test_clear_zeroes_the_buckets_of_members_that_share_one_and_skips_what_is_outside(dev):
    n, R, C = 3 * 2048 - 5, 3, 2048
    plan = ref.sketch_plan(n, C, 11)
    j0 = ref.sketch_hash(plan, torch.tensor([5]), R, C)[0][0]
    second = torch.arange(C, 2 * C)
    twin = int(second[ref.sketch_hash(plan, second, R, C)[0][0] == j0])  # block 1's coordinate in row 0's bucket of 5
    idx = torch.tensor([5, twin, 4000, -1, 3 * C], dtype=torch.int32)
    E = torch.randn(R, C, generator=torch.Generator().manual_seed(1)) + 3.0
    want = ref.sketch_clear_(E.clone(), idx, plan)
    assert int((want == 0).sum()) == 3 * R - 1 and not bool(want.view(torch.int32)[want == 0].any())  # +0.0
    assert torch.equal(_bits(ops.sketch_clear_(E.to(dev), idx.to(dev), plan.to(dev))), _bits(want))


def test_two_rounds_of_the_codec_on_the_device_are_the_hosts_bits_model_and_error_table(dev):
    n, W = 20000, 3
    host, lr = (SketchUpload(0.01, 3, 2048, seed=5).plan_for(n, d) for d in ("cpu", dev))
    theta_h, w = torch.randn(n, generator=torch.Generator().manual_seed(9)), torch.tensor([2.0, 1.0, 4.0])
    theta_d = theta_h.to(dev)
    for rnd in range(2):
        locals_ = [theta_h + 0.1 * _pair(n, 100 * rnd + c)[0] ** 3 for c in range(W)]
        ups_h = [host.compress(x, theta_h, None, c, rnd) for c, x in enumerate(locals_)]
        ups_d = [lr.unpack(lr.pack(lr.compress(x.to(dev), theta_d, None, c, rnd)), n) for c, x in enumerate(locals_)]
        assert torch.equal(_bits(lr.received(theta_d, ups_d[0])), _bits(host.received(theta_h, ups_h[0])))
        theta_h, theta_d = host.combine(theta_h, ups_h, w)[0], lr.combine(theta_d, ups_d, w.to(dev))[0]
        assert torch.equal(_bits(theta_d), _bits(theta_h)) and torch.equal(_bits(lr.basis), _bits(host.basis)), rnd
        assert lr.basis.device.type == "cuda" and bool(host.basis.any())


@pytest.mark.parametrize("n,C", [(1, 1024), (3 * 2048 - 5, 2048), (40 * 1024 + 3, 1024)])
def test_the_sketch_is_within_the_bound_of_its_additions_of_an_fp64_sum_per_bucket(dev, n, C):
    R = 5
    plan = ref.sketch_plan(n, C, 11)
    local, theta = _pair(n, 6)
    got, want = _both(local, theta, plan, R, C, dev)
    a = (local - theta).double()
    j, neg = ref.sketch_hash(plan, torch.arange(n), R, C)
    exact, mass = torch.zeros(R, C, dtype=torch.float64), torch.zeros(R, C, dtype=torch.float64)
    for r in range(R):
        exact[r].index_add_(0, j[r], torch.where(neg[r], -a, a))
        mass[r].index_add_(0, j[r], a.abs())
    nb = plan.shape[0]
    for S in (want, got.cpu()):
        assert bool(((S.double() - exact).abs() <= nb * 2.0 ** -24 * mass).all())
