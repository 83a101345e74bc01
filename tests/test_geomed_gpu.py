"""``fedrec_geomed::`` (csrc/geomed.hip) on the device: the one-wave Weiszfeld kernel against the fp64 reference
recurrence on the same G, the weighted combine bit for bit, the rule end to end against a whole-rule fp64 oracle, and
the two-bucket gather with two processes on one card.

Weights: both sides run one fixed recurrence, so they differ by rounding alone.  The reference summed in ascending
and in descending client order differs, over every (W, kind) below, by at most 1.11e-16 in a weight (MEASURED on
the host: 0 at W <= 2, 1.11e-16 at W = 3 plain, 7e-18 .. 2.1e-17 at W >= 16); the bound is 16 x that and may never
pass 1e-8, where a weight error would show in the fp32 aggregate.
``dist`` is fp32(sqrt(d2)) with d2 carrying a relative error of some 1e-15: one fp32 unit for a rounding that flips.

End to end: 4 x the error of the host contract path (``ops`` on CPU tensors) against the oracle on the same input,
taken in the test; MEASURED on the host: 3.67e-07, 4.23e-07, 5.56e-07 for the three shapes, on
outputs of magnitude up to 3.9 (docs/PARITY.md 2.3)."""
import pytest
import torch

from launch_util import run_ranks

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import reference as ref
from fedrec_with_pytorchdistributed_amd.parallel.robust import RobustRule

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
WS = [1, 2, 3, 16, 17, 32]
KINDS = ["plain", "invalid", "scaled"]
WEIGHT_BOUND = 16 * 1.1102230246251565e-16
E2E = [(5, 9 * 1024 + 37), (17, 2 * 1024), (32, 1024 + 4)]


def _stack(W, n, seed, kind="scaled"):
    """Honest rows base + 1e-3 randn; the last row is NaN at one coordinate (invalid) or scaled by 1e6."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) + 1e-3 * torch.randn(W, n, generator=g)
    if kind == "invalid":
        x[W - 1, (W - 1) % n] = NAN
    elif kind == "scaled":
        x[W - 1] *= 1e6
    return x.contiguous()


def _gram_case(W, kind, dev="cpu"):
    x = _stack(W, 517, 10 * W + len(kind), kind).to(dev)
    return ops.krum_gram(x, ops.trimmed_mean(x, (W - 1) // 2)[0])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W", WS)
def test_weights_kernel_matches_the_reference_recurrence(dev, W, kind):
    G = _gram_case(W, kind, dev)
    (a, dist), (want_a, want_dist) = ops.geomed_weights(G), ref.geomed_weights(G.cpu())
    assert a.dtype == torch.float64 and dist.dtype == torch.float32 and a.shape == dist.shape == (W,)
    a, dist = a.cpu(), dist.cpu()
    ok = ~torch.isnan(want_a)  # W <= 2 with a NaN row: the centre is the mean, nobody is valid, every weight NaN
    assert torch.equal(torch.isnan(a), ~ok) and bool(ok.all()) == (W > 2 or kind != "invalid")
    err = float((a - want_a)[ok].abs().max()) if bool(ok.any()) else 0.0
    print(f"W {W} {kind}: weight err {err:.3e} (bound {WEIGHT_BOUND:.3e}), a[-1] {float(a[-1]):.3e}")
    assert WEIGHT_BOUND <= 1e-8 and err <= WEIGHT_BOUND
    fin = torch.isfinite(want_dist)
    assert torch.equal(torch.isinf(dist), ~fin) and (kind != "invalid" or (dist[-1] == INF and (W <= 2 or a[-1] == 0)))
    assert bool(((dist - want_dist)[fin].abs() <= 2.0 ** -23 * want_dist[fin]).all())


@pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "shifted"])
@pytest.mark.parametrize("n", [1, 1023, 4 * 256 * 3 + 4, 4 * 256 * 3 + 5])
@pytest.mark.parametrize("W", [3, 32])
def test_combine_kernel_is_bitwise_the_reference(dev, W, n, shifted):
    g = torch.Generator().manual_seed(W + n)
    x = torch.randn(W, n, generator=g)
    a = torch.rand(W, generator=g, dtype=torch.float64) + 0.01
    a[0] = 0.0  # the first contributing row comes after a skipped one
    x[0] = NAN  # and a row of weight zero is not read
    if W == 32:
        a[9], x[9, n // 2] = 0.0, INF  # 30 rows: groups of 8, 8, 8, 6
    a = a / a.sum()
    want = ref.geomed_combine(x, a)
    d = x.to(dev)
    if shifted:  # rows at a 4-byte offset: the one-coordinate path
        d = torch.empty(W * n + 1, device=dev)[1:].view(W, n)
        d.copy_(x)
    assert d.is_contiguous() and d.data_ptr() % 16 == (4 if shifted else 0)
    out = ops.geomed_combine(d, a.to(dev))
    assert bool(torch.isfinite(want).all()) and torch.equal(out.cpu().view(torch.int32), want.view(torch.int32))


def _oracle(x):
    """The whole rule in fp64: median centre, Gram, the recurrence, the weighted sum."""
    W = x.shape[0]
    center, _ = ref.trimmed_mean(x, (W - 1) // 2, acc_dtype=torch.float64)
    y = x.double() - center
    a, _ = ref.geomed_weights(y @ y.t())
    return (a[:, None] * x.double()).sum(0)


@pytest.mark.parametrize("W,n", E2E)
def test_rule_end_to_end_matches_the_fp64_oracle(dev, W, n):
    x = _stack(W, n, 31 * W + n)
    want = _oracle(x)
    host, _ = RobustRule("geomed").combine(x)
    tol = 4 * float((host.double() - want).abs().max())
    rule = RobustRule("geomed")
    out, dropped = rule.combine(x.to(dev))
    err = float((out.cpu().double() - want).abs().max())
    print(f"W {W} n {n}: device err {err:.3e}, host contract err {tol / 4:.3e}, weight of the scaled client "
          f"{float(rule.weights[-1]):.3e}")
    assert out.is_cuda and dropped.tolist() == [0] * W and err <= tol


def test_two_bucket_gather_leaves_two_clients_on_one_card_identical(dev):
    share = {"FEDREC_CPU_ONLY": "0", "FEDREC_SHARE_GPU": "1", "FEDREC_QUIET": "1"}
    outs = run_ranks([["tests/_geomed_worker.py", "--device", "cuda"]] * 2, share, timeout=300)
    assert all(rc == 0 and "GEOMED OK" in out for rc, out in outs), outs[0][1][-2000:]
    assert outs[0][1].split("GEOMED OK")[1].split()[0] == outs[1][1].split("GEOMED OK")[1].split()[0]
