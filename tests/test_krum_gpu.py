"""``fedrec_krum::`` (csrc/krum.hip) on the device: the centred Gram against fp64 under a counted bound,
grid independence, containment of a poisoned client, the rule end to end against the fp64 oracle, the
selected mean (the argument checks run before the device check: tests/test_krum_cpu.py).

Shapes: W = 3, 5, 16 (one tile), 17, 32 (three tiles); n = 1, 3, one chunk of L = 1024 coordinates
minus 1, L, L + 1, and 9 chunks (three blocks of four waves) with a ragged tail, odd (4-byte loads)
and a multiple of 4 (16-byte loads, the last step half filled)."""
import pytest
import torch

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import reference as ref
from fedrec_with_pytorchdistributed_amd.parallel.robust import RobustRule

pytestmark = pytest.mark.gpu

L = 1024  # krum.hip KR_L
U = 2.0 ** -24
WS = [3, 5, 16, 17, 32]
NS = [1, 3, L - 1, L, L + 1, 9 * L + 37, 9 * L + 36]
NAN, INF = float("nan"), float("inf")


def _stack(W, n, seed, byz=0, attack="none"):
    """Honest rows base + 1e-3 randn; the LAST ``byz`` rows are Byzantine."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(n, generator=g)
    x = base + 1e-3 * torch.randn(W, n, generator=g)
    for c in range(W - byz, W):
        if attack == "scale":
            x[c] = -50.0 * base
        elif attack == "noise":
            x[c] = base + 8e-3 * torch.randn(n, generator=g)
        elif attack == "nan":
            x[c, c % n] = NAN
    return x.contiguous()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _gram_bound(x, center, n):
    """(G64, bound): G64 = Y Y^T in fp64 of Y = x - center rounded to fp32 as the kernel rounds it.
    Inside a chunk an accumulator chains L / 4 MFMAs, each counted as 4 additions: min(n, L) additions
    of nonzero terms, plus 1 for a product's rounding; the fp64 sum over the chunks adds P 2^-53, far
    below one more unit: c = min(n, L) + 2 covers it and the second-order terms of (1 + u)^c."""
    y = (x - center).double()
    return y @ y.t(), (min(n, L) + 2) * U * (y.abs() @ y.abs().t())


@pytest.mark.parametrize("W", WS)
def test_gram_stays_within_the_counted_bound(dev, W):
    for n in NS:
        x = _stack(W, n, 1000 * W + n % 997)
        d = x.to(dev)
        center, _ = ops.trimmed_mean(d, (W - 1) // 2)
        G = ops.krum_gram(d, center)
        assert G.dtype == torch.float64 and tuple(G.shape) == (W, W) and torch.equal(G, G.t())
        G64, bound = _gram_bound(x, center.cpu(), n)
        err = (G.cpu() - G64).abs()
        print(f"W {W} n {n}: worst err / bound {float((err / bound.clamp(min=1e-300)).max()):.4f}")
        assert bool((err <= bound).all()), (W, n)
    # rows that are not 16-byte aligned (n % 4 == 0 all the same): the 4-byte path, bitwise the same G
    n = 2 * L
    x = _stack(W, n, W).to(dev)
    center, _ = ops.trimmed_mean(x, (W - 1) // 2)
    view = torch.empty(W * n + 1, device=dev)[1:].view(W, n)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 0
    assert torch.equal(_bits(ops.krum_gram(view, center)), _bits(ops.krum_gram(x, center)))


@pytest.mark.parametrize("W,n", [(5, 9 * L + 37), (32, 9 * L + 36)])
def test_gram_is_bitwise_independent_of_the_grid(dev, W, n):
    x = _stack(W, n, 7).to(dev)
    center, _ = ops.trimmed_mean(x, (W - 1) // 2)
    G = ops.krum_gram(x, center)
    for blocks in (1, 2):  # one block walks all 10 chunks; two blocks split them unevenly
        assert torch.equal(_bits(ops.krum_gram(x, center, blocks)), _bits(G)), blocks


@pytest.mark.parametrize("W,n", [(5, 9 * L + 37), (17, 2 * L), (32, L + 4)])
def test_a_poisoned_client_stays_in_its_row_and_column(dev, W, n):
    x = _stack(W, n, 11)
    center, _ = ops.trimmed_mean(x.to(dev), (W - 1) // 2)
    clean = ops.krum_gram(x.to(dev), center)
    b = W - 2
    x[b, 0], x[b, n // 2], x[b, n - 1] = NAN, INF, 1e30
    G = ops.krum_gram(x.to(dev), center)  # the same center: only row b of Y changed
    keep = torch.ones(W, W, dtype=torch.bool)
    keep[b], keep[:, b] = False, False
    assert torch.equal(_bits(G)[keep], _bits(clean)[keep]) and not bool(torch.isfinite(G[b].cpu()).any())
    out, dropped = RobustRule("multi_krum", 1).combine(x.to(dev))  # its own median, f = 1
    assert dropped.tolist() == [n if c == b else 0 for c in range(W)] and bool(torch.isfinite(out).all())


CASES = [(W, n, f) for W in (4, 5, 16, 17, 32) for n in (257, 4099, 65541) for f in sorted({0, min(1, (W - 3) // 2), (W - 3) // 2})]


@pytest.mark.parametrize("W,n,f", CASES)
def test_rule_end_to_end_matches_the_fp64_oracle(dev, W, n, f):
    """b = max(f, 1) Byzantine clients, m = W - b kept: the boundary of the selection lies between the
    honest and the Byzantine clients.  A distance is off by at most E_cj = B_cc + B_jj + 2 B_cj (B the
    Gram bound); a score is the sum of the k = W - f - 2 smallest distances, which moves by at most the
    sum of the k largest E_cj when every distance moves by E_cj, plus k + 1 fp32 roundings (the
    conversion, k - 1 additions, one for second-order terms) of the score itself."""
    b, k = max(f, 1), W - f - 2
    m = W - b
    attack = ("scale", "noise", "nan")[(W + n + f) % 3]
    x = _stack(W, n, 31 * W + n + f, b, attack)
    d = x.to(dev)
    center, _ = ops.trimmed_mean(d, (W - 1) // 2)
    G = ops.krum_gram(d, center)
    sel, scores = ops.krum_select(G, f, m)
    out = ops.krum_mean(d, sel)
    G64, B = _gram_bound(x, center.cpu(), n)
    want_sel, _ = ref.krum_select(G64, f, m)
    g = G64.diagonal()
    d64 = ((g[:, None] + g[None, :]) - 2 * G64).clamp_min(0)
    fin = torch.isfinite(d64)
    E = torch.where(fin, B.diagonal()[:, None] + B.diagonal()[None, :] + 2 * B, torch.zeros_like(B))
    off = ~torch.eye(W, dtype=torch.bool)
    s64 = torch.sort(torch.where(fin, d64, torch.full_like(d64, INF))[off].view(W, W - 1), dim=1).values[:, :k].sum(1)
    ok = torch.isfinite(s64)
    bnd = torch.sort(E[off].view(W, W - 1), dim=1).values[:, W - 1 - k:].sum(1) + (k + 1) * U * s64
    bnd = torch.where(ok, bnd, torch.zeros_like(bnd))
    srt = torch.sort(s64).values
    gap = float(srt[m] - srt[m - 1])
    print(f"W {W} n {n} f {f} {attack}: gap {gap:.3e}, bound {float(bnd.max()):.3e}")
    assert gap >= 100 * float(bnd.max()), "the seed must put the boundary clear of the bound"
    assert sel.cpu().tolist() == want_sel.tolist() == [1] * m + [0] * b
    sc = scores.cpu().double()
    assert bool(((sc - s64).abs()[ok] <= bnd[ok]).all()) and bool((sc[~ok] == INF).all())
    assert torch.equal(_bits(out), _bits(ref.krum_mean(x, want_sel)))


@pytest.mark.parametrize("W", [3, 17, 32])
def test_selected_mean_paths(dev, W):
    n = 4100  # 16-byte path over several blocks; its first 4099 columns and a shifted view: 4-byte path
    x = _stack(W, n, W).to(dev)
    every = torch.ones(W, dtype=torch.int32, device=dev)
    assert torch.equal(_bits(ops.krum_mean(x, every)), _bits(ops.trimmed_mean(x, 0)[0]))
    some = (torch.arange(W, device=dev) % 3 != 1).to(torch.int32)
    full = ops.krum_mean(x, some)
    assert torch.equal(_bits(full), _bits(ref.krum_mean(x.cpu(), some.cpu())))
    view = torch.empty(W * n + 1, device=dev)[1:].view(W, n)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4 and torch.equal(_bits(ops.krum_mean(view, some)), _bits(full))
    assert torch.equal(_bits(ops.krum_mean(x[:, :n - 1].contiguous(), some)), _bits(full[:n - 1]))

