"""Every form of the bf16 GEMM family (csrc/gemm_bf16.hip) on the per-element fp64 oracle of
tests/gemm_oracle.py: ``linear`` (act 0-3, bias, residual, variants -1 / 0 / 6 / 9 / 12 / 13),
``linear_split``, ``linear_gelu_dual`` and ``linear_gelu_bwd`` with its column sums.

A case passes when EVERY output element is within its counted bound (``ratio <= 1``); a failure
names the worst element's tile, wave block and fragment.  The shapes are the smallest at which
each mechanism of the ping-pong kernels can go wrong: two and three K-steps (every stage call
crosses a tile seam; the buffer parity flips from tile to tile), tile counts around the CU count
(read from the device, as the launcher does), grids that do and do not take the XCD remap,
partial row and column tiles.  The fp64 reference of an input set is computed once on the device
and shared by the cases that use it.  Run with ``-s`` for the worst ratio per family.
"""
import functools

import pytest
import torch

import gemm_oracle as go
from fedrec_with_pytorchdistributed_amd.ops import native

pytestmark = pytest.mark.gpu

WORST = {}


def _note(fam: str, ratio: float) -> None:
    WORST[fam] = max(WORST.get(fam, 0.0), ratio)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nworst observed / bound per family: %s" % {k: "%.3f" % v for k, v in sorted(WORST.items())})


@functools.lru_cache(maxsize=None)
def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else go.NOMINAL_CUS


@functools.lru_cache(maxsize=2)
def _linear_set(key):
    """Inputs and oracle of a linear input set, on the device (the last two sets are kept)."""
    M, N, K, act, bias, res, wide = key
    x, w, b, r = go.make_inputs(M, N, K, bias, res, act, wide, device="cuda")
    ref, tol = go.linear_oracle(x, w, b, act, r)
    return x, w, b, r, ref, tol


@functools.lru_cache(maxsize=1)
def _dual_set(M, K):
    x, w, b, _ = go.make_inputs(M, go.FFN_N, K, True, device="cuda")
    return x, w, b, go.dual_oracle(x, w, b)


@functools.lru_cache(maxsize=1)
def _bwd_set(M, K):
    x, w, _, z = go.make_inputs(M, go.FFN_N, K, False, True, 3, device="cuda")
    return (x, w, z) + go.linear_oracle(x, w, None, 3, z)


def _forced(variant: int):
    class _V:
        def __enter__(self):
            native.lib().gemm_set_variant(variant)

        def __exit__(self, *a):
            native.lib().gemm_set_variant(-1)

    return _V()


def _padded(y, M: int, N: int) -> None:
    """The ping-pong stores are unpredicated: the output's storage holds round_up(M, 256) rows."""
    assert y.untyped_storage().nbytes() >= (M + 255) // 256 * 256 * N * 2, (y.untyped_storage().nbytes(), M, N)


def _run_linear(case, repeat: bool = False) -> float:
    M, N, K, act, bias, res, wide, variant = case
    x, w, b, r, ref, tol = _linear_set(go.input_key(case))
    lib = native.lib()
    with _forced(variant):
        y = lib.linear(x, w, b, act, r)
        y2 = lib.linear(x, w, b, act, r) if repeat else None
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    _padded(y, M, N)
    ratio = go.check(y, ref, tol, "linear %s" % (case,))
    if repeat:
        assert torch.equal(y2, y), "not bitwise deterministic run to run: %s" % (case,)
    _note(go.family(case), ratio)
    return ratio


def _ids(cases):
    return ["M%d-N%d-K%d-act%d-b%d-r%d-w%d-v%d" % tuple(int(v) for v in c) for c in cases]


def _by_set(cases):
    return sorted(cases, key=go.input_key)


_K, _MC, _NC, _EP = _by_set(go.k_cases()), _by_set(go.m_cases()), _by_set(go.n_cases()), _by_set(go.epilogue_cases())


@pytest.mark.parametrize("case", _K, ids=_ids(_K))
def test_k_zoo(dev, case):
    """K = 64 (one K-step: the 128x128 kernel) to 3072 under every ping-pong variant; K = 128: every
    stage call of a step crosses into the next tile; K = 192: an odd step count."""
    _run_linear(case)


@pytest.mark.parametrize("case", _MC, ids=_ids(_MC))
def test_m_edges(dev, case):
    """One row to a row past two tiles under the forced variants; auto around its M >= 4096 gate."""
    _run_linear(case)


@pytest.mark.parametrize("case", _NC, ids=_ids(_NC))
def test_n_edges(dev, case):
    """The 128x128 kernel's N, variant 9's partial last column tile, N = PP2_MAXN and past it."""
    _run_linear(case)


@pytest.mark.parametrize("case", _EP, ids=_ids(_EP))
def test_epilogues(dev, case):
    """act 0-3 x bias x residual on two row tiles per variant, and the wide sets (pre-activations and
    saved z over +-40: tanh saturated both ways, the GELU and GELU' tails)."""
    _run_linear(case)


def _walk_params():
    cases = go.walk_cases(_cus())
    return pytest.mark.parametrize("case", cases, ids=_ids(cases))


@_walk_params()
def test_persistent_walk(dev, case):
    """Tile counts 7 / 8 / 9 and around 1x and 3x the CU count, K = 128 and 192, three or nine column
    tiles: the stream crosses tile seams with a changing bias; twice, bitwise equal."""
    M, N = case[0], case[1]
    assert (M + 255) // 256 * (N // 256) in [tm * (n // 256) for tm, n in go.walk_shapes(_cus())]
    _note("walk", _run_linear(case, repeat=True))


_SPLIT = [(M, K, v, npart) for M in go.SPLIT_M for K in go.SPLIT_K for v in go.SPLIT_VARIANTS for npart in go.SPLIT_NP]


@pytest.mark.parametrize("M,K,variant,n_partial", _SPLIT)
def test_linear_split(dev, M, K, variant, n_partial):
    """The row-split tile list against the oracle over the region the contract defines: every column
    of the rows < full_rows, the first n_partial columns of all rows."""
    N = go.SPLIT_N
    x, w, b, _, ref, tol = _linear_set((M, N, K, 0, True, False, False))
    lib = native.lib()
    for fr in go.split_full_rows(M):
        full = torch.tensor([fr], dtype=torch.int32, device=dev)
        with _forced(variant):
            y = lib.linear_split(x, w, b, full, n_partial)
        _padded(y, M, N)
        _note("split", go.check(y, ref, tol, "linear_split M %d K %d variant %d n_partial %d full_rows %d"
                                % (M, K, variant, n_partial, fr), rows=fr, cols=n_partial))


_FFN = [(M, K, v) for M in go.FFN_M for K in go.FFN_K for v in go.FFN_VARIANTS]


@pytest.mark.parametrize("M,K,variant", _FFN)
def test_linear_gelu_dual(dev, M, K, variant):
    """z = bf16(pre) and h = bf16(GELU(pre)); below M = 4096 the op is GEMM + a GELU pass over the
    rounded z, held to the fallback's own bound."""
    N = go.FFN_N
    x, w, b, d = _dual_set(M, K)
    with _forced(variant):
        h, z = native.lib().linear_gelu_dual(x, w, b)
    _padded(h, M, N)
    _padded(z, M, N)
    what = "linear_gelu_dual M %d K %d variant %d" % (M, K, variant)
    _note("dual z", go.check(z, d["z"], d["tol_z"], what + " z"))
    if M >= 4096:
        _note("dual h", go.check(h, d["h"], d["tol_h"], what + " h"))
    else:
        _note("dual h fallback", go.check(h, d["h"], d["tol_h_fallback"], what + " h (fallback)"))


@pytest.mark.parametrize("M,K,variant", _FFN)
def test_linear_gelu_bwd(dev, M, K, variant):
    """dz = (a w^T) GELU'(z) per element, and every column of the fused column sums against the
    fp64 sum of the dz the launch stored."""
    N = go.FFN_N
    x, w, z, ref, tol = _bwd_set(M, K)
    lib = native.lib()
    with _forced(variant):
        dz, cs = lib.linear_gelu_bwd(x, w, z)
        dz2, cs2 = lib.linear_gelu_bwd(x, w, z)
    _padded(dz, M, N)
    what = "linear_gelu_bwd M %d K %d variant %d" % (M, K, variant)
    _note("act3", go.check(dz, ref, tol, what + " dz"))
    assert torch.equal(dz2, dz)
    if M >= 4096:
        assert cs is not None and cs.shape == (N,) and cs.dtype == torch.float32
        cref, ctol = go.colsum_oracle(dz)
        _note("colsum", go.check(cs, cref, ctol, what + " colsum"))
        assert torch.equal(cs2, cs)  # deterministic partials + fixed-order sum
    else:
        assert cs is None


@pytest.mark.parametrize("bias,res", [(True, True), (True, False), (False, False)])
@pytest.mark.parametrize("variant", go.ALL_VARIANTS)
def test_position_coded_exact(dev, variant, bias, res):
    """One-hot rows against a position-coded integer weight, integer bias and residual: every output
    is an exact small integer that names its row, column and K index, so any misplaced row,
    column, K-step or stale stage breaks ``torch.equal`` (K = 192, more than two tiles per block)."""
    M, N, K = go.exact_shape(_cus())
    assert (M + 255) // 256 * (N // 256) > 2 * _cus()
    x, w, b, r, want = go.exact_inputs(M, N, K, bias, res, device=dev)
    with _forced(variant):
        y = native.lib().linear(x, w, b, 0, r)
    if not torch.equal(y, want):
        bad = (y != want).nonzero()
        i, j = int(bad[0, 0]), int(bad[0, 1])
        raise AssertionError("variant %d: %d elements differ, first (row %d, column %d) = tile (%d, %d): got %g, want %g"
                             % (variant, bad.shape[0], i, j, i // 256, j // 256, float(y[i, j]), float(want[i, j])))
