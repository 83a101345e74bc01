"""``fedrec_dp::`` (csrc/dp_clip.hip) on the device: the squared norm and the clipped part bit for bit against the torch
contract (``ops.reference.dp_*``), the noise per element against the fp64 Box-Muller of the oracle's Philox words, and
``ClientDP.privatize`` against a whole-rule fp64 oracle.

Noise bound: ``std * noise_tol(z64, rad)`` is the project's device-measured bound for the same ``box_muller``
(tests/data_oracle.py section 3); ``2 U (|std z64| + |want|)`` is the rounding of the product and of the final add, one
spare unit.  End to end: 4 x the error of the host contract path against the same oracle, taken in the test.
MEASURED on an MI355X: the noise reaches 0.74 of its bound at worst (the probe; 0.05 - 0.73 elsewhere); end to end the
device is off by 2.230e-07 / 2.256e-07 at n = 1025 / 9253 and the host contract path by the same 2.230e-07 / 2.256e-07
(docs/PARITY.md 2.3)."""
import math

import numpy as np
import pytest
import torch

from data_oracle import TINY, U, noise_tol, words

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import reference as ref
from fedrec_with_pytorchdistributed_amd.parallel.cdp import ClientDP

pytestmark = pytest.mark.gpu

NS = [1, 3, 1023, 1024, 1025, 3 * 1024 + 4, 3 * 1024 + 5, 65 * 1024 + 4]
ALIGN = pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "shifted"])
_CACHE = {}


def _pair(n):
    """``(local, base, state)`` on the host, made once per n and left unchanged: a delta of 1e-2 on a unit model."""
    if n not in _CACHE:
        g = torch.Generator().manual_seed(n)
        base = torch.randn(n, generator=g)
        local = base + 1e-2 * torch.randn(n, generator=g)
        _CACHE[n] = (local, base, ref.dp_delta_sqnorm(local, base))
    return _CACHE[n]


def _to(x, dev, shifted):
    """On the device, 16-byte aligned or at a 4-byte offset (the one-coordinate path)."""
    d = torch.empty(x.numel() + 1, device=dev)[1:] if shifted else torch.empty_like(x, device=dev)
    d.copy_(x)
    assert d.is_contiguous() and d.data_ptr() % 16 == (4 if shifted else 0)
    return d


def _bits(t):
    return t.cpu().view(torch.int32)


def _z64(n, seed, offset):
    """fp64 normals and their Box-Muller radii of coordinates 0 .. n - 1 from the oracle's Philox words."""
    u = ((words(seed, offset, np.arange((n + 3) // 4)) >> 8) + 1).astype(np.float64) / 2.0 ** 24
    rad, ang = np.sqrt(-2.0 * np.log(u[:, 0::2])), 2.0 * math.pi * u[:, 1::2]
    z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], -1).reshape(-1)[:n]
    return z, np.repeat(rad, 2, axis=-1).reshape(-1)[:n]


@pytest.mark.parametrize("max_blocks", [0, 1])
@ALIGN
@pytest.mark.parametrize("n", NS)
def test_sqnorm_is_bitwise_the_contract_and_independent_of_the_grid(dev, n, shifted, max_blocks):
    local, base, want = _pair(n)
    st = ops.dp_delta_sqnorm(_to(local, dev, shifted), _to(base, dev, shifted), max_blocks)
    assert st.is_cuda and st.dtype == torch.int32 and torch.equal(st.cpu(), want)
    assert ref.dp_state_fields(st)[0] > 0


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@ALIGN
def test_a_non_finite_model_goes_out_as_it_is(dev, shifted, bad):
    local, base, _ = _pair(3 * 1024 + 5)
    local = local.clone()
    local[1031] = bad
    l, b = _to(local, dev, shifted), _to(base, dev, shifted)
    st = ops.dp_delta_sqnorm(l, b)
    out = ops.dp_clip_noise(l, b, st, 1e-3, 0.0, 1, 2)
    sq, s, clipped = ref.dp_state_fields(st)
    assert not math.isfinite(sq) and s == 1.0 and clipped == 0 and torch.equal(_bits(out), _bits(local))


@pytest.mark.parametrize("base_kind", ["zero", "unit"])
@pytest.mark.parametrize("frac", [1e6, 0.5, 1e-3])
@ALIGN
@pytest.mark.parametrize("n", NS)
def test_clip_without_noise_is_bitwise_the_contract(dev, n, shifted, frac, base_kind):
    """``zero``: the base is 0 and the output is the clipped delta itself, so ``||out - base|| <= clip (1 + 4 n U)`` holds
    as the issue states it (s carries one rounding, each product one).  ``unit``: a model of unit scale with a delta of
    1e-2; ``out = fadd(base, s d)`` lies on the fp32 grid of the MODEL, so each coordinate of ``out - base`` is off by
    up to ``U |out_k|`` whatever computes it, and the bound gains ``U ||out||``.  MEASURED at n = 1, clip = 1e-3 of the
    norm: ``|out - base|`` 2.682e-06 against clip 2.669e-06 -- the grid of 0.66 is 6e-8."""
    local, base, st0 = _pair(n)
    if base_kind == "zero":
        local, base = local - base, torch.zeros(n)
        st0 = ref.dp_delta_sqnorm(local, base)
    clip = frac * math.sqrt(ref.dp_state_fields(st0)[0])
    hst = st0.clone()
    want = ref.dp_clip_noise(local, base, hst, clip, 0.0, 1, 2)
    l, b = _to(local, dev, shifted), _to(base, dev, shifted)
    st = ops.dp_delta_sqnorm(l, b)
    out = ops.dp_clip_noise(l, b, st, clip, 0.0, 1, 2)
    assert torch.equal(st.cpu(), hst) and torch.equal(_bits(out), _bits(want))
    _, s, clipped = ref.dp_state_fields(st)
    if frac > 1:
        assert s == 1.0 and clipped == 0 and torch.equal(_bits(out), _bits(local))
    else:
        assert s < 1.0 and clipped == 1
    out = out.cpu().double()
    grid = U * float(out.norm()) if base_kind == "unit" else 0.0
    assert float((out - base.double()).norm()) <= clip * (1 + 4 * n * U) + grid


@pytest.mark.parametrize("std", [1.0, 1e-3])
@pytest.mark.parametrize("n", [5, 1025, 3 * 1024 + 4])
def test_noise_per_element_against_the_fp64_box_muller(dev, n, std):
    local, base, st0 = _pair(n)
    clip = 0.5 * math.sqrt(ref.dp_state_fields(st0)[0])
    p = ref.dp_clip_noise(local, base, st0.clone(), clip, 0.0, 0, 0).double().numpy()  # bitwise the device's (above)
    l, b = local.to(dev), base.to(dev)
    out = ops.dp_clip_noise(l, b, ops.dp_delta_sqnorm(l, b), clip, std, 11, 3).cpu().double().numpy()
    z, rad = _z64(n, 11, 3)
    want = p + std * z
    tol = std * noise_tol(z, rad) + 2 * U * (np.abs(std * z) + np.abs(want)) + TINY
    worst = float((np.abs(out - want) / tol).max())
    print(f"n {n} std {std}: worst |out - want| / bound {worst:.3f}")
    assert worst <= 1.0


def test_the_pure_probe_is_z_itself_and_keys_differ_by_client_and_round(dev):
    n = 3 * 1024 + 4
    zero = torch.zeros(n, device=dev)

    def field(client, rnd):
        return ops.dp_clip_noise(zero, zero, ops.dp_delta_sqnorm(zero, zero), 1.0, 1.0, 11, (client << 32) | rnd).cpu()

    a, b = field(0, 1), field(1, 0)
    z, rad = _z64(n, 11, 1)
    worst = float((np.abs(a.double().numpy() - z) / (noise_tol(z, rad) + 2 * U * 2 * np.abs(z) + TINY)).max())
    print(f"probe: worst |z_gpu - z64| / bound {worst:.3f}, std {float(a.std()):.4f}")
    assert worst <= 1.0 and float((a != b).float().mean()) > 0.99


@pytest.mark.parametrize("n", [1025, 9 * 1024 + 37])
def test_privatize_matches_the_whole_rule_fp64_oracle(dev, n):
    local, base, _ = _pair(n)
    W, clip, zmul, seed, client, rnd = 4, 0.05, 1.0, 7, 2, 3
    d = local.double().numpy() - base.double().numpy()
    z, _ = _z64(n, seed, (client << 32) | rnd)
    want = base.double().numpy() + min(1.0, clip / math.sqrt(float((d * d).sum()))) * d + zmul * clip / math.sqrt(W) * z
    host = ClientDP(clip, zmul, seed=seed, clients=W).privatize(local, base, client, rnd)
    rule = ClientDP(clip, zmul, seed=seed, clients=W)
    out = rule.privatize(local.to(dev), base.to(dev), client, rnd)
    e_host = float(np.abs(host.double().numpy() - want).max())
    e_dev = float(np.abs(out.cpu().double().numpy() - want).max())
    print(f"n {n}: device err {e_dev:.3e}, host contract err {e_host:.3e}")
    assert out.is_cuda and rule.last["clipped"] == 1 and e_dev <= 4 * e_host
