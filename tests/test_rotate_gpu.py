"""The rotation kernels (csrc/rotate_delta.hip) against the host oracles of ops/reference.py, bit for bit (a NaN
compares equal to a NaN): the transform and its inverse, the fused quantiser, the fused combine, the device codec, and
two clients that share the card and combine among themselves."""
import pytest
import torch

from test_quant_star_cpu import W, assert_global_is, star
from test_quant_star_gpu import FLAGS, SHARE
from test_rotate_cpu import SHAPES_A, expected_round0

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import reference as ref
from fedrec_with_pytorchdistributed_amd.parallel.rotate import RotatedQuantizer

pytestmark = pytest.mark.gpu
SHAPES_B = [4097, 3 * 4096 + 1000]


def _same(got, want):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype
    if got.dtype == torch.float32:
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        got, want = got.nan_to_num(nan=0.0).view(torch.int32), want.nan_to_num(nan=0.0).view(torch.int32)
    assert torch.equal(got, want)


def _randn(n, seed, pad=0):
    return torch.randn(n + pad, generator=torch.Generator().manual_seed(seed))[pad:]


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("n", SHAPES_A)
def test_rotate_and_its_inverse_are_the_host_oracle_bit_for_bit(dev, n, pad):
    x = _randn(n, n, pad)  # pad 1: a view off the 16-byte grid, on the host and on the device
    y = ref.rotate(x.contiguous(), 5)
    dy = ops.rotate(torch.cat([x.new_zeros(pad), x]).to(dev)[pad:], 5)
    _same(dy, y)
    _same(ops.rotate(dy, 5, inverse=True, n=n), ref.rotate(y, 5, inverse=True, n=n))


def test_an_inf_in_the_second_chunk_stays_in_the_second_chunk(dev):
    x = _randn(3 * 4096 + 1000, 3)
    x[4096 + 77] = float("inf")
    y = ref.rotate(x, 5)
    assert bool(torch.isfinite(y[:4096]).all()) and not bool(torch.isfinite(y[4096:8192]).any())
    _same(ops.rotate(x.to(dev), 5), y)


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("n,nan_at", [(SHAPES_B[0], None), (SHAPES_B[1], None), (SHAPES_B[1], 4096 + 5)])
def test_quantize_is_the_host_composition_bit_for_bit(dev, n, nan_at, bits):
    local, theta = _randn(n, n + bits), _randn(n, n + bits + 1)
    if nan_at is not None:
        local[nan_at] = float("nan")
    res = 0.05 * _randn(ref.rotate_pad(n), 9)
    dres = res.to(dev)
    want = ref.rotate_quantize(local, theta, res, bits, 7, (3 << 32) | 2)
    got = ops.rotate_quantize(local.to(dev), theta.to(dev), dres, bits, 7, (3 << 32) | 2)
    for g, w in zip((*got, dres), (*want, res)):
        _same(g, w)
    if nan_at is not None:  # all 16 blocks of the chunk, and no other
        assert torch.equal(torch.isnan(want[1]).nonzero().flatten(), torch.arange(16, 32))


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("Wc", [1, 3])
@pytest.mark.parametrize("n", SHAPES_B)
def test_combine_is_the_host_composition_bit_for_bit(dev, n, Wc, bits):
    n_pad, theta = ref.rotate_pad(n), _randn(n, n)
    ups = [ref.rotate_quantize(theta + 0.1 * _randn(n, 10 * Wc + c), theta, torch.zeros(n_pad), bits, 7, c << 32) for c in range(Wc)]
    codes, scales = (torch.stack(t) for t in zip(*ups))
    w = torch.tensor([2.0, 1.0, 4.5][:Wc])
    _same(ops.rotate_combine(theta.to(dev), codes.to(dev), scales.to(dev), w.to(dev), bits, 7),
          ref.rotate_combine(theta, codes, scales, w, bits, 7))


@pytest.mark.parametrize("bits", [8, 4])
def test_the_device_codec_packs_the_hosts_words_over_two_rounds(dev, bits):
    n = SHAPES_B[1]
    host, devc = (RotatedQuantizer(bits, 5).plan_for(n, d) for d in ("cpu", dev))
    theta = _randn(n, 1)
    for rnd in range(2):  # (the second round starts from the first one's residual)
        local = theta + 0.1 * _randn(n, 20 + rnd) ** 3
        blob_h = host.pack(host.compress(local, theta, None, 1, rnd))
        blob_d = devc.pack(devc.compress(local.to(dev), theta.to(dev), None, 1, rnd))
        _same(blob_d, blob_h)
        _same(devc.basis, host.basis)
        _same(devc.received(theta.to(dev), devc.unpack(blob_d, n)), host.received(theta, host.unpack(blob_h, n)))


def test_two_clients_on_the_card_combine_among_themselves_to_the_host_coordinators_bits(tmp_path, dev):
    (rec,) = star(tmp_path, 1, [*FLAGS, "--upload_bits=4", "--upload_rotate=1"], "allreduce", SHARE, timeout=400)
    want, flat = expected_round0(tmp_path, FLAGS, 4)
    assert_global_is(tmp_path, want, flat)
    assert rec["clients_accepted"] == W and rec["upload_rotate"] == 1 and rec["upload_bytes"] < 0.15 * rec["dense_bytes"]
