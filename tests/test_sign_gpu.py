"""The scaled-sign kernels (csrc/sign_delta.hip, the rotate_sign_* kernels of csrc/rotate_delta.hip) against the host
oracles of ops/reference.py, bit for bit (a NaN compares equal to a NaN): the coder, the combine, their rotated forms,
the device codec, and two clients that share the card and combine among themselves."""
import pytest
import torch

from test_quant_star_cpu import W, assert_global_is, star
from test_quant_star_gpu import FLAGS, SHARE
from test_rotate_gpu import _randn, _same
from test_sign_cpu import expected_round0

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import reference as ref
from fedrec_with_pytorchdistributed_amd.parallel.sign import SignUpload

pytestmark = pytest.mark.gpu
BIG = 3 * 4096 + 1000


def _off(x, pad, dev):
    """``x`` on the device; pad 1: as a view off the 16-byte grid."""
    return torch.cat([x.new_zeros(pad), x]).to(dev)[pad:]


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("n,planted", [(1, 0), (15, 0), (16, 0), (17, 0), (255, 0), (257, 0), (4097, 0), (BIG, 0),
                                       (256 * 64 + 37, 0), (BIG, 1)])
def test_quantize_is_the_host_oracle_bit_for_bit(dev, n, planted, pad):
    local, theta, res = _randn(n, n), _randn(n, n + 1), 0.05 * _randn(n, n + 2)  # (a non-zero starting residual)
    if planted:  # a NaN, an inf, a zero block and -0.0 entries, each in a block of its own
        local[5], local[300] = float("nan"), float("inf")
        local[512:768], theta[512:768], res[512:768] = 0.0, 0.0, 0.0
        local[1024:1040], theta[1024:1040], res[1024:1040] = -0.0, 0.0, -0.0
    dres = _off(res, pad, dev)
    got = ops.sign_quantize(_off(local, pad, dev), _off(theta, pad, dev), dres)
    want = ref.sign_quantize(local, theta, res)
    for g, w in zip((*got, dres), (*want, res)):
        _same(g, w)
    if planted:
        assert want[1][:3].isnan().tolist() == [True, True, False] and float(want[1][2]) == 0.0 and int(want[0][128]) == 0xFF


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("Wc", [1, 2, 3, 33])
@pytest.mark.parametrize("n", [17, 257, 4097, BIG])
def test_combine_is_the_host_oracle_bit_for_bit(dev, n, Wc, pad):
    theta = _randn(n, n)
    ups = [ref.sign_quantize(theta + 0.1 * _randn(n, 100 * Wc + c), theta, torch.zeros(n)) for c in range(Wc)]
    codes, scales = (torch.stack(t) for t in zip(*ups))  # (rows of ceil(n / 8) bytes: odd strides, rows c >= 1 unaligned)
    w = torch.rand(Wc, generator=torch.Generator().manual_seed(Wc)) + 0.5
    _same(ops.sign_combine(_off(theta, pad, dev), codes.to(dev), scales.to(dev), w.to(dev)), ref.sign_combine(theta, codes, scales, w))


@pytest.mark.parametrize("n,nan_at", [(4097, None), (BIG, None), (BIG, 4096 + 5)])
def test_rotate_quantize_is_the_host_composition_bit_for_bit(dev, n, nan_at):
    local, theta = _randn(n, n + 3), _randn(n, n + 4)
    if nan_at is not None:
        local[nan_at] = float("nan")
    res = 0.05 * _randn(ref.rotate_pad(n), 9)
    dres = res.to(dev)
    want = ref.rotate_sign_quantize(local, theta, res, 7)
    got = ops.rotate_sign_quantize(local.to(dev), theta.to(dev), dres, 7)
    for g, w in zip((*got, dres), (*want, res)):
        _same(g, w)
    if nan_at is not None:  # all 16 blocks of the chunk, and no other
        assert torch.equal(torch.isnan(want[1]).nonzero().flatten(), torch.arange(16, 32))


@pytest.mark.parametrize("Wc", [1, 3])
@pytest.mark.parametrize("n", [4097, BIG])
def test_rotate_combine_is_the_host_composition_bit_for_bit(dev, n, Wc):
    n_pad, theta = ref.rotate_pad(n), _randn(n, n)
    ups = [ref.rotate_sign_quantize(theta + 0.1 * _randn(n, 10 * Wc + c), theta, torch.zeros(n_pad), 7) for c in range(Wc)]
    codes, scales = (torch.stack(t) for t in zip(*ups))
    w = torch.tensor([2.0, 1.0, 4.5][:Wc])
    _same(ops.rotate_sign_combine(theta.to(dev), codes.to(dev), scales.to(dev), w.to(dev), 7),
          ref.rotate_sign_combine(theta, codes, scales, w, 7))


@pytest.mark.parametrize("fraction,rotate", [(0.0, 0), (0.05, 0), (0.0, 1)])
def test_the_device_codec_packs_the_hosts_words_over_two_rounds(dev, fraction, rotate):
    n = BIG
    host, devc = (SignUpload(1, 5, fraction, rotate).plan_for(n, d) for d in ("cpu", dev))
    theta = _randn(n, 1)
    rh, rd = (None, None) if rotate else (torch.zeros(n), torch.zeros(n, device=dev))
    for rnd in range(2):  # (the second round starts from the first one's residual)
        local = theta + 0.1 * _randn(n, 20 + rnd) ** 3
        blob_h = host.pack(host.compress(local, theta, rh, 1, rnd))
        blob_d = devc.pack(devc.compress(local.to(dev), theta.to(dev), rd, 1, rnd))
        _same(blob_d, blob_h)
        _same(*((devc.basis, host.basis) if rotate else (rd, rh)))
        _same(devc.received(theta.to(dev), devc.unpack(blob_d, n)), host.received(theta, host.unpack(blob_h, n)))


def test_two_clients_on_the_card_combine_among_themselves_to_the_host_coordinators_bits(tmp_path, dev):
    (rec,) = star(tmp_path, 1, [*FLAGS, "--upload_sign=1"], "allreduce", SHARE, timeout=400)
    want, flat = expected_round0(tmp_path, FLAGS, 0)
    assert_global_is(tmp_path, want, flat)
    assert rec["clients_accepted"] == W and rec["upload_sign"] == 1 and rec["upload_bytes"] < 0.05 * rec["dense_bytes"]
