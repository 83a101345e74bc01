"""The Elias-Fano kernels (csrc/index_code.hip) against the integer oracles of ops/reference.py, bit for bit, the device
codec's words and rejections, and two clients that share the card, code their index lists and decode each other's.

The kernels cut the high section into tiles of 256 words: (2^20, 10486) crosses 4 of them, the two n = 100003 cases 20
and 11 (nearly all of them empty under the clustered pattern), (4097, 4097) ends one word into its second."""
import pytest
import torch

from test_index_code_cpu import PATTERNS, PLANS, indices
from test_quant_star_cpu import W, assert_global_is, expected_round0, star
from test_quant_star_gpu import FLAGS, SHARE

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import reference as ref
from fedrec_with_pytorchdistributed_amd.parallel.control import encode_tensor
from fedrec_with_pytorchdistributed_amd.parallel.index_code import IndexCoded
from fedrec_with_pytorchdistributed_amd.parallel.quantize import Quantizer
from fedrec_with_pytorchdistributed_amd.parallel.sign import SignUpload

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("nk", PLANS)
def test_encode_and_batched_decode_are_the_host_oracles_bit_for_bit(dev, nk, pattern):
    n, k = nk
    rows = [indices(n, k, pattern), indices(n, k, "uniform"), indices(n, k, "strided")]  # W = 3, different rows
    want = torch.stack([ref.ef_encode(r, n) for r in rows])
    assert torch.equal(ops.ef_encode(rows[0].to(dev), n).cpu(), want[0])
    idx, count = ops.ef_decode(want.to(dev), n, k)
    assert torch.equal(idx.cpu(), torch.stack(rows)) and count.tolist() == [k] * 3


@pytest.mark.parametrize("flip", ["extra", "cleared"])
def test_the_device_codec_packs_the_hosts_words_and_refuses_a_flipped_bit(dev, flip):
    n = 3 * 4096 + 1000
    host, devc = (IndexCoded(SignUpload(1, 5, 0.05)).plan_for(n, d) for d in ("cpu", dev))
    g = torch.Generator().manual_seed(2)
    theta = torch.randn(n, generator=g)
    local = theta + 0.1 * torch.randn(n, generator=g)
    blob = devc.pack(devc.compress(local.to(dev), theta.to(dev), torch.zeros(n, device=dev), 1, 0))
    assert torch.equal(blob.cpu(), host.pack(host.compress(local, theta, torch.zeros(n), 1, 0)))
    assert torch.equal(devc.unpack(blob, n).idx.cpu(), host.unpack(blob.cpu(), n).idx)
    _, low_words, high_bits, _ = ref.ef_plan(n, host.sparse.k_for(n))
    high = ref._ef_bits(blob[low_words:host.ef_words(n)].cpu())[:high_bits]
    at = (high == (0 if flip == "extra" else 1)).nonzero().flatten()
    p = int(at[at % 32 < 31][3])  # (bit 31 is the sign of the int32 word)
    blob[low_words + p // 32] ^= 1 << (p % 32)
    for codec, words in ((host, blob.cpu()), (devc, blob)):
        with pytest.raises(ValueError, match=f"{host.sparse.k_for(n) + (1 if flip == 'extra' else -1)} set bits, expected k"):
            codec.unpack(words, n)


def test_two_clients_on_the_card_decode_each_others_lists_to_the_host_oracles_bits(tmp_path, dev):
    (rec,) = star(tmp_path, 1, [*FLAGS, "--upload_bits=4", "--upload_topk=0.05", "--upload_index=ef"], "allreduce", SHARE,
                  timeout=400)
    want, flat, n = expected_round0(tmp_path, FLAGS, 4, 0.05)
    assert_global_is(tmp_path, want, flat)
    words = IndexCoded(Quantizer(4, 0, 0.05)).words_for(n)
    header = len(encode_tensor(torch.zeros(words, dtype=torch.int32))) - 4 * words
    assert rec["clients_accepted"] == W and rec["upload_index"] == "ef" and rec["upload_bytes"] == W * (4 * words + header)
