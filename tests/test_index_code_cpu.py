"""Elias-Fano index coding on the host: the plan written out, the integer oracles' round trip, what the decoder refuses,
the option, the two schemas, and one star round on gloo per top-k form whose global model must not move by a bit."""
import pytest
import torch

from test_quant_star_cpu import TINY, W, star

from fedrec_with_pytorchdistributed_amd.config import FedRecConfig
from fedrec_with_pytorchdistributed_amd.ops import reference as ref
from fedrec_with_pytorchdistributed_amd.parallel.control import encode_tensor
from fedrec_with_pytorchdistributed_amd.parallel.index_code import IndexCoded
from fedrec_with_pytorchdistributed_amd.parallel.upload import StarUpload
from fedrec_with_pytorchdistributed_amd.train.federated import build_model

# (n, k) -> (b, low_words, high_bits, high_words), each worked out by hand from the definition.  (300007, 2344) has
# 2344 << 7 = 300032 > n, so b = 6; (300007, 2343) is the neighbour with b = 7, where 32 % b != 0 as well
PLANS = {(2 ** 20, 1): (20, 1, 2, 1), (2 ** 20, 33): (14, 15, 97, 4), (2 ** 20, 1000): (10, 313, 2024, 64),
         (2 ** 20, 10486): (6, 1967, 26870, 840), (100003, 60000): (0, 0, 160003, 5001),
         (100003, 40000): (1, 1250, 90002, 2813), (4097, 4097): (0, 0, 8194, 257), (300007, 2344): (6, 440, 7032, 220),
         (300007, 2343): (7, 513, 4687, 147)}
PATTERNS = ("uniform", "clustered", "strided")


def indices(n, k, pattern):
    """``k`` strictly ascending int32 positions in ``[0, n)``."""
    if pattern == "uniform":
        return torch.randperm(n, generator=torch.Generator().manual_seed(k))[:k].sort().values.int()
    if pattern == "clustered":  # one saturated stretch, then a long empty one
        return torch.cat([torch.arange(k - 1), torch.tensor([n - 1])]).int()
    return (n - 1 - ((k - 1 - torch.arange(k)) * (n // k))).int()  # evenly strided, ending at n - 1


@pytest.mark.parametrize("nk", PLANS)
def test_the_plan_is_the_definition_written_out(nk):
    assert ref.ef_plan(*nk) == PLANS[nk]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("nk", PLANS)
def test_decode_of_encode_is_the_index_list(nk, pattern):
    (n, k), (b, lw, hb, hw) = nk, PLANS[nk]
    idx = indices(n, k, pattern)
    assert idx.numel() == k and int(idx[-1]) < n and (k == 1 or bool((idx[1:] > idx[:-1]).all()))
    words = ref.ef_encode(idx, n)
    assert words.dtype == torch.int32 and words.numel() == lw + hw
    i = k // 2  # one field and one high bit read straight from the words
    low = sum((w & 0xFFFFFFFF) << (32 * j) for j, w in enumerate(words[:lw].tolist()))
    assert (low >> (i * b)) & ((1 << b) - 1) == int(idx[i]) & ((1 << b) - 1) and low >> (k * b) == 0
    p = (int(idx[i]) >> b) + i
    assert (int(words[lw + p // 32]) >> (p % 32)) & 1
    assert torch.equal(ref.ef_decode(words, n, k), idx)


@pytest.mark.parametrize("what", ["ones", "random", "padding", "extra", "cleared"])
def test_the_host_decoder_refuses_what_no_encoder_made(what):
    n, k = 300007, 2344  # (k b % 32 = 16: the last low word has padding bits)
    b, lw, hb, hw = PLANS[n, k]
    words = ref.ef_encode(indices(n, k, "uniform"), n)
    high = ref._ef_bits(words[lw:])
    if what == "ones":
        words = torch.full_like(words, -1)
    elif what == "random":
        words = torch.randint(-2 ** 31, 2 ** 31, words.shape, generator=torch.Generator().manual_seed(0)).int()
    elif what == "padding":
        words[lw - 1] |= 1 << 30
    elif what == "extra":
        words[lw + int((high[:hb] == 0).nonzero()[7]) // 32] |= 1 << (int((high[:hb] == 0).nonzero()[7]) % 32)
    else:
        words[lw + int(high.nonzero()[7]) // 32] &= ~(1 << (int(high.nonzero()[7]) % 32))
    with pytest.raises(ValueError, match="padding bits" if what == "padding" else "set bits, expected k = 2344"):
        ref.ef_decode(words, n, k)


def test_the_option_is_taken_where_an_index_list_travels_and_refused_elsewhere():
    cfg = FedRecConfig()
    assert cfg.upload_index == "raw" and not isinstance(StarUpload.from_cfg(cfg, "fedavg_star"), IndexCoded)
    for flags in (["--upload_topk=0.1"], ["--upload_topk=0.1", "--upload_bits=4"], ["--upload_topk=0.1", "--upload_sign=1"]):
        cfg = FedRecConfig()
        cfg.apply_overrides([*flags, "--upload_index=ef"])
        qz, raw = StarUpload.from_cfg(cfg, "fedavg_star"), FedRecConfig()
        raw.apply_overrides(flags)
        assert type(qz) is IndexCoded and type(qz.inner) is type(StarUpload.from_cfg(raw, "fedavg_star"))
        assert qz.options == {**qz.inner.options, "upload_index": "ef"}
    for flags, driver, text in [
        (["--upload_index=golomb"], "fedavg_star", "upload_index=golomb: expected raw or ef"),
        (["--upload_index=ef"], "fedavg_star", "upload_index=ef needs upload_topk > 0"),
        (["--upload_index=ef", "--upload_bits=8"], "fedavg_star", "upload_index=ef needs upload_topk > 0"),
        (["--upload_index=ef", "--upload_topk=0.1"], "grad_avg", "upload_index=ef is not available with mode=grad_avg"),
        (["--upload_index=ef", "--upload_topk=0.1"], "param_avg", "upload_index=ef is not available with mode=param_avg"),
        (["--upload_index=ef", "--upload_bits=8", "--upload_rotate=1"], "fedavg_star",
         "upload_index=ef cannot be combined with upload_rotate=1"),
        (["--upload_index=ef", "--upload_rank=4"], "fedavg_star", "upload_index=ef cannot be combined with upload_rank=4"),
        (["--upload_index=ef", "--upload_sketch=0.1"], "fedavg_star",
         "upload_index=ef cannot be combined with upload_sketch=0.1"),
    ]:
        cfg = FedRecConfig()
        cfg.apply_overrides(flags)
        with pytest.raises(ValueError) as e:
            StarUpload.from_cfg(cfg, driver)
        assert text in str(e.value)


def test_the_two_index_schemas_match_the_fixture():
    from test_op_schemas_quant import GOLDEN, _registered
    with open(GOLDEN.replace("_quant", "_index")) as f:
        assert [ln for _, ln in sorted(_registered("fedrec_index::").items())] == f.read().splitlines()


def ef_words(form, n):
    """int32 words of one upload of ``form`` with its index list coded: the plan's words, then what follows ``idx``."""
    cfg = FedRecConfig()
    cfg.apply_overrides(["--upload_topk=0.1", *form])
    raw = StarUpload.from_cfg(cfg, "fedavg_star")
    k = raw.sparse.k_for(n)
    _, low_words, _, high_words = ref.ef_plan(n, k)
    return low_words + high_words + raw.words_for(n) - k


@pytest.mark.slow
@pytest.mark.parametrize("form", [[], ["--upload_bits=4"], ["--upload_sign=1"]])
def test_one_round_with_coded_indices_is_the_raw_round_bit_for_bit_in_fewer_bytes(tmp_path, form):
    flags = [*TINY, "--upload_topk=0.1", *form]
    (rec,) = star(tmp_path / "ef", 1, [*flags, "--upload_index=ef"], "upload")
    (raw,) = star(tmp_path / "raw", 1, flags, "upload")
    a = torch.load(tmp_path / "ef" / "global_model_round0.pt", weights_only=True)
    b = torch.load(tmp_path / "raw" / "global_model_round0.pt", weights_only=True)
    assert set(a) == set(b) and all(torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)) for name in a)
    cfg = FedRecConfig()
    cfg.apply_overrides(list(TINY))
    n = build_model(cfg, torch.device("cpu")).flat.flat.numel()
    words = ef_words(form, n)
    header = len(encode_tensor(torch.zeros(words, dtype=torch.int32))) - 4 * words
    print(f"upload / dense = {rec['upload_bytes'] / rec['dense_bytes']:.4f} coded, {raw['upload_bytes'] / raw['dense_bytes']:.4f} raw")
    assert rec["upload_index"] == "ef" and "upload_index" not in raw and rec["clients_accepted"] == W
    assert rec["dense_bytes"] == raw["dense_bytes"] == 4 * n * W
    assert rec["upload_bytes"] == W * (4 * words + header)
    assert rec["upload_bytes"] < raw["upload_bytes"]
