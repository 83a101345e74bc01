"""Catalog top-k on the host: the torch oracle's ordering contract, the top-k metrics, the engine's
``recommend`` / ``recommend_valid`` on the CPU path and the ``recommend`` CLI command."""
import json
import math

import numpy as np
import pytest
import torch

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.config import BackboneConfig, FedRecConfig
from fedrec_with_pytorchdistributed_amd.data.synthetic import make_client_shards
from fedrec_with_pytorchdistributed_amd.eval.metrics import topk_metrics
from fedrec_with_pytorchdistributed_amd.models.fedrec_model import FedRecModel
from fedrec_with_pytorchdistributed_amd.ops import reference as ref
from fedrec_with_pytorchdistributed_amd.train.engine import LocalEngine

NINF = float("-inf")


def _one_hot_user(D=4):
    u = torch.zeros(1, D, dtype=torch.float64)
    u[0, 0] = 1.0
    return u


def _table(scores, D=4):
    t = torch.zeros(len(scores), D, dtype=torch.float64)
    t[:, 0] = torch.tensor(scores, dtype=torch.float64)
    return t


def test_reference_ties_break_by_ascending_id():
    s, i = ref.topk_scores(_one_hot_user(), _table([1, 3, 3, 2, 3, 0]), 4)
    assert i.dtype == torch.int32 and s.dtype == torch.float64
    assert i.tolist() == [[1, 2, 4, 3]]
    assert s.tolist() == [[3, 3, 3, 2]]
    # the two zeros tie
    s, i = ref.topk_scores(_one_hot_user(), _table([-0.0, 0.0, -0.0, -1.0]), 3)
    assert i.tolist() == [[0, 1, 2]]


def test_reference_min_id_and_exclusion():
    t = _table([9, 8, 7, 6, 5, 4])
    s, i = ref.topk_scores(_one_hot_user(), t, 3, min_id=2)
    assert i.tolist() == [[2, 3, 4]] and s.tolist() == [[7, 6, 5]]
    # duplicate, negative and out-of-range entries are legal and ignored
    ex = torch.tensor([[3, 3, -1, 6, 1000, -7, 2]], dtype=torch.int32)
    s, i = ref.topk_scores(_one_hot_user(), t, 3, ex, 1)
    assert i.tolist() == [[1, 4, 5]] and s.tolist() == [[8, 5, 4]]
    # E = 0 is no exclusion
    s, i = ref.topk_scores(_one_hot_user(), t, 2, torch.zeros(1, 0, dtype=torch.int32), 0)
    assert i.tolist() == [[0, 1]]


def test_reference_short_lists_and_nan_rows():
    t = _table([5, float("nan"), 3, NINF, 1])
    s, i = ref.topk_scores(_one_hot_user(), t, 6, torch.tensor([[4]], dtype=torch.int32), 0)
    # the NaN row never appears; an eligible -inf score does, ahead of the empty tail
    assert i.tolist() == [[0, 2, 3, -1, -1, -1]]
    assert s.tolist() == [[5, 3, NINF, NINF, NINF, NINF]]
    # everything excluded
    s, i = ref.topk_scores(_one_hot_user(), _table([1, 2]), 2, torch.tensor([[0, 1]], dtype=torch.int32))
    assert i.tolist() == [[-1, -1]] and s.tolist() == [[NINF, NINF]]


def test_reference_chunks_agree_and_ops_dispatches_host_tensors():
    g = torch.Generator().manual_seed(0)
    u = torch.randint(-3, 4, (37, 8), generator=g).double()
    t = torch.randint(-3, 4, (211, 8), generator=g).double()
    ex = torch.randint(-5, 230, (37, 6), generator=g).to(torch.int32)
    a = ref.topk_scores(u, t, 9, ex, 1, chunk=5)
    b = ref.topk_scores(u, t, 9, ex, 1, chunk=64)
    c = ops.topk_scores(u, t, 9, ex, 1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    # against a plain python sort of every user
    S = u @ t.t()
    for b_ in range(37):
        bad = set(ex[b_].tolist())
        rows = [n for n in range(1, 211) if n not in bad]
        rows.sort(key=lambda n: (-float(S[b_, n]), n))
        assert a[1][b_].tolist() == rows[:9]


def test_topk_metrics_against_a_direct_loop():
    rng = np.random.default_rng(0)
    ids = np.stack([rng.permutation(40)[:10] for _ in range(200)]).astype(np.int32)
    ids[::7, 5:] = -1
    pos = rng.integers(0, 40, 200).astype(np.int32)
    hr = nd = mrr = 0.0
    for i in range(200):
        lst = ids[i].tolist()
        if int(pos[i]) in lst:
            r = lst.index(int(pos[i])) + 1
            hr += 1
            nd += 1.0 / math.log2(r + 1)
            mrr += 1.0 / r
    m = topk_metrics(ids, pos)
    assert m["n"] == 200 and m["k"] == 10
    assert m["hr@10"] == pytest.approx(hr / 200) and 0 < m["hr@10"] < 1
    assert m["ndcg@10"] == pytest.approx(nd / 200)
    assert m["mrr@10"] == pytest.approx(mrr / 200)
    assert topk_metrics(np.zeros((0, 5), np.int32), np.zeros(0, np.int32))["n"] == 0


@pytest.fixture(scope="module")
def cpu_engine():
    cfg = FedRecConfig(mode="grad_avg", batch_size=16)
    cfg.backbone = BackboneConfig.preset("tiny")
    torch.manual_seed(0)
    model = FedRecModel(cfg)
    model.build_flat()
    shard = make_client_shards("tiny", 1)[0]
    return LocalEngine(cfg, model, shard, torch.device("cpu"))


def test_engine_recommend_matches_brute_force(cpu_engine):
    eng = cpu_engine
    his = torch.zeros(6, 50, dtype=torch.int32)
    g = torch.Generator().manual_seed(1)
    for b in range(6):
        n = 3 + 7 * b
        his[b, :n] = torch.randint(1, eng.N, (n,), generator=g).to(torch.int32)
    table = eng.encode_all()
    ids, scores = eng.recommend(his, k=12, table=table)
    assert ids.shape == (6, 12) and ids.dtype == torch.int32 and scores.dtype == torch.float32
    u = eng.user_vectors(his, table)
    assert u.shape == (6, eng.cfg.news_dim)
    S = u @ table.t()
    for b in range(6):
        seen = set(his[b].tolist())
        got = ids[b].tolist()
        assert 0 not in got and not (set(got) & seen)
        rows = [n for n in range(1, eng.N) if n not in seen]
        rows.sort(key=lambda n: (-float(S[b, n]), n))
        assert got == rows[:12]
        assert torch.equal(scores[b], S[b, got])
    # with the history allowed back in, only row 0 stays out
    ids2, _ = eng.recommend(his, k=12, exclude_history=False, table=table)
    for b in range(6):
        rows = sorted(range(1, eng.N), key=lambda n: (-float(S[b, n]), n))
        assert ids2[b].tolist() == rows[:12]


def test_recommend_valid_is_topk_metrics_of_recommend(cpu_engine):
    from fedrec_with_pytorchdistributed_amd.data.sampler import validation_batches

    eng = cpu_engine
    n, k = 40, 7
    m, ids, scores = eng.recommend_valid(k=k, batch_size=16, limit=n, return_lists=True)
    assert ids.shape == (n, k) and scores.shape == (n, k) and m["n"] == n
    table = eng.encode_all()
    parts = [eng.recommend(h, k=k, table=table)[0]
             for _, h in validation_batches(eng.shard.valid, 16, eng.cfg.npratio, eng.cfg.max_his_len, True, n)]
    want = torch.cat(parts).numpy()
    assert np.array_equal(ids, want)
    assert m == topk_metrics(want, eng.shard.valid.pos[:n])
    assert eng.recommend_valid(k=k, batch_size=16, limit=n) == m


def test_cli_recommend_writes_ranked_lists(tmp_path, capsys):
    from fedrec_with_pytorchdistributed_amd import cli

    out = tmp_path / "recs.jsonl"
    m = cli.main_recommend(["none", "--data_dir=synthetic:tiny", "--backbone.name=tiny", "--device=cpu", "--k=5",
                            "--limit=8", f"--out={out}"])
    lines = [json.loads(x) for x in out.read_text().splitlines()]
    assert len(lines) == 8
    for rec in lines:
        assert set(rec) == {"uid", "news", "scores"}
        assert len(rec["news"]) == 5 and all(isinstance(x, str) and x != "<unk>" for x in rec["news"])
        assert len(set(rec["news"])) == 5
        assert rec["scores"] == sorted(rec["scores"], reverse=True)
    last = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert last == m and m["n"] == 8 and m["k"] == 5 and {"hr@5", "ndcg@5", "mrr@5"} <= set(m)
    assert "recommend" in cli.COMMANDS
