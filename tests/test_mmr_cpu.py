"""Diversity re-rank on the host: the torch oracle of ``mmr_rerank`` against a plain Python double
loop, ``diversity_metrics`` against a direct loop, the host dispatch of ``ops.mmr_rerank``, the
``recommend`` CLI command with ``--diversity`` / ``--pool``, the ``fedrec_rerank::`` schema pin and the
binding's argument checks (they run before the device check, so they can be driven without a GPU)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.eval.metrics import diversity_metrics
from fedrec_with_pytorchdistributed_amd.ops import native
from fedrec_with_pytorchdistributed_amd.ops import reference as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "op_schemas_rerank.txt")
NINF = float("-inf")


def _loop_mmr(table, ids, rel, k, lam):
    """The contract, one user at a time, in Python floats (fp64)."""
    out = []
    for b in range(len(ids)):
        row, r = list(ids[b]), list(rel[b])
        P = len(row)
        valid = [j for j in range(P) if row[j] >= 0]
        rhat = [0.0] * P
        if valid:
            mn, mx = min(r[j] for j in valid), max(r[j] for j in valid)
            for j in range(P):
                rhat[j] = 1.0 if mx == mn else (r[j] - mn) / (mx - mn)
        x = [table[max(i, 0)] for i in row]
        g = [[math.fsum(a * c for a, c in zip(x[i], x[j])) for j in range(P)] for i in range(P)]

        def cos(i, j):
            ok = all(math.isfinite(v) for v in (g[i][i], g[j][j], g[i][j])) and g[i][i] > 0 and g[j][j] > 0
            return g[i][j] / (math.sqrt(g[i][i]) * math.sqrt(g[j][j])) if ok else 0.0

        picked = []
        for t in range(k):
            best, bj = None, -1
            for j in valid:
                if j in picked:
                    continue
                m = lam * rhat[j] - ((1 - lam) * max(cos(i, j) for i in picked) if picked else 0.0)
                m = NINF if math.isnan(m) else m
                if best is None or m > best:
                    best, bj = m, j
            if bj < 0:
                break
            picked.append(bj)
        pairs = [(i, j) for a, i in enumerate(picked) for j in picked[a + 1:]]
        ild = sum(1 - cos(i, j) for i, j in pairs) / len(pairs) if pairs else 0.0
        pad = k - len(picked)
        out.append(([row[j] for j in picked] + [-1] * pad, [r[j] for j in picked] + [NINF] * pad, ild))
    return out


def _check_against_loop(table, ids, rel, k, lam):
    t = torch.tensor(table, dtype=torch.float64)
    i = torch.tensor(ids, dtype=torch.int32)
    r = torch.tensor(rel, dtype=torch.float64)
    io, ro, ild = ref.mmr_rerank(t, i, r, k, lam)
    assert io.dtype == torch.int32 and ro.dtype == torch.float64 and ild.dtype == torch.float64
    assert io.shape == (len(ids), k) and ro.shape == (len(ids), k) and ild.shape == (len(ids),)
    for b, (wi, wr, wild) in enumerate(_loop_mmr(table, ids, rel, k, lam)):
        assert io[b].tolist() == wi, (b, io[b].tolist(), wi)
        assert ro[b].tolist() == wr, b
        assert float(ild[b]) == pytest.approx(wild, abs=1e-12), b
    return io, ro, ild


# ---- the oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.0, 0.3, 0.7, 1.0])
def test_reference_against_a_double_loop_on_random_pools(lam):
    g = torch.Generator().manual_seed(3)
    N, D, B, P, k = 40, 8, 6, 12, 7
    table = torch.randn(N, D, generator=g, dtype=torch.float64)
    table[5] = table[9]  # a duplicate row
    ids = torch.stack([torch.randperm(N, generator=g)[:P] for _ in range(B)])
    rel = torch.sort(torch.randn(B, P, generator=g, dtype=torch.float64), dim=1, descending=True).values
    io, _, _ = _check_against_loop(table.tolist(), ids.tolist(), rel.tolist(), k, lam)
    if lam == 1.0:
        assert torch.equal(io, ids[:, :k].to(torch.int32))


def test_reference_short_pools_constant_rel_and_ties():
    table = [[1.0, 0.0], [2.0, 0.0], [0.0, 1.0], [0.0, 4.0], [1.0, 1.0], [0.0, 0.0]]
    ids = [[0, 2, 4, 1, 3],        # full pool
           [0, 2, -1, -1, -1],     # L = 2 = k - 1
           [3, -1, -1, -1, -1],    # L = 1
           [-1, -1, -1, -1, -1],   # L = 0
           [0, 1, 2, 3, 5]]        # rows 0 / 1 and 2 / 3 are parallel, row 5 is zero
    rel = [[5.0, 4.0, 3.0, 2.0, 1.0],
           [2.0, 1.0, 9.0, 9.0, 9.0],  # the empty slots' rel stays out of min / max
           [7.0, 0.0, 0.0, 0.0, 0.0],
           [0.0, 0.0, 0.0, 0.0, 0.0],
           [1.0, 1.0, 1.0, 1.0, 1.0]]  # rel_max == rel_min: rhat = 1
    io, ro, ild = _check_against_loop(table, ids, rel, 3, 0.5)
    assert io[1].tolist() == [0, 2, -1] and ro[1].tolist() == [2.0, 1.0, NINF]
    assert io[2].tolist() == [3, -1, -1] and float(ild[2]) == 0.0
    assert io[3].tolist() == [-1, -1, -1] and ro[3].tolist() == [NINF] * 3 and float(ild[3]) == 0.0
    # equal rhat everywhere: slot 0 first, then the lowest position among the least similar -- rows 2, 3
    # (cos 0 with row 0) tie with the zero row 5 (cos 0 with everything): position decides
    assert io[4].tolist() == [0, 2, 5]
    assert float(ild[1]) == 1.0  # rows 0 and 2 are orthogonal


def test_reference_nan_objective_counts_as_minus_inf():
    # an infinite relevance makes every rhat of the pool NaN ((x + inf) / inf): all objectives are
    # -inf and the lowest positions win
    table = [[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [1.0, 2.0]]
    io, ro, _ = _check_against_loop(table, [[2, 0, 3, 1]], [[3.0, 2.0, 1.0, NINF]], 3, 0.6)
    assert io[0].tolist() == [2, 0, 3] and ro[0].tolist() == [3.0, 2.0, 1.0]
    # a NaN relevance poisons min / max the same way
    io, _, _ = ref.mmr_rerank(torch.tensor(table), torch.tensor([[2, 0, 3, 1]], dtype=torch.int32),
                              torch.tensor([[3.0, float("nan"), 1.0, 0.0]]), 4, 0.6)
    assert io[0].tolist() == [2, 0, 3, 1]


def test_reference_defers_a_duplicate_and_runs_in_the_input_dtype():
    table = torch.tensor([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]])
    ids = torch.tensor([[0, 1, 2, 3]], dtype=torch.int32)
    rel = torch.tensor([[4.0, 3.9, 3.8, 3.7]])
    io, ro, ild = ref.mmr_rerank(table, ids, rel, 4, 0.5)
    assert io.dtype == torch.int32 and ro.dtype == torch.float32 and ild.dtype == torch.float32
    # rhat = 1, 2/3, 1/3, 0: after slot 0 the objectives are -1/6 (its duplicate), -2/15 (cos 0.6), 0
    assert io[0].tolist() == [0, 3, 2, 1]  # the duplicate of the first pick goes last
    assert torch.equal(ro[0], rel[0][[0, 3, 2, 1]])
    io1, ro1, _ = ref.mmr_rerank(table, ids, rel, 4, 1.0)
    assert torch.equal(io1, ids) and torch.equal(ro1, rel)
    assert ref.mmr_rerank(table.double(), ids, rel.double(), 2, 0.0)[0][0, 0].item() == 0  # lam = 0: slot 0 first
    for bad in ((5, 0.5), (0, 0.5), (2, 1.5), (2, -0.1)):
        with pytest.raises(ValueError):
            ref.mmr_rerank(table, ids, rel, *bad)


def test_ops_dispatches_host_tensors_to_the_reference():
    g = torch.Generator().manual_seed(5)
    table = torch.randn(30, 8, generator=g)
    ids = torch.stack([torch.randperm(30, generator=g)[:10] for _ in range(4)]).to(torch.int32)
    rel = torch.sort(torch.randn(4, 10, generator=g), dim=1, descending=True).values
    got, want = ops.mmr_rerank(table, ids, rel, 5, 0.4), ref.mmr_rerank(table, ids, rel, 5, 0.4)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a, b)


# ---- diversity_metrics ----------------------------------------------------------------------
def test_diversity_metrics_against_a_direct_loop():
    rng = np.random.default_rng(2)
    ids = rng.integers(1, 50, size=(60, 6)).astype(np.int32)
    ids[3, 1:] = -1   # one item: no pair, left out of ild@k
    ids[7, :] = -1    # empty
    ids[9, 2:] = -1   # two items: counted
    ild = rng.random(60).astype(np.float32)
    m = diversity_metrics(ids, ild, 49)
    seen, tot, cnt = set(), 0.0, 0
    for i in range(60):
        items = [int(x) for x in ids[i] if x >= 0]
        seen.update(items)
        if len(items) >= 2:
            tot, cnt = tot + float(ild[i]), cnt + 1
    assert set(m) == {"ild@6", "coverage@6"} and cnt == 58
    assert m["ild@6"] == pytest.approx(tot / cnt) and m["coverage@6"] == pytest.approx(len(seen) / 49)
    e = diversity_metrics(np.zeros((0, 6), np.int32), np.zeros(0), 49)
    assert math.isnan(e["ild@6"]) and math.isnan(e["coverage@6"])
    one = diversity_metrics(np.array([[4, -1]], np.int32), np.zeros(1), 10)
    assert math.isnan(one["ild@2"]) and one["coverage@2"] == pytest.approx(0.1)


# ---- the CLI --------------------------------------------------------------------------------
_CLI = ["none", "--data_dir=synthetic:tiny", "--backbone.name=tiny", "--device=cpu", "--k=5", "--limit=8"]


def _lists(path):
    return [json.loads(x) for x in path.read_text().splitlines()]


def test_cli_diversity_one_reproduces_the_plain_lists(tmp_path, capsys):
    from fedrec_with_pytorchdistributed_amd import cli

    a, b = tmp_path / "plain.jsonl", tmp_path / "lam1.jsonl"
    m0 = cli.main_recommend(_CLI + [f"--out={a}"])
    m1 = cli.main_recommend(_CLI + ["--diversity=1", f"--out={b}"])
    assert _lists(a) == _lists(b)
    assert set(m0) == {"hr@5", "ndcg@5", "mrr@5", "k", "n"}
    assert set(m1) == set(m0) | {"ild@5", "coverage@5", "diversity", "pool"}
    assert all(m1[key] == m0[key] for key in m0)
    assert m1["diversity"] == 1.0 and m1["pool"] == 32 and 0.0 <= m1["ild@5"] <= 2.0 and 0.0 < m1["coverage@5"] <= 1.0
    capsys.readouterr()


def test_cli_diversity_rerank_writes_distinct_eligible_lists(tmp_path, capsys):
    from fedrec_with_pytorchdistributed_amd import cli

    out = tmp_path / "mmr.jsonl"
    m = cli.main_recommend(_CLI + ["--diversity=0.5", "--pool=32", f"--out={out}"])
    lines = _lists(out)
    assert len(lines) == 8
    for rec in lines:
        assert set(rec) == {"uid", "news", "scores"}
        assert len(rec["news"]) == 5 and len(set(rec["news"])) == 5
        assert all(isinstance(x, str) and x != "<unk>" for x in rec["news"])
        assert all(math.isfinite(s) for s in rec["scores"])
    last = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert last == m and m["n"] == 8 and m["k"] == 5 and m["diversity"] == 0.5 and m["pool"] == 32
    from fedrec_with_pytorchdistributed_amd.data.synthetic import make_client_shards

    distinct = len({x for rec in lines for x in rec["news"]})
    assert 0.0 <= m["ild@5"] <= 2.0
    assert m["coverage@5"] == pytest.approx(distinct / (make_client_shards("tiny", 1)[0].num_news - 1))


@pytest.mark.parametrize("args", [["--diversity=1.5"], ["--diversity=-0.1"], ["--diversity=abc"], ["--diversity=nan"],
                                  ["--diversity=0.5", "--pool=4"], ["--diversity=0.5", "--pool=129"],
                                  ["--diversity=0.5", "--pool=x"], ["--pool=32"]])
def test_cli_rejects_bad_diversity_and_pool(args):
    from fedrec_with_pytorchdistributed_amd import cli

    with pytest.raises(SystemExit) as e:
        cli.main_recommend(_CLI + args)
    assert "usage: recommend" in str(e.value)


# ---- the engine on the host path ------------------------------------------------------------
def test_engine_diversity_none_is_the_plain_path_and_pool_bounds():
    from fedrec_with_pytorchdistributed_amd.config import BackboneConfig, FedRecConfig
    from fedrec_with_pytorchdistributed_amd.data.synthetic import make_client_shards
    from fedrec_with_pytorchdistributed_amd.models.fedrec_model import FedRecModel
    from fedrec_with_pytorchdistributed_amd.train.engine import LocalEngine

    cfg = FedRecConfig(mode="grad_avg", batch_size=16)
    cfg.backbone = BackboneConfig.preset("tiny")
    torch.manual_seed(0)
    model = FedRecModel(cfg)
    model.build_flat()
    eng = LocalEngine(cfg, model, make_client_shards("tiny", 1)[0], torch.device("cpu"))
    assert [LocalEngine.mmr_pool(k) for k in (1, 5, 10, 40, 128)] == [32, 32, 40, 128, 128]
    for k, pool in ((10, 9), (10, 129), (129, None)):
        with pytest.raises(ValueError):
            LocalEngine.mmr_pool(k, pool)
    plain = eng.recommend_valid(k=5, batch_size=16, limit=20)
    assert set(plain) == {"hr@5", "ndcg@5", "mrr@5", "k", "n"}
    m1, ids1, sc1 = eng.recommend_valid(k=5, batch_size=16, limit=20, return_lists=True, diversity=1.0)
    _, ids0, sc0 = eng.recommend_valid(k=5, batch_size=16, limit=20, return_lists=True)
    assert np.array_equal(ids0, ids1) and np.array_equal(sc0, sc1)
    assert all(m1[key] == plain[key] for key in plain) and set(m1) - set(plain) == {"ild@5", "coverage@5",
                                                                                   "diversity", "pool"}
    with pytest.raises(ValueError):
        eng.recommend_valid(k=5, limit=4, diversity=1.2)
    # the re-ranked list is a reordering of a subset of the pool, scores are the picks' own
    his = torch.zeros(3, 50, dtype=torch.int32)
    his[:, :4] = torch.tensor([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]], dtype=torch.int32)
    table = eng.encode_all()
    ids, sc = eng.recommend(his, 5, table=table, diversity=0.3, pool=20)
    pid, psc = eng.recommend(his, 20, table=table)
    for b in range(3):
        where = [pid[b].tolist().index(x) for x in ids[b].tolist()]
        assert len(set(where)) == 5 and where[0] == 0
        assert sc[b].tolist() == [float(psc[b, w]) for w in where]


# ---- the registered interface ---------------------------------------------------------------
def _registered_rerank():
    native.lib()
    out = {}
    for name in torch._C._dispatch_get_all_op_names():
        if not name.startswith("fedrec_rerank::"):
            continue
        kinds = [k for k in ("CUDA", "CompositeImplicitAutograd", "CompositeExplicitAutograd")
                 if torch._C._dispatch_has_kernel_for_dispatch_key(name, k)]
        out[name] = f"{torch._C._get_schema(name, '')} | {'+'.join(kinds) or 'none'}"
    return out


def test_rerank_namespace_matches_its_fixture():
    with open(GOLDEN) as f:
        want = {ln.split("(", 1)[0]: ln.rstrip("\n") for ln in f if ln.strip()}
    assert _registered_rerank() == want
    assert set(want) == {"fedrec_rerank::mmr_rerank"}
    assert "(Tensor table, Tensor ids, Tensor rel, int k, float lam) -> (Tensor, Tensor, Tensor)" in want[
        "fedrec_rerank::mmr_rerank"]
    names = torch._C._dispatch_get_all_op_names()
    assert not [n for n in names if n.startswith(("fedrec::mmr", "fedrec_eval::mmr"))]


def test_binding_argument_checks_raise():
    native.lib()
    op = torch.ops.fedrec_rerank.mmr_rerank
    table = torch.zeros(10, 8)
    ids = torch.zeros(2, 6, dtype=torch.int32)
    rel = torch.zeros(2, 6)
    cases = [
        ((table, ids, rel, 7, 0.5), "1 <= k <= P"),
        ((table, ids, rel, 0, 0.5), "1 <= k <= P"),
        ((table, torch.zeros(2, 129, dtype=torch.int32), torch.zeros(2, 129), 5, 0.5), "1 <= P <= 128"),
        ((table, ids, rel, 3, 1.01), "0 <= lam <= 1"),
        ((table, ids, rel, 3, -0.01), "0 <= lam <= 1"),
        ((table, ids, rel, 3, float("nan")), "0 <= lam <= 1"),
        ((torch.zeros(10, 6), ids, rel, 3, 0.5), "D % 4 == 0"),
        ((torch.zeros(10, 516), ids, rel, 3, 0.5), "D % 4 == 0"),
        ((table.double(), ids, rel, 3, 0.5), "must be fp32"),
        ((table, ids, rel.double(), 3, 0.5), "must be fp32"),
        ((table, ids.long(), rel, 3, 0.5), "must be int32"),
        ((table, ids, torch.zeros(2, 5), 3, 0.5), "ids [B, P], rel [B, P]"),
        ((table, ids.reshape(-1), rel.reshape(-1), 3, 0.5), "ids [B, P], rel [B, P]"),
        # everything else in order: a host tensor stops at the device check
        ((table, ids, rel, 3, 0.5), "must be a device tensor"),
    ]
    for args, msg in cases:
        with pytest.raises(RuntimeError) as e:
            op(*args)
        assert msg in str(e.value), (msg, str(e.value)[:200])
