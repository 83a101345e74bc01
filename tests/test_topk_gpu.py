"""Catalog top-k on the MI355X (csrc/topk_scores.hip) against the fp64 torch oracle on the CPU
(``ops.reference.topk_scores``): exact on integer-valued operands (every product and sum is exact
in fp32, ties are massive), bitwise independent of the table split count, the worst-case insertion
orders, short lists, and random fp32 operands within the derived summation bound."""
import copy

import numpy as np
import pytest
import torch

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.config import BackboneConfig, FedRecConfig
from fedrec_with_pytorchdistributed_amd.data.sampler import validation_batches
from fedrec_with_pytorchdistributed_amd.data.synthetic import make_client_shards
from fedrec_with_pytorchdistributed_amd.models.fedrec_model import FedRecModel
from fedrec_with_pytorchdistributed_amd.ops import native
from fedrec_with_pytorchdistributed_amd.ops import reference as ref
from fedrec_with_pytorchdistributed_amd.train.engine import LocalEngine

pytestmark = pytest.mark.gpu


def _bits(x: torch.Tensor) -> torch.Tensor:
    """fp32 bit patterns with the two zeros folded together (the kernel ranks -0 as +0)."""
    return (x.detach().float().cpu() + 0.0).view(torch.int32)


def _oracle(u, t, k, ex, min_id):
    return ref.topk_scores(u.double().cpu(), t.double().cpu(), k, None if ex is None else ex.cpu(), min_id)


def _check_exact(dev, u, t, k, ex, min_id):
    s, i = ops.topk_scores(u.to(dev), t.to(dev), k, None if ex is None else ex.to(dev), min_id)
    so, io = _oracle(u, t, k, ex, min_id)
    assert i.dtype == torch.int32 and s.dtype == torch.float32 and tuple(i.shape) == (u.shape[0], k)
    assert torch.equal(i.cpu(), io), (i.cpu() != io).nonzero()[:8]
    assert torch.equal(_bits(s), _bits(so))
    return s, i


def _ints(B, N, D, E, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.randint(-3, 4, (B, D), generator=g).float()
    t = torch.randint(-3, 4, (N, D), generator=g).float()
    ex = torch.randint(-2, N + 3, (B, E), generator=g).to(torch.int32)
    return u, t, ex


@pytest.mark.parametrize("with_ex", [False, True])
@pytest.mark.parametrize("B,N,D,k", [(1, 1, 4, 1), (17, 1000, 400, 10), (33, 5000, 400, 1), (33, 5000, 400, 10),
                                     (33, 5000, 400, 128), (5, 300, 512, 128)])
def test_exact_on_integer_operands(dev, B, N, D, k, with_ex):
    u, t, ex = _ints(B, N, D, 7, 100 + B + k)
    _check_exact(dev, u, t, k, ex if with_ex else None, 1 if with_ex and N > 1 else 0)


def test_split_count_does_not_change_a_bit(dev):
    u, t, ex = _ints(33, 5000, 400, 7, 5)
    lib = native.lib()
    outs = []
    try:
        for splits in (1, 2, 7, 0):
            lib.topk_set_splits(splits)
            s, i = _check_exact(dev, u, t, 10, ex, 1)
            outs.append((s.cpu().view(torch.int32), i.cpu()))
    finally:
        lib.topk_set_splits(0)
    for s, i in outs[1:]:
        assert torch.equal(s, outs[0][0]) and torch.equal(i, outs[0][1])


def test_adversarial_row_orders(dev):
    """Scores rising strictly with the row index make every table tile a survivor tile (the
    worst-case insertion path); falling scores fill the list once; a constant user ties everything."""
    N, D, k = 4096, 8, 128
    t = torch.zeros(N, D)
    t[:, 0] = torch.arange(N).float()
    t[:, 1] = 1.0
    u = torch.zeros(3, D)
    u[0, 0], u[1, 0], u[2, 1] = 1.0, -1.0, 1.0
    s, i = _check_exact(dev, u, t, k, None, 0)
    assert i[0].tolist() == list(range(N - 1, N - 1 - k, -1))
    assert i[1].tolist() == list(range(k)) and i[2].tolist() == list(range(k))
    lib = native.lib()
    try:
        lib.topk_set_splits(1)  # one block walks the whole rising table
        _check_exact(dev, u, t, k, None, 0)
    finally:
        lib.topk_set_splits(0)


def test_short_lists_excluded_top_and_nan_row(dev):
    g = torch.Generator().manual_seed(3)
    # N = 10, k = 16, 3 rows excluded, min_id = 1: 6 valid slots, then -1 / -inf
    u = torch.randint(-3, 4, (2, 8), generator=g).float()
    t = torch.randint(-3, 4, (10, 8), generator=g).float()
    ex = torch.tensor([[2, 5, 7, 7, -1, 10], [9, 1, 4, 0, 0, 99]], dtype=torch.int32)
    s, i = _check_exact(dev, u, t, 16, ex, 1)
    assert (i[:, :6] >= 1).all() and (i[:, 6:] == -1).all() and torch.isinf(s[:, 6:]).all() and (s[:, 6:] < 0).all()
    # one NaN table row is never returned
    t2 = t.clone()
    t2[4] = float("nan")
    s, i = _check_exact(dev, u, t2, 16, None, 1)
    assert not (i == 4).any() and (i[:, :8] >= 1).all() and (i[:, 8:] == -1).all() and not torch.isnan(s).any()
    # a user whose entire top-k is excluded gets the next k
    u3 = torch.randint(-3, 4, (3, 16), generator=g).float()
    t3 = torch.randint(-3, 4, (700, 16), generator=g).float()
    _, top = _oracle(u3, t3, 9, None, 1)
    s, i = _check_exact(dev, u3, t3, 9, top, 1)
    assert not (i.cpu()[:, :, None] == top[:, None, :]).any()
    # everything excluded: an empty list
    allx = torch.arange(10, dtype=torch.int32).repeat(2, 1)
    s, i = _check_exact(dev, u, t, 4, allx, 0)
    assert (i == -1).all()


def _check_within_bound(s, i, S, tau, elig, k):
    """(a)-(d) of a device result (s, i) [B, k] against fp64 scores S [B, N], per-element bound tau
    and the eligibility mask."""
    B, N = S.shape
    i64 = i.long()
    assert (i64 >= 0).all() and (i64 < N).all()
    for b in range(B):
        assert len(set(i64[b].tolist())) == k                                    # (a) unique
    assert elig.gather(1, i64).all()                                              # (a) eligible
    So, To = S.gather(1, i64), tau.gather(1, i64)
    assert ((s.double() - So).abs() <= To).all(), float(((s.double() - So).abs() - To).max())  # (b)
    d = s[:, 1:] - s[:, :-1]
    assert (d <= 0).all()                                                         # (c) non-increasing
    assert ((d < 0) | (i64[:, 1:] > i64[:, :-1])).all()                           # (c) ties by ascending id
    rest = elig.clone()
    rest.scatter_(1, i64, False)
    lim = (So[:, -1] + To[:, -1])[:, None] + tau                                  # (d)
    assert (~rest | (S <= lim)).all(), float((S - lim)[rest].max())


def test_random_fp32_operands_within_the_summation_bound(dev):
    """tau[b, n] = gamma sum_d |u_d v_d|, gamma = D 2^-24 / (1 - D 2^-24): the worst-case error of a
    D-term fp32 dot product summed in any order (Higham, Accuracy and Stability, eq. 3.5)."""
    B, N, D, k, E = 64, 3000, 400, 20, 7
    g = torch.Generator().manual_seed(11)
    u, t = torch.randn(B, D, generator=g), torch.randn(N, D, generator=g)
    ex = torch.randint(-2, N + 3, (B, E), generator=g).to(torch.int32)
    s, i = ops.topk_scores(u.to(dev), t.to(dev), k, ex.to(dev), 1)
    gamma = D * 2.0 ** -24 / (1 - D * 2.0 ** -24)
    S = u.double() @ t.double().t()
    tau = gamma * (u.double().abs() @ t.double().abs().t())
    elig = torch.ones(B, N, dtype=torch.bool)
    elig[:, 0] = False
    exl = ex.long()
    okx = (exl >= 0) & (exl < N)
    for b in range(B):
        elig[b, exl[b][okx[b]]] = False
    _check_within_bound(s.cpu(), i.cpu(), S, tau, elig, k)


def test_launcher_rejects_what_it_was_not_written_for(dev):
    lib = native.lib()
    u, t = torch.zeros(4, 8, device=dev), torch.zeros(50, 8, device=dev)
    lib.topk_scores(u, t, 3, None, 0)
    bad = [
        lambda: lib.topk_scores(u.cpu(), t.cpu(), 3, None, 0),                    # host tensors
        lambda: lib.topk_scores(u, t.cpu(), 3, None, 0),
        lambda: lib.topk_scores(u.bfloat16(), t, 3, None, 0),                     # bf16 user
        lambda: lib.topk_scores(torch.zeros(4, 6, device=dev), torch.zeros(50, 6, device=dev), 3, None, 0),  # D = 6
        lambda: lib.topk_scores(u, t, 0, None, 0),                                # k = 0
        lambda: lib.topk_scores(u, t, 129, None, 0),                              # k = 129
        lambda: lib.topk_scores(u, torch.zeros(50, 16, device=dev)[:, :8], 3, None, 0),  # non-contiguous table
        lambda: lib.topk_scores(u, t, 3, torch.zeros(4, 2, dtype=torch.int64, device=dev), 0),  # int64 exclude
        lambda: lib.topk_scores(torch.zeros(4, 516, device=dev), torch.zeros(50, 516, device=dev), 3, None, 0),
    ]
    for f in bad:
        with pytest.raises((RuntimeError, NotImplementedError)):
            f()


# ---- engine ---------------------------------------------------------------------------------
N_IMP, K_ENG = 48, 10


@pytest.fixture(scope="module")
def engines(dev):
    cfg = FedRecConfig(mode="grad_avg", batch_size=16, user_dropout=0.0)
    cfg.backbone = BackboneConfig(name="distilbert-1l", n_layers=1)  # DistilBERT widths, 1 block (speed)
    torch.manual_seed(0)
    m_cpu = FedRecModel(cfg)
    m_gpu = copy.deepcopy(m_cpu).to(dev)
    m_cpu.build_flat()
    m_gpu.build_flat()
    shard = make_client_shards("tiny", 1)[0]
    e_cpu = LocalEngine(cfg, m_cpu, shard, torch.device("cpu"))
    e_gpu = LocalEngine(cfg, m_gpu, shard, dev)
    _, his = next(iter(validation_batches(shard.valid, N_IMP, cfg.npratio, cfg.max_his_len, True, N_IMP)))
    his = torch.from_numpy(his)
    t_c = e_cpu.encode_all()
    u_c = e_cpu.user_vectors(his, t_c)
    return e_cpu, e_gpu, his, t_c.double(), u_c.double()


def _engine_bound(e_gpu, his, t_c, u_c):
    """fp64 CPU scores S and the bound tau on |device score - S|: the fp32 summation bound plus the
    measured (max-abs, against the CPU engine) device differences of the user and news vectors
    pushed through the dot product: |u_g.v_g - u_c.v_c| <= |du| ||v_c||_1 + |dv| (||u_c||_1 + D |du|)."""
    t_g = e_gpu.encode_all()
    u_g = e_gpu.user_vectors(his, t_g)
    du = (u_g.cpu().double() - u_c).abs().max(1).values
    dv = float((t_g.cpu().double() - t_c).abs().max())
    D = t_c.shape[1]
    gamma = D * 2.0 ** -24 / (1 - D * 2.0 ** -24)
    S = u_c @ t_c.t()
    tau = (gamma * (u_c.abs() @ t_c.abs().t()) + du[:, None] * t_c.abs().sum(1)[None, :]
           + dv * (u_c.abs().sum(1) + D * du)[:, None])
    return t_g, S, tau


def test_engine_recommend_on_the_device(engines):
    e_cpu, e_gpu, his, t_c, u_c = engines
    t_g, S, tau = _engine_bound(e_gpu, his, t_c, u_c)
    ids, scores = e_gpu.recommend(his, k=K_ENG, table=t_g)
    assert ids.dtype == torch.int32 and tuple(ids.shape) == (N_IMP, K_ENG)
    elig = torch.ones_like(S, dtype=torch.bool)
    elig[:, 0] = False
    elig.scatter_(1, his.long(), False)  # history ids (and the pad id 0)
    _check_within_bound(scores.cpu(), ids.cpu(), S, tau, elig, K_ENG)


def test_engine_recommend_valid_device_vs_cpu(engines):
    e_cpu, e_gpu, his, t_c, u_c = engines
    m_g, ids_g, _ = e_gpu.recommend_valid(k=K_ENG, batch_size=16, limit=N_IMP, return_lists=True)
    m_c, ids_c, _ = e_cpu.recommend_valid(k=K_ENG, batch_size=16, limit=N_IMP, return_lists=True)
    assert m_g["n"] == m_c["n"] == N_IMP and set(m_g) == set(m_c)
    assert (ids_g >= 1).all()
    _, S, tau = _engine_bound(e_gpu, his, t_c, u_c)
    pos = np.asarray(e_cpu.shard.valid.pos[:N_IMP])
    # a device hit is a CPU hit, or the positive is within 2 tau of the CPU list's k-th score: if it
    # is not in the CPU list, some CPU-list row n is missing from the device list, so
    # S[kth] <= S[n] <= s_dev[n] + tau[n] <= s_dev[pos] + tau[n] <= S[pos] + tau[pos] + tau[n]
    for r in range(N_IMP):
        p = int(pos[r])
        if p in ids_g[r].tolist() and p not in ids_c[r].tolist():
            kth = int(ids_c[r][-1])
            assert float(S[r, p]) >= float(S[r, kth]) - 2 * float(tau[r].max()), (r, p)
