"""Full-impression ranking on the MI355X (csrc/rank_impressions.hip) against the fp64 torch oracle
on the CPU (``ops.reference.rank_impressions``): exact on integer-valued operands (every product
and sum is exact in fp32), bitwise independent of the batching, id ties in float data, float data
outside the fp32 dot-product error bound, a NaN table row, the host checks, and the engine's
``validate_full`` against the CPU engine."""
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

I_IMP = 96
# list lengths every corpus holds: around the 4 rows of a wave-instruction, the 8 of a loop turn, the
# 64 ids of an id load, the 128 negatives of a work item (127 / 128 / 129, 255 / 256 / 257, 384: one
# to three chunks, full and ragged), and one list of 40 chunks; the rest is Poisson(24)
FORCED = [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 384, 5000]


class Corpus:
    def __init__(self, N, D, seed, ints):
        rng = np.random.default_rng(seed)
        lens = rng.poisson(24, I_IMP)
        lens[rng.permutation(I_IMP)[:len(FORCED)]] = FORCED
        ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        pos = rng.integers(0, N, I_IMP)
        pos[::11] = 0  # id 0 is an ordinary row
        negs = rng.integers(0, N, int(ptr[-1]))
        negs[::13] = 0
        for i in range(I_IMP):  # planted id ties: the positive's own id inside two lists of three
            if lens[i] and i % 3:
                negs[ptr[i] + rng.integers(0, lens[i], 1 + lens[i] // 40)] = pos[i]
        if ints:
            u = rng.integers(-4, 5, (I_IMP, D)).astype(np.float32)
            t = rng.integers(-4, 5, (N, D)).astype(np.float32)
            t[N // 2:N // 2 + 40] = t[:40]  # equal rows under different ids (and integer scores tie often anyway)
        else:
            u = rng.standard_normal((I_IMP, D)).astype(np.float32)
            t = rng.standard_normal((N, D)).astype(np.float32)
        self.N, self.D, self.lens = N, D, lens
        self.user, self.table = torch.from_numpy(u), torch.from_numpy(t)
        self.pos = torch.from_numpy(pos.astype(np.int32))
        self.neg_ptr = torch.from_numpy(ptr)
        self.negs = torch.from_numpy(negs.astype(np.int32))

    def oracle(self, table=None):
        t = self.table if table is None else table
        return ref.rank_impressions(self.user.double(), t.double(), self.pos, self.neg_ptr, self.negs)

    def device(self, dev, table=None):
        t = self.table if table is None else table
        return [x.to(dev) for x in (self.user, t, self.pos, self.neg_ptr, self.negs)]

    def id_ties(self):
        return np.array([int((self.negs[self.neg_ptr[i]:self.neg_ptr[i + 1]] == self.pos[i]).sum())
                         for i in range(I_IMP)])


def _run(dev, c, batch=I_IMP, table=None):
    u, t, pos, ptr, negs = c.device(dev, table)
    parts = [ops.rank_impressions(u[s:s + batch].contiguous(), t, pos, ptr, negs, s) for s in range(0, I_IMP, batch)]
    out = torch.cat(parts)
    assert out.dtype == torch.int32 and tuple(out.shape) == (I_IMP, 4)
    return out.cpu()


@pytest.fixture(scope="module")
def float_corpus():
    return Corpus(300, 400, 1, ints=False)


@pytest.fixture(scope="module")
def float_full(dev, float_corpus):
    return _run(dev, float_corpus)


@pytest.mark.parametrize("D", [4, 64, 400, 512])
def test_exact_on_integer_operands(dev, D):
    c = Corpus(300, D, 10 + D, ints=True)
    got, want = _run(dev, c), c.oracle()
    assert sorted(set(c.lens.tolist()) & set(FORCED)) == sorted(FORCED)
    assert int(want[:, 1].sum()) > int(c.id_ties().sum())  # ties beyond the planted ids
    assert torch.equal(got, want), (got != want).any(1).nonzero().reshape(-1)[:8]
    assert torch.equal(got[:, 2], torch.from_numpy(c.lens).to(torch.int32)) and int(got[:, 3].sum()) == 0
    assert torch.equal(_run(dev, c, batch=7), want)  # row0 > 0


def test_batching_does_not_change_a_bit(dev, float_corpus, float_full):
    assert torch.equal(float_full[:, 2], torch.from_numpy(float_corpus.lens).to(torch.int32))
    for batch in (1, 7, 64):
        assert torch.equal(_run(dev, float_corpus, batch), float_full), batch
    assert torch.equal(_run(dev, float_corpus), float_full)  # and a second launch of the same inputs


def test_a_negative_with_the_positives_id_ties_in_float_data(float_corpus, float_full):
    ties = float_corpus.id_ties()
    assert (ties > 0).sum() >= 40 and ties.max() > 20
    n_eq = float_full[:, 1].numpy()
    assert (n_eq >= ties).all(), np.nonzero(n_eq < ties)[0]
    # the fp64 oracle sees no other tie in Gaussian data: where the device agrees with it, n_eq is the id ties
    assert np.array_equal(float_corpus.oracle()[:, 1].numpy(), ties)


def near_ties(user, table, pos, neg_ptr, negs, delta=None):
    """Per impression: does some negative with an id other than the positive's lie within the fp32
    dot-product error bound of the positive's fp64 score -- D 2^-24 (sum |u v_neg| + sum |u v_pos|)?
    ``delta [I, N]`` (two engines: the second one's fp64 score minus this one's): the gap between
    the two candidates must also survive the second engine's change of it, ``|delta[i, neg] -
    delta[i, pos]|``, and that engine's own fp32 sum (the bound once more)."""
    u, t = user.double(), table.double()
    D = u.shape[1]
    out = np.zeros(u.shape[0], dtype=bool)
    for i in range(u.shape[0]):
        ids = negs[int(neg_ptr[i]):int(neg_ptr[i + 1])].long()
        p = int(pos[i])
        s_pos, a_pos = (u[i] * t[p]).sum(), (u[i] * t[p]).abs().sum()
        s_neg, a_neg = (u[i][None] * t[ids]).sum(1), (u[i][None] * t[ids]).abs().sum(1)
        margin = D * 2.0 ** -24 * (a_neg + a_pos)
        if delta is not None:
            margin = 2 * margin + (delta[i, ids] - delta[i, p]).abs()
        out[i] = bool((((s_neg - s_pos).abs() <= margin) & (ids != p)).any())
    return out


def test_float_operands_match_fp64_outside_the_error_bound(dev):
    c = Corpus(700, 400, 0, ints=False)
    aside = near_ties(c.user, c.table, c.pos, c.neg_ptr, c.negs)
    print(f"set aside: {int(aside.sum())} of {I_IMP}")
    assert aside.sum() <= 0.10 * I_IMP
    got, want = _run(dev, c), c.oracle()
    bad = np.nonzero((got != want).any(1).numpy() & ~aside)[0]
    print(f"mismatches outside the bound: {len(bad)}; inside: {int(((got != want).any(1).numpy() & aside).sum())}")
    assert len(bad) == 0, (bad[:8], got[bad[:8]], want[bad[:8]])


def test_nan_table_row(dev):
    c = Corpus(300, 64, 3, ints=True)
    R = 7
    tn = c.table.clone()
    tn[R] = float("nan")
    touched = np.array([int(c.pos[i]) == R or bool((c.negs[c.neg_ptr[i]:c.neg_ptr[i + 1]] == R).any())
                        for i in range(I_IMP)])
    assert 10 <= touched.sum() <= I_IMP - 10
    got, clean = _run(dev, c, table=tn), _run(dev, c)
    assert torch.equal(got, c.oracle(tn))
    assert np.array_equal((got[:, 3] > 0).numpy(), touched)
    assert torch.equal(got[~torch.from_numpy(touched)], clean[~torch.from_numpy(touched)])


def test_host_checks_reject_what_the_kernel_was_not_written_for(dev):
    op = torch.ops.fedrec_eval.rank_impressions
    native.lib()
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    u, t = z(4, 8), z(50, 8)
    pos, ptr, negs = z(6, dt=torch.int32), z(7, dt=torch.int64), z(3, dt=torch.int32)
    assert op(u, t, pos, ptr, negs, 2).tolist() == [[0, 0, 0, 0]] * 4
    bad = [
        lambda: op(u.cpu(), t.cpu(), pos.cpu(), ptr.cpu(), negs.cpu(), 0),       # host tensors
        lambda: op(u, t.cpu(), pos, ptr, negs, 0),
        lambda: op(u.bfloat16(), t, pos, ptr, negs, 0),                         # bf16 user
        lambda: op(z(4, 6), z(50, 6), pos, ptr, negs, 0),                       # D = 6
        lambda: op(z(4, 516), z(50, 516), pos, ptr, negs, 0),                   # D = 516
        lambda: op(u, z(50, 16)[:, :8], pos, ptr, negs, 0),                     # non-contiguous table
        lambda: op(u, t, pos, ptr.to(torch.int32), negs, 0),                    # int32 neg_ptr
        lambda: op(u, t, pos, ptr, negs, 3),                                    # row0 + B > I
        lambda: op(u, t, pos, ptr, negs, -1),
        lambda: op(u, t, pos, ptr[:-1], negs, 0),                               # neg_ptr of the wrong length
        lambda: op(u, t, pos, z(8, dt=torch.int64), negs, 0),
    ]
    for f in bad:
        with pytest.raises((RuntimeError, NotImplementedError)):
            f()


# ---- engine ---------------------------------------------------------------------------------
def test_engine_validate_full_device_vs_cpu(dev):
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
    e_cpu.news_table, e_gpu.news_table = e_cpu.encode_all(), e_gpu.encode_all()  # one encode per engine
    m_g, c_g = e_gpu.validate_full(batch_size=16, limit=64, return_counts=True)
    m_c, c_c = e_cpu.validate_full(batch_size=16, limit=64, return_counts=True)
    n = min(64, len(shard.valid))
    assert m_g["n_full"] == m_c["n_full"] == n and set(m_g) == set(m_c) and c_g.shape == c_c.shape == (n, 4)
    assert np.array_equal(c_g[:, 2:], c_c[:, 2:])
    his = np.concatenate([h for _, h in validation_batches(shard.valid, 16, cfg.npratio, cfg.max_his_len, True, n)])
    t_c, t_dev = e_cpu.news_table, e_gpu.news_table
    u_c = e_cpu.user_vectors(torch.from_numpy(his), t_c).double()
    u_g = e_gpu.user_vectors(torch.from_numpy(his), t_dev).cpu().double()
    t_c, t_g = t_c.double(), t_dev.cpu().double()
    # the device path rounds to bf16 at every stage (test_engine_gpu.py: err <= 8 u ||a||, u = 2^-8)
    assert float((u_g - u_c).norm()) <= 8 * 2.0 ** -8 * float(u_c.norm())
    # the near-tie rule between two engines: the device engine's vectors differ from the host's (bf16
    # stages), so a pair of candidates is comparable when its fp64 gap on the host's vectors exceeds
    # what the device's vectors change it by (exact, in fp64) plus both engines' fp32 summation bounds
    delta = u_g @ t_g.t() - u_c @ t_c.t()
    arr = shard.valid
    aside = near_ties(u_c, t_c, torch.as_tensor(arr.pos), torch.as_tensor(arr.neg_ptr), torch.as_tensor(arr.neg_ids),
                      delta)
    print(f"set aside: {int(aside.sum())} of {n}; impressions whose counts differ: {int((c_g != c_c).any(1).sum())}")
    assert (~aside).sum() >= 1  # (measured on the MI355X: 7 of 53 set aside, 3 of those differ)
    assert np.array_equal(c_g[~aside], c_c[~aside]), np.nonzero((c_g != c_c).any(1) & ~aside)[0]
