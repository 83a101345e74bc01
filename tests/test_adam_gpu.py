"""The Adam kernels (csrc/adam.hip) on the MI355X against the fp64 oracle and its derived fp32
bound (``tests/adam_oracle.py``): the eager ``adam_kernel`` (sizes on either side of the
grid-stride loop's first pass, the bf16 copy), the in-graph ``adam_dev_kernel`` (the device
step count's bias correction, the loss ring, the gradient-segment gather branch by branch),
what the launchers refuse, the engine's real parameter layout on both paths, and
``FlatParams.end_backward``'s two ways of filling the flat gradient."""
import copy
import functools

import pytest
import torch

from adam_oracle import HPARAMS, AdamOracle, grad_stream
from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.config import BackboneConfig, FedRecConfig
from fedrec_with_pytorchdistributed_amd.data.synthetic import make_client_shards
from fedrec_with_pytorchdistributed_amd.models.fedrec_model import FedRecModel, FlatParams
from fedrec_with_pytorchdistributed_amd.ops import native
from fedrec_with_pytorchdistributed_amd.train.engine import LocalEngine

pytestmark = pytest.mark.gpu

# 2048 blocks x 256 threads x 4 elements is one pass of the grid-stride loop; 773 threads go round again
N_LARGE = 2048 * 256 * 4 + 4 * 773
GS = 1.0 / 3.0


def _hp_id(hp):
    return f"lr{hp['lr']:g}-b{hp['b1']:g}-{hp['b2']:g}"


def _bits(x: torch.Tensor) -> torch.Tensor:
    return x.detach().cpu().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _stream(n: int, steps: int):
    return tuple(grad_stream(n, steps))  # shared by the cases of a size: never written


def _p0(kind: str, n: int) -> torch.Tensor:
    return torch.zeros(n) if kind == "zero" else torch.randn(n, generator=torch.Generator().manual_seed(3))


def _hp_args(hp):
    return hp["lr"], hp["b1"], hp["b2"], hp["eps"]


# ---------------------------------------------------------------------------------------
# adam_flat (adam_kernel)
@pytest.mark.parametrize("t0", [0, 100000])
@pytest.mark.parametrize("p0", ["zero", "randn"])
@pytest.mark.parametrize("hp", HPARAMS, ids=_hp_id)
@pytest.mark.parametrize("n", [4, 1028, N_LARGE])
def test_adam_flat_within_oracle_bound(dev, n, hp, p0, t0):
    steps = 2 if n == N_LARGE else 6
    ph = _p0(p0, n)
    p, m, v = ph.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    orc = AdamOracle(ph, grad_scale=GS, c=1.0 if p0 == "zero" else 2.0, **hp)
    worst = [0.0, 0.0, 0.0]
    for i, g in enumerate(_stream(n, steps)):
        ops.adam_flat(p, g.to(dev), m, v, t0 + 1 + i, *_hp_args(hp), grad_scale=GS)
        orc.step(g, t0 + 1 + i)
        r = orc.ratios(p, m, v)
        worst = [max(a, b) for a, b in zip(worst, r)]
        print(f"adam_flat n={n} {_hp_id(hp)} p0={p0} t={t0 + 1 + i}: ratios m {r[0]:.3f} v {r[1]:.3f} step {r[2]:.3f}")
        assert max(r) <= 1.0, (i, r)
    # a gradient that is always 0 moves nothing (every 17th element of the stream)
    assert torch.equal(_bits(p)[::17], _bits(ph)[::17])
    assert not bool(m[::17].any()) and not bool(v[::17].any())
    print(f"adam_flat n={n} {_hp_id(hp)} p0={p0} t0={t0}: worst m {worst[0]:.3f} v {worst[1]:.3f} step {worst[2]:.3f}")


@pytest.mark.parametrize("n", [4, N_LARGE])
def test_adam_flat_lowp_copy(dev, n):
    """The optional bf16 copy is the rounded new p, element for element, second pass included."""
    hp = HPARAMS[0]
    steps = 2 if n == N_LARGE else 6
    ph = _p0("randn", n)
    p, m, v = ph.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    low = torch.full((n,), 7.0, dtype=torch.bfloat16, device=dev)
    orc = AdamOracle(ph, grad_scale=GS, **hp)
    for i, g in enumerate(_stream(n, steps)):
        ops.adam_flat(p, g.to(dev), m, v, 1 + i, *_hp_args(hp), grad_scale=GS, p_lowp=low)
        orc.step(g, 1 + i)
        assert torch.equal(low, p.to(torch.bfloat16)), i
        assert max(orc.ratios(p, m, v)) <= 1.0  # the same step as without the copy
    assert not torch.equal(p.cpu(), ph)


def test_adam_flat_refuses_bad_lowp_and_size(dev):
    hp = HPARAMS[0]
    n = 1028
    mk = lambda k: (torch.randn(k, device=dev), torch.randn(k, device=dev), torch.zeros(k, device=dev),
                    torch.zeros(k, device=dev))
    for low in (torch.zeros(n - 4, dtype=torch.bfloat16, device=dev), torch.zeros(n, dtype=torch.float16, device=dev),
                torch.zeros(n, dtype=torch.float32, device=dev)):
        p, g, m, v = mk(n)
        keep = [t.clone() for t in (p, g, m, v)]
        with pytest.raises(RuntimeError):
            ops.adam_flat(p, g, m, v, 1, *_hp_args(hp), p_lowp=low)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip((p, g, m, v), keep)) and not bool(low.any())
    p, g, m, v = mk(1026)  # not a multiple of 4: the launcher's own check
    keep = [t.clone() for t in (p, g, m, v)]
    with pytest.raises(RuntimeError):
        ops.adam_flat(p, g, m, v, 1, *_hp_args(hp))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((p, g, m, v), keep))


# ---------------------------------------------------------------------------------------
# adam_dev (adam_dev_kernel), no segments
def _state(n: int, seed: int = 11):
    """A mid-training state as exact fp32 inputs: p ~ N(0, 1), m over five decades, v >= m^2."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    m = (torch.randn(n, generator=gen) * 10.0 ** (torch.rand(n, generator=gen) * 5.0 - 6.0)).float()
    v = (m.double() ** 2 * (1.0 + 3.0 * torch.rand(n, generator=gen, dtype=torch.float64))).float()
    return p, m, v


def _dev_call(lib, p, g, m, v, step, loss, ring, hp, gs, gsrc=None, goff=None, skip=None):
    lib.adam_dev(p, g, m, v, step, loss, ring, *_hp_args(hp), gs, gsrc, goff, skip)


@pytest.mark.parametrize("hp", HPARAMS, ids=_hp_id)
@pytest.mark.parametrize("t", [1, 2, 8, 9, 1000, 100000])
def test_adam_dev_step_count_and_loss_ring(dev, t, hp):
    """The bias corrections come from the int64 step tensor (read, never written); the loss lands
    in slot (t - 1) % ring and nowhere else; m and v are the eager kernel's bit for bit and p is
    within the same oracle's bound on both paths."""
    n = 1028
    lib = native.lib()
    ph, mh, vh = _state(n)
    g = _stream(n, 6)[1]
    orc = AdamOracle(ph, grad_scale=GS, m0=mh, v0=vh, **hp)
    orc.step(g, t)
    step = torch.full((1,), t, dtype=torch.int64, device=dev)
    loss = torch.full((1,), 1.5, device=dev)
    ring = torch.full((8,), -7.0, device=dev)
    p, m, v, gd = ph.to(dev), mh.to(dev), vh.to(dev), g.to(dev)
    _dev_call(lib, p, gd, m, v, step, loss, ring, hp, GS)
    r = orc.ratios(p, m, v)
    print(f"adam_dev t={t} {_hp_id(hp)}: ratios m {r[0]:.3f} v {r[1]:.3f} step {r[2]:.3f}")
    assert max(r) <= 1.0, r
    assert torch.equal(gd.cpu(), g)  # no segments: the gradient is only read
    want = torch.full((8,), -7.0)
    want[(t - 1) % 8] = 1.5
    assert torch.equal(ring.cpu(), want)
    assert int(step.item()) == t
    # the eager kernel from the same state
    pe, me, ve = ph.to(dev), mh.to(dev), vh.to(dev)
    ops.adam_flat(pe, gd, me, ve, t, *_hp_args(hp), grad_scale=GS)
    re = orc.ratios(pe, me, ve)
    assert max(re) <= 1.0, re
    assert torch.equal(_bits(m), _bits(me)) and torch.equal(_bits(v), _bits(ve))
    # no ring at all (numel 0): accepted, the same step
    p2, m2, v2 = ph.to(dev), mh.to(dev), vh.to(dev)
    _dev_call(lib, p2, gd, m2, v2, step, loss, torch.empty(0, device=dev), hp, GS)
    assert torch.equal(_bits(p2), _bits(p)) and torch.equal(_bits(m2), _bits(m)) and torch.equal(_bits(v2), _bits(v))


# ---------------------------------------------------------------------------------------
# adam_dev gradient segments
SEG_N = 81000
#          offset  numel
SEG_TABLE = [(64, 1), (128, 3), (192, 4), (196, 5), (256, 63), (320, 64), (384, 65), (512, 400 * 200), (80512, 401),
             (SEG_N - 8, 8)]


def _seg_sources(vals: torch.Tensor, gflat: torch.Tensor):
    """The table's sources for one step from a full-length value vector: fresh tensors (aligned
    allocations: the 16-byte path, ragged tails by element), two 4-byte-aligned slices of one
    buffer (by element throughout), None, a 2-D tensor, the flat gradient's own slot."""
    fresh = lambda j: vals[SEG_TABLE[j][0]:SEG_TABLE[j][0] + SEG_TABLE[j][1]].clone()
    buf = vals[1000:1080].clone()
    s8 = gflat[80512:80512 + 401]
    s8.copy_(vals[80512:80512 + 401])
    srcs = [fresh(0), fresh(1), fresh(2), fresh(3), buf[1:64], None, buf[3:68], fresh(7).view(400, 200), s8, fresh(9)]
    for j in (0, 1, 2, 3, 7, 9):
        assert srcs[j].data_ptr() % 16 == 0
    assert srcs[4].data_ptr() % 16 == 4 and srcs[6].data_ptr() % 16 == 12
    expected = torch.zeros_like(vals)
    for (off, _), s in zip(SEG_TABLE, srcs):
        if s is not None:
            expected[off:off + s.numel()] = s.reshape(-1)
    return srcs, expected


def test_adam_dev_gathers_gradient_segments(dev):
    hp, gs = HPARAMS[0], 0.5
    lib = native.lib()
    N = SEG_N
    covered = torch.zeros(N, dtype=torch.bool)
    for off, k in SEG_TABLE:
        covered[off:off + k] = True
    gaps = ~covered
    assert bool(gaps[:64].all()) and bool(covered[N - 8:].all()) and int(gaps.sum()) > 100
    # m = v = 0 except under the source-less segment, whose moments must decay
    ph = _p0("randn", N)
    mh, vh = torch.zeros(N), torch.zeros(N)
    _, ms, vs = _state(64)
    mh[320:384], vh[320:384] = ms, vs
    orc = AdamOracle(ph, grad_scale=gs, m0=mh, v0=vh, **hp)
    p, m, v = ph.to(dev), mh.to(dev), vh.to(dev)  # the segment path
    q, qm, qv = ph.to(dev), mh.to(dev), vh.to(dev)  # the plain path on the expected gradient
    gflat = torch.empty(N, device=dev)
    loss = torch.full((1,), 0.25, device=dev)
    ring = torch.zeros(8, device=dev)
    offs = [o for o, _ in SEG_TABLE]
    for i, vals in enumerate(_stream(N, 2)):
        t = 1 + i
        step = torch.full((1,), t, dtype=torch.int64, device=dev)
        gflat.fill_(float("nan"))
        srcs, expected = _seg_sources(vals.to(dev), gflat)
        _dev_call(lib, p, gflat, m, v, step, loss, ring, hp, gs, srcs, offs)
        assert torch.equal(_bits(gflat), _bits(expected)), (_bits(gflat) != _bits(expected)).nonzero()[:8]
        assert not bool(expected[gaps.to(dev)].any()) and bool(expected[covered.to(dev)].any())
        g2 = expected.clone()
        _dev_call(lib, q, g2, qm, qv, step, loss, ring, hp, gs)
        orc.step(expected, t)
        r = orc.ratios(q, qm, qv)
        print(f"adam_dev segments step {t}: ratios m {r[0]:.3f} v {r[1]:.3f} step {r[2]:.3f}")
        assert max(r) <= 1.0, r
        for a, b in ((p, q), (m, qm), (v, qv)):
            assert torch.equal(_bits(a), _bits(b)), (i, (_bits(a) != _bits(b)).nonzero()[:8])
        assert torch.equal(_bits(p)[gaps], _bits(ph)[gaps])
        assert not bool(m.cpu()[gaps].any()) and not bool(v.cpu()[gaps].any())
        # no source: zeros went in, the moments decayed, p moved on the old momentum
        assert bool((m.cpu()[320:384].abs() < mh[320:384].abs()).all()) and bool((v.cpu()[320:384] < vh[320:384]).all())
        assert not bool((p.cpu()[320:384] == ph[320:384]).all())
    assert bool(m.cpu()[covered].any()) and float(ring[1]) == 0.25


def test_adam_dev_full_segment_table(dev):
    """ADAM_SEG = 48 adjacent 4-element segments, exactly the table's capacity."""
    hp, lib, n = HPARAMS[0], native.lib(), 256
    vals = _stream(1028, 6)[0][:n].to(dev)
    ph = _p0("randn", n)
    srcs = [vals[4 * j:4 * j + 4].clone() for j in range(48)]
    offs = [4 * j for j in range(48)]
    expected = torch.zeros(n, device=dev)
    expected[:192] = vals[:192]
    step = torch.ones(1, dtype=torch.int64, device=dev)
    loss, ring = torch.zeros(1, device=dev), torch.empty(0, device=dev)
    p, m, v = ph.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    g = torch.full((n,), float("nan"), device=dev)
    _dev_call(lib, p, g, m, v, step, loss, ring, hp, GS, srcs, offs)
    q, qm, qv = ph.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    _dev_call(lib, q, expected.clone(), qm, qv, step, loss, ring, hp, GS)
    assert torch.equal(_bits(g), _bits(expected))
    assert torch.equal(_bits(p), _bits(q)) and torch.equal(_bits(m), _bits(qm)) and torch.equal(_bits(v), _bits(qv))
    orc = AdamOracle(ph, grad_scale=GS, **hp)
    orc.step(expected, 1)
    assert max(orc.ratios(p, m, v)) <= 1.0


def _refusals(dev, n):
    f = lambda k: torch.randn(k, device=dev)
    many = ([f(4) for _ in range(49)], [4 * j for j in range(49)])
    return {
        "49 segments": many,
        "offset not a multiple of 4": ([f(4)], [2]),
        "overlapping": ([f(8), f(4)], [0, 4]),
        "unsorted": ([f(4), f(4)], [8, 0]),
        "past the end": ([f(8)], [n - 4]),
        "gsrc without goff": ([f(4)], None),
        "gsrc and goff of different lengths": ([f(4), f(4)], [0]),
        "bf16 source": ([f(4).to(torch.bfloat16)], [0]),
        "non-contiguous source": ([f(8)[::2]], [0]),
    }


def test_adam_dev_refuses_bad_segments(dev):
    """Every case is rejected by a host check (bind_optim.cpp adam_dev, fr_adam_dev) before any
    launch: RuntimeError, and p, g, m, v as they were."""
    hp, lib = HPARAMS[0], native.lib()
    step = torch.ones(1, dtype=torch.int64, device=dev)
    loss, ring = torch.zeros(1, device=dev), torch.full((8,), -7.0, device=dev)
    cases = [(1024, name, a) for name, a in _refusals(dev, 1024).items()]
    cases.append((1026, "n not a multiple of 4", (None, None)))
    for n, name, (gsrc, goff) in cases:
        bufs = [torch.randn(n, device=dev) for _ in range(4)]
        keep = [b.clone() for b in bufs]
        p, g, m, v = bufs
        with pytest.raises(RuntimeError):
            _dev_call(lib, p, g, m, v, step, loss, ring, hp, 1.0, gsrc, goff)
            pytest.fail(f"accepted: {name}")
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(bufs, keep)), name
        assert bool((ring == -7.0).all()), name


# ---------------------------------------------------------------------------------------
# the engine's real layout, both paths
def _engine(dev, cfg, model, shard, graphs):
    c = copy.deepcopy(cfg)
    c.step_graph = graphs
    return LocalEngine(c, model, shard, dev)


@pytest.fixture(scope="module")
def engine_steps(dev):
    """Three prepared steps (then one more from step count 1000) on an eager and a step-graph
    engine; around each, (p, m, v) before and (p, m, v, grad) after, read back to the host."""
    cfg = FedRecConfig(mode="grad_avg", batch_size=8, user_dropout=0.0)
    cfg.backbone = BackboneConfig(name="distilbert-1l", n_layers=1)
    torch.manual_seed(0)
    m0 = FedRecModel(cfg).to(dev)
    m1 = copy.deepcopy(m0)
    m0.build_flat()
    m1.build_flat()
    shard = make_client_shards("tiny", 1)[0]
    engines = {"eager": _engine(dev, cfg, m0, shard, "off"), "graph": _engine(dev, cfg, m1, shard, "on")}
    batches = [b for _, b in zip(range(4), engines["eager"].sampler.epoch(0))]
    torch.cuda.synchronize()
    out = {}
    for name, e in engines.items():
        fl = e.model.flat
        recs = []
        for i, (cand, his) in enumerate(batches):
            if i == 3:
                fl.step = 1000  # as a resume does
            pre = e.prepare(lambda: (cand, his))
            e.sync_params()
            torch.cuda.synchronize()
            before = [t.detach().cpu().clone() for t in (fl.flat, fl.m, fl.v)]
            e.train_prepared(pre)
            e.sync_params()
            torch.cuda.synchronize()
            after = [t.detach().cpu().clone() for t in (fl.flat, fl.m, fl.v, fl.grad)]
            recs.append((fl.step, before, after))
        sd = getattr(e, "_adam_step_dev", None)
        out[name] = dict(recs=recs, counts=dict(e.counts), offsets=list(fl.offsets),
                         numels=[p.numel() for p in fl.params], padded=fl.numel_padded, hp=cfg,
                         step_dev=int(sd.item()) if sd is not None else None)
    return out


@pytest.mark.parametrize("path", ["eager", "graph"])
def test_engine_step_moves_state_as_oracle(engine_steps, path):
    """One-step bound from the exact fp32 snapshot (em = ev = 0 at the start), with the flat
    gradient the step left behind, t = flat.step, grad_scale 1: both kernels at the engine's
    real offsets and parameter count, independent of the gradient's summation order."""
    R = engine_steps[path]
    cfg = R["hp"]
    hp = dict(lr=cfg.lr, b1=cfg.adam_beta1, b2=cfg.adam_beta2, eps=cfg.adam_eps)
    assert R["padded"] % 4 == 0 and R["padded"] > 1_000_000
    gaps = torch.ones(R["padded"], dtype=torch.bool)
    for off, k in zip(R["offsets"], R["numels"]):
        gaps[off:off + k] = False
    assert int(gaps.sum()) > 0
    assert [t for t, _, _ in R["recs"]] == [1, 2, 3, 1001]
    for t, (p0, m0, v0), (p1, m1, v1, g) in R["recs"]:
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
        assert not bool(g[gaps].any())
        orc = AdamOracle(p0, grad_scale=1.0, m0=m0, v0=v0, **hp)
        orc.step(g, t)
        r = orc.ratios(p1, m1, v1)
        print(f"engine {path} t={t}: ratios m {r[0]:.3f} v {r[1]:.3f} step {r[2]:.3f}")
        assert max(r) <= 1.0, (t, r)
        assert not torch.equal(p0, p1)
    if path == "graph":  # neither engine may pass on the other's kernel
        assert R["counts"]["replays_with_optimizer"] == 4 and R["counts"]["eager_optimizer_steps"] == 0
        assert R["step_dev"] == 1001
    else:
        assert R["counts"]["eager_optimizer_steps"] == 4 and R["counts"]["replays_with_optimizer"] == 0


# ---------------------------------------------------------------------------------------
# FlatParams.end_backward: the copy launch and the in-Adam gather fill the same flat gradient
@pytest.mark.parametrize("missing", [False, True], ids=["all-present", "one-missing"])
def test_end_backward_copy_equals_adam_gather(dev, missing):
    """``copy=True`` (every gradient present: the multi_cast launch; one missing: the foreach copy
    and zero) against ``copy=False`` + adam_dev with the returned sources (the segment path)."""
    hp, lib = HPARAMS[0], native.lib()
    shapes = [(1,), (3,), (20,), (400, 200), (401,)]
    gen = torch.Generator().manual_seed(5)
    grads = [torch.randn(*s, generator=gen) for s in shapes]
    flats = []
    for _ in range(2):
        fp = FlatParams([(f"w{i}", torch.nn.Parameter(torch.zeros(*s, device=dev))) for i, s in enumerate(shapes)])
        assert fp.offsets == [0, 64, 128, 192, 80192] and fp.numel_padded == 80640
        fp.begin_backward()
        inplace = set()
        for i, (p, off, g) in enumerate(zip(fp.params, fp.offsets, grads)):
            slot = fp.grad[off:off + p.numel()]
            if i == 2:  # written straight into its slot by the backward
                slot.copy_(g.reshape(-1))
                inplace.add(id(p))
            elif i == 1 and missing:
                slot.fill_(3.0)  # a stale gradient from an earlier step: must read 0 afterwards
            else:
                p.grad = g.to(dev)
        flats.append((fp, inplace))
    (fa, ia), (fb, ib) = flats
    fa.end_backward(copy=True, inplace=ia)
    srcs = fb.end_backward(copy=False, inplace=ib)
    assert len(srcs) == 5 and (srcs[1] is None) == missing and srcs[2].data_ptr() == fb.grad[128:].data_ptr()
    step = torch.ones(1, dtype=torch.int64, device=dev)
    lib.adam_dev(fb.flat, fb.grad, fb.m, fb.v, step, torch.zeros(1, device=dev), torch.empty(0, device=dev),
                 *_hp_args(hp), 1.0, srcs, list(fb.offsets), None)
    want = torch.zeros(80640)
    for i, (off, g) in enumerate(zip(fa.offsets, grads)):
        if not (i == 1 and missing):
            want[off:off + g.numel()] = g.reshape(-1)
    assert torch.equal(_bits(fa.grad), _bits(want))
    assert torch.equal(_bits(fb.grad), _bits(fa.grad))
    for fp in (fa, fb):
        for p, off in zip(fp.params, fp.offsets):
            assert p.grad.data_ptr() == fp.grad[off:].data_ptr() and p.grad.shape == p.shape
