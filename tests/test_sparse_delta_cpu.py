"""Top-k sparsified uploads on the host: the torch oracles of ``topk_delta`` / ``sparse_combine``
against brute-force definitions (and the checks against four mutants of the contract), the upload
validator, the binding's argument checks (they run before the device check, so on host tensors),
the config rejections and the client snapshot's residual field.  No GPU."""
import math

import numpy as np
import pytest
import torch

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.config import BackboneConfig, FedRecConfig
from fedrec_with_pytorchdistributed_amd.models.fedrec_model import FedRecModel
from fedrec_with_pytorchdistributed_amd.ops import native
from fedrec_with_pytorchdistributed_amd.ops import reference as ref
from fedrec_with_pytorchdistributed_amd.parallel.sparsify import Sparsifier
from fedrec_with_pytorchdistributed_amd.train import checkpoint as ckpt

NAN, INF = float("nan"), float("inf")


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ---- the definition, by brute force -----------------------------------------------------------
def _a_of(local, glob, res):
    """(local - global) + residual in numpy fp32: one rounding each."""
    l, g, e = (t.numpy().astype(np.float32) for t in (local, glob, res))
    return (l - g).astype(np.float32) + e


def _brute_set(a, k):
    key = a.view(np.uint32) & np.uint32(0x7FFFFFFF)
    order = sorted(range(len(a)), key=lambda i: (-int(key[i]), i))  # Python's sort is stable
    return sorted(order[:k])


def _violations(local, glob, res0, k, idx, val, res1):
    """Which parts of the contract ``(idx, val, res1)`` breaks for these inputs."""
    a = _a_of(local, glob, res0)
    want = _brute_set(a, k)
    bad = []
    got = [int(i) for i in idx]
    if idx.dtype != torch.int32 or val.dtype != torch.float32 or len(got) != k:
        bad.append("types")
    if sorted(got) != want:
        bad.append("set")
    if any(b <= a_ for a_, b in zip(got, got[1:])):
        bad.append("ascending")
    if not np.array_equal(val.numpy().view(np.uint32), a[got].view(np.uint32)):
        bad.append("val")
    exp = a.copy()
    exp[want] = 0.0
    if not np.array_equal(res1.numpy().view(np.uint32), exp.view(np.uint32)):
        bad.append("residual")
    return bad


def _families(n, seed):
    g = torch.Generator().manual_seed(seed)
    normal = lambda: torch.randn(n, generator=g) * 2.0 ** torch.randint(-20, 21, (n,), generator=g).float()
    ints = lambda: torch.randint(-3, 4, (n,), generator=g).float()
    yield "distinct", normal(), normal(), normal()
    yield "ties", ints(), ints(), ints()
    yield "constant", torch.full((n,), 2.5), torch.zeros(n), torch.zeros(n)
    z = torch.zeros(n)
    z[::2] = -0.0
    yield "zeros", z, torch.zeros(n), torch.zeros(n)
    sp = normal()
    sp[::5], sp[1::7], sp[2::11], sp[3::13] = NAN, INF, -INF, 1e-41
    yield "special", sp, torch.zeros(n), torch.zeros(n)


@pytest.mark.parametrize("n", [1, 2, 7, 64, 257])
def test_oracle_equals_the_brute_force_definition(n):
    for name, l, g, e in _families(n, n):
        for k in sorted({1, 2, max(1, n // 10), n // 2, n - 1, n} & set(range(1, n + 1))):
            res = e.clone()
            idx, val = ref.topk_delta(l, g, res, k)
            assert _violations(l, g, e, k, idx, val, res) == [], (name, n, k)
            assert bool((res[idx.long()] == 0).all()) and not bool(torch.signbit(res[idx.long()]).any())
            keep = torch.ones(n, dtype=torch.bool)
            keep[idx.long()] = False
            a = torch.from_numpy(_a_of(l, g, e))
            assert torch.equal(_bits(res)[keep], _bits(a)[keep])  # the residual is cleared exactly at idx


def test_nan_ranks_above_inf_above_finite_and_signs_tie():
    l = torch.tensor([1.0, -INF, 3.0, NAN, -3.0, INF, 0.0, -0.0])
    z = torch.zeros(8)
    for k, want in [(1, [3]), (2, [1, 3]), (3, [1, 3, 5]), (4, [1, 2, 3, 5]), (5, [1, 2, 3, 4, 5]), (7, [0, 1, 2, 3, 4, 5, 6])]:
        idx, _ = ref.topk_delta(l, z, z.clone(), k)
        assert idx.tolist() == want, k


def test_conservation_over_rounds_is_exact_on_integers():
    """Nothing is lost, only delayed: scattered uploads + final residual == the dense deltas' sum."""
    n, k = 301, 17
    g = torch.Generator().manual_seed(5)
    res = torch.zeros(n)
    sent, dense = torch.zeros(n), torch.zeros(n)
    for _ in range(5):
        theta_g = torch.randint(-50, 51, (n,), generator=g).float()
        local = theta_g + torch.randint(-9, 10, (n,), generator=g).float()
        dense += local - theta_g
        idx, val = ref.topk_delta(local, theta_g, res, k)
        sent[idx.long()] += val
    assert torch.equal(_bits(sent + res), _bits(dense))
    assert bool((res != 0).any())


# ---- mutants of the contract: the checks above must reject each ---------------------------------
def _mutant(kind, local, glob, res, k):
    a = (local - glob) + res
    key = ref.magnitude_keys(a).long()
    n = a.numel()
    if kind == "ties_to_higher_index":
        order = torch.sort(key * n + torch.arange(n), descending=True).indices[:k]
    elif kind == "signed_key":
        order = torch.sort(a, descending=True, stable=True).indices[:k]
    else:
        order = torch.sort(key, descending=True, stable=True).indices[:k]
    idx = order if kind == "selection_order" else torch.sort(order).values
    val = a[idx].clone()
    res.copy_(a)
    if kind != "residual_kept":
        res[idx] = 0.0
    return idx.to(torch.int32), val


@pytest.mark.parametrize("kind,broken", [("ties_to_higher_index", "set"), ("signed_key", "set"),
                                         ("selection_order", "ascending"), ("residual_kept", "residual")])
def test_the_checks_reject_each_mutant(kind, broken):
    g = torch.Generator().manual_seed(11)
    n, k = 64, 9
    l = torch.randint(-3, 4, (n,), generator=g).float()
    l[:4] = torch.tensor([-7.0, 6.0, -6.5, 5.0])  # the signed key would miss -7 and -6.5
    z, e = torch.zeros(n), torch.zeros(n)
    res = e.clone()
    idx, val = _mutant(kind, l, z, res, k)
    assert broken in _violations(l, z, e, k, idx, val, res), kind
    res = e.clone()
    idx, val = ref.topk_delta(l, z, res, k)  # ... and pass the oracle on the same input
    assert _violations(l, z, e, k, idx, val, res) == []


# ---- combine -------------------------------------------------------------------------------------
def _dense_combine(base, idx, val, w):
    acc = np.zeros(base.numel(), dtype=np.float32)
    ws = np.float32(0.0)
    for c in range(idx.shape[0]):
        for j in range(idx.shape[1]):
            i = int(idx[c, j])
            acc[i] = np.float32(acc[i] + np.float32(np.float32(w[c]) * np.float32(val[c, j])))
        ws = np.float32(ws + np.float32(w[c]))
    return torch.from_numpy(base.numpy() + acc / ws)


@pytest.mark.parametrize("W,n,k", [(1, 1, 1), (2, 65, 7), (3, 300, 300), (8, 257, 25)])
def test_sparse_combine_equals_a_dense_fp32_loop(W, n, k):
    g = torch.Generator().manual_seed(W * 1000 + n)
    base = torch.randn(n, generator=g)
    idx = torch.stack([torch.sort(torch.randperm(n, generator=g)[:k]).values for _ in range(W)]).to(torch.int32)
    val = torch.randn(W, k, generator=g)
    w = torch.rand(W, generator=g) + 0.5
    out = ref.sparse_combine(base, idx, val, w)
    assert torch.equal(_bits(out), _bits(_dense_combine(base, idx, val, w)))
    assert torch.equal(_bits(ops.sparse_combine(base, idx, val, w)), _bits(out))  # host tensors -> the oracle


def test_one_client_weight_one_full_density_gives_base_plus_delta():
    g = torch.Generator().manual_seed(3)
    n = 129
    base, local = torch.randn(n, generator=g), torch.randn(n, generator=g)
    res = torch.zeros(n)
    idx, val = ops.topk_delta(local, base, res, n)
    assert idx.tolist() == list(range(n)) and not bool(res.any())
    out = ops.sparse_combine(base, idx[None], val[None], torch.ones(1))
    assert torch.equal(_bits(out), _bits(base + (local - base)))


# ---- the upload validator --------------------------------------------------------------------------
def test_sparse_upload_check():
    n, k = 10, 3
    ok_i, ok_v = torch.tensor([1, 4, 9], dtype=torch.int32), torch.ones(3)
    ref.sparse_upload_check(ok_i, ok_v, n, k)
    i32 = lambda *x: torch.tensor(x, dtype=torch.int32)
    for idx, val, what in [(i32(4, 1, 9), ok_v, "not strictly ascending at 1"),
                           (i32(1, 4, 4), ok_v, "not strictly ascending at 2"),
                           (i32(-1, 4, 9), ok_v, r"idx\[0\] = -1 is outside"),
                           (i32(1, 4, 10), ok_v, r"idx\[2\] = 10 is outside"),
                           (i32(1, 4), ok_v, "idx must have length 3"),
                           (ok_i, torch.ones(4), "val must have length 3"),
                           (ok_i.long(), ok_v, "idx must be int32"),
                           (ok_i, ok_v.double(), "val must be fp32")]:
        with pytest.raises(ValueError, match=what):
            ref.sparse_upload_check(idx, val, n, k)


def test_pack_and_unpack_round_trip_the_bits():
    idx = torch.tensor([0, 5, 6], dtype=torch.int32)
    val = torch.tensor([1.5, NAN, -0.0])
    blob = Sparsifier.pack(idx, val)
    assert blob.dtype == torch.int32 and tuple(blob.shape) == (2, 3)
    i2, v2 = Sparsifier.unpack(blob, 7, 3)
    assert torch.equal(i2, idx) and torch.equal(_bits(v2), _bits(val))
    with pytest.raises(ValueError, match=r"int32 \[2, 3\]"):
        Sparsifier.unpack(blob.float(), 7, 3)
    with pytest.raises(ValueError, match="outside"):
        Sparsifier.unpack(blob, 6, 3)


# ---- the binding's checks: before any launch, and with the oracle's messages -----------------------
def _bad_topk_calls():
    x = lambda n=8: torch.zeros(n)
    buf = torch.zeros(16)
    return [((x().double(), x(), x(), 1), "local must be fp32"),
            ((x(), x(), x().half(), 1), "residual must be fp32"),
            ((x(), x(), x(), 0), r"1 <= k <= n \(got k 0, n 8\)"),
            ((x(), x(), x(), 9), r"1 <= k <= n \(got k 9, n 8\)"),
            ((torch.zeros(16)[::2], x(), x(), 1), "local must be contiguous"),
            ((x(), x(9), x(), 1), "must have one length"),
            ((buf[:8], x(), buf[4:12], 1), "residual must not overlap local or global"),
            ((x(), buf[8:], buf[8:], 1), "residual must not overlap local or global")]


@pytest.mark.parametrize("case", range(8))
def test_topk_delta_argument_checks_binding_and_oracle_agree(case):
    native.lib()
    args, msg = _bad_topk_calls()[case]
    with pytest.raises(RuntimeError, match=msg):
        torch.ops.fedrec_sparse.topk_delta(*args)
    with pytest.raises(RuntimeError, match=msg):
        ref.topk_delta_check(*args)


def test_combine_argument_checks_binding_and_oracle_agree():
    native.lib()
    base, idx, val, w = torch.zeros(8), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3), torch.ones(2)
    for args, msg in [((base, idx.long(), val, w), "idx must be int32"),
                      ((base, idx, val.double(), w), "val must be fp32"),
                      ((base, idx, val[:, :2], w), r"idx and val \[W, k\] of one shape"),
                      ((base, idx, val, torch.ones(3)), r"weights \[W\]"),
                      ((base[:2].contiguous(), idx, val, w), r"1 <= k <= n \(got k 3, n 2\)"),
                      ((base, idx.t().contiguous().t(), val, w), "idx and val must be contiguous")]:
        with pytest.raises(RuntimeError, match=msg):
            torch.ops.fedrec_sparse.combine(*args)
        with pytest.raises(RuntimeError, match=msg):
            ref.sparse_combine_check(*args)


def test_a_host_tensor_fails_the_device_check_last():
    native.lib()
    with pytest.raises(RuntimeError, match="must be device tensors"):
        torch.ops.fedrec_sparse.topk_delta(torch.zeros(8), torch.zeros(8), torch.zeros(8), 2)
    with pytest.raises(RuntimeError, match="must be device tensors"):
        torch.ops.fedrec_sparse.combine(torch.zeros(8), torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, 2),
                                        torch.ones(1))


# ---- the option ---------------------------------------------------------------------------------------
def _cfg(*overrides):
    cfg = FedRecConfig()
    cfg.apply_overrides(list(overrides))
    return cfg


def test_from_cfg_is_inactive_at_the_default_and_counts_k():
    for driver in ("fedavg_star", "grad_avg", "param_avg"):
        assert not Sparsifier.from_cfg(_cfg(), driver).active
    sp = Sparsifier.from_cfg(_cfg("--upload_topk=0.01"), "fedavg_star")
    assert sp.active and sp.k_for(1000) == 10 and sp.k_for(1001) == 11 and sp.k_for(5) == 1
    assert sp.k_for(1164289) == math.ceil(0.01 * 1164289)
    assert Sparsifier(1.0).k_for(77) == 77


@pytest.mark.parametrize("overrides,driver,why", [
    (["--secagg.enabled=1"], "fedavg_star", "secagg.enabled=1"),
    (["--robust_agg=median"], "fedavg_star", "robust_agg=median"),
    (["--robust_agg=trimmed_mean"], "fedavg_star", "robust_agg=trimmed_mean"),
    ([], "grad_avg", "mode=grad_avg"),
    ([], "param_avg", "mode=param_avg")])
def test_from_cfg_rejects_what_cannot_hold(overrides, driver, why):
    with pytest.raises(ValueError, match=why):
        Sparsifier.from_cfg(_cfg("--upload_topk=0.05", *overrides), driver)
    Sparsifier.from_cfg(_cfg(*overrides), driver)  # the same without the option is fine


@pytest.mark.parametrize("f", ["-0.1", "1.5", "nan"])
def test_fraction_outside_the_unit_interval_is_rejected(f):
    with pytest.raises(ValueError, match="0 <= upload_topk <= 1"):
        Sparsifier.from_cfg(_cfg(f"--upload_topk={f}"), "fedavg_star")


# ---- the client snapshot ------------------------------------------------------------------------------
def _tiny_model():
    cfg = FedRecConfig()
    cfg.backbone = BackboneConfig.preset("tiny")
    torch.manual_seed(0)
    m = FedRecModel(cfg)
    m.build_flat()
    return m


def test_client_snapshot_round_trips_the_residual(tmp_path):
    m = _tiny_model()
    n = m.flat.flat.numel()
    res = torch.randn(n, generator=torch.Generator().manual_seed(1))
    ckpt.save_client_state(str(tmp_path / "c.pt"), m, 3, {}, res)
    back = torch.ones(n)
    info = ckpt.load_client_state(str(tmp_path / "c.pt"), m, back)
    assert info["residual_restored"] and info["round"] == 3 and torch.equal(_bits(back), _bits(res))
    # another length, or no key: a zero residual
    short = torch.ones(n - 1)
    assert not ckpt.load_client_state(str(tmp_path / "c.pt"), m, short)["residual_restored"]
    assert not bool(short.any())
    ckpt.save_client_state(str(tmp_path / "d.pt"), m, 3, {})
    back = torch.ones(n)
    assert not ckpt.load_client_state(str(tmp_path / "d.pt"), m, back)["residual_restored"]
    assert not bool(back.any())


def test_snapshot_without_the_option_has_todays_keys(tmp_path):
    m = _tiny_model()
    ckpt.save_client_state(str(tmp_path / "d.pt"), m, 0, {})
    snap = torch.load(tmp_path / "d.pt", weights_only=True)
    assert set(snap) == {"FLAT_PARAMS", "OPTIM_STATE", "ROUND", "ENGINE", "FLAT_NAMES", *ckpt.rng_state()}
    ckpt.save_client_state(str(tmp_path / "c.pt"), m, 0, {}, torch.zeros(m.flat.flat.numel()))
    assert set(torch.load(tmp_path / "c.pt", weights_only=True)) - set(snap) == {"UPLOAD_RESIDUAL"}
