"""Byzantine-robust aggregation on the host: the torch oracle of ``trimmed_mean`` against numpy and
hand-written order cases, the ``fedrec_agg::`` schema pin and argument checks, the ``scale`` fault
action, the config rejections, and the three drivers on gloo (star upload / star all-gather with a
poisoned client, parameter averaging)."""
import json
import os

import numpy as np
import pytest
import torch

from launch_util import run_ranks

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.config import FedRecConfig
from fedrec_with_pytorchdistributed_amd.ops import native
from fedrec_with_pytorchdistributed_amd.ops import reference as ref
from fedrec_with_pytorchdistributed_amd.parallel.robust import RobustRule
from fedrec_with_pytorchdistributed_amd.utils.fault import FaultInjector, parse

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "op_schemas_agg.txt")
TINY = ["--data_dir=synthetic:tiny", "--backbone.name=tiny", "--round_timeout_s=120", "--collective_timeout_s=120"]
NAN, INF = float("nan"), float("inf")


def _ok(outs):
    for rc, out in outs:
        assert rc == 0, out[-3000:]


def _metrics(path):
    with open(path) as f:
        rows = [json.loads(l) for l in f if l.strip()]
    return [r for r in rows if not r.get("final_global")]


# ---- the registered interface ---------------------------------------------------------------
def _registered_agg():
    native.lib()
    out = {}
    for name in torch._C._dispatch_get_all_op_names():
        if not name.startswith("fedrec_agg::"):
            continue
        kinds = [k for k in ("CUDA", "CompositeImplicitAutograd", "CompositeExplicitAutograd")
                 if torch._C._dispatch_has_kernel_for_dispatch_key(name, k)]
        out[name] = f"{torch._C._get_schema(name, '')} | {'+'.join(kinds) or 'none'}"
    return out


def test_agg_namespace_matches_its_fixture():
    with open(GOLDEN) as f:
        want = {ln.split("(", 1)[0]: ln.rstrip("\n") for ln in f if ln.strip()}
    assert _registered_agg() == want
    assert set(want) == {"fedrec_agg::trimmed_mean"}
    assert not [n for n in torch._C._dispatch_get_all_op_names() if n.startswith("fedrec::trimmed_mean")]


BAD = [("fp64", lambda: (torch.zeros(3, 4, dtype=torch.float64), 1), "must be fp32"),
       ("int", lambda: (torch.zeros(3, 4, dtype=torch.int32), 1), "must be fp32"),
       ("1d", lambda: (torch.zeros(4), 0), r"stack \[W, n\]"),
       ("3d", lambda: (torch.zeros(3, 4, 2), 1), r"stack \[W, n\]"),
       ("strided", lambda: (torch.zeros(4, 3).t(), 1), "must be contiguous"),
       ("W33", lambda: (torch.zeros(33, 2), 1), "1 <= W <= 32"),
       ("W0", lambda: (torch.zeros(0, 2), 0), "1 <= W <= 32"),
       ("n0", lambda: (torch.zeros(3, 0), 1), "n >= 1"),
       ("trim_neg", lambda: (torch.zeros(3, 4), -1), r"0 <= 2 \* trim < W"),
       ("trim_half", lambda: (torch.zeros(4, 4), 2), r"0 <= 2 \* trim < W"),
       ("trim_W1", lambda: (torch.zeros(1, 4), 1), r"0 <= 2 \* trim < W")]


@pytest.mark.parametrize("name,make,msg", BAD, ids=[b[0] for b in BAD])
def test_argument_checks_raise_on_host_tensors_with_one_message(name, make, msg):
    """The oracle (what ops.trimmed_mean runs on a host tensor) and the registered op raise the same
    message for the same bad argument; the op's checks run before its device check."""
    stack, trim = make()
    native.lib()
    errs = []
    for fn in (ops.trimmed_mean, ref.trimmed_mean, torch.ops.fedrec_agg.trimmed_mean):
        with pytest.raises(RuntimeError, match=msg) as e:
            fn(stack, trim)
        errs.append(str(e.value).splitlines()[0])
    assert errs[0] == errs[1] == errs[2]


def test_registered_op_rejects_a_host_tensor_after_its_checks():
    native.lib()
    with pytest.raises(RuntimeError, match="must be a device tensor"):
        torch.ops.fedrec_agg.trimmed_mean(torch.zeros(3, 4), 1)


# ---- the oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 3, 5, 9, 17, 31])
def test_odd_w_median_equals_numpy_bitwise(W):
    g = torch.Generator().manual_seed(W)
    x = torch.randn(W, 4099, generator=g) * torch.exp(torch.randn(W, 4099, generator=g) * 3)
    out, dropped = ops.trimmed_mean(x, (W - 1) // 2)
    assert out.dtype == torch.float32 and dropped.dtype == torch.int64
    assert np.array_equal(out.numpy().view(np.uint32), np.median(x.numpy(), axis=0).view(np.uint32))
    assert int(dropped.sum()) == (W - 1) * 4099


def test_even_w_median_is_the_mean_of_the_two_middle_values():
    x = torch.randn(6, 1001, generator=torch.Generator().manual_seed(0))
    out, _ = ops.trimmed_mean(x, 2)
    s = np.sort(x.numpy(), axis=0)
    assert np.array_equal(out.numpy(), (s[2] + s[3]) / np.float32(2))


@pytest.mark.parametrize("W", [1, 2, 7, 32])
def test_trim_zero_is_the_client_order_fp32_mean_bitwise(W):
    x = torch.randn(W, 2053, generator=torch.Generator().manual_seed(W)) * 1e3
    out, dropped = ops.trimmed_mean(x, 0)
    a = x.numpy()
    acc = a[0].copy()
    for c in range(1, W):
        acc = acc + a[c]
    assert np.array_equal(out.numpy().view(np.uint32), (acc / np.float32(W)).view(np.uint32))
    assert dropped.tolist() == [0] * W


def test_order_cases():
    col = torch.tensor([[NAN], [0.0], [-0.0], [INF], [-INF]])
    out, dropped = ops.trimmed_mean(col, 1)  # ranked -inf < -0.0 < +0.0 < +inf < NaN: the ends go
    assert out.tolist() == [INF] and dropped.tolist() == [1, 0, 0, 0, 1]
    out, dropped = ops.trimmed_mean(col, 0)
    assert torch.isnan(out).all() and dropped.tolist() == [0] * 5
    out, dropped = ops.trimmed_mean(col, 2)  # the median is +0.0 (rank 2), not -0.0
    assert out.tolist() == [0.0] and not np.signbit(out.numpy()[0]) and dropped.tolist() == [1, 0, 1, 1, 1]
    # -0.0 ranks below +0.0 whatever the client order (column 1: -0.0, -0.0, +0.0 -> the median is the
    # second -0.0); a negative-sign NaN still ranks highest
    z = torch.tensor([[0.0, -0.0, 1.0], [-0.0, 0.0, -NAN], [0.0, -0.0, 2.0]])
    out, dropped = ops.trimmed_mean(z, 1)
    assert out.tolist() == [0.0, -0.0, 2.0] and np.signbit(out.numpy()).tolist() == [False, True, False]
    assert dropped.tolist() == [2, 3, 1]
    k = ref.order_keys(torch.tensor([-INF, -1.0, -0.0, 0.0, 1.0, INF, NAN, -NAN]))
    assert k.tolist() == sorted(k.tolist()) and k[-1] == k[-2] == 0xFFFFFFFF and len(set(k.tolist())) == 7


def test_all_equal_values_charge_the_lowest_and_highest_client_indices():
    out, dropped = ops.trimmed_mean(torch.full((6, 7), 1.5), 2)
    assert out.tolist() == [1.5] * 7 and dropped.tolist() == [7, 7, 0, 0, 7, 7]
    out, dropped = ops.trimmed_mean(torch.full((5, 3), -2.0), 1)
    assert out.tolist() == [-2.0] * 3 and dropped.tolist() == [3, 0, 0, 0, 3]


@pytest.mark.parametrize("W,trim", [(3, 1), (8, 1), (8, 3), (16, 5), (32, 15)])
def test_dropped_sums_to_two_trim_n_and_chunking_changes_nothing(W, trim):
    x = torch.randint(0, 3, (W, 1500), generator=torch.Generator().manual_seed(W)).float()
    out, dropped = ref.trimmed_mean(x, trim)
    assert int(dropped.sum()) == 2 * trim * 1500
    out2, dropped2 = ref.trimmed_mean(x, trim, chunk=129)
    assert torch.equal(out, out2) and torch.equal(dropped, dropped2)
    o64, d64 = ref.trimmed_mean(x, trim, acc_dtype=torch.float64)
    assert o64.dtype == torch.float64 and torch.equal(d64, dropped)
    assert torch.equal(o64.float(), out)  # integer-valued: exact sums, one rounding on each side


# ---- fault injection, rule, config ----------------------------------------------------------
def test_fault_injector_parses_and_applies_scale():
    (r,) = parse("client:1:round:0:scale:-50")
    assert (r.role, r.index, r.round, r.action, r.arg) == ("client", 1, 0, "scale", -50.0)
    t = torch.tensor([1.0, -2.0, 0.5])
    FaultInjector("client", 1, "client:1:round:0:scale:-50").before_upload(0, t)
    assert t.tolist() == [-50.0, 100.0, -25.0]
    FaultInjector("client", 0, "client:1:round:0:scale:-50").before_upload(0, t)  # another client: untouched
    FaultInjector("client", 1, "client:1:round:0:scale:-50").before_upload(1, t)  # another round
    assert t.tolist() == [-50.0, 100.0, -25.0]


def test_rule_trim_for_and_its_errors():
    assert not RobustRule().active and RobustRule("median").active
    med, tm = RobustRule("median"), RobustRule("trimmed_mean", 2)
    assert [med.trim_for(W) for W in (1, 2, 3, 4, 8, 9)] == [0, 0, 1, 1, 3, 4]
    assert tm.trim_for(5) == 2 and tm.trim_for(32) == 2
    for W in (1, 3, 4):
        with pytest.raises(ValueError, match="robust_trim=2 needs more than 4 clients"):
            tm.trim_for(W)
    with pytest.raises(ValueError, match="robust_agg='krum'"):
        RobustRule("krum")
    with pytest.raises(ValueError, match="robust_trim=-1"):
        RobustRule("trimmed_mean", -1)
    x = torch.randn(5, 40)
    out, dropped = med.combine(x)
    assert torch.equal(out, x.median(0).values) and int(dropped.sum()) == 4 * 40
    rec = tm.record(torch.tensor([40, 0, 0, 20, 100]), 100, 5)
    assert rec == {"robust_agg": "trimmed_mean", "robust_trim": 2, "dropped_share": [0.4, 0.0, 0.0, 0.2, 1.0]}


def test_config_defaults_and_rejections():
    cfg = FedRecConfig()
    assert (cfg.robust_agg, cfg.robust_trim) == ("none", 1)
    cfg.secagg.enabled = cfg.weighted_fedavg = True
    assert not RobustRule.from_cfg(cfg, "grad_avg").active  # off: nothing to reject
    cfg = FedRecConfig()
    cfg.apply_overrides(["--robust_agg=median", "--robust_trim=2"])
    assert (cfg.robust_agg, cfg.robust_trim) == ("median", 2) and RobustRule.from_cfg(cfg, "param_avg").active
    with pytest.raises(ValueError, match="robust_agg=median.*mode=grad_avg"):
        RobustRule.from_cfg(cfg, "grad_avg")
    cfg.secagg.enabled = True
    with pytest.raises(ValueError, match="robust_agg=median.*secagg.enabled"):
        RobustRule.from_cfg(cfg, "fedavg_star")
    cfg.secagg.enabled, cfg.weighted_fedavg = False, True
    with pytest.raises(ValueError, match="robust_agg=median.*weighted_fedavg"):
        RobustRule.from_cfg(cfg, "param_avg")
    bad = FedRecConfig()
    bad.robust_agg = "mean"
    with pytest.raises(ValueError, match="robust_agg='mean'"):
        RobustRule.from_cfg(bad)


def test_grad_avg_driver_rejects_the_rule_at_start_up():
    from fedrec_with_pytorchdistributed_amd.train.federated import run_grad_avg
    cfg = FedRecConfig()
    cfg.robust_agg = "trimmed_mean"
    with pytest.raises(ValueError, match="mode=grad_avg"):
        run_grad_avg(cfg, None)  # before anything touches the context


# ---- drivers on gloo ------------------------------------------------------------------------
def _star_upload(tmp_path, tag, extra):
    d = tmp_path / tag
    server = ["server.py", "1", *TINY, f"--snapshot_path={d}/s.pt", "--round_artifacts=1", *extra]
    client = ["client.py", "1", "16", "1", "0", "c", *TINY, f"--snapshot_path={d}/c.pt", "--round_artifacts=1", *extra]
    _ok(run_ranks([server] + [client] * 3, {"FEDREC_STAR_AGG": "upload",
                                            "FEDREC_FAULT": "client:1:round:0:scale:-50"}, timeout=300))
    return d


@pytest.mark.slow
def test_star_upload_median_ignores_a_poisoned_client(tmp_path):
    """1 coordinator + 3 clients, client 1 uploads -50 x its model: the global model is the
    elementwise median of the three uploads bit for bit, and client 1 is the one that is cut."""
    d = _star_upload(tmp_path, "median", ["--robust_agg=median"])
    g = torch.load(d / "global_model_round0.pt", weights_only=True)
    rs = [torch.load(d / f"received_model_{k}.pt", weights_only=True) for k in range(3)]
    assert set(g) == set(rs[0])
    trainable = 0
    for key in g:
        want = np.median(np.stack([r[key].numpy() for r in rs]), axis=0)
        assert np.array_equal(g[key].numpy().view(np.uint32), want.view(np.uint32)), key
        trainable += int(not torch.equal(rs[0][key], rs[1][key]))
    assert trainable >= 10  # the uploads do differ (the poisoned client's, by a factor of -50)
    (rec,) = _metrics(str(d / "metrics.jsonl"))
    assert rec["robust_agg"] == "median" and rec["robust_trim"] == 1 and rec["clients_accepted"] == 3
    share = rec["dropped_share"]
    assert len(share) == 3 and share[1] == max(share) and share[1] > 0.9
    assert sum(share) == pytest.approx(2.0)  # 2 trim of 3 values cut at every coordinate
    # the same run with the plain mean is dragged away by the poisoned upload
    d0 = _star_upload(tmp_path, "mean", [])
    g0 = torch.load(d0 / "global_model_round0.pt", weights_only=True)
    key = "text_encoder.fc.weight"
    assert not torch.equal(g0[key], g[key])
    assert float(g0[key].abs().max()) > 5 * float(g[key].abs().max())
    assert "dropped_share" not in _metrics(str(d0 / "metrics.jsonl"))[0]


@pytest.mark.slow
def test_star_allgather_trimmed_mean_survives_a_nan_client(tmp_path):
    """Client-side aggregation, W = 3, client 1 uploads NaN: the all-reduce would spread it to every
    coordinate of the global model; the trimmed mean ranks NaN highest and cuts it."""
    server = ["server.py", "1", *TINY, f"--snapshot_path={tmp_path}/s.pt", "--robust_agg=trimmed_mean"]
    client = ["client.py", "1", "16", "1", "0", "c", *TINY, "--robust_agg=trimmed_mean"]
    _ok(run_ranks([server] + [client] * 3, {"FEDREC_STAR_AGG": "allreduce", "FEDREC_FAULT": "client:1:round:0:nan",
                                            "FEDREC_COLL_CHECK": "1"}, timeout=300))
    g = torch.load(tmp_path / "global_model_round0.pt", weights_only=True)
    assert all(torch.isfinite(v).all() for v in g.values())
    (rec,) = _metrics(str(tmp_path / "metrics.jsonl"))
    assert rec["robust_agg"] == "trimmed_mean" and rec["robust_trim"] == 1
    assert rec["dropped_share"][1] == 1.0 and sum(rec["dropped_share"]) == pytest.approx(2.0)


@pytest.mark.slow
def test_param_avg_three_ranks_stay_bitwise_identical(tmp_path):
    argv = ["Parameter_Averaging_main.py", "1", "16", "1", *TINY, "--robust_agg=trimmed_mean",
            f"--snapshot_path={tmp_path}/s.pt"]
    _ok(run_ranks([argv] * 3, {"FEDREC_DUMP_FLAT": str(tmp_path / "dump"), "FEDREC_COLL_CHECK": "1"}, timeout=300))
    a, b, c = (torch.load(tmp_path / "dump" / f"rank{i}.pt") for i in range(3))
    assert torch.equal(a, b) and torch.equal(a, c) and torch.isfinite(a).all()
    (rec,) = _metrics(str(tmp_path / "metrics.jsonl"))
    assert rec["robust_agg"] == "trimmed_mean" and rec["robust_trim"] == 1
    assert len(rec["dropped_share"]) == 3 and sum(rec["dropped_share"]) == pytest.approx(2.0)
