"""Multi-client GPU rehearsal on a one-GPU box: two client processes share the card
(``FEDREC_SHARE_GPU=1``) and talk over a gloo data plane (``FEDREC_DATA_BACKEND=gloo``;
RCCL refuses two ranks on one device).  Everything else is the 8-GPU code path: the real
kernels, the side-stream gradient all-reduce + Adam overlapped with the next step's
backbone forward, the lookahead sampler stream, the bench.py launch contract."""
import json

import pytest
import torch

from launch_util import run_ranks

SHARE = {"FEDREC_CPU_ONLY": "0", "FEDREC_SHARE_GPU": "1", "FEDREC_DATA_BACKEND": "gloo", "FEDREC_QUIET": "1"}


def _ok(outs):
    for rc, out in outs:
        assert rc == 0, out[-3000:]


@pytest.mark.gpu
def test_grad_avg_two_clients_on_gpu_stay_identical(tmp_path, dev):
    snap = str(tmp_path / "snapshot.pt")
    argv = ["Gradient_Averaging_main.py", "2", "32", "1", "--data_dir=synthetic:tiny", "--round_timeout_s=300",
            "--collective_timeout_s=300", f"--snapshot_path={snap}"]
    env = dict(SHARE, FEDREC_DUMP_FLAT=str(tmp_path / "dump"))
    outs = run_ranks([argv, argv], env, timeout=400)
    _ok(outs)
    a = torch.load(tmp_path / "dump" / "rank0.pt")
    b = torch.load(tmp_path / "dump" / "rank1.pt")
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), "GA clients must hold bit-identical parameters after every step"


@pytest.mark.gpu
def test_bench_two_clients_on_gpu(dev):
    argv = ["bench.py", "--gpus", "2", "--steps", "3", "--warmup", "2", "--preset", "small", "--valid-limit", "64",
            "--full"]
    outs = run_ranks([argv, argv], SHARE, timeout=400)
    _ok(outs)
    lines = [[l for l in out.splitlines() if l.startswith("{")] for _, out in outs]
    assert len(lines[0]) == 1 and lines[1] == []
    r = json.loads(lines[0][0])
    assert r["n_gpus"] == 2 and r["config"]["parallelism"] == "dp2" and r["value"] > 0
    assert r["dtype"] == "bf16" and r["train_loss"] == r["train_loss"]  # not NaN
    # the data-plane self-check ran, and the custom IPC all-reduce matched the group's sum
    assert r["data_plane_selfcheck"]["ok"] and r["data_plane_selfcheck"]["size"] == 2
    ipc = r["ipc_allreduce"]
    assert ipc.get("matches_rccl") is True and ipc.get("status") == 0, ipc


@pytest.mark.gpu
def test_grad_avg_two_clients_ipc_allreduce(tmp_path, dev):
    """GA with the gradient bucket summed by the custom IPC all-reduce (FEDREC_ALLREDUCE=ipc,
    real IPC handles between the two processes): both clients bit-identical, and the same
    parameters as the gloo data plane up to summation order."""
    base = ["Gradient_Averaging_main.py", "1", "32", "0", "--data_dir=synthetic:tiny", "--round_timeout_s=300",
            "--collective_timeout_s=300", "--user_dropout=0"]
    outs = run_ranks([base, base], dict(SHARE, FEDREC_DUMP_FLAT=str(tmp_path / "gloo")), timeout=400)
    _ok(outs)
    outs = run_ranks([base, base], dict(SHARE, FEDREC_DUMP_FLAT=str(tmp_path / "ipc"), FEDREC_ALLREDUCE="ipc"),
                     timeout=400)
    _ok(outs)
    a = torch.load(tmp_path / "ipc" / "rank0.pt")
    assert torch.equal(a, torch.load(tmp_path / "ipc" / "rank1.pt"))
    ref = torch.load(tmp_path / "gloo" / "rank0.pt")
    d = (a - ref).abs()
    assert float(torch.quantile(d, 0.999)) < 1e-5 and float(d.max()) < 5e-5 * 40


@pytest.mark.gpu
@pytest.mark.parametrize("config,ranks", [(2, 4), (3, 2), (4, 2), (5, 2)])
def test_bench_configs_multi_client_on_gpu(dev, config, ranks):
    """Every BASELINE config through bench.py with several clients on one GPU (gloo data
    plane): GA at 4 ranks, parameter averaging, LDP, and the unfrozen BERT-base with secure
    aggregation (pairwise masks over the store, int32 all-reduce)."""
    argv = ["bench.py", "--gpus", str(ranks), "--steps", "2", "--warmup", "1", "--preset", "small", "--valid-limit", "32",
            "--config", str(config), "--pa-every", "1", "--full"]
    if config == 5:
        argv += ["--batch", "16"]
    outs = run_ranks([argv] * ranks, SHARE, timeout=600)
    _ok(outs)
    lines = [l for l in outs[0][1].splitlines() if l.startswith("{")]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["n_gpus"] == ranks and r["config"]["baseline_config"] == config
    assert r["value"] > 0 and r["train_loss"] == r["train_loss"]


@pytest.mark.gpu
def test_grad_avg_unfrozen_secure_buckets_two_clients_on_gpu(tmp_path, dev):
    """Unfrozen backbone GA with pairwise-masked buckets reduced from autograd hooks on a
    side stream during the backward (device-side histogram bound, no host read): both
    clients end bit-identical -- over the gloo data plane and over the custom IPC all-reduce
    (FEDREC_ALLREDUCE=ipc, real IPC handles), and the two transports agree BITWISE (the
    masked fixed-point sums are exact integer sums, whatever moves them)."""
    argv = ["Gradient_Averaging_main.py", "1", "16", "1", "--data_dir=synthetic:tiny", "--backbone.frozen=0",
            "--backbone.n_layers=2", "--secagg.enabled=1", "--round_timeout_s=300", "--collective_timeout_s=300",
            f"--snapshot_path={tmp_path}/s.pt"]
    got = {}
    for plane in ("gloo", "ipc"):
        env = dict(SHARE, FEDREC_DUMP_FLAT=str(tmp_path / plane), FEDREC_BUCKET_MB="8")
        if plane == "ipc":
            env["FEDREC_ALLREDUCE"] = "ipc"
        outs = run_ranks([argv, argv], env, timeout=500)
        _ok(outs)
        a = torch.load(tmp_path / plane / "rank0.pt")
        b = torch.load(tmp_path / plane / "rank1.pt")
        assert a.numel() > 20_000_000 and torch.isfinite(a).all()
        assert torch.equal(a, b), plane
        got[plane] = a
    assert torch.equal(got["gloo"], got["ipc"])


@pytest.mark.gpu
def test_secure_sum_exact_four_clients_device_kernels(dev):
    """The W-client exact secure sum through the HIP histogram / mask / unmask kernels (four
    client processes on the one card, gloo moving the int32 buffers): equal to the plain sum
    within the fixed-point grid at every step of tests/_secagg_worker.py."""
    outs = run_ranks([["tests/_secagg_worker.py", "--device", "cuda"]] * 4, SHARE, timeout=300)
    _ok(outs)
    for _, out in outs:
        assert "SECAGG OK" in out, out[-2000:]


@pytest.mark.gpu
def test_ipc_allreduce_dead_peer_raises(dev):
    """A client that vanishes makes the surviving client's IPC all-reduce time out within the
    configured bound, poison its output and raise at check() -- a wrong gradient sum is never
    returned silently; later calls fail fast."""
    outs = run_ranks([["tests/_ipc_peer_worker.py"]] * 2, SHARE, timeout=120)
    _ok(outs)
    assert "PEER OK" in outs[0][1], outs[0][1][-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("ranks", [2, 4])
def test_graph_allreduce_one_replay_per_step(dev, ranks):
    """N > 1 as one graph replay per step: the device-epoch IPC all-reduce of the flat gradient
    and the device-step Adam run inside the captured step graph (engine counters: every step a
    replay with the optimizer in it, no eager optimizer step); clients bit-identical; the same
    trajectory as the eager all-reduce + Adam path within fp32 summation order.  The hidden-
    state cache is built cooperatively over the (gloo) data plane."""
    outs = run_ranks([["tests/_graph_ar_worker.py"]] * ranks, SHARE, timeout=400)
    _ok(outs)
    for _, out in outs:
        assert "GRAPH_AR OK" in out, out[-2000:]


@pytest.mark.gpu
@pytest.mark.slow
def test_grad_avg_four_clients_learns_like_one(tmp_path, dev):
    """Federated quality at W = 4: gradient averaging over four clients that
    share the card (batch 16 each = the one-client run's 64 impressions per step, the same
    users split four ways) lifts the planted-signal validation AUC past 0.6 in three epochs,
    as the one-client run does (profiles/r5_quality_fed: 0.6559 at W = 4, 0.6546 at W = 8,
    0.6568 at W = 1)."""
    mp = tmp_path / "metrics.jsonl"
    argv = ["Gradient_Averaging_main.py", "3", "16", "0", "--data_dir=synthetic:small", "--lr=1e-4",
            "--score_act=identity", "--round_timeout_s=300", "--collective_timeout_s=300", f"--metrics_path={mp}",
            f"--snapshot_path={tmp_path}/s.pt"]
    outs = run_ranks([argv] * 4, SHARE, timeout=400)
    _ok(outs)
    rows = [json.loads(l) for l in open(mp) if l.strip()]
    assert len(rows) == 3 and rows[-1]["clients"] == 4
    assert rows[-1]["valid_auc"] > 0.6, [r["valid_auc"] for r in rows]
