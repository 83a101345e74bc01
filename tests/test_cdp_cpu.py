"""Client-level DP on the host: the two contract oracles (``ops.reference.dp_*``) against plain numpy / Python floats,
the accountant of ``ClientDP``, its config rejections, a two-client star run on gloo (pass-through, the clip bound in
the clear and under secure aggregation, the noise record) and the ``fedrec_dp::`` schema pin.  No GPU.

A deliberate interface change regenerates the fixture: ``python tests/test_cdp_cpu.py``."""
import json
import math
import os

import numpy as np
import pytest
import torch

from launch_util import run_ranks

from fedrec_with_pytorchdistributed_amd.config import FedRecConfig
from fedrec_with_pytorchdistributed_amd.ops import native
from fedrec_with_pytorchdistributed_amd.ops import reference as ref
from fedrec_with_pytorchdistributed_amd.parallel import secagg
from fedrec_with_pytorchdistributed_amd.parallel.cdp import ClientDP
from fedrec_with_pytorchdistributed_amd.privacy import rdp
from fedrec_with_pytorchdistributed_amd.train.federated import build_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "op_schemas_dp.txt")
TINY = ["--data_dir=synthetic:tiny", "--backbone.name=tiny", "--round_timeout_s=120", "--collective_timeout_s=120"]


def _pair(n):
    g = torch.Generator().manual_seed(n)
    base = torch.randn(n, generator=g)
    return base + 1e-2 * torch.randn(n, generator=g), base


# ---- the contract oracles -------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 9, 1025, 65 * 1024 + 4, (1 << 20) + 77])
def test_sqnorm_oracle_against_numpy(n):
    local, base = _pair(n)
    sq, s, clipped = ref.dp_state_fields(ref.dp_delta_sqnorm(local, base))
    want = float(np.sum((local - base).numpy().astype(np.float64) ** 2))
    assert abs(sq - want) <= n * 2.0 ** -52 * want and (s, clipped) == (0.0, 0)


@pytest.mark.parametrize("frac", [2.0, 0.5, 1e-3])
@pytest.mark.parametrize("n", [1, 5, 9])
def test_clip_oracle_against_a_python_float_loop(n, frac):
    local, base = _pair(n)
    state = ref.dp_delta_sqnorm(local, base)
    clip = frac * math.sqrt(ref.dp_state_fields(state)[0])
    out = ref.dp_clip_noise(local, base, state, clip, 0.0, 1, 2)
    _, s, clipped = ref.dp_state_fields(state)
    f32 = lambda x: float(np.float32(x))  # a product or sum of two fp32 values, taken in fp64, rounded once to fp32
    want = [l if s == 1.0 else f32(b + f32(s * f32(l - b))) for l, b in zip(local.tolist(), base.tolist())]
    assert out.tolist() == want and clipped == int(frac < 1) and s == f32(min(1.0, frac))


# ---- accounting -----------------------------------------------------------------------------
@pytest.mark.parametrize("z", [0.5, 1.0])
@pytest.mark.parametrize("R", [1, 5])
def test_epsilon_after_r_rounds_is_the_rdp_of_r_gaussian_releases(R, z):
    rule = ClientDP(1.0, z, delta=1e-5, seed=1, clients=4)
    for _ in range(R):
        rec = rule.record(4, 4)
    want = rdp.get_privacy_spent(rdp.DEFAULT_ALPHAS, rdp.compute_rdp(1.0, z, R, rdp.DEFAULT_ALPHAS), 1e-5)[0]
    assert rec["cdp_epsilon"] == want and rec["cdp_noise_effective"] == z and rule.std_for(4) == z / 2
    part = rule.record(3, 4)  # three of four shares arrived
    assert part["cdp_noise_effective"] == z * math.sqrt(3 / 4) and rule.accountant.history[-1] == (z * math.sqrt(3 / 4), 1.0, 1)
    assert rule.record(4, 4, spent=False)["cdp_epsilon"] == part["cdp_epsilon"]  # a rejected aggregate spends nothing
    again = ClientDP(1.0, z, seed=1)
    again.load(json.loads(json.dumps(rule.state())))  # what the coordinator's snapshot keeps
    assert again.accountant.history == rule.accountant.history


def test_epsilon_calibrates_the_multiplier_over_the_rounds():
    cfg = FedRecConfig()
    cfg.apply_overrides(["--cdp.clip=1", "--cdp.epsilon=8", "--global_rounds=5"])
    rule = ClientDP.from_cfg(cfg, "fedavg_star", 4)
    for _ in range(5):
        rec = rule.record(4, 4)
    assert 8 - 0.01 <= rec["cdp_epsilon"] <= 8 and rec["cdp_noise_multiplier"] == rule.z > 0
    cfg.apply_overrides(["--cdp.noise_multiplier=0"])  # clip only
    assert ClientDP.from_cfg(cfg, "fedavg_star", 4).record(4, 4)["cdp_epsilon"] == math.inf


# ---- config ---------------------------------------------------------------------------------
REJECTED = [(["--robust_agg=median"], "fedavg_star", "cdp.clip=.*robust_agg=median"),
            (["--weighted_fedavg=1"], "fedavg_star", "cdp.clip=.*weighted_fedavg=1"),
            (["--upload_topk=0.1"], "fedavg_star", "cdp.clip=.*upload_topk=0.1"),
            (["--upload_bits=8"], "fedavg_star", "cdp.clip=.*upload_bits=8"),
            ([], "param_avg", "cdp.clip=.*mode=param_avg"),
            ([], "grad_avg", "cdp.clip=.*mode=grad_avg")]


@pytest.mark.parametrize("extra,driver,msg", REJECTED, ids=[r[2].split("*")[1] for r in REJECTED])
def test_from_cfg_rejects_what_the_bound_does_not_cover(extra, driver, msg):
    cfg = FedRecConfig()
    cfg.apply_overrides(extra)
    assert not ClientDP.from_cfg(cfg, driver).active  # off: nothing to reject
    cfg.apply_overrides(["--cdp.clip=0.5", "--cdp.noise_multiplier=1"])
    with pytest.raises(ValueError, match=msg):
        ClientDP.from_cfg(cfg, driver)


def test_from_cfg_accepts_secure_aggregation_and_the_server_step():
    cfg = FedRecConfig()
    cfg.apply_overrides(["--cdp.clip=0.5", "--cdp.noise_multiplier=1", "--secagg.enabled=1", "--server_lr=0.5"])
    rule = ClientDP.from_cfg(cfg, "fedavg_star", 4)
    assert rule.active and (rule.clip, rule.z, rule.std_for(4)) == (0.5, 1.0, 0.25)
    assert ClientDP(0.5, 1.0)._key != ClientDP(0.5, 1.0)._key  # seed 0: a fresh key from OS entropy each


# ---- a two-client star run on gloo ----------------------------------------------------------
def _star(tmp_path, tag, extra):
    """Two rounds, coordinator + two clients -> (the initial global model and the one after each round, flat fp64; the
    round records).  The coordinator's initial model is ``build_model`` of the same config (seeded)."""
    d = tmp_path / tag
    common = [*TINY, "--global_rounds=2", *extra]
    server = ["server.py", "2", *common, f"--snapshot_path={d}/s.pt"]
    client = ["client.py", "1", "16", "1", "0", "c", *common, f"--snapshot_path={d}/c.pt"]
    for rc, out in run_ranks([server] + [client] * 2, {"FEDREC_STAR_AGG": "upload"}, timeout=300):
        assert rc == 0, out[-3000:]
    with open(d / "metrics.jsonl") as f:
        recs = [r for r in map(json.loads, filter(str.strip, f)) if not r.get("final_global")]
    flat = lambda sd: torch.cat([sd[k].reshape(-1).double() for k in sorted(sd) if sd[k].is_floating_point()])
    cfg = FedRecConfig()
    cfg.apply_overrides(TINY)
    first = flat(build_model(cfg, torch.device("cpu")).state_dict())
    return [first] + [flat(torch.load(d / f"global_model_round{r}.pt", weights_only=True)) for r in range(2)], recs


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _star(tmp_path_factory.mktemp("cdp"), "plain", [])


CLIP = 1e-3
RUNS = {"loose": ["--cdp.clip=1e9", "--cdp.noise_multiplier=0", "--cdp.seed=5"],
        "tight": [f"--cdp.clip={CLIP}", "--cdp.noise_multiplier=0"],
        "secure": [f"--cdp.clip={CLIP}", "--cdp.noise_multiplier=0", "--secagg.enabled=1"],
        "noise": [f"--cdp.clip={CLIP}", "--cdp.noise_multiplier=1"]}


@pytest.mark.slow
@pytest.mark.parametrize("kind", list(RUNS))
def test_two_client_star_run(tmp_path, plain, kind):
    models, recs = _star(tmp_path, kind, RUNS[kind])
    assert len(recs) == 2 and all(r["cdp_clip"] == float(RUNS[kind][0].split("=")[1]) for r in recs)
    if kind == "loose":  # nothing is clipped: the models pass through bit for bit
        assert all(torch.equal(a, b) for a, b in zip(models, plain[0])) and "cdp_clip" not in plain[1][0]
    elif kind == "noise":
        eps = [r["cdp_epsilon"] for r in recs]
        assert all(r["cdp_noise_effective"] == 1.0 and r["cdp_noise_multiplier"] == 1.0 and r["cdp_delta"] == 1e-5
                   for r in recs) and 0 < eps[0] < eps[1] < math.inf
    else:
        # the mean of deltas of norm <= C has norm <= C.  Under secure aggregation each of the W = 2 uploads u_k =
        # delta_k / W (max |u_k| <= C / W) is rounded to the agreed grid 2^-f: at most W 2^(-f-1) per coordinate
        n, slack = models[0].numel(), 0.0
        if kind == "secure":
            f, _ = secagg.hist_frac_bits(secagg.hist_local(torch.tensor([CLIP / 2])), 2)
            slack = math.sqrt(n) * 2 * 2.0 ** (-f - 1)
        assert recs[0]["cdp_epsilon"] == math.inf and float((plain[0][1] - plain[0][0]).norm()) > CLIP  # unclipped: more
        for r in range(2):  # every round's new global model against that round's theta_g
            step = float((models[r + 1] - models[r]).norm())
            print(f"{kind} round {r}: ||new - theta_g|| {step:.6e}, bound {CLIP * (1 + 1e-5) + slack:.6e} (grid {slack:.3e})")
            assert 0 < step <= CLIP * (1 + 1e-5) + slack


# ---- the registered interface ---------------------------------------------------------------
def _registered(prefix="fedrec_dp::"):
    native.lib()
    out = {}
    for name in torch._C._dispatch_get_all_op_names():
        if name.startswith(prefix):
            kinds = [k for k in ("CUDA", "CompositeImplicitAutograd", "CompositeExplicitAutograd")
                     if torch._C._dispatch_has_kernel_for_dispatch_key(name, k)]
            out[name] = f"{torch._C._get_schema(name, '')} | {'+'.join(kinds) or 'none'}"
    return out


def test_dp_schemas_match_the_fixture_and_fedrec_keeps_its_80_ops():
    with open(GOLDEN) as f:
        assert [ln for _, ln in sorted(_registered().items())] == [ln.rstrip("\n") for ln in f if ln.strip()]
    assert sorted(_registered()) == ["fedrec_dp::clip_noise", "fedrec_dp::delta_sqnorm"]
    assert len(_registered("fedrec::")) == 80


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        f.write("".join(ln + "\n" for _, ln in sorted(_registered().items())))
    print(f"wrote {len(_registered())} schemas to {GOLDEN}")
