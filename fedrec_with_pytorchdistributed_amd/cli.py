"""Command-line front end.  The reference's positional contracts are kept verbatim:

* ``client.py <total_epochs> <batch_size> <save_every> <dp_epsilon:int> <run_name>``  (client.py:300-305)
* ``server.py <global_epochs>``                                                  (server.py:113)
* ``Gradient_Averaging_main.py / Parameter_Averaging_main.py / main.py
  <total_epochs> <batch_size> <save_every>``                                      (…_main.py:190-195)

and any trailing ``--key=value`` overrides a :class:`FedRecConfig` field (``--data_dir=...``,
``--dp.epsilon=10``, ``--backbone.name=bert-base``, ``--compat.reference_quirks=1`` ...).

All of them run under ``torchrun`` (RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* from the env), as in
the README recipe (``README.md:24-46``): two torchrun invocations (server node and client
node) join one c10d rendezvous; roles come from the entrypoint, never from rank numbers.
For a one-invocation single-node star run, ``python -m fedrec_with_pytorchdistributed_amd.cli
star <rounds> <epochs> <batch> [--k=v]`` under ``torchrun --nproc-per-node W+1`` makes rank 0
the coordinator and ranks 1..W the GPU clients.

Star upload compression (both off by default, both with an error-feedback residual kept in the client
snapshot): ``--upload_topk=F`` sends the ``k = max(1, ceil(F n))`` largest-magnitude coordinates of the
round delta (``8 k`` bytes instead of ``4 n``); ``--upload_bits=8`` / ``--upload_bits=4`` sends stochastic
8- or 4-bit codes with one fp32 scale per 256 coordinates (``n bits / 8 + 4 ceil(n / 256)`` bytes; with
``--upload_topk`` as well ``4 k + k bits / 8 + 4 ceil(k / 256)``).  Neither combines with
``--secagg.enabled=1``, ``--robust_agg`` or the averaging modes.
"""
from __future__ import annotations

import os
import sys
from typing import List, Optional

from .config import FedRecConfig


def _cfg(rest: List[str]) -> FedRecConfig:
    cfg = FedRecConfig()
    leftover = cfg.apply_overrides(rest)
    if leftover:
        raise SystemExit(f"unexpected arguments: {leftover}")
    return cfg


def _client_dev_offset() -> int:
    return int(os.environ.get("FEDREC_GPU_OFFSET", "0"))


def main_client(argv: Optional[List[str]] = None) -> int:
    argv = sys.argv[1:] if argv is None else argv
    pos = [a for a in argv if not a.startswith("--")]
    if len(pos) < 5:
        raise SystemExit("usage: client.py <total_epochs> <batch_size> <save_every> <dp_epsilon> <run_name> [--k=v]")
    cfg = _cfg([a for a in argv if a.startswith("--")])
    cfg.total_epochs, cfg.batch_size, cfg.save_every = int(pos[0]), int(pos[1]), int(pos[2])
    eps = int(pos[3])
    cfg.dp.epsilon, cfg.dp.enabled = float(eps), bool(eps)  # dp_enabled = bool(dp_Epsilon) (client.py:304)
    cfg.run_name = pos[4]
    cfg.mode = "fedavg_star"
    from .parallel import dist as fdist
    from .train.federated import run_star_client

    ctx = fdist.init("client", cfg.device, cfg.collective_timeout_s, gpu_offset=_client_dev_offset())
    try:
        run_star_client(cfg, ctx)
    finally:
        fdist.shutdown(ctx)
    return 0


def main_server(argv: Optional[List[str]] = None) -> int:
    argv = sys.argv[1:] if argv is None else argv
    pos = [a for a in argv if not a.startswith("--")]
    if len(pos) < 1:
        raise SystemExit("usage: server.py <global_epochs> [--k=v]")
    cfg = _cfg([a for a in argv if a.startswith("--")])
    cfg.global_rounds = int(pos[0])
    cfg.mode = "fedavg_star"
    from .parallel import dist as fdist
    from .train.federated import run_star_server

    ctx = fdist.init("server", "cpu", cfg.collective_timeout_s)
    try:
        run_star_server(cfg, ctx)
    finally:
        fdist.shutdown(ctx)
    return 0


def _main_dp(mode: str, argv: Optional[List[str]]) -> int:
    argv = sys.argv[1:] if argv is None else argv
    pos = [a for a in argv if not a.startswith("--")]
    if len(pos) < 3:
        raise SystemExit("usage: <total_epochs> <batch_size> <save_every> [--k=v]")
    cfg = _cfg([a for a in argv if a.startswith("--")])
    cfg.total_epochs, cfg.batch_size, cfg.save_every = int(pos[0]), int(pos[1]), int(pos[2])
    cfg.mode = mode
    from .parallel import dist as fdist
    from .train.federated import run_grad_avg, run_param_avg

    ctx = fdist.init("client", cfg.device, cfg.collective_timeout_s)
    try:
        (run_grad_avg if mode == "grad_avg" else run_param_avg)(cfg, ctx)
    finally:
        fdist.shutdown(ctx)
    return 0


def main_grad_avg(argv=None) -> int:
    return _main_dp("grad_avg", argv)


def main_param_avg(argv=None) -> int:
    return _main_dp("param_avg", argv)


def main_star(argv: Optional[List[str]] = None) -> int:
    """One torchrun: rank 0 coordinator, ranks 1..W GPU clients."""
    argv = sys.argv[1:] if argv is None else argv
    pos = [a for a in argv if not a.startswith("--")]
    if len(pos) < 3:
        raise SystemExit("usage: star <global_rounds> <local_epochs> <batch_size> [--k=v]")
    rank = int(os.environ.get("RANK", "0"))
    extra = [a for a in argv if a.startswith("--")]
    if rank == 0:
        return main_server([pos[0], *extra])
    os.environ["FEDREC_GPU_OFFSET"] = "1"
    return main_client([pos[1], pos[2], "1", "0", "star", *extra])


def _offline_engine(argv: List[str], own: dict, usage: str):
    """The single-process commands' setup (no process group): ``SNAPSHOT`` (a snapshot of
    ``train/checkpoint.py``, or ``none`` for the freshly initialised model) and ``--key=value``
    arguments -- the command's ``own`` keys are filled in place, the rest override the config ->
    ``(engine, shard)``."""
    import types

    pos = [a for a in argv if not a.startswith("--")]
    if len(pos) != 1:
        raise SystemExit(usage)
    rest = []
    for a in argv:
        if a.startswith("--"):
            key, _, val = a[2:].partition("=")
            if key in own:
                own[key] = val
            else:
                rest.append(a)
    cfg = _cfg(rest)
    import torch

    from .train import checkpoint as ckpt
    from .train.engine import LocalEngine
    from .train.federated import build_model, load_client_shard

    cuda = cfg.device == "cuda" or (cfg.device == "auto" and torch.cuda.is_available()
                                    and os.environ.get("FEDREC_CPU_ONLY", "0") != "1")
    dev = torch.device("cuda", 0) if cuda else torch.device("cpu")
    shard = load_client_shard(cfg, types.SimpleNamespace(client_index=0, num_clients=1))
    model = build_model(cfg, dev)
    if pos[0].lower() != "none":
        ckpt.load_snapshot(pos[0], model, rng=False)
    return LocalEngine(cfg, model, shard, dev), shard


def _uid_name(shard, i: int) -> str:
    uids = getattr(shard, "_uids", None) or []
    u = int(shard.valid.uid[i])
    return uids[u] if u < len(uids) else f"U{u}"


def main_recommend(argv: Optional[List[str]] = None):
    """``recommend SNAPSHOT --data_dir=... --k=10 [--limit=N] [--out=recs.jsonl] [--diversity=L [--pool=P]]
    [--key=value ...]``: rank the whole catalog for every validation impression of the shard (single
    process, no process group).  ``SNAPSHOT``: a snapshot of ``train/checkpoint.py``, or ``none`` for
    the freshly initialised model.  Writes one JSON line per impression (``uid``, ``news``: the nid
    strings best first, ``scores``) to ``--out`` (default: stdout); prints and returns the hr / ndcg /
    mrr metrics as the final JSON line.  ``--diversity=L`` (MMR's lambda, 0..1) re-ranks the ``--pool``
    most relevant news (k..128; default ``min(128, max(4 k, 32))``) for diversity
    (``LocalEngine.recommend``) and adds ``ild@k`` / ``coverage@k`` to the metrics; ``--diversity=1``
    keeps the relevance lists and reports their diversity."""
    import json

    argv = sys.argv[1:] if argv is None else argv
    own = {"k": "10", "limit": "", "out": "", "batch": "256", "diversity": "", "pool": ""}
    usage = ("usage: recommend <snapshot|none> --data_dir=... [--k=10] [--limit=N] [--out=FILE] "
             "[--diversity=0..1 [--pool=k..128]] [--k=v]")
    # the command's own numbers are checked before the engine is built
    given = {a[2:].partition("=")[0]: a[2:].partition("=")[2] for a in argv if a.startswith("--")}
    diversity = pool = None
    try:
        k = int(given.get("k", own["k"]))
        if given.get("diversity", ""):
            diversity = float(given["diversity"])
        if given.get("pool", ""):
            pool = int(given["pool"])
    except ValueError:
        raise SystemExit(usage)
    if diversity is not None and not (0.0 <= diversity <= 1.0):
        raise SystemExit(f"recommend: --diversity must lie in [0, 1] (got {given['diversity']})\n{usage}")
    if pool is not None and diversity is None:
        raise SystemExit(f"recommend: --pool needs --diversity\n{usage}")
    if diversity is not None and not (1 <= k <= (k if pool is None else pool) <= 128):
        raise SystemExit(f"recommend: --diversity needs 1 <= k <= pool <= 128 (got k {k}, pool {pool})\n{usage}")
    eng, shard = _offline_engine(argv, own, usage)
    limit = int(own["limit"]) if own["limit"] else None
    metrics, ids, scores = eng.recommend_valid(k, int(own["batch"]), limit, return_lists=True, diversity=diversity,
                                               pool=pool)
    i2n = shard.index2nid
    f = open(own["out"], "w") if own["out"] else sys.stdout
    try:
        for i in range(ids.shape[0]):
            keep = ids[i] >= 0
            f.write(json.dumps({"uid": _uid_name(shard, i),
                                "news": [i2n[int(x)] for x in ids[i][keep]],
                                "scores": [float(x) for x in scores[i][keep]]}) + "\n")
    finally:
        if f is not sys.stdout:
            f.close()
    print(json.dumps(metrics), flush=True)
    return metrics


def main_evaluate(argv: Optional[List[str]] = None):
    """``evaluate SNAPSHOT --data_dir=... [--limit=N] [--batch=256] [--out=FILE] [--key=value ...]``:
    full-impression evaluation of the shard's validation split (single process, no process group):
    every impression's positive ranked against ALL the negatives it showed
    (``LocalEngine.validate_full``).  ``SNAPSHOT`` as for ``recommend``.  With ``--out``, one JSON
    line per impression: ``uid``, ``pos`` (the positive's nid), ``rank`` (ties against the positive;
    null where a score is NaN) and ``candidates`` (negatives + 1).  Prints and returns the
    ``full_*`` metrics as the final stdout line."""
    import json

    argv = sys.argv[1:] if argv is None else argv
    own = {"limit": "", "out": "", "batch": "256"}
    eng, shard = _offline_engine(
        argv, own, "usage: evaluate <snapshot|none> --data_dir=... [--limit=N] [--batch=256] [--out=FILE] [--k=v]")
    limit = int(own["limit"]) if own["limit"] else None
    metrics, counts = eng.validate_full(int(own["batch"]), limit, return_counts=True)
    if own["out"]:
        i2n = shard.index2nid
        with open(own["out"], "w") as f:
            for i in range(counts.shape[0]):
                gt, eq, nn, nan = (int(x) for x in counts[i])
                f.write(json.dumps({"uid": _uid_name(shard, i), "pos": i2n[int(shard.valid.pos[i])],
                                    "rank": None if nan else 1 + gt + eq, "candidates": nn + 1}) + "\n")
    print(json.dumps(metrics), flush=True)
    return metrics


COMMANDS = {"client": main_client, "server": main_server, "grad_avg": main_grad_avg, "param_avg": main_param_avg,
            "star": main_star, "recommend": main_recommend, "evaluate": main_evaluate}


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else argv
    if not argv or argv[0] not in COMMANDS:
        raise SystemExit(f"usage: python -m fedrec_with_pytorchdistributed_amd.cli {{{','.join(COMMANDS)}}} ...")
    rc = COMMANDS[argv[0]](argv[1:])
    return rc if isinstance(rc, int) else 0


if __name__ == "__main__":
    sys.exit(main())
