"""Diversity re-rank: the fused kernel (``ops.mmr_rerank``, csrc/mmr_rerank.hip) against the library
composition on the same device -- gather the pool's rows (``[B, P, D]``), normalise, ``bmm`` to the
``[B, P, P]`` cosines, then a k-step host loop of ``max`` / ``argmax`` / ``scatter`` launches -- at B =
4096, P = 128, k = 10, D = 400, N = the mind-small catalog size; and ``ops.topk_scores`` alone
against ``topk_scores`` + re-rank, the cost of diversity per request.

Device events around each call, warm-up first, the sides alternating within a round, median over
the rounds' medians; peak extra device memory of one call of each side.  ``--quality`` adds the
``hr@10`` / ``ild@10`` / ``coverage@10`` of ``LocalEngine.recommend_valid`` on the synthetic mind-small
shard (freshly initialised model) at lam in {1, 0.7, 0.5}.  One JSON line per measurement.

    python benchmarks/rerank_bench.py [--quality] [--out rerank_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import native

NINF = float("-inf")


def composed(table, ids, rel, k, lam):
    """The torch composition of the contract (full pools: every slot valid)."""
    B, P = ids.shape
    x = table.index_select(0, ids.reshape(-1).long()).view(B, P, -1)
    x = x / x.norm(dim=2, keepdim=True)
    c = torch.bmm(x, x.transpose(1, 2))
    mn, mx = rel.amin(1, keepdim=True), rel.amax(1, keepdim=True)
    rhat = (rel - mn) / (mx - mn)
    ms = torch.zeros_like(rel)
    taken = torch.zeros_like(rel, dtype=torch.bool)
    sel = torch.empty(B, k, dtype=torch.int64, device=ids.device)
    for t in range(k):
        m = lam * rhat - (1.0 - lam) * ms if t else lam * rhat
        j = m.masked_fill(taken, NINF).argmax(1)
        sel[:, t] = j
        taken.scatter_(1, j[:, None], True)
        cj = c.gather(2, j[:, None, None].expand(B, P, 1)).squeeze(2)
        ms = torch.maximum(ms, cj) if t else cj
    sub = c.gather(1, sel[:, :, None].expand(B, k, P)).gather(2, sel[:, None, :].expand(B, k, k))
    ild = (1.0 - sub).triu(1).sum((1, 2)) / (k * (k - 1) / 2)
    return ids.gather(1, sel), rel.gather(1, sel), ild


def timeit(fn, iters, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def quality(lams, k, limit, cfg_args):
    """``recommend_valid`` of the ``recommend`` command's engine (freshly initialised model) per lam."""
    from fedrec_with_pytorchdistributed_amd import cli

    eng, _ = cli._offline_engine(["none", *cfg_args], {}, "rerank_bench --quality_cfg: --key=value config overrides")
    eng.news_table = eng.encode_all(grad=False)  # one table for every lam
    out = []
    for lam in lams:
        m = eng.recommend_valid(k, 256, limit, diversity=lam)
        out.append({"bench": "rerank_quality", "cfg": list(cfg_args), "model": "random init", **m})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=65000)
    ap.add_argument("--D", type=int, default=400)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--P", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--lam", type=float, default=0.7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--quality_limit", type=int, default=4096)
    ap.add_argument("--quality_cfg", nargs="*", default=["--data_dir=synthetic:mind-small"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rerank_bench needs a HIP device")
    native.lib()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    # clustered rows (120 centres + 0.5 noise): a pool holds near-duplicates, as a news catalog does
    centres = torch.randn(120, a.D, generator=g)
    t = (centres[torch.randint(0, 120, (a.N,), generator=g)] + 0.5 * torch.randn(a.N, a.D, generator=g)).to(dev)
    u = torch.randn(a.B, a.D, generator=g).to(dev)
    topk = lambda: ops.topk_scores(u, t, a.k, None, 1)
    pool = lambda: ops.topk_scores(u, t, a.P, None, 1)
    rel, ids = pool()
    fused = lambda: ops.mmr_rerank(t, ids, rel, a.k, a.lam)
    comp = lambda: composed(t, ids, rel, a.k, a.lam)
    both = lambda: ops.mmr_rerank(t, *reversed(pool()), a.k, a.lam)
    p_def = min(128, max(4 * a.k, 32))  # LocalEngine.mmr_pool's default
    both_def = lambda: ops.mmr_rerank(t, *reversed(ops.topk_scores(u, t, p_def, None, 1)), a.k, a.lam)
    # the two sides sum in different orders: report how many lists agree, do not require it
    (fi, fr, fd), (ci, cr, cd) = fused(), comp()
    agree = float((fi == ci).all(1).float().mean())
    ild_diff = float((fd - cd).abs().max())
    tf, tc, tk, tb, tp, td = [], [], [], [], [], []
    for _ in range(a.rounds):
        tf.append(timeit(fused, a.iters, a.warmup))
        tc.append(timeit(comp, a.iters, a.warmup))
        tk.append(timeit(topk, a.iters, a.warmup))
        tb.append(timeit(both, a.iters, a.warmup))
        tp.append(timeit(pool, a.iters, a.warmup))
        td.append(timeit(both_def, a.iters, a.warmup))
    med = statistics.median
    gather_bytes = a.B * a.P * a.D * 4
    lines = [{"bench": "rerank", "B": a.B, "P": a.P, "k": a.k, "D": a.D, "N": a.N, "lam": a.lam,
              "fused_ms": round(med(tf), 4), "fused_all_ms": [round(x, 4) for x in tf],
              "composed_ms": round(med(tc), 4), "composed_all_ms": [round(x, 4) for x in tc],
              "speedup": round(med(tc) / med(tf), 3),
              "fused_gather_tbps": round(gather_bytes / (med(tf) * 1e-3) / 1e12, 3),
              "fused_gram_tflops": round(2.0 * a.B * a.P * a.P * a.D / (med(tf) * 1e-3) / 1e12, 2),
              "topk_k_ms": round(med(tk), 4), "topk_k_all_ms": [round(x, 4) for x in tk],
              "topk_pool_plus_rerank_ms": round(med(tb), 4), "topk_pool_plus_rerank_all_ms": [round(x, 4) for x in tb],
              "topk_pool_ms": round(med(tp), 4), "topk_pool_all_ms": [round(x, 4) for x in tp],
              "default_pool": p_def, "topk_default_pool_plus_rerank_ms": round(med(td), 4),
              "topk_default_pool_plus_rerank_all_ms": [round(x, 4) for x in td],
              "fused_peak_extra_mb": round(peak_extra(fused) / 2 ** 20, 2),
              "composed_peak_extra_mb": round(peak_extra(comp) / 2 ** 20, 2),
              "lists_agree": round(agree, 6), "ild_max_abs_diff": ild_diff,
              "mean_ild_fused": float(fd.mean()), "device": torch.cuda.get_device_name(0)}]
    print(json.dumps(lines[0]), flush=True)
    if a.quality:
        for rec in quality((1.0, 0.7, 0.5), a.k, a.quality_limit, a.quality_cfg):
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
