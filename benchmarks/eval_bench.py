"""Full-impression ranking: the fused kernel (``ops.rank_impressions``, csrc/rank_impressions.hip)
against the library composition on the same device -- ``table.index_select(0, negs)``, a row-dot
with the repeated user rows and a segment compare, which writes and re-reads ``[M, D]`` fp32
tensors -- at a mind-small-like corpus: N = 65,000 news, D = 400, 73,000 impressions in one call,
Poisson(37) negatives clipped to [1, 300] (``even``), and the same with 1 % of the lists at 2,000
negatives (``skewed``).

Operands are integer-valued floats in [-4, 4]: every product and sum is exact in fp32 whatever
the order, so the two sides must agree bit for bit (``torch.equal`` on the counts, checked before
any timing); neither side's time depends on the values.  The composition is handed its int64
index tensors and the candidate -> impression map ready-made (building them is not timed).

Device events around each call, warm-up first, the two sides alternating within a round, median
over the rounds' medians; peak extra device memory of one call of each side.  ``fused_tb_s`` is
the bytes the algorithm needs -- per impression its user row, its positive's row and one table row
per negative, plus the ids and the pointers -- over the fused CALL time (three launches and the
output / workspace allocation, not kernel time).  One JSON line per shape.

    python benchmarks/eval_bench.py [--out profiles/eval_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import native


def composed(u, t, pos_l, negs_l, seg, lens):
    B = u.shape[0]
    V = t.index_select(0, negs_l)                                   # [M, D]
    s = (u.index_select(0, seg) * V).sum(1)                         # the row-dot with the repeated user rows
    p = (u * t.index_select(0, pos_l)).sum(1)
    pm = p.index_select(0, seg)
    z = lambda: torch.zeros(B, dtype=torch.int32, device=u.device)
    gt = z().index_add_(0, seg, (s > pm).to(torch.int32))
    eq = z().index_add_(0, seg, (s == pm).to(torch.int32))
    nan = z().index_add_(0, seg, torch.isnan(s).to(torch.int32)) + torch.isnan(p).to(torch.int32)
    return torch.stack([gt, eq, lens, nan], 1)


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


def list_lengths(I, skewed, rng):
    lens = np.clip(rng.poisson(37, I), 1, 300)
    if skewed:
        lens[rng.permutation(I)[:I // 100]] = 2000
    return lens.astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=65000)
    ap.add_argument("--D", type=int, default=400)
    ap.add_argument("--I", type=int, default=73000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs a HIP device")
    native.lib()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    ints = lambda *s: torch.from_numpy(rng.integers(-4, 5, s).astype(np.float32)).to(dev)
    t, u = ints(a.N, a.D), ints(a.I, a.D)
    pos = torch.from_numpy(rng.integers(0, a.N, a.I).astype(np.int32)).to(dev)
    lines = []
    for shape in ("even", "skewed"):
        lens = list_lengths(a.I, shape == "skewed", rng)
        M = int(lens.sum())
        ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)])).to(dev)
        negs = torch.from_numpy(rng.integers(0, a.N, M).astype(np.int32)).to(dev)
        lens_d = torch.from_numpy(lens.astype(np.int32)).to(dev)
        seg = torch.repeat_interleave(torch.arange(a.I, device=dev), torch.from_numpy(lens).to(dev))
        pos_l, negs_l = pos.long(), negs.long()
        fused = lambda: ops.rank_impressions(u, t, pos, ptr, negs, 0)
        comp = lambda: composed(u, t, pos_l, negs_l, seg, lens_d)
        cf, cc = fused(), comp()
        if not torch.equal(cf, cc):
            raise SystemExit(f"{shape}: the fused and composed counts differ in "
                             f"{int((cf != cc).any(1).sum())} impressions")
        del cf, cc
        tf, tc = [], []
        for _ in range(a.rounds):
            tf.append(timeit(fused, a.iters, a.warmup))
            tc.append(timeit(comp, a.iters, a.warmup))
        mf, mc = statistics.median(tf), statistics.median(tc)
        nbytes = (M + 2 * a.I) * a.D * 4 + (M + a.I) * 4 + (a.I + 1) * 8 + a.I * 16
        rec = {"bench": "eval", "shape": shape, "I": a.I, "N": a.N, "D": a.D, "candidates": M,
               "max_list": int(lens.max()), "median_list": int(np.median(lens)),
               "fused_ms": round(mf, 4), "fused_all_ms": [round(x, 4) for x in tf],
               "composed_ms": round(mc, 4), "composed_all_ms": [round(x, 4) for x in tc],
               "speedup": round(mc / mf, 3), "fused_ns_per_candidate": round(mf * 1e6 / M, 4),
               "bytes_per_impression": round(nbytes / a.I, 1), "fused_tb_s": round(nbytes / (mf * 1e-3) / 1e12, 3),
               "fused_peak_extra_mb": round(peak_extra(fused) / 2 ** 20, 2),
               "composed_peak_extra_mb": round(peak_extra(comp) / 2 ** 20, 2),
               "counts_equal": True, "device": torch.cuda.get_device_name(0)}
        if lines:  # the skewed shape's time per candidate over the even shape's
            rec["ns_per_candidate_vs_even"] = round(rec["fused_ns_per_candidate"] / lines[0]["fused_ns_per_candidate"], 3)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del ptr, negs, seg, negs_l, lens_d
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
