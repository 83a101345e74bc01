"""Count-sketch (FetchSGD) uploads: the kernels (``ops.sketch_*``; csrc/sketch_delta.hip) against the same method
composed from torch ops on the same device, at the head's flat length (1,165,312 coordinates), ``R`` rows, the automatic
``C`` of ``F`` and ``W`` clients.

The composed side is what a user would write with the same hash tables (bucket and sign of every coordinate and row,
precomputed outside the timed window)::

    sketch    a = l - g;  S[r].index_add_(0, bucket[r], sign[r] * a)   per row (atomic adds: not deterministic)
    estimate  (sign * S.gather(1, bucket)).median(0).values
    combine   E += (w[:, None] * stack).sum(0) / w.sum();  est = estimate(E);  idx = est.abs().topk(k).indices;
              out = base.clone();  out[idx] += est[idx];  E[rows, bucket[:, idx]] = 0

against ``ops.sketch_delta``, ``ops.sketch_estimate`` and ``SketchUpload.combine`` (accumulate, estimate, the radix
select of ``ops.topk_delta``, clear, ``ops.sparse_combine``).  Device events around each call, warm-up first, the two
sides alternating within a round, median over the rounds; the error table is restored outside the timed window.  GB/s
counts the bytes a stage needs: ``8 n + 4 R C`` for the sketch, ``4 R C + 4 n`` for the estimate.  One JSON line per
case.

    python benchmarks/sketch_bench.py [--fraction F] [--rows R] [--w W] [--out sketch_bench.jsonl]
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
from fedrec_with_pytorchdistributed_amd.ops import reference as ref
from fedrec_with_pytorchdistributed_amd.parallel.sketch import SketchUpload

HEAD_N = 1165312


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_pair(fused, comp, iters, reset=lambda: None):
    tf, tc = [], []
    for it in range(iters + 3):  # three warm-up rounds
        reset()
        torch.cuda.synchronize()
        t1, t2 = once(fused), once(comp)
        if it >= 3:
            tf.append(t1), tc.append(t2)
    return statistics.median(tf), statistics.median(tc)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=HEAD_N)
    ap.add_argument("--fraction", type=float, default=0.01)
    ap.add_argument("--rows", type=int, default=5)
    ap.add_argument("--w", type=int, default=8)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "sketch_bench.jsonl"))
    a = ap.parse_args(argv)
    native.lib()
    dev = torch.device("cuda", 0)
    name = torch.cuda.get_device_name(0)
    n, R, W = a.n, a.rows, a.w
    sk = SketchUpload(a.fraction, R, 0, seed=1).plan_for(n, dev)
    C, k, plan = sk.cols, sk.k, sk._plan(dev)
    bucket, neg = (t.to(dev) for t in ref.sketch_hash(sk._plan("cpu"), torch.arange(n), R, C))
    sign = torch.where(neg, -1.0, 1.0)
    rows_ix = torch.arange(R, device=dev)[:, None]
    gen = torch.Generator(device=dev).manual_seed(n)
    g = torch.randn(n, device=dev, generator=gen) * 0.05
    l = g + 1e-3 * torch.randn(n, device=dev, generator=gen) ** 3
    common = {"n": n, "rows": R, "cols": C, "k": k, "iters": a.iters, "device": name}
    out = []

    def composed_sketch():
        d, S = l - g, torch.zeros(R, C, device=dev)
        for r in range(R):
            S[r].index_add_(0, bucket[r], sign[r] * d)
        return S

    def composed_estimate(S):
        return (sign * S.gather(1, bucket)).median(0).values

    mf, mc = median_pair(lambda: ops.sketch_delta(l, g, plan, R, C), composed_sketch, a.iters)
    S = ops.sketch_delta(l, g, plan, R, C)
    out.append({"bench": "sketch_delta", **common, "kernel_ms": round(mf, 4), "composed_ms": round(mc, 4),
                "speedup": round(mc / mf, 2), "kernel_GBps": round((8 * n + 4 * R * C) / mf / 1e6, 1),
                "max_abs_diff": float((S - composed_sketch()).abs().max())})
    print(json.dumps(out[-1]), flush=True)

    mf, mc = median_pair(lambda: ops.sketch_estimate(S, plan, n), lambda: composed_estimate(S), a.iters)
    out.append({"bench": "sketch_estimate", **common, "kernel_ms": round(mf, 4), "composed_ms": round(mc, 4),
                "speedup": round(mc / mf, 2), "kernel_GBps": round((4 * R * C + 4 * n) / mf / 1e6, 1),
                "max_abs_diff": float((ops.sketch_estimate(S, plan, n) - composed_estimate(S)).abs().max())})
    print(json.dumps(out[-1]), flush=True)

    ups = [S * (1 + 0.1 * c) for c in range(W)]
    stack = torch.stack([u.reshape(-1) for u in ups])
    w = torch.rand(W, device=dev, generator=gen) + 0.5
    E0 = 0.1 * S
    E2 = E0.clone()

    def composed_combine():
        E2.add_(((w[:, None] * stack).sum(0) / w.sum()).view(R, C))
        est = composed_estimate(E2)
        idx = est.abs().topk(k).indices
        new = g.clone()
        new[idx] += est[idx]
        E2[rows_ix, bucket[:, idx]] = 0
        return new

    reset = lambda: (sk.basis.copy_(E0), E2.copy_(E0))  # noqa: E731
    mf, mc = median_pair(lambda: sk.combine(g, ups, w), composed_combine, a.iters, reset)
    reset()
    o1, o2 = sk.combine(g, ups, w)[0], composed_combine()
    out.append({"bench": "combine", **common, "W": W, "kernel_ms": round(mf, 4), "composed_ms": round(mc, 4),
                "speedup": round(mc / mf, 2), "max_abs_diff": float((o1 - o2).abs().max()),
                "upload_bytes": 4 * R * C, "topk_upload_bytes": 8 * k, "dense_bytes": 4 * n})
    print(json.dumps(out[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")
    return out


if __name__ == "__main__":
    main()
