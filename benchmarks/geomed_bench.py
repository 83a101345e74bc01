"""Geometric median (RFA): the fused rule (``ops.trimmed_mean`` median -> ``ops.krum_gram`` -> ``ops.geomed_weights``
-> ``ops.geomed_combine``, csrc/krum.hip + csrc/geomed.hip) against Weiszfeld composed in torch on the same device --
32 rounds of ``stack - z``, row norms, weighted mean, each round a pass over the ``[W, n]`` stack -- at n = the flat
trainable buffer (1,165,312: 4.66 MB per client) and n = one 28 MB bucket (7,340,032), W = 4, 8, 32; the last client
sends 1000 x its model.

Device events around each call, warm-up first, the sides alternating within a round, median over the rounds.  GB/s
counts the STACK bytes, W n 4, over the whole rule.  ``weights_ms`` and ``combine_ms`` are the two new kernels alone
(event times of one launch each: at these sizes the weights kernel's time includes the launch).  One JSON line per
shape.

    python benchmarks/geomed_bench.py [--n N ...] [--w W ...] [--out geomed_bench.jsonl]
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
from fedrec_with_pytorchdistributed_amd.ops.reference import GM_ITERS

N_FLAT, N_BUCKET = 1_165_312, (28 << 20) // 4  # FedRecConfig(): model.flat.flat / comm.BUCKET_BYTES of fp32


def fused(stack):
    center, _ = ops.trimmed_mean(stack, (stack.shape[0] - 1) // 2)
    a, _ = ops.geomed_weights(ops.krum_gram(stack, center))
    return ops.geomed_combine(stack, a), a


def composed(stack):
    z = stack.mean(0)
    for _ in range(GM_ITERS):
        w = 1.0 / (stack - z).norm(dim=1).clamp_min(1e-30)
        w = w / w.sum()
        z = (w[:, None] * stack).sum(0)
    return z, w


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[N_FLAT, N_BUCKET])
    ap.add_argument("--w", type=int, nargs="*", default=[4, 8, 32])
    ap.add_argument("--iters", type=int, default=0, help="rounds per shape (0 = 50 below 2^22 coordinates, else 10)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "geomed_bench.jsonl"))
    a = ap.parse_args(argv)
    native.lib()
    dev = torch.device("cuda", 0)
    rows = []
    for n in a.n:
        iters = a.iters or (50 if n < (1 << 22) else 10)
        for W in a.w:
            g = torch.Generator(device=dev).manual_seed(W)
            stack = torch.randn(n, device=dev, generator=g) + 1e-3 * torch.randn(W, n, device=dev, generator=g)
            stack[W - 1] *= 1000.0
            center, _ = ops.trimmed_mean(stack, (W - 1) // 2)
            G = ops.krum_gram(stack, center)
            wts, _ = ops.geomed_weights(G)
            sides = {"fused": lambda: fused(stack), "composed": lambda: composed(stack),
                     "weights": lambda: ops.geomed_weights(G), "combine": lambda: ops.geomed_combine(stack, wts)}
            for _ in range(3):
                for fn in sides.values():
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in sides}
            for _ in range(iters):
                for k, fn in sides.items():
                    t[k].append(once(fn))
            (out, aw), (want, ww) = sides["fused"](), sides["composed"]()
            med = {k: statistics.median(v) for k, v in t.items()}
            need = W * n * 4
            row = {"bench": "geomed", "n": n, "W": W, "fused_ms": round(med["fused"], 4),
                   "composed_ms": round(med["composed"], 4), "speedup": round(med["composed"] / med["fused"], 2),
                   "weights_ms": round(med["weights"], 4), "combine_ms": round(med["combine"], 4),
                   "fused_GBps": round(need / med["fused"] / 1e6, 1), "composed_GBps": round(need / med["composed"] / 1e6, 1),
                   "combine_GBps": round((need + 4 * n) / med["combine"] / 1e6, 1),
                   "max_weight_diff": float((aw.float() - ww).abs().max()), "max_abs_diff": float((out - want).abs().max()),
                   "iters": iters, "device": torch.cuda.get_device_name(0)}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del stack, center, out, want, sides
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")
    return rows


if __name__ == "__main__":
    main()
