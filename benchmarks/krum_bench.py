"""Multi-Krum: the fused path (``ops.trimmed_mean`` median -> ``ops.krum_gram`` -> ``ops.krum_select`` ->
``ops.krum_mean``, csrc/krum.hip) against the library composition on the same device -- median, ``Y =
stack - median`` (a second ``[W, n]`` tensor), ``Y @ Y.T``, the select contract in torch, ``index_select
+ mean`` -- at n = the flat trainable buffer (1,165,312) and n = the ``sync=full`` set (67,528,192), W = 4,
8, 16, 32, f = (W - 3) // 2 (that many clients send -50 x their model), m = W - f.

Device events around each call, warm-up first, the sides alternating within a round, median over the
rounds.  GB/s counts the STACK bytes, W n 4, over the whole rule and over ``centered_gram`` alone (both
sides start from the same median kernel; the composition's select syncs the host once for its index
list, as a user's code would).  ``trimmed_mean_GBps`` is the existing single-read streaming kernel on
the same stack (its median), counted the same way.  One JSON line per shape.

    python benchmarks/krum_bench.py [--n N ...] [--w W ...] [--out krum_bench.jsonl]
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

N_FLAT, N_FULL = 1_165_312, 67_528_192  # FedRecConfig(): model.flat.flat / model.sync_tensors(True)


def fused(stack, f, m):
    center, _ = ops.trimmed_mean(stack, (stack.shape[0] - 1) // 2)
    sel, _ = ops.krum_select(ops.krum_gram(stack, center), f, m)
    return ops.krum_mean(stack, sel), sel


def composed(stack, f, m):
    center, _ = ops.trimmed_mean(stack, (stack.shape[0] - 1) // 2)
    y = stack - center
    sel, _ = ref.krum_select((y @ y.t()).double().cpu(), f, m)
    rows = torch.nonzero(sel).reshape(-1).to(stack.device)
    return stack.index_select(0, rows).mean(0), sel


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[N_FLAT, N_FULL])
    ap.add_argument("--w", type=int, nargs="*", default=[4, 8, 16, 32])
    ap.add_argument("--iters", type=int, default=0, help="rounds per shape (0 = 50 below 2^22 coordinates, else 10)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "krum_bench.jsonl"))
    a = ap.parse_args(argv)
    native.lib()
    dev = torch.device("cuda", 0)
    rows = []
    for n in a.n:
        iters = a.iters or (50 if n < (1 << 22) else 10)
        for W in a.w:
            g = torch.Generator(device=dev).manual_seed(W)
            f = (W - 3) // 2
            m = W - f
            stack = torch.randn(n, device=dev, generator=g) + 1e-3 * torch.randn(W, n, device=dev, generator=g)
            stack[m:] *= -50.0  # the last f clients are Byzantine: the selection has a clear boundary
            center, _ = ops.trimmed_mean(stack, (W - 1) // 2)
            sides = {"fused": lambda: fused(stack, f, m), "composed": lambda: composed(stack, f, m),
                     "gram": lambda: ops.krum_gram(stack, center),
                     "trimmed_mean": lambda: ops.trimmed_mean(stack, (W - 1) // 2)}
            for _ in range(3):
                for fn in sides.values():
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in sides}
            for _ in range(iters):
                for k, fn in sides.items():
                    t[k].append(once(fn))
            (out, sel), (want, wsel) = sides["fused"](), sides["composed"]()
            med = {k: statistics.median(v) for k, v in t.items()}
            need = W * n * 4
            row = {"bench": "krum", "n": n, "W": W, "f": f, "m": m, "fused_ms": round(med["fused"], 4),
                   "composed_ms": round(med["composed"], 4), "speedup": round(med["composed"] / med["fused"], 2),
                   "gram_ms": round(med["gram"], 4), "trimmed_mean_ms": round(med["trimmed_mean"], 4),
                   "fused_GBps": round(need / med["fused"] / 1e6, 1), "composed_GBps": round(need / med["composed"] / 1e6, 1),
                   "gram_GBps": round(need / med["gram"] / 1e6, 1),
                   "trimmed_mean_GBps": round(need / med["trimmed_mean"] / 1e6, 1),
                   "same_selection": sel.cpu().tolist() == wsel.tolist(), "max_abs_diff": float((out - want).abs().max()),
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
