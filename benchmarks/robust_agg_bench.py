"""Robust aggregation: the fused kernel (``ops.trimmed_mean``, csrc/robust_agg.hip) against the
library composition on the same device -- ``torch.sort(stack, dim=0)`` (sorted values + int64
indices, 3 W n 4 bytes written and read back), slice, mean -- at n = the flat trainable buffer
(1,165,312) and n = the ``sync=full`` set (67,528,192), W = 4, 8, 16, 32, trim = 1 and the median.

Device events around each call, warm-up first, the sides alternating within a round, median over
the rounds.  GB/s counts the needed bytes, (W + 1) n 4: every client's value read once, one float
written.  The composition ranks with torch's float order (it does not tell -0.0 from +0.0 and has no
client-index tie rule): it is what a user would write, not the contract; the inputs here have no
ties, so its values are compared with the kernel's as a sanity check.  One JSON line per shape.

    python benchmarks/robust_agg_bench.py [--n N ...] [--w W ...] [--out robust_agg_bench.jsonl]
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

N_FLAT, N_FULL = 1_165_312, 67_528_192  # FedRecConfig(): model.flat.flat / model.sync_tensors(True)


def composed(stack, trim):
    W = stack.shape[0]
    s, _ = torch.sort(stack, dim=0)
    return s[trim:W - trim].mean(0)


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
                                                  "profiles", "robust_agg_bench.jsonl"))
    a = ap.parse_args(argv)
    native.lib()
    dev = torch.device("cuda", 0)
    rows = []
    for n in a.n:
        iters = a.iters or (50 if n < (1 << 22) else 10)
        for W in a.w:
            g = torch.Generator(device=dev).manual_seed(W)
            stack = torch.randn(W, n, device=dev, generator=g)
            for name, trim in (("trim1", 1), ("median", (W - 1) // 2)):
                fused = lambda: ops.trimmed_mean(stack, trim)
                comp = lambda: composed(stack, trim)
                for _ in range(3):
                    fused(), comp()
                torch.cuda.synchronize()
                tf, tc = [], []
                for _ in range(iters):
                    tf.append(once(fused))
                    tc.append(once(comp))
                out, dropped = fused()
                ref = comp()
                need = (W + 1) * n * 4
                mf, mc = statistics.median(tf), statistics.median(tc)
                row = {"bench": "robust_agg", "n": n, "W": W, "rule": name, "trim": trim, "fused_ms": round(mf, 4),
                       "composed_ms": round(mc, 4), "speedup": round(mc / mf, 2),
                       "fused_GBps": round(need / mf / 1e6, 1), "composed_GBps": round(need / mc / 1e6, 1),
                       "max_abs_diff": float((out - ref).abs().max()), "dropped_sum_ok":
                       int(dropped.sum()) == 2 * trim * n, "iters": iters, "device": torch.cuda.get_device_name(0)}
                print(json.dumps(row), flush=True)
                rows.append(row)
                del out, ref
            del stack
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return rows


if __name__ == "__main__":
    main()
