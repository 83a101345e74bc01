"""Sparsified uploads: the kernels (``ops.topk_delta``, ``ops.sparse_combine``; csrc/sparse_delta.hip)
against the library compositions on the same device, at n = the flat trainable buffer (1,165,312) and
n = 66 M (an unfrozen backbone with ``sync=full``), density F = 0.001, 0.01, 0.1, W = 8 clients.

``topk_delta`` against what a user would write::

    a = (l - g) + e;  i = topk(|a|, k).indices;  i = sort(i);  v = a[i];  e = a;  e[i] = 0

(torch.topk leaves the order among equal magnitudes open, so it is not the contract; the inputs here
are continuous draws, and ``same_idx`` reports whether it picked the kernel's set).  ``sparse_combine``
against W ``index_add_`` calls on a zero accumulator, one division, one addition.

Device events around each call, warm-up first, the two sides alternating within a round, median over
the rounds; the residual is restored outside the timed window, so every call does the same work.
GB/s counts the needed bytes: 16 n + 8 k for the select (three vectors read, one written, the lists),
8 n + 8 W k for the combine.  One JSON line per case.

    python benchmarks/sparsify_bench.py [--n N ...] [--f F ...] [--out sparsify_bench.jsonl]
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import native

N_FLAT, N_FULL = 1_165_312, 66_000_000


def composed_topk(l, g, e, k):
    a = (l - g) + e
    i = torch.topk(a.abs(), k, sorted=False).indices
    i = torch.sort(i).values
    v = a[i]
    e.copy_(a)
    e[i] = 0
    return i, v


def composed_combine(base, idx, val, w):
    acc = torch.zeros_like(base)
    for c in range(idx.shape[0]):
        acc.index_add_(0, idx[c], val[c] * w[c])
    return base + acc / w.sum()


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
    ap.add_argument("--f", type=float, nargs="*", default=[0.001, 0.01, 0.1])
    ap.add_argument("--w", type=int, default=8)
    ap.add_argument("--iters", type=int, default=0, help="rounds per case (0 = 30 below 2^22 coordinates, else 6)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "sparsify_bench.jsonl"))
    a = ap.parse_args(argv)
    native.lib()
    dev = torch.device("cuda", 0)
    name = torch.cuda.get_device_name(0)
    rows = []
    for n in a.n:
        iters = a.iters or (30 if n < (1 << 22) else 6)
        gen = torch.Generator(device=dev).manual_seed(n)
        g = torch.randn(n, device=dev, generator=gen) * 0.05
        l = g + 1e-3 * torch.randn(n, device=dev, generator=gen)   # a round's delta: a few exponents wide
        e0 = 1e-3 * torch.randn(n, device=dev, generator=gen)
        e1, e2 = e0.clone(), e0.clone()
        for F in a.f:
            k = max(1, math.ceil(F * n))
            fused = lambda: ops.topk_delta(l, g, e1, k)
            comp = lambda: composed_topk(l, g, e2, k)
            tf, tc = [], []
            for it in range(iters + 2):  # two warm-up rounds
                e1.copy_(e0), e2.copy_(e0)
                torch.cuda.synchronize()
                t1, t2 = once(fused), once(comp)
                if it >= 2:
                    tf.append(t1), tc.append(t2)
            e1.copy_(e0), e2.copy_(e0)
            (i1, v1), (i2, v2) = fused(), comp()
            mf, mc = statistics.median(tf), statistics.median(tc)
            need = 16 * n + 8 * k
            row = {"bench": "topk_delta", "n": n, "F": F, "k": k, "kernel_ms": round(mf, 4), "composed_ms": round(mc, 4),
                   "speedup": round(mc / mf, 2), "kernel_GBps": round(need / mf / 1e6, 1),
                   "same_idx": bool(torch.equal(i1.long(), i2)), "same_residual": bool(torch.equal(e1, e2)),
                   "iters": iters, "device": name}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del i1, v1, i2, v2
        del l, e0, e1, e2
        torch.cuda.empty_cache()
        W = a.w
        for F in a.f:
            k = max(1, math.ceil(F * n))
            idx = torch.stack([torch.sort(torch.randperm(n, device=dev, generator=gen)[:k]).values
                               for _ in range(W)]).to(torch.int32)
            val = 1e-3 * torch.randn(W, k, device=dev, generator=gen)
            w = torch.rand(W, device=dev, generator=gen) + 0.5
            fused = lambda: ops.sparse_combine(g, idx, val, w)
            comp = lambda: composed_combine(g, idx, val, w)
            tf, tc = [], []
            for it in range(iters + 2):
                t1, t2 = once(fused), once(comp)
                if it >= 2:
                    tf.append(t1), tc.append(t2)
            o1, o2 = fused(), comp()
            mf, mc = statistics.median(tf), statistics.median(tc)
            need = 8 * n + 8 * W * k
            row = {"bench": "sparse_combine", "n": n, "F": F, "k": k, "W": W, "kernel_ms": round(mf, 4),
                   "composed_ms": round(mc, 4), "speedup": round(mc / mf, 2), "kernel_GBps": round(need / mf / 1e6, 1),
                   "max_abs_diff": float((o1 - o2).abs().max()), "iters": iters, "device": name}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del idx, val, o1, o2
            torch.cuda.empty_cache()
        del g
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return rows


if __name__ == "__main__":
    main()
