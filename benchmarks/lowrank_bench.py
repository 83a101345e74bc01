"""Low-rank (PowerSGD) uploads: the kernels (``ops.lowrank_*``; csrc/lowrank_delta.hip) against the same method
composed from torch ops on the same device, on two layouts at rank R: the head layout (the flat trainable buffer,
1,165,312 coordinates: six matrices) and the unfrozen ``sync=full`` layout (the DistilBERT backbone's matrices as
well: word and position embeddings, six layers of four 768 x 768 and two 768 x 3072 matrices).

``compress`` (project + orth + backproject + residual, five launches) against what a user would write, per matrix::

    a = (l - g) + e;  P = a @ Q;  P, _ = qr(P);  Q = a.T @ P;  e = a - P @ Q.T

and ``combine`` at W clients against ``acc += w[c] * (P_c @ Q_c.T)`` per client and matrix, one division, one
addition.  (The composed form orthogonalises by Householder QR, the kernel by Gram-Schmidt: the same span.)

Device events around each call, warm-up first, the two sides alternating within a round, median over the rounds;
the residual is restored outside the timed window.  ``project`` and ``backproject`` are timed alone as well: GB/s
counts the bytes they need, the three inputs of every matrix coordinate (12 bytes).  One JSON line per case.

    python benchmarks/lowrank_bench.py [--rank R] [--w W] [--layout head full] [--out lowrank_bench.jsonl]
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

ALIGN = 64
HEAD = [(384, 768), (384,), (1, 384), (1,), (400, 768), (400,), (400, 400), (400,), (400, 400), (400,), (400, 400), (400,),
        (200, 400), (200,), (1, 200), (1,)]
LAYER = [(768, 768), (768,)] * 4 + [(768,), (768,), (3072, 768), (3072,), (768, 3072), (768,), (768,), (768,)]
FULL = [(30522, 768), (512, 768), (768,), (768,)] + LAYER * 6 + HEAD


def plan_of(shapes, R):
    layout, o = [], 0
    for s in shapes:
        layout.append((o, s))
        numel = 1
        for d in s:
            numel *= d
        o += -(-numel // ALIGN) * ALIGN
    return ref.LowRankPlan(layout, o, R)


def composed_compress(l, g, e, basis, plan):
    out = torch.zeros(plan.L, device=l.device)
    for m, (off, rows, cols, _) in enumerate(plan.mats):
        s = slice(off, off + rows * cols)
        a = ((l[s] - g[s]) + e[s]).view(rows, cols)
        P, Q = plan.factors(out, m)
        P.copy_(torch.linalg.qr(a @ plan.factors(basis, m)[1])[0])
        Q.copy_(a.t() @ P)
        e[s] = (a - P @ Q.t()).reshape(-1)
    for start, ln, pay in plan.rest:
        s = slice(start, start + ln)
        out[pay:pay + ln] = (l[s] - g[s]) + e[s]
        e[s] = 0
    return out


def composed_combine(base, stack, w, plan):
    out = base.clone()
    ws = w.sum()
    for m, (off, rows, cols, _) in enumerate(plan.mats):
        acc = torch.zeros(rows, cols, device=base.device)
        for c in range(stack.shape[0]):
            P, Q = plan.factors(stack[c], m)
            acc += w[c] * (P @ Q.t())
        out[off:off + rows * cols] += (acc / ws).reshape(-1)
    for start, ln, pay in plan.rest:
        out[start:start + ln] += (w[:, None] * stack[:, pay:pay + ln]).sum(0) / ws
    return out


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_pair(fused, comp, iters, reset=lambda: None):
    tf, tc = [], []
    for it in range(iters + 2):  # two warm-up rounds
        reset()
        torch.cuda.synchronize()
        t1, t2 = once(fused), once(comp)
        if it >= 2:
            tf.append(t1), tc.append(t2)
    return statistics.median(tf), statistics.median(tc)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--layout", nargs="*", default=["head", "full"])
    ap.add_argument("--rank", type=int, default=4)
    ap.add_argument("--w", type=int, default=8)
    ap.add_argument("--iters", type=int, default=0, help="rounds per case (0 = 30 on the head layout, else 8)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "lowrank_bench.jsonl"))
    a = ap.parse_args(argv)
    native.lib()
    dev = torch.device("cuda", 0)
    name = torch.cuda.get_device_name(0)
    rows, R, W = [], a.rank, a.w
    for lay in a.layout:
        plan = plan_of(HEAD if lay == "head" else FULL, R)
        n, iters = plan.n, a.iters or (30 if lay == "head" else 8)
        dense = sum(r * c for _, r, c, _ in plan.mats)
        gen = torch.Generator(device=dev).manual_seed(n)
        g = torch.randn(n, device=dev, generator=gen) * 0.05
        l = g + 1e-3 * torch.randn(n, device=dev, generator=gen)
        e0 = 1e-4 * torch.randn(n, device=dev, generator=gen)
        e1, e2 = e0.clone(), e0.clone()
        basis = plan.initial_basis(1).to(dev)
        reset = lambda: (e1.copy_(e0), e2.copy_(e0))  # noqa: E731
        mf, mc = median_pair(lambda: ops.lowrank_compress(l, g, e1, basis, plan),
                             lambda: composed_compress(l, g, e2, basis, plan), iters, reset)
        reset()
        p1, p2 = ops.lowrank_compress(l, g, e1, basis, plan), composed_compress(l, g, e2, basis, plan)
        target = (l - g) + e0
        zero = torch.zeros(n, device=dev)
        one = torch.ones(1, device=dev)
        err = [float(((ops.lowrank_combine(zero, p[None], one, plan) + e) - target).abs().max()) for p, e in ((p1, e1), (p2, e2))]
        left = [float(e.norm() / target.norm()) for e in (e1, e2)]
        row = {"bench": "compress", "layout": lay, "n": n, "matrices": len(plan.mats), "rank": R, "payload_floats": plan.L,
               "kernel_ms": round(mf, 4), "composed_ms": round(mc, 4), "speedup": round(mc / mf, 2),
               "kernel_feedback_err": err[0], "composed_feedback_err": err[1], "kernel_residual_share": round(left[0], 4),
               "composed_residual_share": round(left[1], 4), "iters": iters, "device": name}
        print(json.dumps(row), flush=True)
        rows.append(row)
        pay = torch.zeros(plan.L, device=dev)
        ops.lowrank_project(l, g, e0, basis, pay, plan)
        ops.lowrank_orth(pay, plan)
        stages = {"project": lambda: ops.lowrank_project(l, g, e0, basis, pay, plan), "orth": lambda: ops.lowrank_orth(pay, plan),
                  "backproject": lambda: ops.lowrank_backproject(l, g, e0, pay, plan),
                  "residual": lambda: ops.lowrank_residual(l, g, e1, pay, plan)}
        for stage, fn in stages.items():
            ts = [once(fn) for _ in range(iters + 2)][2:]
            ms = statistics.median(ts)
            row = {"bench": stage, "layout": lay, "n": n, "rank": R, "kernel_ms": round(ms, 4), "iters": iters, "device": name}
            if stage in ("project", "backproject"):
                row["kernel_GBps"] = round(12 * dense / ms / 1e6, 1)
            print(json.dumps(row), flush=True)
            rows.append(row)
        stack = torch.stack([p1] + [p1 * (1 + 0.1 * c) for c in range(1, W)])
        w = torch.rand(W, device=dev, generator=gen) + 0.5
        mf, mc = median_pair(lambda: ops.lowrank_combine(g, stack, w, plan), lambda: composed_combine(g, stack, w, plan), iters)
        o1, o2 = ops.lowrank_combine(g, stack, w, plan), composed_combine(g, stack, w, plan)
        row = {"bench": "combine", "layout": lay, "n": n, "rank": R, "W": W, "kernel_ms": round(mf, 4),
               "composed_ms": round(mc, 4), "speedup": round(mc / mf, 2), "kernel_GBps": round((4 * W * plan.L + 8 * n) / mf / 1e6, 1),
               "max_abs_diff": float((o1 - o2).abs().max()), "iters": iters, "device": name}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del g, l, e0, e1, e2, stack, pay, p1, p2, o1, o2, target, zero
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return rows


if __name__ == "__main__":
    main()
