"""Block-quantized uploads: the kernels (``ops.quantize_delta``, ``ops.dequant_combine``;
csrc/quant_delta.hip) against the same arithmetic composed from torch ops on the same device, at n = the
flat trainable buffer (1,165,312) and n = 64 M floats (an unfrozen backbone with ``sync=full``), both bit
widths, W = 2, 8, 32 clients.

``quantize_delta`` against what a user would write::

    a = (l - g) + e;  s = amax(|a| per 256) / Q;  x = a / s;  f = floor(x)
    q = clamp(f + (rand < x - f), -Q, Q);  e = a - q s;  codes = int8(q)  (or two nibbles a byte)

(``torch.rand_like`` is not the contract's Philox stream, so the codes differ where the draw does; the
row reports how far ``d + e`` is from ``a`` on both sides instead).  ``dequant_combine`` against W
decodes, ``acc += w[c] * (q * s)`` each, one division, one addition.

Device events around each call, warm-up first, the two sides alternating within a round, median over the
rounds; the residual is restored outside the timed window, so every call does the same work.  GB/s counts
the needed bytes: 12 n read and 4 n + n bits / 8 + n / 64 written for the quantizer, W (n bits / 8 + n /
64) + 4 n read and 4 n written for the combine.  One JSON line per case.

    python benchmarks/quantize_bench.py [--n N ...] [--w W ...] [--bits B ...] [--out quantize_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import native

N_FLAT, N_FULL = 1_165_312, 64 << 20
G = 256


def _per_coordinate(s, n):
    return s.repeat_interleave(G)[:n]


def composed_quantize(l, g, e, bits):
    Q = float((1 << (bits - 1)) - 1)
    n = l.numel()
    a = (l - g) + e
    amax = F.pad(a.abs(), (0, -n % G)).view(-1, G).amax(1)
    s = amax / torch.full_like(amax, Q)
    se = _per_coordinate(torch.where(s > 0, s, torch.ones_like(s)), n)
    x = a / se
    f = torch.floor(x)
    q = torch.clamp(f + (torch.rand_like(x) < x - f).float(), -Q, Q)
    e.copy_(a - q * se)
    qi = q.to(torch.int8)
    if bits == 8:
        return qi.view(torch.uint8), s
    nib = F.pad(qi, (0, n & 1)).view(torch.uint8) & 0xF
    return nib[0::2] | (nib[1::2] << 4), s


def composed_decode(codes, bits, n):
    if bits == 8:
        return codes.view(torch.int8).float()
    nib = torch.stack([codes & 0xF, codes >> 4], -1).reshape(-1)[:n].to(torch.int8)
    return ((nib ^ 8) - 8).float()


def composed_combine(base, codes, scales, w, bits):
    n = base.numel()
    acc = torch.zeros_like(base)
    for c in range(codes.shape[0]):
        acc += w[c] * (composed_decode(codes[c], bits, n) * _per_coordinate(scales[c], n))
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
    ap.add_argument("--w", type=int, nargs="*", default=[2, 8, 32])
    ap.add_argument("--bits", type=int, nargs="*", default=[8, 4])
    ap.add_argument("--iters", type=int, default=0, help="rounds per case (0 = 30 below 2^22 coordinates, else 6)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "quantize_bench.jsonl"))
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
        e0 = 1e-4 * torch.randn(n, device=dev, generator=gen)
        e1, e2 = e0.clone(), e0.clone()
        for bits in a.bits:
            fused = lambda: ops.quantize_delta(l, g, e1, bits, 1, 2)
            comp = lambda: composed_quantize(l, g, e2, bits)
            tf, tc = [], []
            for it in range(iters + 2):  # two warm-up rounds
                e1.copy_(e0), e2.copy_(e0)
                torch.cuda.synchronize()
                t1, t2 = once(fused), once(comp)
                if it >= 2:
                    tf.append(t1), tc.append(t2)
            e1.copy_(e0), e2.copy_(e0)
            (c1, s1), (c2, s2) = fused(), comp()
            target = (l - g) + e0
            err = [float(((ops.dequantize(c, s, bits, n) + e) - target).abs().max()) for c, s, e in ((c1, s1, e1), (c2, s2, e2))]
            mf, mc = statistics.median(tf), statistics.median(tc)
            need = 12 * n + 4 * n + n * bits // 8 + n // 64
            row = {"bench": "quantize_delta", "n": n, "bits": bits, "kernel_ms": round(mf, 4), "composed_ms": round(mc, 4),
                   "speedup": round(mc / mf, 2), "kernel_GBps": round(need / mf / 1e6, 1),
                   "same_scales": bool(torch.equal(s1, s2)), "kernel_feedback_err": err[0], "composed_feedback_err": err[1],
                   "iters": iters, "device": name}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del c1, s1, c2, s2, target
        del l, e0, e1, e2
        torch.cuda.empty_cache()
        for bits in a.bits:
            for W in a.w:
                nbytes, nb = (n * bits + 7) // 8, (n + G - 1) // G
                codes = torch.randint(0, 256, (W, nbytes), device=dev, generator=gen, dtype=torch.uint8)
                scales = 1e-5 * (torch.rand(W, nb, device=dev, generator=gen) + 0.5)
                w = torch.rand(W, device=dev, generator=gen) + 0.5
                fused = lambda: ops.dequant_combine(g, codes, scales, w, bits)
                comp = lambda: composed_combine(g, codes, scales, w, bits)
                tf, tc = [], []
                for it in range(iters + 2):
                    t1, t2 = once(fused), once(comp)
                    if it >= 2:
                        tf.append(t1), tc.append(t2)
                o1, o2 = fused(), comp()
                mf, mc = statistics.median(tf), statistics.median(tc)
                need = W * (n * bits // 8 + n // 64) + 8 * n
                row = {"bench": "dequant_combine", "n": n, "bits": bits, "W": W, "kernel_ms": round(mf, 4),
                       "composed_ms": round(mc, 4), "speedup": round(mc / mf, 2), "kernel_GBps": round(need / mf / 1e6, 1),
                       "max_abs_diff": float((o1 - o2).abs().max()), "iters": iters, "device": name}
                print(json.dumps(row), flush=True)
                rows.append(row)
                del codes, scales, o1, o2
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
