"""1-bit scaled-sign uploads (``--upload_sign=1``; csrc/sign_delta.hip and the rotate_sign_* kernels of
csrc/rotate_delta.hip): what the coder costs and what one bit loses.

Time (needs the GPU): ``ops.sign_quantize``, ``ops.sign_combine``, ``ops.rotate_sign_quantize`` and
``ops.rotate_sign_combine`` (W = 8) at n = the flat trainable buffer (1,165,312) and n = 64 M floats, against (a) the
same arithmetic composed in torch on the device and (b) the 4-bit ``ops.quantize_delta`` / ``ops.dequant_combine`` (the
rotated forms: ``ops.rotate_quantize`` / ``ops.rotate_combine`` at 4 bits).  Device events around each call, warm-up
first, the three sides alternating within a round, median and interquartile range over the rounds; residuals are
restored outside the timed window.

Error (``--error``, host oracles only, no GPU): the relative L2 error ``||decode - v|| / ||v||`` of one upload with a zero
residual under the sign code, the rotated sign code, and the 4-bit and rotated 4-bit quantiser, on a Gaussian vector, a
heavy-tailed one (Student t, 2 degrees of freedom), an exactly two-valued one and the real ``delta + residual`` of
client 0 entering rounds 1 and 3 of a tiny two-client star on gloo.

    python benchmarks/sign_bench.py [--error] [--out profiles/sign_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "benchmarks")]

import torch

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import reference as ref
from rotate_bench import N_FLAT, N_FULL, SEED, W, composed_rotate, once, star_round_input


def composed_code(a, residual):
    """:func:`ops.reference.sign_quantize`'s coder in torch on ``a``'s device (whole blocks only)."""
    n, dev = a.numel(), a.device
    mag = a.abs().view(-1, 16, 16)
    p = torch.zeros(n // 256, 16, device=dev)
    for e in range(16):
        p = p + mag[:, :, e]
    j = torch.arange(16, device=dev)
    for o in (1, 2, 4, 8):
        p = p + p[:, j ^ o]
    p = p[:, 0]
    s = p / 256.0
    nonfinite = (p.view(torch.int32) & 0x7FFFFFFF) >= 0x7F800000
    live = ~nonfinite & (s >= 2.0 ** -126)
    zero = torch.zeros((), device=dev)
    scales = torch.where(nonfinite, torch.full((), float("nan"), device=dev), torch.where(live, s, zero))
    live_e = live.repeat_interleave(256)
    r = a - torch.copysign(s.repeat_interleave(256), a)
    residual.copy_(torch.where(live_e, r, torch.where(nonfinite.repeat_interleave(256), zero, a)))
    bit = ((a.view(torch.int32) < 0) & live_e).to(torch.int64).view(-1, 8)
    return (bit << torch.arange(8, device=dev)).sum(1).to(torch.uint8), scales


def composed_mean(codes, scales, w, m):
    acc, ws = torch.zeros(m, device=codes.device), torch.zeros((), device=codes.device)
    sh = torch.arange(8, device=codes.device)
    for c in range(codes.shape[0]):
        t = (w[c] * scales[c]).repeat_interleave(256)
        bit = ((codes[c].to(torch.int64)[:, None] >> sh) & 1).reshape(-1) == 1
        acc = acc + torch.where(bit, -t, t)
        ws = ws + w[c]
    return acc / ws


def alternate(fns, iters, reset=lambda: None):
    """(median, interquartile range) in ms of ``fns`` called in turn ``iters`` times after two warm-up rounds; the side
    that goes first behind the reset changes from round to round, so that no side always pays for the idle gap."""
    ts = [[] for _ in fns]
    for it in range(iters + 2):
        reset()
        torch.cuda.synchronize()
        for k in range(len(fns)):
            k = (k + it) % len(fns)
            ms = once(fns[k])
            if it >= 2:
                ts[k].append(ms)
    q = lambda t: statistics.quantiles(t, n=4)  # noqa: E731
    return [(round(statistics.median(t), 4), round(q(t)[2] - q(t)[0], 4)) for t in ts]


def time_rows(ns, iters):
    from fedrec_with_pytorchdistributed_amd.ops import native
    native.lib()
    dev, rows = torch.device("cuda", 0), []

    def row(bench, n, ts, need, **extra):
        (tf, sf), (tc, _), (t4, s4) = ts
        rows.append({"bench": bench, "n": n, "fused_ms": tf, "fused_iqr_ms": sf, "composed_ms": tc, "four_bit_ms": t4,
                     "four_bit_iqr_ms": s4, "fused_GBps": round(need / tf / 1e6, 1), **extra})
        print(json.dumps(rows[-1]), flush=True)

    for n in ns:  # (whole scale blocks; the flat buffer is not whole chunks: the rotated forms run over n_pad)
        assert n % 256 == 0
        n_pad = ref.rotate_pad(n)
        it = iters or (30 if n < (1 << 22) else 12)
        gen = torch.Generator(device=dev).manual_seed(n)
        g = torch.randn(n, device=dev, generator=gen) * 0.05
        l = g + 1e-3 * torch.randn(n, device=dev, generator=gen)
        d, zero = ref.rotate_signs(n_pad, SEED).to(dev), torch.zeros(n_pad, device=dev)
        e0 = 1e-4 * torch.randn(n_pad, device=dev, generator=gen)
        e = [e0.clone() for _ in range(3)]
        w = torch.rand(W, device=dev, generator=gen) + 0.5
        restore = lambda: [x.copy_(e0) for x in e]  # noqa: E731
        for rot in (False, True):
            if rot:
                fused = lambda: ops.rotate_sign_quantize(l, g, e[0], SEED)
                comp = lambda: composed_code(composed_rotate(l - g, d, False, n) + e[1], e[1])
                four = lambda: ops.rotate_quantize(l, g, e[2], 4, SEED, 2)
            else:
                fused = lambda: ops.sign_quantize(l, g, e[0][:n])
                comp = lambda: composed_code((l - g) + e[1][:n], e[1][:n])
                four = lambda: ops.quantize_delta(l, g, e[2][:n], 4, SEED, 2)
            ts = alternate((fused, comp, four), it, restore)
            restore()
            same = all(torch.equal(a, b) for a, b in zip(fused(), comp())) and torch.equal(e[0], e[1])
            m = n_pad if rot else n
            row("rotate_sign_quantize" if rot else "sign_quantize", n, ts, 8 * n + 8 * m + m // 8 + m // 64, iters=it,
                bitwise_same_as_composed=same)
            q1 = (lambda c: ops.rotate_sign_quantize(g + (c + 1) * (l - g), g, zero.clone(), SEED)) if rot else \
                 (lambda c: ops.sign_quantize(g + (c + 1) * (l - g), g, zero[:n].clone()))
            q4 = (lambda c: ops.rotate_quantize(g + (c + 1) * (l - g), g, zero.clone(), 4, SEED, c << 32)) if rot else \
                 (lambda c: ops.quantize_delta(g + (c + 1) * (l - g), g, zero[:n].clone(), 4, SEED, c << 32))
            codes, scales = (torch.stack(t) for t in zip(*[q1(c) for c in range(W)]))
            c4 = torch.stack([q4(c)[0] for c in range(W)])
            if rot:
                fused = lambda: ops.rotate_sign_combine(g, codes, scales, w, SEED)
                comp = lambda: g + composed_rotate(composed_mean(codes, scales, w, n_pad), d, True, n)
                four = lambda: ops.rotate_combine(g, c4, scales, w, 4, SEED)
            else:
                fused = lambda: ops.sign_combine(g, codes, scales, w)
                comp = lambda: g + composed_mean(codes, scales, w, n)
                four = lambda: ops.dequant_combine(g, c4, scales, w, 4)
            ts = alternate((fused, comp, four), it)
            row("rotate_sign_combine" if rot else "sign_combine", n, ts, W * (m // 8 + m // 64) + 8 * n, W=W, iters=it,
                max_abs_diff_to_composed=float((fused() - comp()).abs().max()))
            del codes, scales, c4
        del g, l, d, zero, e0, e
        torch.cuda.empty_cache()
    name = torch.cuda.get_device_name(0)
    return [{**r, "device": name} for r in rows]


def error_rows():
    gen = torch.Generator().manual_seed(0)
    n = N_FLAT
    t2 = torch.randn(n, generator=gen) / torch.sqrt((torch.randn(n, generator=gen) ** 2 + torch.randn(n, generator=gen) ** 2) / 2)
    inputs = {"gaussian": torch.randn(n, generator=gen), "student_t2": t2,
              "two_valued": 1e-4 * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0),
              "star_round1": star_round_input(1), "star_round3": star_round_input(3)}
    rows, one = [], torch.ones(1)
    for name, v in inputs.items():
        m, zero = v.numel(), torch.zeros(v.numel())
        m_pad = ref.rotate_pad(m)
        rel = lambda dec: float((dec - v).norm() / v.norm())  # noqa: E731
        row = {"bench": "sign_error", "input": name, "n": m, "max_over_rms": round(float(v.abs().max() / v.pow(2).mean().sqrt()), 2),
               "mean_abs_over_rms": round(float(v.abs().mean() / v.pow(2).mean().sqrt()), 4)}
        codes, scales = ref.sign_quantize(v, zero, torch.zeros(m))
        row["sign"] = rel(ref.sign_dequantize(codes, scales, m))
        codes, scales = ref.rotate_sign_quantize(v, zero, torch.zeros(m_pad), SEED)
        row["rotated_sign"] = rel(ref.rotate_sign_combine(zero, codes[None], scales[None], one, SEED))
        codes, scales = ref.quantize_delta(v, zero, torch.zeros(m), 4, SEED, 0)
        row["plain_4"] = rel(ref.dequantize(codes, scales, 4, m))
        codes, scales = ref.rotate_quantize(v, zero, torch.zeros(m_pad), 4, SEED, 0)
        row["rotated_4"] = rel(ref.rotate_combine(zero, codes[None], scales[None], one, 4, SEED))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--error", action="store_true", help="the error table (host oracles, no GPU) instead of the timings")
    ap.add_argument("--n", type=int, nargs="*", default=[N_FLAT, N_FULL])
    ap.add_argument("--iters", type=int, default=0, help="rounds per case (0 = 30 below 2^22 coordinates, else 12; a multiple of 3 keeps the order balanced)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sign_bench.jsonl"))
    a = ap.parse_args(argv)
    rows = error_rows() if a.error else time_rows(a.n, a.iters)
    if a.out:  # one file for both tables: the rows of the other kind are kept
        keep = []
        if os.path.exists(a.out):
            with open(a.out) as f:
                keep = [r for r in map(json.loads, filter(str.strip, f)) if (r["bench"] == "sign_error") != a.error]
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in keep + rows:
                f.write(json.dumps(r) + "\n")
    return rows


if __name__ == "__main__":
    main()
