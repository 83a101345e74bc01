"""Rotated quantised uploads (``--upload_rotate=1``; csrc/rotate_delta.hip): what the rotation costs and what it buys.

Time (needs the GPU): ``ops.rotate_quantize`` and ``ops.rotate_combine`` (W = 8) at n = the flat trainable buffer
(1,165,312) and n = 64 M floats (an unfrozen backbone with ``sync=full``), both bit widths, against (a) the same
arithmetic composed on the device from twelve reshaped torch passes and the existing ``ops.quantize_delta`` /
``ops.dequant_combine`` kernels and (b) those unrotated kernels alone.  Device events around each call, warm-up first,
the three sides alternating within a round, median over the rounds; residuals are restored outside the timed window.

Error (``--error``, host oracles only, no GPU): the relative L2 error ``||decode - v|| / ||v||`` of one upload at 8 and 4
bits with and without rotation on a Gaussian vector, a heavy-tailed one (Student t, 2 degrees of freedom) and the real
``delta + residual`` of client 0 in rounds 1 and 3 of a tiny two-client star on gloo with ``--upload_bits=4``.

    python benchmarks/rotate_bench.py [--error] [--out profiles/rotate_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import reference as ref

N_FLAT, N_FULL, W, SEED = 1_165_312, 64 << 20, 8, 1
TINY = ["--data_dir=synthetic:tiny", "--backbone.name=tiny", "--round_timeout_s=120", "--collective_timeout_s=120"]


def composed_rotate(x, d, inverse, n):
    """:func:`ops.reference.rotate` with the signs ``d`` precomputed on the device."""
    t = torch.nn.functional.pad(x, (0, d.numel() - x.numel()))
    if not inverse:
        t = d * t
    for s in range(12):
        v = t.view(-1, 2, 1 << s)
        t = torch.stack([v[:, 0] + v[:, 1], v[:, 0] - v[:, 1]], 1).reshape(-1)
    t = t * 2.0 ** -6
    return (d * t)[:n] if inverse else t


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fns, iters, reset=lambda: None):
    """Medians (ms) of ``fns`` called in turn ``iters`` times after two warm-up rounds."""
    ts = [[] for _ in fns]
    for it in range(iters + 2):
        reset()
        torch.cuda.synchronize()
        for t, fn in zip(ts, fns):
            ms = once(fn)
            if it >= 2:
                t.append(ms)
    return [round(statistics.median(t), 4) for t in ts]


def time_rows(ns, iters):
    from fedrec_with_pytorchdistributed_amd.ops import native
    native.lib()
    dev, rows = torch.device("cuda", 0), []
    for n in ns:
        it = iters or (30 if n < (1 << 22) else 6)
        n_pad = ref.rotate_pad(n)
        gen = torch.Generator(device=dev).manual_seed(n)
        g = torch.randn(n, device=dev, generator=gen) * 0.05
        l = g + 1e-3 * torch.randn(n, device=dev, generator=gen)
        d, zero = ref.rotate_signs(n_pad, SEED).to(dev), torch.zeros(n_pad, device=dev)
        e0 = 1e-4 * torch.randn(n_pad, device=dev, generator=gen)
        e = [e0.clone() for _ in range(3)]
        w = torch.rand(W, device=dev, generator=gen) + 0.5
        for bits in (8, 4):
            fused = lambda: ops.rotate_quantize(l, g, e[0], bits, SEED, 2)
            comp = lambda: ops.quantize_delta(composed_rotate(l - g, d, False, n), zero, e[1], bits, SEED, 2)
            plain = lambda: ops.quantize_delta(l, g, e[2][:n], bits, SEED, 2)
            tf, tc, tp = alternate((fused, comp, plain), it, lambda: [x.copy_(e0) for x in e])
            [x.copy_(e0) for x in e]
            same = all(torch.equal(a, b) for a, b in zip(fused(), comp())) and torch.equal(e[0], e[1])
            need = 8 * n + 8 * n_pad + n_pad * bits // 8 + n_pad // 64
            rows.append({"bench": "rotate_quantize", "n": n, "bits": bits, "fused_ms": tf, "composed_ms": tc, "unrotated_ms": tp,
                         "fused_GBps": round(need / tf / 1e6, 1), "bitwise_same_as_composed": same, "iters": it})
            print(json.dumps(rows[-1]), flush=True)
            codes = torch.stack([ops.rotate_quantize(g + (c + 1) * (l - g), g, zero.clone(), bits, SEED, c << 32)[0] for c in range(W)])
            scales = 1e-5 * (torch.rand(W, n_pad // 256, device=dev, generator=gen) + 0.5)
            nbp, nbs = (n * bits + 7) // 8, (n + 255) // 256
            cp, sp = codes[:, :nbp].contiguous(), scales[:, :nbs].contiguous()
            fused = lambda: ops.rotate_combine(g, codes, scales, w, bits, SEED)
            comp = lambda: g + composed_rotate(ops.dequant_combine(zero, codes, scales, w, bits), d, True, n)
            plain = lambda: ops.dequant_combine(g, cp, sp, w, bits)
            tf, tc, tp = alternate((fused, comp, plain), it)
            need = W * (n_pad * bits // 8 + n_pad // 64) + 8 * n
            rows.append({"bench": "rotate_combine", "n": n, "bits": bits, "W": W, "fused_ms": tf, "composed_ms": tc,
                         "unrotated_ms": tp, "fused_GBps": round(need / tf / 1e6, 1),
                         "max_abs_diff_to_composed": float((fused() - comp()).abs().max()), "iters": it})
            print(json.dumps(rows[-1]), flush=True)
            del codes, scales, cp, sp
        del g, l, d, zero, e0, e
        torch.cuda.empty_cache()
    name = torch.cuda.get_device_name(0)
    return [{**r, "device": name} for r in rows]


def star_round_input(r):
    """``(local - theta_g) + residual`` of client 0 entering round ``r`` of a tiny star with ``--upload_bits=4``: two runs
    from scratch (they repeat bit for bit), ``r`` rounds for the residual and the global model, ``r + 1`` for the dump."""
    from launch_util import run_ranks

    def run(d, rounds):
        flags = [*TINY, "--upload_bits=4", f"--snapshot_path={d}/s.pt"]
        outs = run_ranks([["server.py", str(rounds), *flags]] + [["client.py", "1", "16", "1", "0", "c", *flags]] * 2,
                         {"FEDREC_DUMP_FLAT": str(d / "dump"), "FEDREC_STAR_AGG": "upload"}, timeout=300)
        assert all(rc == 0 for rc, _ in outs), outs[0][1][-2000:]

    from fedrec_with_pytorchdistributed_amd.config import FedRecConfig
    from fedrec_with_pytorchdistributed_amd.train.federated import build_model
    cfg = FedRecConfig()
    cfg.apply_overrides(list(TINY))
    flat = build_model(cfg, torch.device("cpu")).flat
    with tempfile.TemporaryDirectory() as tmp:
        a, b = Path(tmp) / "a", Path(tmp) / "b"
        run(a, r), run(b, r + 1)
        g = torch.load(a / f"global_model_round{r - 1}.pt", weights_only=True)
        theta = flat.flat.detach().float().clone()  # (the alignment gaps between parameters never train)
        for name, p, off in flat.views():
            theta[off:off + p.numel()] = g[name].reshape(-1).float()
        residual = torch.load(a / "client0_s.pt", weights_only=True)["UPLOAD_RESIDUAL"]
        local = torch.load(b / "dump" / "rank1.pt").float()
    return (local - theta) + residual


def error_rows():
    gen = torch.Generator().manual_seed(0)
    n = N_FLAT
    t2 = torch.randn(n, generator=gen) / torch.sqrt((torch.randn(n, generator=gen) ** 2 + torch.randn(n, generator=gen) ** 2) / 2)
    inputs = {"gaussian": torch.randn(n, generator=gen), "student_t2": t2,
              "star_round1": star_round_input(1), "star_round3": star_round_input(3)}
    rows = []
    for name, v in inputs.items():
        m, zero = v.numel(), torch.zeros(v.numel())
        row = {"bench": "rotate_error", "input": name, "n": m, "max_over_rms": round(float(v.abs().max() / v.pow(2).mean().sqrt()), 2)}
        for bits in (8, 4):
            codes, scales = ref.quantize_delta(v, zero, torch.zeros(m), bits, SEED, 0)
            row[f"plain_{bits}"] = float((ref.dequantize(codes, scales, bits, m) - v).norm() / v.norm())
            codes, scales = ref.rotate_quantize(v, zero, torch.zeros(ref.rotate_pad(m)), bits, SEED, 0)
            dec = ref.rotate_combine(zero, codes[None], scales[None], torch.ones(1), bits, SEED)
            row[f"rotated_{bits}"] = float((dec - v).norm() / v.norm())
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--error", action="store_true", help="the error table (host oracles, no GPU) instead of the timings")
    ap.add_argument("--n", type=int, nargs="*", default=[N_FLAT, N_FULL])
    ap.add_argument("--iters", type=int, default=0, help="rounds per case (0 = 30 below 2^22 coordinates, else 6)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rotate_bench.jsonl"))
    a = ap.parse_args(argv)
    rows = error_rows() if a.error else time_rows(a.n, a.iters)
    if a.out:  # one file for both tables: the rows of the other kind are kept
        keep = []
        if os.path.exists(a.out):
            with open(a.out) as f:
                keep = [r for r in map(json.loads, filter(str.strip, f)) if (r["bench"] == "rotate_error") != a.error]
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in keep + rows:
                f.write(json.dumps(r) + "\n")
    return rows


if __name__ == "__main__":
    main()
