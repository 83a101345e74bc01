"""Client-level DP on a round delta: the two fused ops (``ops.dp_delta_sqnorm`` -> ``ops.dp_clip_noise``,
csrc/dp_clip.hip: three launches) against the same rule composed in torch on the same device -- ``sub, norm, mul,
add, randn, mul, add`` -- at n = the flat trainable buffer (1,165,312: 4.66 MB) and n = the ``sync=full`` set of an
unfrozen model (67,528,192), clipped to half the delta's norm, with and without noise.

Device events around each call, warm-up first, the sides alternating within a round, median over the rounds.
``sqnorm_ms`` and ``clip_noise_ms`` are the two ops alone.  Bytes moved: the fused pair reads ``local`` and ``base``
twice and writes ``out`` once, 20 n; GB/s is that over the fused time, and 8 n / 12 n over the two ops' own.  One
JSON line per shape.

    python benchmarks/dp_clip_bench.py [--n N ...] [--out dp_clip_bench.jsonl]
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
from fedrec_with_pytorchdistributed_amd.ops.reference import dp_state_fields

N_FLAT, N_FULL = 1_165_312, 67_528_192  # FedRecConfig(): model.flat.flat / model.sync_tensors(True)


def fused(local, base, clip, std):
    return ops.dp_clip_noise(local, base, ops.dp_delta_sqnorm(local, base), clip, std, 11, 3)


def composed(local, base, clip, std):
    d = local - base
    out = base + d * (clip / d.norm()).clamp(max=1.0)
    return out + std * torch.randn_like(out) if std > 0 else out


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
    ap.add_argument("--iters", type=int, default=0, help="rounds per shape (0 = 50 below 2^22 coordinates, else 10)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "dp_clip_bench.jsonl"))
    a = ap.parse_args(argv)
    native.lib()
    dev = torch.device("cuda", 0)
    rows = []
    for n in a.n:
        iters = a.iters or (50 if n < (1 << 22) else 10)
        g = torch.Generator(device=dev).manual_seed(n)
        base = torch.randn(n, device=dev, generator=g)
        local = base + 1e-2 * torch.randn(n, device=dev, generator=g)
        state = ops.dp_delta_sqnorm(local, base)
        clip = 0.5 * dp_state_fields(state)[0] ** 0.5
        for std in (0.0, 1e-3):
            sides = {"fused": lambda: fused(local, base, clip, std), "composed": lambda: composed(local, base, clip, std),
                     "sqnorm": lambda: ops.dp_delta_sqnorm(local, base),
                     "clip_noise": lambda: ops.dp_clip_noise(local, base, state, clip, std, 11, 3)}
            for _ in range(3):
                for fn in sides.values():
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in sides}
            for _ in range(iters):
                for k, fn in sides.items():
                    t[k].append(once(fn))
            med = {k: statistics.median(v) for k, v in t.items()}
            out, want = sides["fused"](), sides["composed"]()
            row = {"bench": "dp_clip", "n": n, "std": std, "fused_ms": round(med["fused"], 4),
                   "composed_ms": round(med["composed"], 4), "speedup": round(med["composed"] / med["fused"], 2),
                   "sqnorm_ms": round(med["sqnorm"], 4), "clip_noise_ms": round(med["clip_noise"], 4),
                   "fused_bytes": 20 * n, "fused_GBps": round(20 * n / med["fused"] / 1e6, 1),
                   "sqnorm_GBps": round(8 * n / med["sqnorm"] / 1e6, 1),
                   "clip_noise_GBps": round(12 * n / med["clip_noise"] / 1e6, 1),
                   "norm_after": float((out - base).double().norm()), "clip": clip,
                   "max_abs_diff_no_noise": float((out - want).abs().max()) if std == 0 else None,
                   "iters": iters, "device": torch.cuda.get_device_name(0)}
            print(json.dumps(row), flush=True)
            rows.append(row)
        del base, local
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")
    return rows


if __name__ == "__main__":
    main()
