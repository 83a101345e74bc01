"""Elias-Fano coded index lists (``--upload_index=ef``; csrc/index_code.hip): what the coder costs and what it saves.

Time (needs the GPU): ``ops.ef_encode`` of one list and ``ops.ef_decode`` of W = 8 blobs at the flat trainable buffer
(n = 1,165,312, F = 0.01) and at n = 64 M with F in {0.001, 0.01, 0.1}, against the same arithmetic composed in torch on
the device: shifts, the cumsum of the high section's bits for the ranks, ``index_add_`` on integer tensors for the
scatters (bits of distinct fields are disjoint, so an integer add is the OR).  Device events around each call, warm-up
first, the two sides alternating within a round, median and interquartile range over the rounds.  ``GBps`` is the bytes
the call has to move -- the list and the words, each once -- over its time; ``hbm_floor_ms`` the same bytes at 6.3 TB/s.

Bytes (``--bytes``, host only, no GPU): the encoded size of one upload of each top-k form at the flat buffer, raw and
coded, against the dense ``4 n``.

    python benchmarks/index_bench.py [--bytes] [--out profiles/index_bench.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "benchmarks")]

import torch

from fedrec_with_pytorchdistributed_amd import ops
from fedrec_with_pytorchdistributed_amd.ops import reference as ref
from fedrec_with_pytorchdistributed_amd.parallel.sparsify import Sparsifier
from rotate_bench import N_FLAT, N_FULL, W
from sign_bench import alternate

HBM = 6.3e12  # bytes / s a float4 copy reaches on this part


def composed_encode(idx, n):
    """:func:`ops.reference.ef_encode` with scatters instead of bit matrices, on ``idx``'s device."""
    k, dev = idx.numel(), idx.device
    b, low_words, _, high_words = ref.ef_plan(n, k)
    i, r = idx.long(), torch.arange(k, device=dev)
    low = torch.zeros(low_words + 2, dtype=torch.int64, device=dev)  # (a field may run into the next word; b = 0: none)
    v = (i & ((1 << b) - 1)) << ((r * b) & 31)
    low.index_add_(0, (r * b) >> 5, v & 0xFFFFFFFF)
    low.index_add_(0, ((r * b) >> 5) + 1, v >> 32)
    high = torch.zeros(high_words, dtype=torch.int64, device=dev)
    pos = (i >> b) + r
    high.index_add_(0, pos >> 5, torch.ones((), dtype=torch.int64, device=dev) << (pos & 31))
    return ref._wrap_i32(torch.cat([low[:low_words], high]))


def composed_decode(words, n, k):
    """The device decoder's arithmetic in torch, fixed shapes and no synchronisation -> ``(idx [W, k], count [W])``."""
    dev = words.device
    b, low_words, _, high_words = ref.ef_plan(n, k)
    sh = torch.arange(32, device=dev)
    rows, counts = [], []
    for c in range(words.shape[0]):
        w = words[c].long() & 0xFFFFFFFF
        bits = ((w[low_words:, None] >> sh) & 1).reshape(-1)
        rank = torch.cumsum(bits, 0) - bits
        at = rank.clamp(max=k - 1) * b
        lw = torch.cat([w[:low_words], w.new_zeros(2)])
        low = (((lw[at >> 5] | (lw[(at >> 5) + 1] << 32)) >> (at & 31)) & ((1 << b) - 1)) if b else 0
        val = ((torch.arange(bits.numel(), device=dev) - rank) << b) | low
        out = torch.full((k + 1,), -1, dtype=torch.int64, device=dev)
        out.index_add_(0, torch.where((bits == 1) & (rank < k), rank, k), (val + 1) * bits)
        rows.append(out[:k].to(torch.int32))
        counts.append(bits.sum())
    return torch.stack(rows), torch.stack(counts)


def time_rows(cases, iters):
    from fedrec_with_pytorchdistributed_amd.ops import native
    native.lib()
    dev, rows = torch.device("cuda", 0), []
    for n, F in cases:
        k = Sparsifier(F).k_for(n)
        b, low_words, high_bits, high_words = ref.ef_plan(n, k)
        L = low_words + high_words
        it = iters or (30 if n < (1 << 22) else 12)
        gen = torch.Generator(device=dev).manual_seed(n + k)
        lists = [torch.randperm(n, device=dev, generator=gen)[:k].sort().values.int() for _ in range(W)]
        blobs = torch.stack([ops.ef_encode(x, n) for x in lists])
        for bench, fused, comp, need in (
                ("ef_encode", lambda: ops.ef_encode(lists[0], n), lambda: composed_encode(lists[0], n), 4 * k + 4 * L),
                ("ef_decode", lambda: ops.ef_decode(blobs, n, k), lambda: composed_decode(blobs, n, k), W * (4 * L + 4 * k))):
            (tf, sf), (tc, sc) = alternate((fused, comp), it)
            got, want = fused(), comp()
            if bench == "ef_encode":
                same = torch.equal(got, want)
            else:
                same = all(torch.equal(g, w) for g, w in zip(got, want)) and torch.equal(got[0], torch.stack(lists))
            rows.append({"bench": bench, "n": n, "F": F, "k": k, "b": b, "words": L, "bits_per_index": round(32 * L / k, 3),
                         "fused_ms": tf, "fused_iqr_ms": sf, "composed_ms": tc, "composed_iqr_ms": sc,
                         "fused_GBps": round(need / tf / 1e6, 1), "hbm_floor_ms": round(need / HBM * 1e3, 5),
                         "bitwise_same_as_composed": bool(same), "iters": it, **({"W": W} if bench == "ef_decode" else {})})
            print(json.dumps(rows[-1]), flush=True)
        del lists, blobs
        torch.cuda.empty_cache()
    name = torch.cuda.get_device_name(0)
    return [{**r, "device": name} for r in rows]


def byte_rows(n, fraction):
    """One upload of every top-k form at ``n`` coordinates, raw and coded: the encoded bytes against ``4 n``."""
    from fedrec_with_pytorchdistributed_amd.config import FedRecConfig
    from fedrec_with_pytorchdistributed_amd.parallel.control import encode_tensor
    from fedrec_with_pytorchdistributed_amd.parallel.upload import StarUpload
    gen, rows = torch.Generator().manual_seed(0), []
    theta = torch.randn(n, generator=gen) * 0.05
    local = theta + 1e-3 * torch.randn(n, generator=gen)
    for form in ([], ["--upload_bits=8"], ["--upload_bits=4"], ["--upload_sign=1"]):
        size = {}
        for index in ("raw", "ef"):
            cfg = FedRecConfig()
            cfg.apply_overrides([f"--upload_topk={fraction}", f"--upload_index={index}", *form])
            codec = StarUpload.from_cfg(cfg, "fedavg_star")
            if index == "ef":
                codec.plan_for(n)
            up = codec.compress(local, theta, torch.zeros(n), 0, 0)
            size[index] = len(encode_tensor(codec.pack(up)))
            k = up[0].numel()
        rows.append({"bench": "index_bytes", "form": " ".join(["--upload_topk", *form]), "n": n, "F": fraction, "k": k,
                     "raw_bytes": size["raw"], "ef_bytes": size["ef"], "raw_per_coordinate": round(size["raw"] / k, 3),
                     "ef_per_coordinate": round(size["ef"] / k, 3), "ef_over_raw": round(size["ef"] / size["raw"], 3),
                     "raw_over_dense": round(size["raw"] / (4 * n), 5), "ef_over_dense": round(size["ef"] / (4 * n), 5)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", action="store_true", help="the size table (host only, no GPU) instead of the timings")
    ap.add_argument("--iters", type=int, default=0, help="rounds per case (0 = 30 below 2^22 coordinates, else 12)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_bench.jsonl"))
    a = ap.parse_args(argv)
    if a.bytes:
        rows = byte_rows(N_FLAT, 0.01)
    else:
        rows = time_rows([(N_FLAT, 0.01), (N_FULL, 0.001), (N_FULL, 0.01), (N_FULL, 0.1)], a.iters)
    if a.out:  # one file for both tables: the rows of the other kind are kept
        keep = []
        if os.path.exists(a.out):
            with open(a.out) as f:
                keep = [r for r in map(json.loads, filter(str.strip, f)) if (r["bench"] == "index_bytes") != a.bytes]
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in keep + rows:
                f.write(json.dumps(r) + "\n")
    return rows


if __name__ == "__main__":
    main()
