"""The registered ``torch.ops.fedrec_sketch`` interface (csrc/bind_sketch.cpp): the four ops' full schemas and the
kind of kernel behind them, against ``tests/golden/op_schemas_sketch.txt``.  No GPU.

A deliberate interface change regenerates the fixture: ``python tests/test_op_schemas_sketch.py``."""
import os

import torch

from fedrec_with_pytorchdistributed_amd.ops import native

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "op_schemas_sketch.txt")


def _registered(prefix="fedrec_sketch::"):
    native.lib()
    out = {}
    for name in torch._C._dispatch_get_all_op_names():
        if not name.startswith(prefix):
            continue
        kinds = [k for k in ("CUDA", "CompositeImplicitAutograd", "CompositeExplicitAutograd")
                 if torch._C._dispatch_has_kernel_for_dispatch_key(name, k)]
        out[name] = f"{torch._C._get_schema(name, '')} | {'+'.join(kinds) or 'none'}"
    return out


def test_sketch_schemas_and_kernel_kinds_match_the_fixture():
    with open(GOLDEN) as f:
        assert [ln for _, ln in sorted(_registered().items())] == [ln.rstrip("\n") for ln in f if ln.strip()]


def test_the_four_ops_are_there_have_kernels_and_mark_what_they_write():
    got = _registered()
    assert sorted(got) == [f"fedrec_sketch::{op}" for op in ("accumulate_", "clear_", "delta", "estimate")]
    assert not [ln for ln in got.values() if ln.endswith("| none")]
    assert "Tensor(a!) table" in got["fedrec_sketch::accumulate_"] and "Tensor(a!) table" in got["fedrec_sketch::clear_"]
    assert "(a!)" not in got["fedrec_sketch::delta"] and "(a!)" not in got["fedrec_sketch::estimate"]


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        f.write("".join(ln + "\n" for _, ln in sorted(_registered().items())))
    print(f"wrote {len(_registered())} schemas to {GOLDEN}")
