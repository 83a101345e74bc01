"""The registered ``torch.ops.fedrec_quant`` interface (csrc/bind_quant.cpp): both ops' full schemas and
the kind of kernel behind them, against ``tests/golden/op_schemas_quant.txt``; the ``fedrec::`` namespace
keeps its 80 ops and ``fedrec_sparse::`` its two.  No GPU.

A deliberate interface change regenerates the fixture: ``python tests/test_op_schemas_quant.py``."""
import os

import torch

from fedrec_with_pytorchdistributed_amd.ops import native

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "op_schemas_quant.txt")


def _registered(prefix="fedrec_quant::"):
    native.lib()
    out = {}
    for name in torch._C._dispatch_get_all_op_names():
        if not name.startswith(prefix):
            continue
        kinds = [k for k in ("CUDA", "CompositeImplicitAutograd", "CompositeExplicitAutograd")
                 if torch._C._dispatch_has_kernel_for_dispatch_key(name, k)]
        out[name] = f"{torch._C._get_schema(name, '')} | {'+'.join(kinds) or 'none'}"
    return out


def _golden():
    with open(GOLDEN) as f:
        return [ln.rstrip("\n") for ln in f if ln.strip()]


def test_quant_schemas_and_kernel_kinds_match_the_fixture():
    assert [ln for _, ln in sorted(_registered().items())] == _golden()


def test_the_two_ops_are_there_and_have_kernels():
    got = _registered()
    assert sorted(got) == ["fedrec_quant::dequant_combine", "fedrec_quant::quantize_delta"]
    assert not [ln for ln in got.values() if ln.endswith("| none")]
    assert "Tensor(a!) residual" in got["fedrec_quant::quantize_delta"]
    assert "int bits, int seed, int offset" in got["fedrec_quant::quantize_delta"]


def test_the_pinned_namespaces_keep_their_op_sets():
    assert len(_registered("fedrec::")) == 80
    assert sorted(_registered("fedrec_sparse::")) == ["fedrec_sparse::combine", "fedrec_sparse::topk_delta"]


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        f.write("".join(ln + "\n" for _, ln in sorted(_registered().items())))
    print(f"wrote {len(_registered())} schemas to {GOLDEN}")
