"""The registered ``torch.ops.fedrec`` interface: every op's full schema (argument names, types,
alias annotations, defaults, returns) and the kind of kernel behind it, against the recorded
lines of ``tests/golden/op_schemas.txt``.  The registrations are spread over the binding
sources (``csrc/bind_*.cpp``, one ``TORCH_LIBRARY_FRAGMENT`` per kernel family); a dropped kernel
registration, a changed default or a lost op shows here, without a GPU.

A deliberate interface change regenerates the fixture: ``python tests/test_op_schemas.py``."""
import os

import torch

from fedrec_with_pytorchdistributed_amd.ops import native

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "op_schemas.txt")


def _registered():
    """name -> "<schema> | <kernel kind>" for every fedrec:: op of the loaded library."""
    native.lib()
    out = {}
    for name in torch._C._dispatch_get_all_op_names():
        if not name.startswith("fedrec::"):
            continue
        kinds = [k for k in ("CUDA", "CompositeImplicitAutograd", "CompositeExplicitAutograd")
                 if torch._C._dispatch_has_kernel_for_dispatch_key(name, k)]
        out[name] = f"{torch._C._get_schema(name, '')} | {'+'.join(kinds) or 'none'}"
    return out


def _golden():
    with open(GOLDEN) as f:
        lines = [ln.rstrip("\n") for ln in f if ln.strip()]
    return {ln.split("(", 1)[0]: ln for ln in lines}


def test_op_set_matches_fixture():
    got, want = set(_registered()), set(_golden())
    assert len(want) == 80
    assert got == want, f"missing: {sorted(want - got)}; unexpected: {sorted(got - want)}"


def test_every_schema_and_kernel_kind_matches_fixture():
    got, want = _registered(), _golden()
    diff = [f"{n}:\n  recorded   {want[n]}\n  registered {got.get(n)}" for n in sorted(want) if got.get(n) != want[n]]
    assert not diff, "\n".join(diff)


def test_every_op_has_a_kernel():
    assert not [ln for ln in _registered().values() if ln.endswith("| none")]


if __name__ == "__main__":
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as f:
        f.write("".join(ln + "\n" for _, ln in sorted(_registered().items())))
    print(f"wrote {len(_registered())} schemas to {GOLDEN}")
