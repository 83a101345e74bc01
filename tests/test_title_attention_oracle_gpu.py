"""Every title-attention kernel form against the fp64 oracle and its per-element bound
(``tests/attn_oracle.py``), judged per (title, head): the one-shot and persistent MFMA forwards,
the dropout forward in both forms, the packed-row forward, the one-shot and persistent
backwards, the dropout backward (split and unsplit prefetch, one-shot), and the T > 64
online-softmax forward and backward.  Every call is repeated and must be bit-identical; the
forms the kernel comments promise equal are held to ``torch.equal``.  The walk cases size
themselves from the device's CU count so every persistent wave takes 3 or 4 pairs.

The inputs are the shared builders of ``attn_oracle`` (a mask zoo with an all-masked title, a
title whose first key is padding, one with only its last key, whole masked 64-key chunks for
T > 64; q also scaled by 4); ``tests/test_attn_oracle_cpu.py`` runs a rounding model of the
kernels over the same sets.  Each test prints its worst ratio (``-rP`` shows them)."""
import functools

import pytest
import torch

import attn_oracle as ao
from attn_oracle import AttnOracle
from fedrec_with_pytorchdistributed_amd.ops import native

pytestmark = pytest.mark.gpu

FWD_FORMS = [-2, -1, 0, 1, 2, 4]  # title_attn_set_waves


@functools.lru_cache(maxsize=None)
def case(n, H, T, qs, drop=None):
    qkv, mask, dout = ao.make_inputs(n, H, T, qs)
    return qkv, mask, dout, AttnOracle(qkv, mask, H, dout, drop)


def _twice(f):
    a = f()
    assert torch.equal(f(), a), "a second call differs"
    assert bool(torch.isfinite(a.float()).all())
    return a


def run_fwd(lib, waves, qkv, mask, H, drop=None):
    lib.title_attn_set_waves(waves)
    try:
        if drop is None:
            return _twice(lambda: lib.title_attention(qkv, mask, H))
        return _twice(lambda: lib.title_attention_drop(qkv, mask, H, *drop))
    finally:
        lib.title_attn_set_waves(-2)


def run_bwd(lib, variant, qkv, dout, mask, H, drop=None, split=1):
    lib.title_attn_bwd_set_variant(variant)
    lib.title_attn_bwd_set_variant(10 + split)
    try:
        if drop is None:
            return _twice(lambda: lib.title_attention_bwd(qkv, dout, mask, H))
        return _twice(lambda: lib.title_attention_bwd_drop(qkv, dout, mask, H, *drop))
    finally:
        lib.title_attn_bwd_set_variant(1)
        lib.title_attn_bwd_set_variant(11)


def run_packed(lib, qkv, mask, H, dev):
    """title_plan + title_attention_packed, scattered back to title-major rows."""
    D = H * ao.DH
    rowmap, src, kv_start, kv_len, qstart, n_kv = lib.title_plan(mask.to(dev))
    srcl = src.long().cpu()
    packed = qkv[srcl].clone()
    packed[int(n_kv.item()):, D:] = float("nan")  # K / V of query-only rows must never be read
    packed = packed.to(dev)
    out = _twice(lambda: lib.title_attention_packed(packed, rowmap, kv_start, kv_len, qstart, H)).cpu()
    got = torch.empty_like(out)
    got[srcl] = out
    return got


def report(form, worst):
    print("attn-oracle ratio %-28s %.3f" % (form, worst))


def cus_of(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


# ------------------------------------------------------------------------------ small cases
@pytest.mark.parametrize("n,H,T,qs", ao.small_cases())
def test_forward_every_form(dev, n, H, T, qs):
    qkv, mask, _, orc = case(n, H, T, qs)
    lib = native.lib()
    q, m = qkv.to(dev), mask.to(dev)
    for waves in FWD_FORMS:
        report("fwd waves=%d" % waves, orc.check_fwd(run_fwd(lib, waves, q, m, H), "waves=%d" % waves))


@pytest.mark.parametrize("n,H,T,qs", ao.small_cases())
def test_backward_both_variants(dev, n, H, T, qs):
    qkv, mask, dout, orc = case(n, H, T, qs)
    lib = native.lib()
    q, m, g = qkv.to(dev), mask.to(dev), dout.to(dev)
    d1 = run_bwd(lib, 1, q, g, m, H)
    d0 = run_bwd(lib, 0, q, g, m, H)
    report("bwd variant=1", orc.check_bwd(d1, "variant=1"))
    report("bwd variant=0", orc.check_bwd(d0, "variant=0"))
    assert torch.equal(d1, d0)  # title_attn_bwd.hip: "Same math, same outputs as title_attn_bwd_kernel"


@pytest.mark.parametrize("seed,offset", ao.DROP_SEEDS)
@pytest.mark.parametrize("p", ao.P_DROP)
@pytest.mark.parametrize("n,H,T,qs", ao.drop_cases())
def test_dropout_forward_and_backward_every_form(dev, n, H, T, qs, p, seed, offset):
    """Forward and backward are held to ONE oracle mask: a backward that regenerates another
    mask than the forward applied fails."""
    drop = (p, seed, offset)
    qkv, mask, dout, orc = case(n, H, T, qs, drop)
    lib = native.lib()
    q, m, g = qkv.to(dev), mask.to(dev), dout.to(dev)
    for waves in (-2, 2):  # persistent 2-deep prefetching; one-shot
        report("drop fwd waves=%d" % waves, orc.check_fwd(run_fwd(lib, waves, q, m, H, drop), "drop waves=%d" % waves))
    ds = [run_bwd(lib, 1, q, g, m, H, drop, split=1), run_bwd(lib, 1, q, g, m, H, drop, split=0),
          run_bwd(lib, 0, q, g, m, H, drop)]
    for d, form in zip(ds, ("variant=1 split", "variant=1 unsplit", "variant=0")):
        report("drop bwd " + form, orc.check_bwd(d, "drop " + form))
    assert torch.equal(ds[0], ds[1])  # split and unsplit prefetch: the same arithmetic
    # The one-shot form is NOT bit-equal to the persistent ones in dQ / dK: the compiler contracts
    # the terms of D_t = sum P dP into fma differently per instantiation (title_attn_bwd.hip, the
    # comment on the persistent form), a legitimately different rounding -- each form is on the
    # oracle above.  dV = P~^T dO has no such freedom (products only, then bf16, then MFMA).
    assert torch.equal(ds[0][:, 2 * orc.D:], ds[2][:, 2 * orc.D:])
    differ = int((ds[0] != ds[2]).sum())
    print("attn-oracle drop bwd one-shot vs persistent: %d of %d elements differ" % (differ, ds[0].numel()))
    # Last-bit flips, not another mask or another pair: a few fp32 ulps in D_t move a bf16 rounding
    # of dS or of an output with probability ~ 2^-16 per element; 1e-3 is sixty times that.
    assert differ <= ds[0].numel() // 1000


@pytest.mark.parametrize("n,H,T,qs", ao.packed_cases())
def test_packed_forward(dev, n, H, T, qs):
    qkv, mask, _, orc = case(n, H, T, qs)
    report("packed", orc.check_fwd(run_packed(native.lib(), qkv, mask, H, dev), "packed"))


@pytest.mark.parametrize("n,H,T,qs", ao.long_cases())
def test_long_forward_and_backward(dev, n, H, T, qs):
    qkv, mask, dout, orc = case(n, H, T, qs)
    assert orc.long
    lib = native.lib()
    q, m, g = qkv.to(dev), mask.to(dev), dout.to(dev)
    report("long fwd", orc.check_fwd(run_fwd(lib, -2, q, m, H), "long"))
    report("long bwd", orc.check_bwd(run_bwd(lib, 1, q, g, m, H), "long"))


# ------------------------------------------------------------------------------- walk cases
def _walk(dev, blocks_per_cu=1, drop=None):
    """Inputs on which every persistent wave of a ``cus * blocks_per_cu``-block grid walks 3 or
    4 pairs; asserts that precondition from the launchers' grid clamp."""
    H, T = 12, ao.WALK_T
    cus = cus_of(dev)
    n = ao.walk_titles(cus, H, blocks_per_cu)
    pairs = n * H
    blocks = min(cus * blocks_per_cu, (pairs + 3) // 4)  # title_attn.hip / title_attn_bwd.hip launchers
    assert pairs > 8 * blocks and pairs % (4 * blocks) != 0, (cus, n, pairs, blocks)
    return (H,) + case(n, H, T, 1.0, drop)


@pytest.mark.parametrize("waves", [-2, -1, 0])
def test_walk_forward(dev, waves):
    H, qkv, mask, _, orc = _walk(dev, 2 if waves == 0 else 1)
    out = run_fwd(native.lib(), waves, qkv.to(dev), mask.to(dev), H)
    report("walk fwd waves=%d" % waves, orc.check_fwd(out, "walk waves=%d" % waves))


def test_walk_packed(dev):
    H, qkv, mask, _, orc = _walk(dev)
    report("walk packed", orc.check_fwd(run_packed(native.lib(), qkv, mask, H, dev), "walk packed"))


def test_walk_backward(dev):
    H, qkv, mask, dout, orc = _walk(dev)
    d = run_bwd(native.lib(), 1, qkv.to(dev), dout.to(dev), mask.to(dev), H)
    report("walk bwd variant=1", orc.check_bwd(d, "walk variant=1"))


@pytest.mark.parametrize("p,seed,offset", ao.WALK_DROPS)
def test_walk_dropout(dev, p, seed, offset):
    drop = (p, seed, offset)
    H, qkv, mask, dout, orc = _walk(dev, drop=drop)
    lib = native.lib()
    q, m, g = qkv.to(dev), mask.to(dev), dout.to(dev)
    report("walk drop fwd waves=-2", orc.check_fwd(run_fwd(lib, -2, q, m, H, drop), "walk drop fwd"))
    d1 = run_bwd(lib, 1, q, g, m, H, drop, split=1)
    d0 = run_bwd(lib, 1, q, g, m, H, drop, split=0)
    report("walk drop bwd split", orc.check_bwd(d1, "walk drop split"))
    report("walk drop bwd unsplit", orc.check_bwd(d0, "walk drop unsplit"))
    assert torch.equal(d1, d0)
