"""The attention oracle of ``tests/attn_oracle.py`` on the CPU: its explicit fp64 gradients are
fp64 autograd; a rounding model of the kernels (fp32 torch with bf16 rounding exactly where the
kernels round) sits inside the per-element bound on every input set the GPU tests use; mutants
of that model -- a lost (title, head) pair, a mis-masked key, a wrong dropout mask, a wrong
softmax Jacobian, a missing scale -- all leave it; and a lost pair at n = 700 passes the
aggregate ``rel_err < 2e-2`` the older tests assert while failing the per-pair ratios."""
import functools

import pytest
import torch

import attn_oracle as ao
from attn_oracle import DH, FMIN, AttnOracle
from fedrec_with_pytorchdistributed_amd.ops import reference as ref


def _bf(x):
    return x.to(torch.bfloat16).float()


def model(qkv, mask, H, dout=None, drop=None, Z=None, softmax_mask=None, pad_keys=False, d_from_dropped=False,
          no_keep=False, dq_scale=0.125, dk_scale=0.125):
    """The kernels' arithmetic in fp32 torch: bf16 rounding of P~ and dS (T <= 64 only) and of
    the outputs.  -> (out bf16, dqkv bf16 | None).  The keyword arguments after ``drop`` are the
    mutants: another dropout mask ``Z``; another key mask in the softmax; tile-padding keys
    (K row clamped to T - 1, V zero) counted in the softmax; D from P~; dS without its keep
    factor; a wrong scale on dQ / dK."""
    n, T = mask.shape
    long = T > 64
    q, k, v = qkv.float().view(n, T, 3, H, DH).permute(2, 0, 3, 1, 4)
    kp = ((mask if softmax_mask is None else softmax_mask) != 0).view(n, 1, 1, T)
    sc = (q @ k.transpose(-1, -2)) * 0.125
    sc = sc.masked_fill(~kp, FMIN)
    if pad_keys:
        pad = -T % 16
        sc = torch.cat([sc, sc[..., T - 1:].expand(n, H, T, pad)], -1)
    e = torch.exp(sc - sc.amax(-1, keepdim=True))
    P = (e / e.sum(-1, keepdim=True))[..., :T]
    if Z is None and drop is not None:
        Z = ref.attention_dropout_scale(n, H, T, *drop)
    Pt = P if Z is None else P * Z
    Pr = Pt if long else _bf(Pt)
    out = ao._rows(Pr @ v).to(torch.bfloat16)
    if dout is None:
        return out, None
    g = ao._heads(dout.float(), n, T, H)
    dPt = g @ v.transpose(-1, -2)
    if Z is not None:
        dPt = dPt * Z
    Dt = ((Pt if d_from_dropped else P) * dPt).sum(-1, keepdim=True)
    dS = P * (dPt - Dt)
    if not no_keep:
        dS = dS * (mask != 0).view(n, 1, 1, T).float()
    dSq, dSk = dS * dq_scale, dS * dk_scale
    if not long:
        dSq, dSk = _bf(dSq), _bf(dSk)
    dqkv = torch.cat([ao._rows(dSq @ k), ao._rows(dSk.transpose(-1, -2) @ q), ao._rows(Pr.transpose(-1, -2) @ g)], 1)
    return out, dqkv.to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def case(n, H, T, qs, drop=None, keep=False):
    qkv, mask, dout = ao.make_inputs(n, H, T, qs)
    return qkv, mask, dout, AttnOracle(qkv, mask, H, dout, drop, keep=keep)


def worst(orc, out, dqkv):
    r = {}
    if out is not None:
        r.update(orc.ratios_fwd(out))
    if dqkv is not None:
        r.update(orc.ratios_bwd(dqkv))
    return {k: float(v.max()) for k, v in r.items()}


# ---------------------------------------------------------------------------- the oracle itself
@pytest.mark.parametrize("T,drop", [(17, None), (50, (0.1,) + ao.DROP_SEEDS[1]), (130, None)])
def test_explicit_gradients_are_autograd(T, drop):
    qkv, mask, dout, orc = case(9 + (T > 64), 5, T, 1.0, drop, True)
    assert torch.allclose(orc.x["o"], orc.o, rtol=1e-12, atol=1e-13)
    assert torch.allclose(orc.x["dqkv"], orc.dqkv, rtol=1e-11, atol=1e-12)
    assert float(orc.dqkv.abs().max()) > 0.1 and bool((orc.tol_dqkv > 0).all()) and bool((orc.tol_o > 0).all())
    assert not orc.dqkv[T:2 * T, :2 * orc.D].any()  # the all-masked title: dQ = dK = 0 exactly


def test_ratios_name_the_pair():
    qkv, mask, dout, orc = case(12, 5, 17, 1.0)
    out, _ = model(qkv, mask, 5)
    bad = out.clone()
    bad[3 * 17 + 4, 2 * DH + 7] += 1.0
    r = orc.ratios_fwd(bad)["out"]
    assert r.shape == (12, 5) and float(r[3, 2]) > 1 and int((r > 1).sum()) == 1
    with pytest.raises(AssertionError, match=r"title 3, head 2, row 4, column 7"):
        orc.check_fwd(bad, "probe")
    bad[0, 0] = float("nan")
    assert float(orc.ratios_fwd(bad)["out"][0, 0]) == float("inf")


# ------------------------------------------------------------------- the bound is not too tight
def _walk_cases():
    n1, n2 = ao.walk_titles(ao.NOMINAL_CUS, 12), ao.walk_titles(ao.NOMINAL_CUS, 12, 2)
    return [(n1, 12, ao.WALK_T, 1.0), (n2, 12, ao.WALK_T, 1.0)]


@pytest.mark.parametrize("n,H,T,qs", sorted(set(ao.small_cases() + ao.packed_cases() + ao.long_cases())) + _walk_cases())
def test_rounding_model_is_within_the_bound(n, H, T, qs):
    qkv, mask, dout, orc = case(n, H, T, qs)
    out, dqkv = model(qkv, mask, H, dout)
    w = worst(orc, out, dqkv)
    assert max(w.values()) <= 1.0, w


@pytest.mark.parametrize("n,H,T,qs,p,seed,offset",
                         [c + (p,) + so for c in ao.drop_cases() for p in ao.P_DROP for so in ao.DROP_SEEDS] +
                         [_walk_cases()[0] + d for d in ao.WALK_DROPS])
def test_rounding_model_with_dropout_is_within_the_bound(n, H, T, qs, p, seed, offset):
    qkv, mask, dout, orc = case(n, H, T, qs, (p, seed, offset))
    out, dqkv = model(qkv, mask, H, dout, (p, seed, offset))
    w = worst(orc, out, dqkv)
    assert max(w.values()) <= 1.0, w


# ------------------------------------------------------------------------ the bound is not blind
MUT_SETS = [(12, 12, 50, 1.0), (11, 5, 17, 1.0), (12, 12, 33, 4.0)]
MUT_LONG = [(11, 2, 200, 1.0)]


@pytest.mark.parametrize("n,H,T,qs", MUT_SETS + MUT_LONG)
def test_mutant_a_lost_pair(n, H, T, qs):
    qkv, mask, dout, orc = case(n, H, T, qs)
    out, dqkv = model(qkv, mask, H, dout)
    title, h = n - 1, H - 1  # the last pair of the walk: the one a short tail loses
    rows, cols = slice(title * T, (title + 1) * T), slice(h * DH, (h + 1) * DH)
    prev = slice((h - 1) * DH, h * DH)
    for name, x, width in (("out", out, 1), ("dqkv", dqkv, 3)):
        for fill in ("zeros", "neighbour"):
            bad = x.clone()
            for part in range(width):
                c = slice(cols.start + part * orc.D, cols.stop + part * orc.D)
                pc = slice(prev.start + part * orc.D, prev.stop + part * orc.D)
                bad[rows, c] = 0 if fill == "zeros" else x[rows, pc]
            r = orc.ratios_fwd(bad) if width == 1 else orc.ratios_bwd(bad)
            for key, v in r.items():
                assert float(v[title, h]) > 1, (name, fill, key)
                v = v.clone()
                v[title, h] = 0
                assert float(v.max()) <= 1, (name, fill, key)  # and only that pair


@pytest.mark.parametrize("n,H,T,qs", MUT_SETS + MUT_LONG)
def test_mutant_b_one_key_mis_masked(n, H, T, qs):
    qkv, mask, dout, orc = case(n, H, T, qs, None, True)
    P = orc.x["P"]
    # a kept key treated as masked: title 7 (random keys at 0.4), its key with the largest probability
    title = 7
    s = int((P[title] * (mask[title] != 0)).amax((0, 1)).argmax())
    assert mask[title, s] != 0 and int(mask[title].sum()) > 1
    m2 = mask.clone()
    m2[title, s] = 0
    w = worst(orc, *model(qkv, mask, H, dout, softmax_mask=m2))
    assert min(w.values()) > 1, w
    # a masked key treated as kept: title 2 (only key 0 kept) with key T - 1 let in
    m2 = mask.clone()
    assert m2[2, T - 1] == 0
    m2[2, T - 1] = 1
    w = worst(orc, *model(qkv, mask, H, dout, softmax_mask=m2))
    assert w["out"] > 1 and w["dV"] > 1, w


@pytest.mark.parametrize("n,H,T,qs", MUT_SETS + MUT_LONG)
def test_mutant_c_all_masked_title_returns_zeros(n, H, T, qs):
    qkv, mask, dout, orc = case(n, H, T, qs)
    assert not mask[1].any()
    out, _ = model(qkv, mask, H)
    out[T:2 * T] = 0
    r = orc.ratios_fwd(out)["out"]
    assert float(r[1].min()) > 1 and float(r[[0] + list(range(2, n))].max()) <= 1


@pytest.mark.parametrize("n,H,T,qs", MUT_SETS)
def test_mutant_d_tile_padding_keys_in_the_softmax(n, H, T, qs):
    qkv, mask, dout, orc = case(n, H, T, qs)
    assert T % 16
    w = worst(orc, *model(qkv, mask, H, dout, pad_keys=True))
    assert min(w.values()) > 1, w


@pytest.mark.parametrize("n,H,T,qs", MUT_SETS)
def test_mutant_e_wrong_dropout_mask(n, H, T, qs):
    seed, offset = ao.DROP_SEEDS[1]
    for p in (0.1, 0.5):
        qkv, mask, dout, orc = case(n, H, T, qs, (p, seed, offset))
        Z = ref.attention_dropout_scale(n + 1, H, T, p, seed, offset).view(-1, T, T)[1:n * H + 1].view(n, H, T, T)  # pair + 1
        w = worst(orc, *model(qkv, mask, H, dout, Z=Z))
        assert min(w.values()) > 1, (p, w)
        for drop in ((p, seed & 0xFFFFFFFF, offset), (p, seed, offset & 0xFFFFFFFF)):  # k1 / c3 dropped
            w = worst(orc, *model(qkv, mask, H, dout, drop))
            assert min(w.values()) > 1, (drop, w)
        # forward and backward under different masks: the backward alone fails
        out, _ = model(qkv, mask, H, dout, (p, seed, offset))
        _, dqkv = model(qkv, mask, H, dout, (p, seed, offset + 1))
        w = worst(orc, out, dqkv)
        assert w["out"] <= 1 and min(w["dQ"], w["dK"], w["dV"]) > 1, w


@pytest.mark.parametrize("n,H,T,qs", MUT_SETS)
def test_mutant_f_softmax_jacobian_from_dropped_probabilities(n, H, T, qs):
    drop = (0.1,) + ao.DROP_SEEDS[0]
    qkv, mask, dout, orc = case(n, H, T, qs, drop)
    w = worst(orc, *model(qkv, mask, H, dout, drop, d_from_dropped=True))
    assert w["out"] <= 1 and w["dV"] <= 1 and w["dQ"] > 1 and w["dK"] > 1, w


@pytest.mark.parametrize("n,H,T,qs", MUT_SETS + MUT_LONG)
def test_mutant_g_no_keep_factor_on_ds(n, H, T, qs):
    qkv, mask, dout, orc = case(n, H, T, qs)
    _, dqkv = model(qkv, mask, H, dout, no_keep=True)
    r = orc.ratios_bwd(dqkv)
    for key in ("dQ", "dK"):  # only the all-masked title shows it: P is 0 on every other masked key
        assert float(r[key][1].min()) > 1 and float(r[key][[0] + list(range(2, n))].max()) <= 1, key
    assert float(r["dV"].max()) <= 1


@pytest.mark.parametrize("n,H,T,qs", MUT_SETS + MUT_LONG)
def test_mutant_h_missing_scale(n, H, T, qs):
    qkv, mask, dout, orc = case(n, H, T, qs)
    w = worst(orc, *model(qkv, mask, H, dout, dq_scale=1.0))
    assert w["dQ"] > 1 and max(w["out"], w["dK"], w["dV"]) <= 1, w
    w = worst(orc, *model(qkv, mask, H, dout, dk_scale=1.0))
    assert w["dK"] > 1 and max(w["out"], w["dQ"], w["dV"]) <= 1, w


# ------------------------------------------------------------------------------ the gap, shown
def test_lost_pair_passes_the_aggregate_metric_and_fails_the_ratios():
    """The input of test_title_attention_launch_variants[700-50]: 8400 pairs."""
    n, T, H, D = 700, 50, 12, 768
    g = torch.Generator().manual_seed(n + T)
    qkv = torch.randn(n * T, 3 * D, generator=g).to(torch.bfloat16)
    lens = torch.randint(1, T + 1, (n,), generator=g)
    mask = (torch.arange(T)[None, :] < lens[:, None]).to(torch.int32)
    mask[0] = 0
    out, _ = model(qkv, mask, H)
    orc = AttnOracle(qkv, mask, H)
    assert float(orc.ratios_fwd(out)["out"].max()) <= 1
    want = ref.title_attention(qkv.float(), mask, H)

    def rel_err(a, b):  # tests/test_kernels_gpu.py
        a, b = a.float().cpu(), b.float().cpu()
        return float((a - b).norm() / (b.norm() + 1e-12))

    title, h = 699, 11
    rows, cols = slice(title * T, (title + 1) * T), slice(h * DH, (h + 1) * DH)
    for fill in ("zeros", "neighbour"):
        bad = out.clone()
        bad[rows, cols] = 0 if fill == "zeros" else out[rows, (h - 1) * DH:h * DH]
        assert rel_err(bad, want) < 2e-2, fill  # the old metric lets it through
        r = orc.ratios_fwd(bad)["out"]
        assert float(r[title, h]) > 1 and int((r > 1).sum()) == 1, fill  # the new one names the pair
        with pytest.raises(AssertionError, match="title 699, head 11"):
            orc.check_fwd(bad, fill)
