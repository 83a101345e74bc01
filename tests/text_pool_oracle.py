"""The additive pool's bf16 text-head forms (csrc/additive_pool.hip: ``pool_fwd16`` / ``pool_bwd16``, the
16-byte vectorised kernels, and ``pool_fwd_kernel<bf16>`` / ``pool_bwd_kernel<bf16>``, the generic
ones) under the fp64 pool oracle of ``tests/user_oracle.py`` (a plain helper module for
tests/test_text_pool_oracle_cpu.py and tests/test_text_pool_oracle_gpu.py, not a conftest).

``x`` and ``e`` are rounded to bf16 first and the oracle gets ``x.float()``, ``e.float()``: the bf16
values are the exact operands and the kernels accumulate in fp32, so every bound of section 2 of
``user_oracle`` applies unchanged -- ``tol_alpha``, ``tol_pooled``, ``dx``, ``dw2``, ``db2``, and
``dpre_b`` for ``dpre``, which these kernels store rounded to bf16.  Every input set has n >= 2
sequences: then ``T + 4 n + 3``, the adds ``dw2``'s bound counts, covers the ``ceil(T / TG) + TG + n``
adds of the vectorised backward as well (``T = 1, TG = 8``: ``9 + n <= 4 + 4 n``).

One quantity is new.  The vectorised backward also returns ``dsum``, the column sums over (n, t) of
the ROUNDED ``dpre`` it wrote (``AdditivePoolFn.backward`` uses it as the ``att_fc1`` bias gradient).
Its reference is the fp64 column sum of the bf16 ``dpre`` the kernel itself wrote, its bound::

    tol_dsum_q = k u sum_{n,t} |dpre_b_ntq| + TINY ,   k = ceil(T / TG) + TG + n ,   TG = 256 / (Q / 8)

A thread (t-group ``tg`` of TG, 8-column chunk) adds its ``ceil(T / TG)`` rounded values in fp32, the
TG t-group partials are added in order through LDS, and the n partial rows (one per block) go
through ``colsum_f32``: for n <= 128 rows one pass, a wave adding at most 32 contiguous rows in order
and then ``(w0 + w1) + (w2 + w3)`` -- n - 1 roundings when n <= 32 (the other waves hold exact
zeros), at most 31 + 2 otherwise; beyond 128 rows the second pass adds ``ceil(chunks / 4) + 2`` more.
n bounds them all.  Every add acts on partial sums of magnitude at most ``sum |dpre_b|``.

``vec_ok`` is the launcher's predicate for the vectorised kernels; the backward takes them only when
``dx`` is not wanted (they do not write it).
"""
import functools

import torch

import user_oracle as uo

BF = torch.bfloat16


def vec_ok(T: int, D: int, Q: int) -> bool:
    return T <= 128 and D % 8 == 0 and Q % 8 == 0 and D <= 1024 and 256 <= Q <= 512


# (T, D, Q).  Vectorised: the production shape (TG = 5, DC = 96: one idle t-group in each phase); every
# limit at once (TG = 4, DC = 128, the second 64-lane chunk over D live); TG = 8, DC = 64; T < TG with
# QC = 33 (25 idle threads); DC = 1
VEC_SHAPES = [(50, 768, 384), (128, 1024, 512), (17, 512, 256), (3, 64, 264), (1, 8, 256)]
# generic, each missing exactly one condition of vec_ok: T, Q below, Q above, D above, D % 8
NEAR_SHAPES = [(129, 768, 384), (50, 768, 248), (50, 768, 520), (50, 1032, 384), (50, 772, 384)]
# generic: nothing divides; long T; MAXT_G
GENERIC_SHAPES = NEAR_SHAPES + [(17, 36, 5), (300, 64, 32), (2048, 8, 8)]
FORMS = {"vectorised": VEC_SHAPES, "generic": GENERIC_SHAPES}
assert all(vec_ok(*s) for s in VEC_SHAPES) and not any(vec_ok(*s) for s in GENERIC_SHAPES)


@functools.lru_cache(maxsize=None)
def inputs(T: int, D: int, Q: int, masked: bool):
    """``uo.pool_inputs`` with ``x`` and ``e`` rounded to bf16: ``(x, e, w2, b2, keep | None, g)``."""
    x, e, w2, b2, keep, g = uo.pool_inputs(T, D, Q, masked)
    assert x.shape[0] >= 2
    return x.to(BF), e.to(BF), w2, b2, keep, g


@functools.lru_cache(maxsize=None)
def oracle(T: int, D: int, Q: int, masked: bool) -> uo.PoolOracle:
    x, e, w2, b2, keep, _ = inputs(T, D, Q, masked)
    return uo.PoolOracle(x.float(), e.float(), w2, b2, keep)


def dsum_depth(T: int, Q: int, n: int) -> int:
    TG = 256 // (Q // 8)
    return (T + TG - 1) // TG + TG + n


def dsum_ref(dpre_b: torch.Tensor):
    """-> (value, tol) [Q] fp64 from the bf16 ``dpre`` [n, T, Q] a vectorised backward wrote."""
    n, T, Q = dpre_b.shape
    d = dpre_b.detach().cpu().double()
    return d.sum((0, 1)), dsum_depth(T, Q, n) * uo.U * d.abs().sum((0, 1)) + uo.TINY
