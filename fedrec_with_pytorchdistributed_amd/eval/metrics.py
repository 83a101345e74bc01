"""Ranking metrics: AUC, MRR, nDCG@k (reference ``evaluation_functions.py:5-31``).

Definitions match the reference:

* ``dcg_score``: gain ``2^y - 1``, discount ``log2(rank + 1)``, top ``k`` by score.
* ``ndcg_score``: ``dcg(y_true, y_score) / dcg(y_true, y_true)``.
* ``mrr_score``: ``sum(y / rank) / sum(y)`` in score order.
* ``roc_auc_score``: the Mann-Whitney statistic with average ranks for ties, i.e. what
  ``sklearn.metrics.roc_auc_score`` returns for binary labels (the reference imports
  sklearn's; this implementation removes the dependency and is checked against sklearn
  in the tests).

Sorting uses a stable descending order on ``-score`` so ties resolve like the reference's
``np.argsort(y_score)[::-1]`` (which reverses a stable ascending sort).

:func:`batch_metrics` evaluates many impressions at once (``[I, C]`` score matrix with the
positive in column 0, as in validation, ``client.py:160-165``) and returns the corpus
mean -- the fix for quirk Q9 (the reference returns only the last impression's numbers,
``client.py:171``), with the last impression's values kept for compat logging.
"""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np


def _order(y_score: np.ndarray) -> np.ndarray:
    return np.argsort(y_score, kind="stable")[::-1]


def dcg_score(y_true: Sequence[float], y_score: Sequence[float], k: int = 10) -> float:
    y_true = np.asarray(y_true, dtype=np.float64)
    order = _order(np.asarray(y_score))
    yt = np.take(y_true, order[:k])
    gains = 2.0 ** yt - 1.0
    disc = np.log2(np.arange(len(yt)) + 2.0)
    return float(np.sum(gains / disc))


def ndcg_score(y_true, y_score, k: int = 10) -> float:
    best = dcg_score(y_true, y_true, k)
    return dcg_score(y_true, y_score, k) / best


def mrr_score(y_true, y_score) -> float:
    y_true = np.asarray(y_true, dtype=np.float64)
    yt = np.take(y_true, _order(np.asarray(y_score)))
    rr = yt / (np.arange(len(yt)) + 1.0)
    return float(np.sum(rr) / np.sum(yt))


def _avg_ranks(x: np.ndarray) -> np.ndarray:
    order = np.argsort(x, kind="mergesort")
    xs = x[order]
    ranks = np.empty(len(x), dtype=np.float64)
    i = 0
    n = len(x)
    while i < n:
        j = i
        while j + 1 < n and xs[j + 1] == xs[i]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    return ranks


def roc_auc_score(y_true, y_score) -> float:
    y_true = np.asarray(y_true).astype(bool)
    y_score = np.asarray(y_score, dtype=np.float64)
    n_pos = int(y_true.sum())
    n_neg = len(y_true) - n_pos
    if n_pos == 0 or n_neg == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    r = _avg_ranks(y_score)
    return float((r[y_true].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def compute_amn(y_true, y_score):
    """AUC, MRR, nDCG@5, nDCG@10 of one impression (``evaluation_functions.py:26-31``)."""
    return (roc_auc_score(y_true, y_score), mrr_score(y_true, y_score),
            ndcg_score(y_true, y_score, 5), ndcg_score(y_true, y_score, 10))


def batch_metrics(scores: np.ndarray) -> Dict[str, float]:
    """Vectorised metrics for ``[I, C]`` scores whose positive is column 0.

    With exactly one positive per impression: AUC = fraction of negatives ranked below
    the positive (ties count 1/2); MRR = 1/rank; nDCG@k = 1/log2(rank+1) if rank <= k.
    ``rank`` breaks ties like the reference's reversed stable argsort: among equal
    scores the *later* column ranks first.
    """
    s = np.asarray(scores, dtype=np.float64)
    if s.ndim != 2 or s.shape[0] == 0:
        return {"auc": float("nan"), "mrr": float("nan"), "ndcg5": float("nan"), "ndcg10": float("nan"),
                "n": 0}
    p = s[:, :1]
    neg = s[:, 1:]
    C = s.shape[1]
    auc = ((neg < p).sum(1) + 0.5 * (neg == p).sum(1)) / (C - 1)
    # reversed stable argsort: all strictly-greater items, and equal items after column 0,
    # rank ahead of the positive
    rank = 1 + (neg > p).sum(1) + (neg == p).sum(1)
    mrr = 1.0 / rank
    nd5 = np.where(rank <= 5, 1.0 / np.log2(rank + 1.0), 0.0)
    nd10 = np.where(rank <= 10, 1.0 / np.log2(rank + 1.0), 0.0)
    out = {"auc": float(auc.mean()), "mrr": float(mrr.mean()), "ndcg5": float(nd5.mean()),
           "ndcg10": float(nd10.mean()), "n": int(s.shape[0])}
    out.update({"last_auc": float(auc[-1]), "last_mrr": float(mrr[-1]),
                "last_ndcg5": float(nd5[-1]), "last_ndcg10": float(nd10[-1])})
    return out


def metric_sums(scores: np.ndarray) -> np.ndarray:
    """Per-corpus sums ``[auc, mrr, ndcg5, ndcg10, count]`` (for an all-reduce of metrics)."""
    m = batch_metrics(scores)
    n = m["n"]
    if n == 0:
        return np.zeros(5)
    return np.array([m["auc"] * n, m["mrr"] * n, m["ndcg5"] * n, m["ndcg10"] * n, n], dtype=np.float64)


def impression_sums(counts: np.ndarray) -> np.ndarray:
    """``[auc, mrr, ndcg5, ndcg10, candidates, n, n_skipped]`` summed over the impressions of
    ``counts [I, 4]`` that :func:`impression_metrics` keeps (its definitions; the form that can be
    all-reduced across clients)."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 4)
    keep = (c[:, 2] > 0) & (c[:, 3] == 0)
    gt, eq, nn = (c[keep, j].astype(np.float64) for j in range(3))
    rank = 1.0 + gt + eq
    auc = ((nn - gt - eq) + 0.5 * eq) / nn
    inv = 1.0 / np.log2(rank + 1.0)
    return np.array([auc.sum(), (1.0 / rank).sum(), np.where(rank <= 5, inv, 0.0).sum(),
                     np.where(rank <= 10, inv, 0.0).sum(), nn.sum() + keep.sum(), float(keep.sum()),
                     float((~keep).sum())], dtype=np.float64)


def impression_means(sums: np.ndarray) -> Dict[str, float]:
    """:func:`impression_sums` (of one client, or summed over clients) -> the corpus means."""
    n = int(sums[5])
    d = float(n) if n else float("nan")
    return {"auc": float(sums[0] / d), "mrr": float(sums[1] / d), "ndcg5": float(sums[2] / d),
            "ndcg10": float(sums[3] / d), "mean_candidates": float(sums[4] / d), "n": n, "n_skipped": int(sums[6])}


def impression_metrics(counts: np.ndarray) -> Dict[str, float]:
    """Full-impression ranking quality from ``counts [I, 4]`` = ``(n_gt, n_eq, n_neg, n_nan)`` per
    impression (``ops.rank_impressions``): the single positive ranked against EVERY negative the
    impression showed -- the protocol MIND numbers are quoted in -- with the definitions of
    :func:`batch_metrics`: ``rank = 1 + n_gt + n_eq``, ``auc = ((n_neg - n_gt - n_eq) + n_eq / 2) /
    n_neg``, ``mrr = 1 / rank``, ``ndcg@k = 1 / log2(rank + 1)`` if ``rank <= k`` else 0.  Impressions
    without a negative (AUC undefined) or with a NaN score are left out of every mean and counted in
    ``n_skipped``.  -> corpus means ``auc`` / ``mrr`` / ``ndcg5`` / ``ndcg10``, ``mean_candidates``
    (positive included), ``n`` and ``n_skipped``; the means are NaN when ``n == 0``."""
    return impression_means(impression_sums(counts))


def topk_metrics(ids: np.ndarray, pos: np.ndarray) -> Dict[str, float]:
    """Full-catalog ranking quality of ordered top-k lists ``ids [I, k]`` (-1 = empty slot) against
    one held-out positive ``pos [I]`` per impression: ``hr@k`` (the positive is in the list),
    ``ndcg@k`` (``1 / log2(rank + 1)`` if it is ranked within k, else 0 -- the ideal DCG of a
    single positive is 1), ``mrr@k`` (``1 / rank`` or 0), corpus means, and ``n``."""
    ids = np.asarray(ids)
    pos = np.asarray(pos).reshape(-1)
    k = int(ids.shape[1]) if ids.ndim == 2 else 0
    if ids.ndim != 2 or ids.shape[0] == 0:
        return {f"hr@{k}": float("nan"), f"ndcg@{k}": float("nan"), f"mrr@{k}": float("nan"), "k": k, "n": 0}
    hit = ids == pos[:, None]
    found = hit.any(1)
    rank = np.where(found, hit.argmax(1) + 1, 1).astype(np.float64)
    return {f"hr@{k}": float(found.mean()), f"ndcg@{k}": float(np.where(found, 1.0 / np.log2(rank + 1.0), 0.0).mean()),
            f"mrr@{k}": float(np.where(found, 1.0 / rank, 0.0).mean()), "k": k, "n": int(ids.shape[0])}


def diversity_metrics(ids: np.ndarray, ild: np.ndarray, n_catalog: int) -> Dict[str, float]:
    """Beyond-accuracy quality of recommendation lists ``ids [n, k]`` (-1 = empty slot) with their
    intra-list diversity ``ild [n]`` (``ops.mmr_rerank``: a list's mean pairwise ``1 - cos``):
    ``ild@k``, the mean of ``ild`` over the lists with at least two items (NaN when there is none), and
    ``coverage@k``, the distinct recommended ids divided by ``n_catalog``, the number of catalog rows
    that were eligible for recommendation."""
    ids = np.asarray(ids)
    ild = np.asarray(ild, dtype=np.float64).reshape(-1)
    k = int(ids.shape[1]) if ids.ndim == 2 else 0
    if ids.ndim != 2 or ids.shape[0] == 0:
        return {f"ild@{k}": float("nan"), f"coverage@{k}": float("nan")}
    two = (ids >= 0).sum(1) >= 2
    distinct = np.unique(ids[ids >= 0]).size
    return {f"ild@{k}": float(ild[two].mean()) if two.any() else float("nan"),
            f"coverage@{k}": float(distinct / n_catalog) if n_catalog > 0 else float("nan")}
