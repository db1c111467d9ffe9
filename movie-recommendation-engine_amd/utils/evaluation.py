"""utils.evaluation -- drop-in for the reference module of the same name (reference utils/evaluation.py): hit rate @ k and the
reference's scaled MRR, computed on the device from ONE number per (query, ground truth) pair.

The reference runs, per metric and per query, a GEMV against the whole catalogue followed by torch.topk (hit rate) or a full
torch.sort (MRR).  Every one of those numbers follows from the rank of the ground-truth item in the query's similarity order:
    hit@k = (rank <= k)            MRR = mean(scale / rank)
and the rank is a count: 1 + the number of items that come before the ground truth.  `pinsage_hip.dense.target_rank` counts it
in the epilogue of one fp32-MFMA GEMM (ps_rank_count; the [nq, N] similarity matrix is never written), so evaluate_embeddings
makes ONE rank launch for all of its metrics.

Order and ties: similarity descending, ties by ascending item id -- the order of ps_dot_topk / generate_recommendations.
torch.topk and torch.sort leave the order of equal similarities unspecified, so where the ground truth ties with another item
the reference's result depends on its CPU kernels; with no ties the ranks, and so every metric, are the reference's exactly
(the similarities themselves are the device GEMM's: the ranks agree wherever no other item is closer to the ground truth's
similarity than the two summation orders can differ).

Return types and edge cases follow the reference: hit rates are Python floats (hits / total), MRR is np.float64 computed on the
host as np.mean(1.0 / (rank / scale)); k > number of items raises RuntimeError (as torch.topk does), an empty query list makes
the hit rate raise ZeroDivisionError, negative query indices wrap, a ground truth that is not an item index is a miss for the
hit rate and an IndexError for the MRR.
"""
from __future__ import annotations

import operator

import numpy as np
import torch

from pinsage_hip import dense
from pinsage_hip import native as nv
from utils.nearest_neighbors import generate_recommendations  # noqa: F401  (utils/evaluation.py:106-132, on the device)


def _device_embeddings(item_embeddings):
    E = torch.as_tensor(item_embeddings, dtype=torch.float32)
    if not E.is_cuda:
        E = E.to(nv.require_gpu())
    if E.dim() != 2:
        raise ValueError(f"item_embeddings must be [N, D], got {tuple(E.shape)}")
    return E.contiguous()


def _index_array(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x).reshape(-1).astype(np.int64, copy=False)


def _target_ranks(item_embeddings, query_indices, ground_truth_indices):
    """-> (rank int64 [P], is_item bool [P]): the 1-based rank of every pair's ground truth in its query's similarity order
    (N + 1 where the ground truth is not an item index), one ps_rank_count launch"""
    E = _device_embeddings(item_embeddings)
    N = int(E.size(0))
    q = _index_array(query_indices)
    gt = _index_array(ground_truth_indices)
    if gt.size < q.size:                      # the reference reads ground_truth_indices[i] for every query
        raise IndexError(f"index {gt.size} is out of bounds for axis 0 with size {gt.size}")
    gt = gt[:q.size]
    bad = (q < -N) | (q >= N)
    if bad.any():
        raise IndexError(f"index {int(q[bad][0])} is out of bounds for dimension 0 with size {N}")
    q = np.where(q < 0, q + N, q)
    is_item = (gt >= 0) & (gt < N)
    rank = np.full(q.size, N + 1, dtype=np.int64)
    if is_item.any():
        r = dense.target_rank(E, torch.from_numpy(q[is_item]), torch.from_numpy(gt[is_item]))
        rank[is_item] = r.cpu().numpy()
    return rank, is_item, N


def _hit_rate(rank, n_items, k):
    total = rank.size
    if total == 0:
        hits = 0
        return hits / total                   # ZeroDivisionError, as the reference
    k = operator.index(k)
    if k < 0 or k > n_items:
        raise RuntimeError(f"selected index k out of range (k = {k}, {n_items} items)")
    hits = int(np.count_nonzero(rank <= k))
    return hits / total


def _mrr(rank, is_item, scale):
    if not is_item.all():                     # np.where(indices == gt_idx)[0][0] of the reference
        raise IndexError("index 0 is out of bounds for axis 0 with size 0")
    return np.mean(1.0 / (rank / scale))


def calculate_hit_rate(item_embeddings, query_indices, ground_truth_indices, k=500):
    """Hit rate @ k: the share of pairs whose ground truth is among the k items most similar to the query (the query itself
    included, as in the reference)."""
    if len(query_indices) == 0:
        return _hit_rate(np.zeros(0, np.int64), 0, k)
    rank, _, n = _target_ranks(item_embeddings, query_indices, ground_truth_indices)
    return _hit_rate(rank, n, k)


def calculate_mrr(item_embeddings, query_indices, ground_truth_indices, scale=100):
    """The reference's scaled mean reciprocal rank: mean over pairs of 1 / (rank / scale), np.float64."""
    rank, is_item, _ = _target_ranks(item_embeddings, query_indices, ground_truth_indices)
    return _mrr(rank, is_item, scale)


def evaluate_embeddings(item_embeddings, test_data, k_values=[10, 50, 100, 500]):  # noqa: B006  (the reference's default)
    """{'hit_rate@k' for k in k_values, 'mrr'} of test_data['positive_pairs'] ([P, 2] int64: query, ground truth), from one
    rank computation."""
    positive_pairs = test_data['positive_pairs']
    query_indices = positive_pairs[:, 0].numpy()
    ground_truth_indices = positive_pairs[:, 1].numpy()
    rank, is_item, n = _target_ranks(item_embeddings, query_indices, ground_truth_indices)
    results = {}
    for k in k_values:
        results[f'hit_rate@{k}'] = _hit_rate(rank, n, k)
    results['mrr'] = _mrr(rank, is_item, 100)
    return results
