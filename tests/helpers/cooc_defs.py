"""Restatement of GraphBuilder.build_item_similarity_graph (reference data/graph_builder.py:59-116) as five rules, in numpy,
independent of the device path (no planes, no windows, no packed keys):

  1. users are visited in groupby('userId') order (ascending raw id); rows keep their dataframe order inside a group;
  2. count(a, b) = sum_u m_ua m_ub for a < b, count(a, a) = sum_u m_ua (m_ua - 1) / 2;
  3. a pair survives when count >= threshold (pairs with count 0 never exist);
  4. pairs are ordered by (u, p, q): u the first user (groupby order) holding the pair, p < q the first positions of a and b
     in u's group (the first two positions of a for a self pair);
  5. pair k emits [a -> b, b -> a] (a <= b) at columns 2k, 2k + 1, weight = count as float32.

The pair enumeration is per user (sum_u d_u^2 / 2 pairs), fine for test-sized data."""
import numpy as np


def _groups(user_ids, item_idx):
    """(user rank, position in group, item) per row, rows in (user, dataframe) order"""
    users = np.asarray(user_ids, dtype=np.int64)
    items = np.asarray(item_idx, dtype=np.int64)
    order = np.lexsort((np.arange(users.size), users))
    _, rank = np.unique(users[order], return_inverse=True)
    start = np.searchsorted(rank, rank, side="left")
    return rank, np.arange(users.size) - start, items[order]


def pair_table(user_ids, item_idx, num_items):
    """-> dict of arrays over every pair with count >= 1: a, b (a <= b), count, u, p, q (the rule-4 key), unsorted"""
    rank, pos, items = _groups(user_ids, item_idx)
    M = int(num_items)
    # distinct (user, item) entries: multiplicity, first and second position
    ekey = rank * M + items
    o = np.lexsort((pos, ekey))
    ek, first_idx, mult = np.unique(ekey[o], return_index=True, return_counts=True)
    eu, ei = ek // M, ek % M
    p1 = pos[o][first_idx]
    p2 = np.where(mult >= 2, pos[o][np.minimum(first_idx + 1, o.size - 1)], -1)
    A, B, CNT, Uu, P, Q = [], [], [], [], [], []
    bounds = np.flatnonzero(np.diff(np.concatenate([[-1], eu, [eu.max() + 1 if eu.size else 0]])))
    for s, e in zip(bounds[:-1], bounds[1:]):
        if e - s < 2:
            continue
        i, j = np.triu_indices(e - s, 1)
        i, j = i + s, j + s                     # ei ascending inside a user: ei[i] < ei[j]
        A.append(ei[i]); B.append(ei[j]); CNT.append(mult[i] * mult[j]); Uu.append(eu[i])
        P.append(np.minimum(p1[i], p1[j])); Q.append(np.maximum(p1[i], p1[j]))
    s = mult >= 2
    A.append(ei[s]); B.append(ei[s]); CNT.append(mult[s] * (mult[s] - 1) // 2); Uu.append(eu[s]); P.append(p1[s]); Q.append(p2[s])
    a, b, c, u, p, q = (np.concatenate(x).astype(np.int64) for x in (A, B, CNT, Uu, P, Q))
    # aggregate over users: count summed, key = the smallest (u, p, q)
    o = np.lexsort((q, p, u, b, a))
    a, b, c, u, p, q = a[o], b[o], c[o], u[o], p[o], q[o]
    head = np.ones(a.size, dtype=bool)
    head[1:] = (a[1:] != a[:-1]) | (b[1:] != b[:-1])
    starts = np.flatnonzero(head)
    return dict(a=a[starts], b=b[starts], count=np.add.reduceat(c, starts) if starts.size else c[:0], u=u[starts], p=p[starts],
                q=q[starts])


def item_similarity_graph(user_ids, item_idx, num_items, threshold=5):
    """-> (edge_index int64 [2, 2P], edge_weight float32 [2P]) as numpy arrays, the reference's output by rules 1-5"""
    t = pair_table(user_ids, item_idx, num_items)
    keep = np.array([int(c) >= threshold for c in t["count"]], dtype=bool) if t["count"].size else np.zeros(0, bool)
    o = np.lexsort((t["q"][keep], t["p"][keep], t["u"][keep]))
    a, b, c = t["a"][keep][o], t["b"][keep][o], t["count"][keep][o]
    ei = np.stack([np.stack([a, b], 1).reshape(-1), np.stack([b, a], 1).reshape(-1)]).astype(np.int64).reshape(2, -1)
    return ei, np.repeat(c, 2).astype(np.float32)
