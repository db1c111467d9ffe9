"""The case table of the personalized-PageRank tests, a plain-python restatement of what the reference's
compute_ppr_matrix / precompute_top_neighbors do (utils/random_walk.py:144-229), written from their description, and the
level-scheduled pull model whose arithmetic the kernels of csrc/ppr_push.hip perform.

  reference   per source: score[s] = mass[s] = 1; `sweeps` times, for v ascending over the LIVE mass vector: if mass[v] > 0,
              score[v] += alpha mass[v], every out-edge (t, w) of v gets mass[t] += ((1 - alpha) mass[v]) (w / sum(row v)), the
              row sum taken left to right, then mass[v] = 0.  A push to a larger id is seen in the same sweep, to a smaller id in
              the next one, to v itself never.
  pull model  c_k(u) = (1 - alpha) m if the mass m that u holds in sweep k is > 0, else 0; the mass of v in sweep k is the
              left-to-right sum  init + sum_{u > v, ascending} c_{k-1}(u) share(u -> v) + sum_{u < v, ascending} c_k(u) share(u -> v)
              (init = 1 for v = source in sweep 0; multi-edges in adjacency order; self-loops left out).  v needs only
              lower-numbered in-neighbours of the same sweep: nodes are visited level by level, level(v) = 1 + max level of
              its in-neighbours u < v.

python floats throughout (IEEE doubles, one rounding per operation).  Shared by tests/test_ppr_cases.py (CPU),
tests/test_hip_ppr.py (GPU) and tests/golden/make_golden_ppr.py (which records the reference's own outputs)."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "reference_golden_ppr.npz")
BIP_M, BIP_U = 24, 17
DEFAULT_ALPHA, DEFAULT_SWEEPS = 0.15, 10          # what precompute_top_neighbors always uses (utils/random_walk.py:209)


def _float_weights(rs, n):
    """0.1 + 4.9 u as fp32: sums of such weights round, so the order of additions shows"""
    return (rs.random_sample(n) * 4.9 + 0.1).astype(np.float32)


def _bipartite():
    from conftest import bipartite_graph
    return bipartite_graph(BIP_M, BIP_U, 150, 7, "float")


def _chain():
    """0 -> 1 -> ... -> 47 (48 levels) with back edges, so that later sweeps carry mass down again"""
    rs = np.random.RandomState(52)
    src = list(range(47)) + [47, 30, 30, 12, 40, 5]
    dst = list(range(1, 48)) + [0, 2, 29, 3, 11, 4]
    return np.array([src, dst], dtype=np.int64), _float_weights(rs, len(src))


def _random_directed():
    """V = 40, E = 300: self-loops, duplicate edges, sinks (3, 11, 26), an isolated node (17)"""
    rs = np.random.RandomState(53)
    senders = np.array([v for v in range(40) if v not in (3, 11, 17, 26)])
    receivers = np.array([v for v in range(40) if v != 17])
    src = senders[rs.randint(0, senders.size, size=300)]
    dst = receivers[rs.randint(0, receivers.size, size=300)]
    src[:8] = dst[:8] = [0, 5, 9, 14, 21, 30, 38, 39]            # self-loops
    src[8:20], dst[8:20] = src[20:32], dst[20:32]                # duplicate edges, apart from their originals
    dst[290:293] = [3, 11, 26]
    src[299], dst[299] = 39, 0                                   # the largest id exists: V = 40
    return np.stack([src, dst]).astype(np.int64), _float_weights(rs, 300)


HUB = 150


def _hub():
    """node 150 has in-degree 300, from 0..149 and 151..300, and feeds all of them"""
    rs = np.random.RandomState(54)
    others = np.array([v for v in range(301) if v != HUB])
    src = np.concatenate([others, np.full(300, HUB), others[:-1]])
    dst = np.concatenate([np.full(300, HUB), rs.permutation(others), others[1:]])
    return np.stack([src, dst]).astype(np.int64), _float_weights(rs, src.size)


def _stars():
    """two symmetric stars with unit weights: centre 0 with leaves 1..8, centre 17 with leaves 9..16.  From a centre every leaf of
    its star gets exactly the same score, so a top-4 must resolve the tie to the smaller ids."""
    a, b = np.arange(1, 9), np.arange(9, 17)
    src = np.concatenate([np.zeros(8, np.int64), a, np.full(8, 17), b])
    dst = np.concatenate([a, np.zeros(8, np.int64), b, np.full(8, 17)])
    return np.stack([src, dst]).astype(np.int64), np.ones(32, dtype=np.float32)


_ALL_BIP = tuple(range(BIP_M + BIP_U)) + (BIP_M + BIP_U + 2,)          # every node and one source >= V
# name -> (graph, sources, alpha, sweeps, k of the recorded precompute_top_neighbors)
CASES = {
    "bip10": (_bipartite, _ALL_BIP, 0.15, 10, 10),
    "bip4": (_bipartite, (0, 23, 24, 40, 43, 7, 7, 31), 0.15, 4, 3),
    "bip1": (_bipartite, (0, 23, 24, 40, 43), 0.15, 1, 50),
    "chain": (_chain, (0, 5, 47, 20, 30), 0.15, 4, 10),
    "random": (_random_directed, (0, 17, 3, 39, 21, 12, 26, 41), 0.3, 10, 10),
    "hub": (_hub, (HUB, 0, 300, 77, 200), 0.15, 4, 10),
    "stars": (_stars, (0, 17, 3, 12, 20), 0.15, 10, 4),
}
NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    """(edge_index int64[2, E], edge_weights fp32[E], sources tuple, alpha, sweeps, k) -- made once, shared, read-only"""
    make, sources, alpha, sweeps, k = CASES[name]
    ei, ew = make()
    ei.setflags(write=False)
    ew.setflags(write=False)
    return ei, ew, sources, alpha, sweeps, k


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(GOLDEN)


def num_nodes(name):
    return int(case(name)[0].max()) + 1


def size_of(name, sources=None):
    """the reference sizes its vectors max(V, max(nodes) + 1) (utils/random_walk.py:159)"""
    return max(num_nodes(name), max(case(name)[2] if sources is None else sources) + 1)


@functools.lru_cache(maxsize=None)
def adjacency(name):
    """adj[v] = [(t, w), ...] in edge-column order, w the fp32 weight as a python float (utils/random_walk.py:39-50)"""
    ei, ew = case(name)[:2]
    adj = [[] for _ in range(num_nodes(name))]
    for e in range(ei.shape[1]):
        adj[int(ei[0, e])].append((int(ei[1, e]), float(ew[e])))
    return adj


def shares(adj):
    """share[v][j] = w_j / sum(row v), python's left-to-right sum()"""
    out = []
    for row in adj:
        total = 0.0
        for _, w in row:
            total = total + w
        out.append([w / total for _, w in row])
    return out


def reference_scores(adj, size, source, alpha, sweeps):
    """the reference's loop, restated"""
    score = [0.0] * size
    mass = [0.0] * size
    score[source] = mass[source] = 1.0
    for _ in range(sweeps):
        for v in range(size):
            m = mass[v]                                   # the live value: pushes of this sweep from lower ids are in it
            if m > 0:
                score[v] += alpha * m
                row = adj[v] if v < len(adj) else []
                if row:
                    out = (1 - alpha) * m
                    total = 0.0
                    for _, w in row:
                        total = total + w
                    for t, w in row:
                        mass[t] += out * (w / total)
                mass[v] = 0.0
    return score


def in_edges(adj, size):
    """inn[v] = [(u, share)] over the edges u -> v, u ascending, multi-edges in adjacency order (self-loops included)"""
    sh = shares(adj)
    inn = [[] for _ in range(size)]
    for u, row in enumerate(adj):
        for j, (t, _) in enumerate(row):
            inn[t].append((u, sh[u][j]))
    return inn


def levels(adj, size):
    """level(v) = 1 + max level(u) over the in-neighbours u < v, 0 without any"""
    inn = in_edges(adj, size)
    lev = [0] * size
    for v in range(size):
        for u, _ in inn[v]:
            if u < v:
                lev[v] = max(lev[v], lev[u] + 1)
    return lev


def pull_scores(adj, size, source, alpha, sweeps, variant=None):
    """the kernel's arithmetic: one pull pass per level, every (node, source) sum on its own.  `variant` names one of the
    mistakes the cases have to tell apart: 'jacobi' (no same-sweep visibility), 'lower_first' (u < v added before u > v),
    'descending' (sources descending within each part), 'keep_self' (a self-loop's mass survives the reset)."""
    inn = in_edges(adj, size)
    lev = levels(adj, size)
    order = sorted(range(size), key=lambda v: lev[v])                      # stable: ascending id within a level
    score = [0.0] * size
    score[source] = 1.0
    c_prev = [0.0] * size
    for k in range(sweeps):
        c_cur = [0.0] * size
        for v in order:
            upper = [(u, s) for u, s in inn[v] if u > v]
            lower = [(u, s) for u, s in inn[v] if u < v]
            if variant == "descending":
                upper, lower = upper[::-1], lower[::-1]
            parts = [(upper, c_prev), (lower, c_prev if variant == "jacobi" else c_cur)]
            if variant == "keep_self":
                parts.insert(1, ([(u, s) for u, s in inn[v] if u == v], c_prev))
            if variant == "lower_first":
                parts = parts[::-1]
            m = 1.0 if (k == 0 and v == source) else 0.0
            for edges, c in parts:
                for u, s in edges:
                    m = m + c[u] * s
            if m > 0:
                score[v] += alpha * m
                c_cur[v] = (1 - alpha) * m
        c_prev = c_cur
    return score


VARIANTS = ("jacobi", "lower_first", "descending", "keep_self")


def select(score, k, max_target=None):
    """precompute_top_neighbors' cut of one score vector (utils/random_walk.py:213-227): the k best positive targets, a stable
    descending sort over the ascending-target list (ties to the smaller id), weights = score / left-to-right sum in rank order"""
    n = len(score) if max_target is None else min(len(score), max_target)
    ranked = sorted(((t, float(score[t])) for t in range(n) if score[t] > 0), key=lambda tv: tv[1], reverse=True)[:k]
    total = 0.0
    for _, v in ranked:
        total = total + v
    return [t for t, _ in ranked], [v / total for _, v in ranked]
