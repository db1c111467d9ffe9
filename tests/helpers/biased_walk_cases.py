"""Node2vec-biased walks (csrc/walk_biased.hip), numpy only: the restatement everything is held to, the case graph, planted uniforms.

The restatement is the reference's `_single_walk` / `sample_neighbors` loop (utils/random_walk.py:52-117) with ONE change: on every
step that has a previous node t, the row's weights are multiplied elementwise by alpha before `probabilities = weights /
weights.sum()` -- alpha[e] of the edge v -> x is 1/p if x == t, 1.0 if t has an out-edge to x, 1/q otherwise (x == t first;
parallel edges judged by their destination).  1/p and 1/q arrive as python floats (`inv_p`, `inv_q`).  The draw is
`np.random.choice(dest, p=probs)` on the global stream, so numpy itself supplies the sum, the cumsum, the division by cdf[-1] and
the searchsorted.  `plain_single_walk` is the reference's loop without the change.

`plant` walks paths with uniforms computed FROM the biased CDF of the row a walk stands on, given where it came from: an exact
tie u == cdf'[e], its two fp64 neighbours, 0.0 and 1 - 2^-53 (the kinds of tests/helpers/walk_cases.py, applied to biased rows).
The expected step is np.searchsorted(cdf', u, 'right') and nothing else."""
from collections import Counter

import numpy as np

U_MAX = 1.0 - 2.0 ** -53                  # the largest double random_sample() returns
DEGREES = (1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 257, 300)     # numpy's pairwise-sum boundaries and the 64-lane chunk boundaries
BIASES = ((0.25, 4.0), (4.0, 0.25), (1.0, 2.0), (2.0, 1.0), (0.5, 0.5))       # (p, q)
KINDS = ("tie", "tie_dn", "tie_up", "zero", "umax", "random")
TIE_KINDS = ("tie", "tie_dn", "tie_up")


# ------------------------------------------------------------------------------------------------------------ restatement

def out_sets(adj_list):
    """per node, the set of destinations of its out-edges"""
    return [set(d for d, _ in row) for row in adj_list]


def alpha_row(destinations, t, outs, inv_p, inv_q):
    """alpha of every edge of a row, for a walk that came from t"""
    return np.array([inv_p if x == t else (1.0 if x in outs[t] else inv_q) for x in destinations])


def alpha_classes(destinations, t, outs):
    """0 = back to t, 1 = t has an out-edge to it, 2 = neither, per edge"""
    return np.array([0 if x == t else (1 if x in outs[t] else 2) for x in destinations])


def biased_weights(adj_list, outs, v, t, inv_p, inv_q):
    """(destinations, weights * alpha) of row v for a walk that came from t (t None: the first step, plain weights)"""
    neighbors = adj_list[v]
    destinations = [n[0] for n in neighbors]
    weights = np.array([n[1] for n in neighbors])
    if t is not None:
        weights = weights * alpha_row(destinations, t, outs, inv_p, inv_q)
    return destinations, weights


def choice_cdf(weights):
    """the CDF np.random.choice(dest, p=weights / weights.sum()) searches: cumsum(p), divided by its last entry"""
    cdf = (weights / weights.sum()).cumsum()
    cdf /= cdf[-1]
    return cdf


def single_walk(adj_list, start, L, inv_p=1.0, inv_q=1.0, outs=None):
    """the reference's _single_walk with the alpha multiplication; draws from the global np.random stream"""
    outs = out_sets(adj_list) if outs is None else outs
    walk = [start]
    current_node, previous = start, None
    for _ in range(L):
        neighbors = adj_list[current_node]
        if not neighbors:
            break
        destinations = [neighbor[0] for neighbor in neighbors]
        weights = np.array([neighbor[1] for neighbor in neighbors])
        if previous is not None:
            weights = weights * alpha_row(destinations, previous, outs, inv_p, inv_q)
        probabilities = weights / weights.sum()
        next_node = np.random.choice(destinations, p=probabilities)
        walk.append(next_node)
        previous, current_node = current_node, next_node
    return walk


def plain_single_walk(adj_list, start, L):
    """the reference's _single_walk (utils/random_walk.py:52-83), restated"""
    walk = [start]
    current_node = start
    for _ in range(L):
        neighbors = adj_list[current_node]
        if not neighbors:
            break
        destinations = [neighbor[0] for neighbor in neighbors]
        weights = np.array([neighbor[1] for neighbor in neighbors])
        probabilities = weights / weights.sum()
        next_node = np.random.choice(destinations, p=probabilities)
        walk.append(next_node)
        current_node = next_node
    return walk


def rank_visits(walks):
    """[(node, count)] by count descending, ties in first-visit order (Counter insertion order under a stable sort)"""
    visit_counts = Counter()
    for walk in walks:
        for node in walk[1:]:
            visit_counts[node] += 1
    return sorted(visit_counts.items(), key=lambda x: x[1], reverse=True)


def sample_neighbors(adj_list, node, num_neighbors, W, L, inv_p=1.0, inv_q=1.0, outs=None):
    """the reference's sample_neighbors (utils/random_walk.py:85-117) over the biased single_walk"""
    outs = out_sets(adj_list) if outs is None else outs
    walks = [single_walk(adj_list, node, L, inv_p, inv_q, outs) for _ in range(W)]
    top = rank_visits(walks)[:num_neighbors]
    if not top:
        return [], []
    neighbors, counts = zip(*top)
    total = sum(counts)
    return list(neighbors), [c / total for c in counts]


def hard_negatives(adj_list, num_movies, queries, L, inv_p, inv_q, num_hard_samples, max_rank, min_rank):
    """the reference's sample_hard_negatives (data/negative_sampler.py:44-99) over the biased single_walk -> int array"""
    outs = out_sets(adj_list)
    all_movie_indices = list(range(num_movies))
    hard = []
    for idx in queries:
        ranked = rank_visits([single_walk(adj_list, int(idx), L, inv_p, inv_q, outs) for _ in range(100)])
        candidates = [item for item, _ in ranked[min_rank:max_rank] if item in all_movie_indices]
        if not candidates:
            sampled = np.random.choice(all_movie_indices, size=num_hard_samples, replace=False)
        else:
            sampled = np.random.choice(candidates, size=min(num_hard_samples, len(candidates)), replace=False)
            if len(sampled) < num_hard_samples:
                additional = np.random.choice([i for i in all_movie_indices if i not in sampled],
                                              size=num_hard_samples - len(sampled), replace=False)
                sampled = np.concatenate([sampled, additional])
        hard.append(sampled)
    return np.asarray(hard)


# ------------------------------------------------------------------------------------------------------------------ graph

def _ratings(rs, n):
    return rs.randint(1, 11, size=n).astype(np.float32) * np.float32(0.5)


N_ORDINARY = 280
REPEATS = 2                               # nodes per degree of DEGREES


def build_case_graph(seed=0, sinks=False):
    """(edge_index int64[2, E], weights fp32[E], V, info): directed, not bipartite, every node with out-edges (sinks=False).
    Nodes 0 .. len(DEGREES) * REPEATS - 1 are the class nodes (info['class'][d] = the nodes of out-degree d); the rest are ordinary
    nodes of 3 .. 40 edges.  Destinations are drawn with replacement (parallel edges; the long rows hold many), half of an ordinary
    node's towards the class nodes, so walks stand on them.  Constructed: info['returner'] = (r, t): r's ONLY out-edge goes to t
    and t has an edge to r; info['self_loop'] = a node with an edge to itself; info['parallel'] = (a, b): a has two edges to b.
    The edge list is shuffled: a row's order is the order of its edges in edge_index (the CSR build is stable).
    sinks=True: the ordinary nodes whose id is 0 mod 4 lose their out-edges (a graph with reachable sinks)."""
    rs = np.random.RandomState(seed)
    nclass = len(DEGREES) * REPEATS
    V = nclass + N_ORDINARY
    deg = np.concatenate([np.repeat(DEGREES, REPEATS), rs.randint(3, 41, size=N_ORDINARY)])
    classes = {d: [int(v) for v in np.flatnonzero(deg[:nclass] == d)] for d in DEGREES}
    src, dst = [], []
    for v in range(V):
        d = int(deg[v])
        to_class = rs.random_sample(d) < (0.5 if v >= nclass else 0.2)
        t = np.where(to_class, rs.randint(0, nclass, size=d), rs.randint(0, V, size=d))
        src.append(np.full(d, v, dtype=np.int64))
        dst.append(t.astype(np.int64))
    # the node whose only out-edge returns to its predecessor: the first node of degree 1 and an ordinary feeder
    r, feeder = classes[1][0], nclass + 1
    dst[r][0] = feeder
    dst[feeder][:-1] = r                  # (all but one of the feeder's edges: its walks do go there)
    loop = nclass + 2
    dst[loop][1] = loop
    a, b = nclass + 3, nclass + 5
    dst[a][0] = dst[a][2] = b
    src, dst = np.concatenate(src), np.concatenate(dst)
    w = _ratings(rs, src.size)
    order = rs.permutation(src.size)
    src, dst, w = src[order], dst[order], w[order]
    info = {"class": classes, "returner": (r, feeder), "self_loop": loop, "parallel": (a, b), "nclass": nclass}
    if sinks:
        sink = np.arange(nclass, V)[np.arange(nclass, V) % 4 == 0]
        keep = ~np.isin(src, sink)
        src, dst, w = src[keep], dst[keep], w[keep]
        info["sink"] = sink
    return np.stack([src, dst]), w, V, info


def adjacency(edge_index, weights, V):
    """the reference's adj_list (utils/random_walk.py:39-50): per node [(dst, python float of the fp32 weight)] in edge order"""
    adj = [[] for _ in range(V)]
    for s, d, x in zip(edge_index[0].tolist(), edge_index[1].tolist(), np.asarray(weights, dtype=np.float32).tolist()):
        adj[s].append((d, x))
    return adj


_cache = {}


def case_graph(sinks=False):
    """(edge_index, weights, V, info, adj_list, out_sets) of the case graph, built once per process"""
    if sinks not in _cache:
        ei, w, V, info = build_case_graph(0, sinks=sinks)
        adj = adjacency(ei, w, V)
        _cache[sinks] = (ei, w, V, info, adj, out_sets(adj))
    return _cache[sinks]


# --------------------------------------------------------------------------------------------------------------- planting

class Planted:
    """starts int64[B]; uniforms fp64[B * L] (walk i, step s at i * L + s); picks int64[B, L]; per step of a walk: row (the node
    stood on), prev (-1 at step 0), kind (-1 at step 0, whose uniform is random), deg"""


def plant(adj_list, outs, starts, L, inv_p, inv_q, seed=0, tail_edges=0):
    """One walk of L steps per entry of `starts` on a graph without sinks.  Step 0 draws a seeded random uniform over the row's own
    CDF.  Every later step stands on a known row with a known previous node: it picks a target edge e of the row (seeded), a kind
    (seeded, uniform over KINDS), computes u from the biased CDF cdf' of the row -- tie: cdf'[e], tie_dn / tie_up: its fp64
    neighbours, zero: 0.0, umax: 1 - 2^-53, random: seeded -- and takes np.searchsorted(cdf', u, 'right').  A u outside
    [0, 1 - 2^-53] becomes tie_dn of the same edge, then zero.  tail_edges > 0: a third of the planted steps take their target among
    the last tail_edges edges of the row, half of those among its last two (the end of a long row: its last chunks of 64, its last buffer of 8192)."""
    rs = np.random.RandomState(seed)
    starts = np.asarray(starts, dtype=np.int64)
    B = starts.size
    p = Planted()
    p.starts = starts
    p.uniforms = np.full(B * L, 0.5)
    p.picks = np.full((B, L), -1, dtype=np.int64)
    p.row = np.full((B, L), -1, dtype=np.int64)
    p.prev = np.full((B, L), -1, dtype=np.int64)
    p.kind = np.full((B, L), -1, dtype=np.int64)
    p.deg = np.zeros((B, L), dtype=np.int64)
    p.target = np.full((B, L), -1, dtype=np.int64)            # the target edge's position in its row
    for i in range(B):
        cur, prev = int(starts[i]), None
        for st in range(L):
            dest, wts = biased_weights(adj_list, outs, cur, prev, inv_p, inv_q)
            cdf = choice_cdf(wts)
            r = rs.random_sample()
            if prev is None:
                u, kind = r, -1
            else:
                e = int(rs.randint(0, len(dest)))
                if tail_edges and rs.randint(0, 3) == 2:
                    e = len(dest) - 1 - int(rs.randint(0, min(tail_edges if rs.randint(0, 2) else 2, len(dest))))
                kind = int(rs.randint(0, len(KINDS)))
                c = cdf[e]
                u = (c, np.nextafter(c, -1.0), np.nextafter(c, 2.0), 0.0, U_MAX, r)[kind]
                if not (0.0 <= u <= U_MAX):
                    u, kind = np.nextafter(c, -1.0), KINDS.index("tie_dn")
                if not (0.0 <= u <= U_MAX):
                    u, kind = 0.0, KINDS.index("zero")
            k = min(int(np.searchsorted(cdf, u, side="right")), len(dest) - 1)
            p.uniforms[i * L + st] = u
            p.row[i, st], p.prev[i, st], p.kind[i, st], p.deg[i, st] = cur, -1 if prev is None else prev, kind, len(dest)
            p.picks[i, st] = dest[k]
            p.target[i, st] = -1 if prev is None else e
            prev, cur = cur, dest[k]
    return p


PLANT_REPEATS, PLANT_L = 6, 3             # every node starts PLANT_REPEATS one-walk paths of PLANT_L steps


def planted_paths(p, q):
    """the Planted batch of the case graph for (p, q), built once per process: every node starts PLANT_REPEATS paths"""
    key = ("plant", p, q)
    if key not in _cache:
        _, _, V, _, adj, outs = case_graph()
        starts = np.repeat(np.arange(V), PLANT_REPEATS)
        _cache[key] = plant(adj, outs, starts, PLANT_L, 1.0 / p, 1.0 / q, seed=int(p * 100 + q * 10))
    return _cache[key]


# ------------------------------------------------------------------------------------------------ given uniforms, given paths

def replay_walk(adj_list, outs, start, L, uniforms, pos, inv_p, inv_q):
    """the biased walk over GIVEN uniforms (step s taken reads uniforms[pos + s]) -> int32[L], -1 once the walk has stopped: a
    start outside the graph or a node without out-edges.  The pick is np.searchsorted(choice_cdf, u, 'right')."""
    out = np.full(L, -1, dtype=np.int32)
    if not 0 <= start < len(adj_list):
        return out
    cur, prev = int(start), None
    for st in range(L):
        if not adj_list[cur]:
            break
        dest, wts = biased_weights(adj_list, outs, cur, prev, inv_p, inv_q)
        k = min(int(np.searchsorted(choice_cdf(wts), uniforms[pos + st], side="right")), len(dest) - 1)
        out[st] = dest[k]
        prev, cur = cur, dest[k]
    return out


def topk_from_paths(paths, T):
    """(ids int32[B, T] -1 pad, counts int32[B, T] 0 pad, nvalid int32[B]) of paths int[B, n]: the entries >= 0 of a row by visit
    count, descending, ties in first-visit order (python's stable sorted(Counter.items(), reverse=True)[:T])"""
    B = paths.shape[0]
    ids = np.full((B, T), -1, dtype=np.int32)
    counts = np.zeros((B, T), dtype=np.int32)
    nvalid = np.zeros(B, dtype=np.int32)
    for i in range(B):
        top = rank_visits([[None] + [int(v) for v in paths[i] if v >= 0]])[:T]
        for j, (v, c) in enumerate(top):
            ids[i, j], counts[i, j] = v, c
        nvalid[i] = len(top)
    return ids, counts, nvalid


def host_csr(edge_index, weights, V):
    """(rowptr int64[V + 1], col int32[E], wsorted fp64[E], cdf fp64[E], nbr_sorted int32[E]) as the device graph holds them:
    rows in edge order (stable by source), the CDF np.random.choice searches on the plain row, destinations sorted per row"""
    src, dst = edge_index
    order = np.argsort(src, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=V))]).astype(np.int64)
    col = dst[order].astype(np.int32)
    wsorted = np.asarray(weights, dtype=np.float32)[order].astype(np.float64)
    cdf = np.empty_like(wsorted)
    nbr = np.empty_like(col)
    for v in range(V):
        lo, hi = rowptr[v], rowptr[v + 1]
        if hi > lo:
            cdf[lo:hi] = choice_cdf(wsorted[lo:hi])
            nbr[lo:hi] = np.sort(col[lo:hi])
    return rowptr, col, wsorted, cdf, nbr


# ------------------------------------------------------------------------------------------------------------- long rows
# The kernel (csrc/walk_biased.hip) treats a row by its length: up to WB_CAP = 1024 edges the products w * alpha stay in LDS,
# longer rows recompute them in every pass; beyond 8192 edges numpy's sum takes a second ufunc buffer; beyond CEND_CAP = 128
# chunks of 64 (8192 edges) the chain is replayed past the kept accumulators.  A row on either side of each threshold:
LONG_DEGREES = (1023, 1024, 1025, 8191, 8192, 8193, 8300)
N_FEEDERS = 56
LONG_TAIL = 120                           # planted targets among the last edges: beyond edge 8192 in the rows of 8193 and 8300
LONG_REPEATS, LONG_L = 16, 3


def build_long_graph(seed=0):
    """(edge_index, weights fp32, V, info): nodes 0 .. 6 are the hubs (info['hub'][d] = the node of out-degree d, destinations
    drawn with replacement over all nodes: parallel edges throughout), the rest feeders of 4 .. 12 edges, three in four of
    them to hubs, so a walk from a feeder stands on a hub with a previous node from its second step on -- a feeder, or another
    hub, whose long sorted row the membership search then runs over.  No sinks; the edge list is shuffled."""
    rs = np.random.RandomState(seed)
    nh = len(LONG_DEGREES)
    V = nh + N_FEEDERS
    deg = np.concatenate([LONG_DEGREES, rs.randint(4, 13, size=N_FEEDERS)])
    src, dst = [], []
    for v in range(V):
        d = int(deg[v])
        to_hub = rs.random_sample(d) < (0.75 if v >= nh else 0.02)
        src.append(np.full(d, v, dtype=np.int64))
        dst.append(np.where(to_hub, rs.randint(0, nh, size=d), rs.randint(0, V, size=d)).astype(np.int64))
    src, dst = np.concatenate(src), np.concatenate(dst)
    w = _ratings(rs, src.size)
    order = rs.permutation(src.size)
    return np.stack([src[order], dst[order]]), w[order], V, {"hub": {d: i for i, d in enumerate(LONG_DEGREES)}, "nhub": nh}


def long_graph():
    """(edge_index, weights, V, info, adj_list, out_sets) of the long-row graph, built once per process"""
    if "long" not in _cache:
        ei, w, V, info = build_long_graph(0)
        adj = adjacency(ei, w, V)
        _cache["long"] = (ei, w, V, info, adj, out_sets(adj))
    return _cache["long"]


def long_starts():
    """every feeder LONG_REPEATS times, every hub twice"""
    _, _, V, info = long_graph()[:4]
    return np.concatenate([np.repeat(np.arange(info["nhub"], V), LONG_REPEATS), np.repeat(np.arange(info["nhub"]), 2)]).astype(np.int64)


def planted_long_paths(p, q):
    """the Planted batch of the long-row graph for (p, q), built once per process"""
    key = ("plant-long", p, q)
    if key not in _cache:
        adj, outs = long_graph()[4:]
        _cache[key] = plant(adj, outs, long_starts(), LONG_L, 1.0 / p, 1.0 / q, seed=int(p * 100 + q * 10) + 1, tail_edges=LONG_TAIL)
    return _cache[key]
