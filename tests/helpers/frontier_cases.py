"""ps_frontier_build (include/pinsage_hip.h, csrc/frontier.hip) and RandomWalkSampler.sample_blocks restated in numpy, the
set definitions both are held to, and the named case table of the family.  No device, no package import.

restate          (frontier, local) of the header's contract, vectorised: unique + searchsorted
brute            the same from the set definition, slot by slot, with python sets and dicts
CASES            name -> (seeds int32[S], ids int32[B, T], nvalid int32[B], T, limit)
restate_blocks   sample_blocks over GIVEN full-catalogue neighbour tables (row r of layer i's table = node r's list)
khop_sets        the K-hop definition the blocks are held to: the node set of every level, as python sets"""
import numpy as np

SCAN_BLOCK_IDS = 32768           # ids per scan block of csrc/frontier.hip: FR_BLOCK_WORDS = 1024 words of 32 bits
WORKGROUP = 256                  # threads, = slots, per workgroup of its mark and relabel passes


def kept_mask(ids, nvalid, T, limit):
    """slot (i, j) is kept iff j < min(nvalid[i], T) and 0 <= ids[i, j] < limit; a negative nvalid[i] means 0"""
    ids = np.asarray(ids, np.int64).reshape(-1, T)
    k = np.clip(np.asarray(nvalid, np.int64).reshape(-1), 0, T)
    return (np.arange(T)[None, :] < k[:, None]) & (ids >= 0) & (ids < limit)


def restate(seeds, ids, nvalid, T, limit):
    """-> (frontier int32[S + n], local int32[B, T]): the seeds in the given order, then every kept id that is not a seed, once,
    ascending; local = the position of a kept slot's id in frontier, -1 elsewhere"""
    seeds = np.asarray(seeds, np.int32).reshape(-1)
    ids = np.asarray(ids, np.int32).reshape(-1, T)
    keep = kept_mask(ids, nvalid, T, limit)
    distinct = np.unique(ids[keep])
    frontier = np.concatenate([seeds, distinct[~np.isin(distinct, seeds)]]).astype(np.int32)
    local = np.full(ids.shape, -1, np.int32)
    if keep.any():
        order = np.argsort(frontier, kind="stable")
        local[keep] = order[np.searchsorted(frontier[order], ids[keep])]
    return frontier, local


def brute(seeds, ids, nvalid, T, limit):
    """the set definition, one slot at a time"""
    seeds = [int(s) for s in np.asarray(seeds).reshape(-1)]
    ids = np.asarray(ids).reshape(-1, T)
    nvalid = np.asarray(nvalid).reshape(-1)
    kept = []
    for i in range(ids.shape[0]):
        for j in range(T):
            v = int(ids[i, j])
            if j < nvalid[i] and 0 <= v < limit:
                kept.append((i, j, v))
    frontier = seeds + sorted({v for _, _, v in kept} - set(seeds))
    where = {v: p for p, v in enumerate(frontier)}
    local = np.full(ids.shape, -1, np.int32)
    for i, j, v in kept:
        local[i, j] = where[v]
    return np.asarray(frontier, np.int32), local


def _case(seeds, ids, nvalid, limit, T=None):
    ids = np.asarray(ids, np.int32)
    T = ids.shape[1] if T is None else T
    ids = np.ascontiguousarray(ids.reshape(-1, T))
    return (np.asarray(seeds, np.int32).reshape(-1), ids, np.asarray(nvalid, np.int32).reshape(-1), T, int(limit))


def _random(seed, S, B, T, limit, lo=-3, hi=None):
    """distinct random seeds in [0, limit), ids in [lo, hi) (default: a few below 0 and a few at or above limit), nvalid in [0, T]"""
    rs = np.random.RandomState(seed)
    hi = limit + 3 if hi is None else hi
    return _case(rs.permutation(limit)[:S], rs.randint(lo, hi, (B, T)), rs.randint(0, T + 1, B), limit)


def _build():
    c = {}
    c["no_seeds"] = _random(1, 0, 7, 4, 50)                                             # S = 0: the sorted distinct kept ids
    c["seeds_only"] = _case([9, 2, 30, 0, 17], np.zeros((0, 3), np.int32), [], 40)       # B = 0 with S > 0
    c["limit_1"] = _case([], [[0, 1], [-1, 0], [1, 1]], [2, 2, 2], 1)
    c["limit_1_seed"] = _case([0], [[0, 1], [-1, 0]], [2, 2], 1)
    c["limit_33"] = _case([5], [[31, 32, 33], [32, 0, 31], [33, 34, 5]], [3, 3, 3], 33)  # ids 31 and 32: either side of a word
    c["range_edges"] = _case([50], [[99, 100, -1, -7], [100, 99, 0, 101]], [4, 4], 100)  # limit - 1, limit, -1, -7
    c["T_1"] = _random(2, 3, 9, 1, 20)
    c["T_70"] = _random(3, 4, 5, 70, 400)
    c["B_ne_S"] = _random(4, 9, 4, 3, 60)
    # nvalid negative and above T: 0 and T
    c["nvalid_outside"] = _case([1], [[2, 3, 4], [5, 6, 7], [8, 9, 10], [11, 12, 13]], [-1, 7, -2 ** 31, 2 ** 31 - 1], 20)
    # slots beyond nvalid hold in-range ids (40 .. 45) that occur nowhere else: they must not enter the frontier
    c["beyond_nvalid"] = _case([0, 7], [[3, 40, 41], [4, 5, 42], [43, 44, 45], [6, 3, 4]], [1, 2, 0, 3], 60)
    # every slot dropped: pads, ids outside the range, rows with nvalid 0
    c["all_dropped"] = _case([4, 2], [[-1, 30, 31], [5, 6, 7], [30, -1, -1]], [3, 0, 1], 30)
    c["no_seeds_all_dropped"] = _case([], [[-1, 30], [5, 6]], [2, 0], 30)
    # a seed's own id among the neighbours (its own row and another's), seeds not in ascending order
    c["seed_among_neighbours"] = _case([12, 3, 8], [[12, 3, 20], [8, 8, 1], [3, 19, 12]], [3, 3, 3], 25)
    # one id in about 5 000 slots: every atomic of the mark pass lands on one word
    hot = np.full((500, 10), 17, np.int32)
    hot[::50, 3] = np.arange(10) + 100
    c["hot_id"] = _case([200, 17], hot, np.full(500, 10), 256)
    # B * T = 3 000 slots: twelve workgroups of the mark and relabel passes, the last one ragged
    c["many_workgroups"] = _random(5, 29, 300, 10, 5000)
    assert 300 * 10 > 11 * WORKGROUP and (29 + 300 * 10) % WORKGROUP != 0
    # a limit of three scan blocks (32 768 ids each, the last one ragged); kept ids only in the first and the last, the seeds too
    limit = 2 * SCAN_BLOCK_IDS + 77
    rs = np.random.RandomState(6)
    ids = np.where(rs.randint(0, 2, (40, 6)) == 0, rs.randint(0, SCAN_BLOCK_IDS, (40, 6)), rs.randint(2 * SCAN_BLOCK_IDS, limit, (40, 6)))
    ids[0, :4] = [0, SCAN_BLOCK_IDS - 1, 2 * SCAN_BLOCK_IDS, limit - 1]
    c["three_scan_blocks"] = _case([limit - 2, 5, SCAN_BLOCK_IDS - 2], ids, np.full(40, 6), limit)
    return c


CASES = _build()


# ---- sample_blocks ------------------------------------------------------------------------------------------------------------
def restate_blocks(seeds, tables, n_items):
    """sample_blocks over given tables.  tables[i] = (ids [N, T], nvalid [N], payload [N, T]): layer i's neighbour list of EVERY
    node r in row r (what sample_batches(range(N), T, layers)[i] holds; payload = its counts or weights).
    -> (input_nodes, inverse, blocks): blocks[i] = dict(src_nodes, n_dst, ids (local), nvalid, payload), blocks[0] the widest."""
    seeds = np.asarray(seeds, np.int64).reshape(-1)
    if seeds.size == 0 or seeds.min() < 0 or seeds.max() >= n_items:
        raise ValueError("seeds must be item ids in [0, n_items)")
    nodes, inverse = np.unique(seeds, return_inverse=True)
    nodes = nodes.astype(np.int32)
    blocks = [None] * len(tables)
    for i in range(len(tables) - 1, -1, -1):
        ids, nvalid, payload = (np.asarray(t) for t in tables[i])
        T = ids.shape[1]
        src, local = restate(nodes, ids[nodes], nvalid[nodes], T, n_items)
        blocks[i] = dict(src_nodes=src, n_dst=len(nodes), ids=local, nvalid=nvalid[nodes].astype(np.int32), payload=payload[nodes])
        nodes = src
    return blocks[0]["src_nodes"], inverse.astype(np.int64).reshape(-1), blocks


def khop_sets(seeds, tables, n_items):
    """level[k] for k = layers .. 0 as python sets: level[layers] = the seeds, level[i] = level[i + 1] and the kept neighbours
    (layer i's lists, ids below n_items) of its members"""
    level = {len(tables): {int(s) for s in np.asarray(seeds).reshape(-1)}}
    for i in range(len(tables) - 1, -1, -1):
        ids, nvalid, _ = tables[i]
        T = ids.shape[1]
        out = set(level[i + 1])
        for r in level[i + 1]:
            out |= {int(v) for j, v in enumerate(ids[r]) if j < min(max(int(nvalid[r]), 0), T) and 0 <= v < n_items}
        level[i] = out
    return level
