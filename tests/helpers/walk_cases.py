"""Planted uniforms for the walk sampler's CDF search (csrc/walk_sample.hip), numpy only.

Random uniforms almost never reach the branches of the search where an off-by-one would live: an exact tie u == cdf[e], the
fp32 sliver of the half records, the fourth / fifth candidate of a bucket record, the switch from forward scan to bisection,
the single load at slot 7 of a packed block.  This module builds a small graph whose rows hold those situations, walks every
path with uniforms computed FROM the row the walk stands on (`plant`), and classifies every planted step into the branch
each search form must take (`classify`).  The expected visit of every step is np.searchsorted(cdf[lo:hi], u, 'right') and
nothing else; the classification restates the kernels' control flow from the record definitions (guide position, candidates,
fp32 round-down) and is used only to prove coverage, never to compute an expected value."""
import numpy as np

LIN_PROBES = 12                           # walk_sample.hip: forward-scan entries before the search bisects
GUIDE_SHRINK = 1.0 - 2.0 ** -50           # guide_build_kernel: t = (j / deg) * (1 - 2^-50)
U_MAX = 1.0 - 2.0 ** -53                  # the largest double random_sample() returns
# Which start rows walk_sample_launch stages in LDS (step 0 is then searched there, not through a record).  Its arithmetic: np = the
# power of two with np * 64 >= W * L; hash table 3 * 2^h words with 2^h * 4 >= 5 * W * L (h >= 6); bitmap 40 words;
# region = max(1664 - rounds * np * 64 - 40, hash words) & ~31 words; stage_blocks = region / 32, or / 48 with destination
# records (dropped for np > 4).  (100, 2): np 4, hash 768, region 1344 -> 42 blocks, 28 with destination records; two fused
# rounds: region 1088 -> 34 / 22; (192, 3): np 16, hash 3072 = region -> 96; (1, 1): np 1, region 1536 -> 48 / 32.  A row of d
# edges spans at most (d + 6) / 8 + 1 blocks: 9 for d <= 64, never more than the smallest bound (22); a row of >= 4000 edges
# spans >= 500, more than the largest (96).  Rows in between would make the split depend on the launch: the graph has none
# (asserted in tests/test_walk_cases.py), and STAGE_BLOCKS_RANGE is checked against these figures there.
STAGED_MAX_DEG = 64                       # start rows up to this degree are searched in LDS in every (W, L) used here
HUB_MIN_DEG = 4000                        # start rows from this degree on are never staged


def stage_blocks(W, L, rounds=1, dest=False):
    """walk_sample_launch's bound on the 128-byte blocks of a staged start row (the arithmetic above)"""
    P = W * L
    np_ = 1
    while np_ * 64 < P:
        np_ <<= 1
    h = 6
    while (1 << h) * 4 < 5 * P:
        h += 1
    region = max(6656 // 4 - rounds * np_ * 64 - (40 if P <= 1024 else ((P >> 5) + 8) & ~7), 3 * (1 << h)) & ~31
    return region // (48 if dest and np_ <= 4 else 32)

KINDS = ("tie", "tie_dn", "tie_up", "sliver_lo", "sliver_hi", "sliver_in_lo", "sliver_in_hi",
         "bucket", "bucket_m1", "bucket_p1", "bucket_m2", "bucket_p2", "bucket_s50", "bucket_s53",
         "zero", "tiny", "umax", "random")
K = {name: i for i, name in enumerate(KINDS)}
KIND_STRIDE = 7                           # kinds go round-robin over the walks: coprime to 64, and 64 * 7 is no multiple of len(KINDS)
TIE_KINDS = ("tie", "tie_dn", "tie_up")


def round_down_f32(c):
    """the nearest fp32 at or below c >= 0 (bucket_half_build_kernel)"""
    c = np.asarray(c, dtype=np.float64)
    f = c.astype(np.float32)
    return np.where(f.astype(np.float64) > c, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def next_f32(f):
    return np.nextafter(np.asarray(f, dtype=np.float32), np.float32(np.inf))


# ------------------------------------------------------------------------------------------------------------------ graph

def _ratings(rs, n):
    return rs.randint(1, 11, size=n).astype(np.float32) * np.float32(0.5)


def _cluster_row(rs, deg, n, at):
    """ratings with a run of n weights 10^-7 of the others from position `at` on: n CDF entries inside one 1/deg bucket"""
    w = _ratings(rs, deg)
    w[at:at + n] = np.float32(2e-7)
    return w


CLUSTERS = (3, 4, 5, 6, 11, 12, 13, 14, 40)
BOUNDARY_DEGREES = (7, 8, 9, 15, 16, 17)


def build_case_graph(seed=0, sinks=False):
    """(edge_index int64[2, E], weights fp32[E], V, info).  Every row is listed in CSR order (the CSR build is stable), every node
    has out-edges.  info: 'special' = ids of the constructed rows, 'boundary' = ids of the rows of degree 7 / 8 / 9 / 15 / 16 / 17,
    'hubs', 'zero', 'cluster', 'tiny' likewise.  sinks=True: the same graph with the out-edges of every ordinary node whose id
    is 0 mod 4 removed (a directed graph with reachable sinks)."""
    rs = np.random.RandomState(seed)
    rows, tag = [], []

    def add(w, t):
        rows.append(np.asarray(w, dtype=np.float32))
        tag.append(t)

    n_ord = 1200
    specials = []
    for rep in range(12):
        for d in BOUNDARY_DEGREES:
            specials.append((_ratings(rs, d), "boundary"))
        specials.append((_ratings(rs, 1), "deg1"))
        specials.append((_ratings(rs, 2), "deg2"))
    zero_rows = ([0, 0, 1, 2.5], [1, 0, 0, 2], [1, 2, 0, 0], [0, 3, 0, 0, 1.5, 0], [0, 0, 0, 1, 0, 0, 0],
                 [0, 0.5, 1, 0, 0, 0, 0, 0, 2, 0, 0, 4, 0], [0] * 7 + [1, 1] + [0] * 7 + [3.5], [2] + [0] * 15, [0] * 15 + [2])
    for rep in range(4):
        for z in zero_rows:
            specials.append((np.asarray(z, dtype=np.float32), "zero"))
    for rep in range(6):
        for n in CLUSTERS:
            deg = 64 if n == 40 else 40 + n
            at = int(rs.randint(2, deg - n - 2))
            specials.append((_cluster_row(rs, deg, n, at), "cluster"))
        # two clusters in one row, the second one ending the row
        w = _cluster_row(rs, 60, 5, 10)
        w[60 - 13:] = np.float32(2e-7)
        w[-1] = np.float32(3.0)
        specials.append((w, "cluster"))
    for rep in range(3):
        specials.append((np.asarray([1e-30] * 3 + [1e10] * 5, dtype=np.float32), "tiny"))       # CDF entries below the smallest normal fp32
        specials.append((np.asarray([1e10, 1e-30, 1e-30, 1e10, 1e-30], dtype=np.float32), "tiny"))
    for deg in (4096, 5003):
        w = _ratings(rs, deg)
        for n in CLUSTERS:
            at = int(rs.randint(0, deg - 64))
            w[at:at + n] = np.float32(2e-7)
        w[100:104] = 0.0
        specials.append((w, "hub"))
    # ordinary rows and constructed rows interleaved, so that the constructed rows start at every residue mod 8
    order = rs.permutation(n_ord + len(specials))
    for o in order:
        if o < n_ord:
            add(_ratings(rs, int(rs.randint(3, 61))), "ordinary")
        else:
            add(*specials[o - n_ord])
    V = len(rows)
    tag = np.asarray(tag)
    special = np.flatnonzero(tag != "ordinary")
    src, dst, wts = [], [], []
    for v, w in enumerate(rows):
        d = w.size
        to_special = rs.random_sample(d) < 0.5
        t = np.where(to_special, special[rs.randint(0, special.size, size=d)], rs.randint(0, V, size=d))
        src.append(np.full(d, v, dtype=np.int64))
        dst.append(t.astype(np.int64))
        wts.append(w)
    src, dst, wts = np.concatenate(src), np.concatenate(dst), np.concatenate(wts)
    info = {"special": special, "tag": tag}
    for t in ("boundary", "hub", "zero", "cluster", "tiny", "deg1", "deg2", "ordinary"):
        info[t] = np.flatnonzero(tag == t)
    if sinks:
        sink = info["ordinary"][info["ordinary"] % 4 == 0]
        keep = ~np.isin(src, sink)
        src, dst, wts = src[keep], dst[keep], wts[keep]
        info["sink"] = sink
    return np.stack([src, dst]), wts, V, info


def sink_case_starts(info, n_ordinary=24):
    """start nodes of the sink graph's batch: constructed rows of every sort, some ordinary nodes, some sinks (isolated starts)"""
    pick = [info[t][:3] for t in ("boundary", "zero", "cluster", "tiny", "deg1", "deg2")]
    pick.append(info["hub"][:1])
    pick.append(info["ordinary"][:n_ordinary])
    pick.append(info["sink"][:3])
    return np.concatenate(pick).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- planting

def _kind_uniforms(cdf, lo, deg, e, third, r):
    """candidate uniform of every kind for target edge e of row (lo, deg): fp64[len(KINDS), n]"""
    with np.errstate(over="ignore", invalid="ignore"):
        c = cdf[e]
        j = (e - lo).astype(np.float64)
        d = deg.astype(np.float64)
        js = np.choose(third, [np.minimum(1, deg - 1), deg // 2, deg - 1]).astype(np.float64)       # first, a middle, the last bucket
        s_lo = round_down_f32(c)
        s_hi = next_f32(s_lo)
        b = j / d
        out = np.empty((len(KINDS), e.size), dtype=np.float64)
        out[K["tie"]] = c
        out[K["tie_dn"]] = np.nextafter(c, -1.0)
        out[K["tie_up"]] = np.nextafter(c, 2.0)
        out[K["sliver_lo"]] = s_lo.astype(np.float64)
        out[K["sliver_hi"]] = s_hi.astype(np.float64)
        out[K["sliver_in_lo"]] = np.nextafter(s_lo.astype(np.float64), 2.0)
        out[K["sliver_in_hi"]] = np.nextafter(s_hi.astype(np.float64), -1.0)
        out[K["bucket"]] = b
        out[K["bucket_m1"]] = np.nextafter(b, -1.0)
        out[K["bucket_p1"]] = np.nextafter(b, 2.0)
        out[K["bucket_m2"]] = np.nextafter(np.nextafter(b, -1.0), -1.0)
        out[K["bucket_p2"]] = np.nextafter(np.nextafter(b, 2.0), 2.0)
        out[K["bucket_s50"]] = (js / d) * GUIDE_SHRINK
        out[K["bucket_s53"]] = (js / d) * (1.0 - 2.0 ** -53)
        out[K["zero"]] = 0.0
        out[K["tiny"]] = 5e-324
        out[K["umax"]] = U_MAX
        out[K["random"]] = r
    return out


def searchsorted_rows(rowptr, cdf, rows, u):
    """np.searchsorted(cdf[lo:hi], u, side='right') clamped to hi - 1, for every (row, u): absolute edge indices"""
    out = np.empty(rows.size, dtype=np.int64)
    order = np.argsort(rows, kind="stable")
    srt = rows[order]
    cuts = np.flatnonzero(np.diff(srt)) + 1
    for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [srt.size]])):
        lo, hi = int(rowptr[srt[a]]), int(rowptr[srt[a] + 1])
        idx = np.searchsorted(cdf[lo:hi], u[order[a:b]], side="right")
        out[order[a:b]] = lo + np.minimum(idx, hi - lo - 1)
    return out


class Planted:
    """uniforms: fp64 stream; pos / row / edge / pick / kind: [B, W, L] (-1 where the walk had stopped); u: fp64 [B, W, L]"""

    def histogram(self, T):
        """(ids int64[B, T], counts int32[B, T], nvalid int32[B]): visited nodes by visit count, descending, ties in
        first-visit order (python's stable sorted(Counter.items(), reverse=True)[:T])"""
        B = self.pick.shape[0]
        ids = np.full((B, T), -1, dtype=np.int64)
        counts = np.zeros((B, T), dtype=np.int32)
        nvalid = np.zeros(B, dtype=np.int32)
        for i in range(B):
            seq = self.pick[i].reshape(-1)
            seq = seq[seq >= 0]
            if seq.size == 0:
                continue
            uniq, first, cnt = np.unique(seq, return_index=True, return_counts=True)
            o = np.lexsort((first, -cnt))[:T]
            ids[i, :o.size], counts[i, :o.size], nvalid[i] = uniq[o], cnt[o], o.size
        return ids, counts, nvalid


def plant(rowptr, col, cdf, starts, W, L, seed=0, sequential=False, uoff=None):
    """Walk every path and plant its uniforms.  Step (i, w, st) stands on a known row, picks a target edge of it (seeded) and a
    kind (round-robin: (w * KIND_STRIDE + st + i) mod len(KINDS)), computes u, takes np.searchsorted's step.  A kind whose u
    would leave [0, 1 - 2^-53] becomes 'tie_dn' of the same edge, and 'zero' if that leaves it too.
    Layout: sink-free (uoff from Graph.uniform_offsets) step (i, w, st) is uniforms[uoff[i] + w * L + st]; sequential=True
    (graphs with sinks): the steps really taken, in walk order, one after the other."""
    rs = np.random.RandomState(seed)
    starts = np.asarray(starts, dtype=np.int64)
    B = starts.size
    shape = (B, W, L)
    p = Planted()
    p.row = np.full(shape, -1, dtype=np.int64)
    p.edge = np.full(shape, -1, dtype=np.int64)
    p.pick = np.full(shape, -1, dtype=np.int64)
    p.kind = np.full(shape, -1, dtype=np.int64)
    p.u = np.full(shape, np.nan)
    ii, ww = np.meshgrid(np.arange(B), np.arange(W), indexing="ij")
    cur = np.repeat(starts[:, None], W, axis=1)
    alive = np.ones((B, W), dtype=bool)
    for st in range(L):
        lo, hi = rowptr[cur], rowptr[cur + 1]
        alive &= hi > lo
        m = alive
        n = int(m.sum())
        if n == 0:
            break
        lo_, deg = lo[m], (hi - lo)[m]
        e = lo_ + rs.randint(0, 1 << 30, size=n) % deg
        kind = (ww[m] * KIND_STRIDE + st + ii[m]) % len(KINDS)
        cand = _kind_uniforms(cdf, lo_, deg, e, rs.randint(0, 3, size=n), rs.random_sample(n))
        sel = np.arange(n)
        u = cand[kind, sel]
        bad = ~((u >= 0.0) & (u <= U_MAX))
        kind = np.where(bad, K["tie_dn"], kind)
        u = np.where(bad, cand[K["tie_dn"], sel], u)
        bad = ~((u >= 0.0) & (u <= U_MAX))
        kind = np.where(bad, K["zero"], kind)
        u = np.where(bad, 0.0, u)
        a = searchsorted_rows(rowptr, cdf, cur[m], u)
        p.row[:, :, st][m], p.edge[:, :, st][m], p.kind[:, :, st][m], p.u[:, :, st][m] = cur[m], a, kind, u
        nxt = col[a].astype(np.int64)
        p.pick[:, :, st][m] = nxt
        cur[m] = nxt
    taken = p.edge >= 0
    if sequential:
        flat = taken.reshape(-1)
        pos = np.cumsum(flat) - flat
        p.pos = np.where(flat, pos, -1).reshape(shape)
        total = int(flat.sum())
        p.walk_off = p.pos[:, :, 0].copy()
    else:
        assert bool(taken.all()), "the sink-free layout needs a graph without reachable sinks"
        p.pos = uoff[:, None, None] + np.arange(W)[None, :, None] * L + np.arange(L)[None, None, :]
        total = B * W * L
    p.uniforms = np.full(total, 0.5)
    p.uniforms[p.pos[taken]] = p.u[taken]
    p.taken = taken
    return p


# ---------------------------------------------------------------------------------------------------------- classification

def host_guide(rowptr, cdf):
    """guide[lo + j] = #{k : cdf[lo + k] <= (j / deg) * (1 - 2^-50)}, 0 for j = 0 (numpy restatement of graph_defs.expected_guide)"""
    guide = np.zeros(cdf.size, dtype=np.int64)
    for v in range(rowptr.size - 1):
        lo, hi = int(rowptr[v]), int(rowptr[v + 1])
        if hi > lo + 1:
            t = (np.arange(1, hi - lo, dtype=np.float64) / float(hi - lo)) * GUIDE_SHRINK
            guide[lo + 1:hi] = np.searchsorted(cdf[lo:hi], t, side="right")
    return guide


def scan_model(rowptr, cdf, guide, row, u, ans, packed):
    """The forward scan of search_two from the guide position, as control flow: every iteration looks at entry l and, if l + 1
    is inside the row (and, in packed blocks, l is not slot 7 of its block), at l + 1; after LIN_PROBES entries it bisects.
    Returns dict of boolean / integer vectors over the steps: 'found' (by the scan), 'second' (as the second entry of a pair),
    'single7' (an iteration took the single load at slot 7 with the next entry still inside the row), 'pairs' (some iteration
    took a pair load), 'n_bisect' (entries scanned when bisection began, -1 if it never did), 's' (answer - guide position), 'j_clamped'."""
    lo, hi = rowptr[row], rowptr[row + 1]
    deg = hi - lo
    jf = (u * deg.astype(np.float64)).astype(np.int64)
    clamped = jf >= deg
    j = np.minimum(jf, deg - 1)
    l = lo + guide[lo + j]
    s = ans - l
    assert bool((s >= 0).all()), "the guide position lies beyond searchsorted's answer"
    n = np.zeros(row.size, dtype=np.int64)
    found = np.zeros(row.size, dtype=bool)
    second = np.zeros(row.size, dtype=bool)
    single7 = np.zeros(row.size, dtype=bool)
    pairs = np.zeros(row.size, dtype=bool)
    for _ in range(LIN_PROBES):
        act = ~found & (n < LIN_PROBES) & (l < hi)
        at7 = (l & 7) == 7 if packed else np.zeros(row.size, dtype=bool)
        pair = act & (l + 1 < hi) & ~at7
        single7 |= act & (l + 1 < hi) & at7 & (ans != l)
        pairs |= pair
        hit0 = act & (ans == l)
        hit1 = pair & (ans == l + 1)
        found |= hit0 | hit1
        second |= hit1
        adv = act & ~hit0 & ~hit1
        step = np.where(pair, 2, 1)
        l = np.where(adv, l + step, l)
        n = np.where(adv, n + step, n)
    return {"found": found, "second": second, "single7": single7, "pairs": pairs, "n_bisect": np.where(found, -1, n), "s": s,
            "j_clamped": clamped, "gpos": lo + guide[lo + j]}


def record_classes(rowptr, col, cdf, guide, row, u, ans):
    """Branch of bucket_pick (64-byte records: 1..4 = candidate, 5 = fifth, 6 = beyond: the long way) and of half_pick (32-byte
    records: 1..4 = candidate proven, 11..14 = u inside that candidate's fp32 sliver, 6 = beyond the fourth) for every step,
    from the records' definition: candidate i is CDF entry guide position + i, 2.0 past the row end.
    Also where a wrong comparison would SHOW: full_tie = i (0..4) if candidate i is the first with c_i >= u, c_i == u, and its
    destination is not the answer's (`c_i >= u` for `c_i > u` picks it); half_tie = i (0..3) likewise for the half records, with
    u == l_i == c_i, i.e. a tie on a CDF entry that fp32 holds exactly (`u <= l_i` for `u < l_i` picks it); -1 otherwise."""
    lo, hi = rowptr[row], rowptr[row + 1]
    deg = hi - lo
    j = np.minimum((u * deg.astype(np.float64)).astype(np.int64), deg - 1)
    first = lo + guide[lo + j]
    idx = first[:, None] + np.arange(5)[None, :]
    c = np.where(idx < hi[:, None], cdf[np.minimum(idx, cdf.size - 1)], 2.0)
    gt = c > u[:, None]
    full = np.where(gt.any(axis=1), gt.argmax(axis=1) + 1, 6)
    cl = round_down_f32(c[:, :4])
    below_hi = u[:, None] < next_f32(cl).astype(np.float64)
    i = below_hi.argmax(axis=1)
    proven = u < cl[np.arange(row.size), i].astype(np.float64)
    half = np.where(~below_hi.any(axis=1), 6, np.where(proven, i + 1, i + 11))
    # a proven candidate is searchsorted's answer
    ok = half <= 4
    assert bool((first[ok] + half[ok] - 1 == ans[ok]).all()) and bool((first[full <= 5] + full[full <= 5] - 1 == ans[full <= 5]).all())
    ge = c >= u[:, None]
    i5 = ge.argmax(axis=1)
    r = np.arange(row.size)
    other = col[np.minimum(idx, hi[:, None] - 1)] != col[ans][:, None]
    full_tie = np.where(ge.any(axis=1) & (c[r, i5] == u) & other[r, i5], i5, -1)
    sliver = (half >= 11) & (half <= 14)
    half_tie = np.where(sliver & (cl[r, i].astype(np.float64) == u) & (c[r, i] == u) & other[r, i], i, -1)
    return full, half, full_tie, half_tie


def classify(rowptr, col, cdf, guide, p, start_deg):
    """Flat vectors over the steps taken of a Planted batch (in (i, w, st) order) + the index arrays to find them again."""
    t = p.taken
    row, u, ans = p.row[t], p.u[t], p.edge[t]
    ii, ww, ss = np.nonzero(t)
    out = {"i": ii, "w": ww, "st": ss, "kind": p.kind[t], "row": row, "u": u, "ans": ans}
    out["guide_scan"] = scan_model(rowptr, cdf, guide, row, u, ans, packed=False)
    out["packed_scan"] = scan_model(rowptr, cdf, guide, row, u, ans, packed=True)
    out["full"], out["half"], out["full_tie"], out["half_tie"] = record_classes(rowptr, col, cdf, guide, row, u, ans)
    out["lds"] = (ss == 0) & (start_deg[ii] <= STAGED_MAX_DEG)            # step 0 of a staged start row: searched in LDS, no record
    lo, hi = rowptr[row], rowptr[row + 1]
    out["tie"] = (ans > lo) & (cdf[np.maximum(ans - 1, 0)] == u)             # u equals the CDF entry just below the answer
    out["sliver"] = (out["half"] >= 11) & (out["half"] <= 14)
    return out


def lane_pairs(cl, fallback, applies, shape):
    """The (A falls back, B falls back) combinations seen over the lane pairs (w, w + 64) of one start node and step, both walks
    alive and served by the form."""
    dense = np.full(shape, -1, dtype=np.int8)
    dense[cl["i"][applies], cl["w"][applies], cl["st"][applies]] = fallback[applies]
    wa = np.array([w for w in range(shape[1]) if w % 128 < 64 and w + 64 < shape[1]], dtype=np.int64)
    if wa.size == 0:
        return set()
    a, b = dense[:, wa, :], dense[:, wa + 64, :]
    both = (a >= 0) & (b >= 0)
    return {(bool(x), bool(y)) for x, y in set(zip(a[both].tolist(), b[both].tolist()))}


# ------------------------------------------------------------------------------------------------------------------ cases

SHAPES = ((100, 2), (192, 3), (1, 1))     # (W, L); T = W * L, so nothing of the visit histogram is truncated
PATH_REPEATS, PATH_L = 40, 3              # ps_walk_paths: every node starts PATH_REPEATS one-walk paths of PATH_L steps
_cache = {}


def case_graph(sinks=False):
    """(host Graph of the C oracle, info, guide, edge_index, weights) of the case graph, built once per process"""
    if sinks not in _cache:
        from oracle import c_oracle as co
        ei, ew, V, info = build_case_graph(0, sinks=sinks)
        cg = co.Graph(ei, ew, num_nodes=V)
        _cache[sinks] = (cg, info, host_guide(cg.rowptr, cg.cdf), ei, ew)
    return _cache[sinks]


def planted_batch(W, L):
    """(start nodes, uoff, Planted) of the sink-free batch: every node starts W walks"""
    key = ("batch", W, L)
    if key not in _cache:
        cg = case_graph()[0]
        nodes = np.arange(cg.V)
        uoff, n = cg.uniform_offsets(nodes, W, L)
        p = plant(cg.rowptr, cg.col, cg.cdf, nodes, W, L, seed=W * 10 + L, uoff=uoff)
        assert p.uniforms.size == n
        _cache[key] = (nodes, uoff, p)
    return _cache[key]


def planted_sink_batch(W, L):
    """(start nodes, Planted) on the graph with sinks: sequential stream layout"""
    key = ("sink", W, L)
    if key not in _cache:
        cg, info = case_graph(True)[:2]
        nodes = sink_case_starts(info)
        _cache[key] = (nodes, plant(cg.rowptr, cg.col, cg.cdf, nodes, W, L, seed=W * 10 + L + 5, sequential=True))
    return _cache[key]


def planted_paths():
    """(start nodes, uoff, Planted) for ps_walk_paths: W = 1, one path per entry of `starts`"""
    if "paths" not in _cache:
        cg = case_graph()[0]
        starts = np.repeat(np.arange(cg.V), PATH_REPEATS)
        uoff, n = cg.uniform_offsets(starts, 1, PATH_L)
        _cache["paths"] = (starts, uoff, plant(cg.rowptr, cg.col, cg.cdf, starts, 1, PATH_L, seed=77, uoff=uoff))
    return _cache["paths"]
