"""Planted walks for the walk sampler's count and select phases (csrc/walk_sample.hip), numpy only.

The walk phase has its table in walk_cases.py; this one steers whole walks so that the visit histogram lands where the
LDS hash table, the count-class bitmap and the ballot sweep could go wrong: counts on bitmap word boundaries, tie classes cut by
T, first-visit orders that differ from every other plausible order, probe chains at the tightest load the launcher allows,
holes in the position buffer, every position-slot count.  One shared graph: a start node per row of m distinct destinations
with equal weights (step 0 of walk w is steered to destination j(w) with the midpoint of its CDF interval), every other node
has out-degree 1 (the planted uniform is 0.5) or, in the sink variant, 0.  The walk a test expects is np.searchsorted on the
host CSR step by step; the expected ids / counts / nvalid are the reference's own words (`restate`) and nothing else.
`classify` restates the kernel's table arithmetic -- for COVERAGE only: it picks the colliding ids, chooses the cut positions
and proves that a case reaches what it is named for; no expected value comes from it."""
from collections import Counter

import numpy as np

import walk_cases as wc

V = 1 << 18
START0, BAND = 100_000, 1024              # start node of row r: START0 + 2 r; START0 + 2 r + 1 is isolated (no edge in or out)
RET0 = 110_000                            # RET0 + r: one edge, to the start node of row r (a walk that returns to its start)
HASH_MULT = 2654435761                    # walk_visits.h: h = id * 2654435761u >> (32 - hs_log2)
MAX_P = 4096                              # walk_sample_launch: P > 4096 is unsupported
RET = -2                                  # placeholder in a case's picks: the return node of its own row
SLOTS = 64                                # positions per slot j: p = j * 64 + lane


def chain_next(d):
    """the one out-edge of an ordinary node: 4k -> 4k+1 -> 4k+3 -> 4k, and 4k+2 -> 4k+1 (a merge)"""
    d = np.asarray(d, dtype=np.int64)
    return d + np.choose(d & 3, [1, 2, -1, -3])


def is_ordinary(d):
    d = np.asarray(d, dtype=np.int64)
    return ~(((d >= START0) & (d < START0 + BAND)) | ((d >= RET0) & (d < RET0 + BAND // 2)))


def is_sink(d):
    """sink variant: ordinary nodes 1 mod 8 lose their out-edge (8k and 8k+2 lead there; 8k+4 -> 8k+5 -> 8k+7 stays whole)"""
    return is_ordinary(d) & ((np.asarray(d, dtype=np.int64) & 7) == 1)


# ---------------------------------------------------------------------------------------------- the table arithmetic, restated

def hs_log2(P):
    h = 6
    while (1 << h) * 4 < 5 * P:
        h += 1
    return h


def home_slot(ids, h):
    return (((np.asarray(ids, dtype=np.uint64) * np.uint64(HASH_MULT)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - h)).astype(np.int64)


def bitmap_words(P):
    return (P >> 5) + 1


def n_slots(P):
    """NP of the launch: the power of two with NP * 64 >= P"""
    n = 1
    while n * SLOTS < P:
        n <<= 1
    return n


_ORD = np.flatnonzero(is_ordinary(np.arange(V)))


def ids_at_home(P, home, n, mod4=None, skip=()):
    """n ordinary ids whose home slot in the table of a P-position launch is `home`, spread over the id range"""
    c = _ORD[home_slot(_ORD, hs_log2(P)) == home]
    if mod4 is not None:
        c = c[(c & 3) == mod4]
    c = c[~np.isin(c, np.asarray(skip, dtype=np.int64))]
    assert c.size >= n, (P, home, n, c.size)
    return c[np.linspace(0, c.size - 1, n).astype(np.int64)]


def spread_ids(n, seed, mod4=None, skip=()):
    """n distinct ordinary ids, seeded"""
    rs = np.random.RandomState(seed)
    c = _ORD if mod4 is None else _ORD[(_ORD & 3) == mod4]
    c = c[~np.isin(c, np.asarray(skip, dtype=np.int64))]
    return c[rs.permutation(c.size)[:n]]


# ------------------------------------------------------------------------------------------------------------------ cases

class Case:
    """name, row (index of the start row), W, L, sinks (graph variant), picks int64[W] (destination of step 0 per walk),
    cuts ('all' / 'edges' / None: which cut positions of its tie classes are run), extra (more T), want (what classify must find)"""

    def __init__(self, name, row, W, L, sinks, picks, cuts, extra, want):
        self.name, self.row, self.W, self.L, self.sinks, self.picks, self.cuts, self.extra, self.want = \
            name, row, W, L, sinks, picks, cuts, tuple(extra), want
        self.start = START0 + 2 * row

    @property
    def P(self):
        return self.W * self.L


ROWS = []                                 # ROWS[r] = int64[m]: destinations of start node START0 + 2 r, in CSR order
CASES = {}


def _new_row(dests):
    ROWS.append(np.asarray(dests, dtype=np.int64))
    assert len(ROWS) * 2 <= BAND
    return len(ROWS) - 1


def _case(name, W, L, picks, sinks=False, cuts=None, extra=(), row=None, **want):
    picks = np.asarray(picks, dtype=np.int64)
    assert picks.size == W and name not in CASES and W * L <= MAX_P
    if row is None:
        r = len(ROWS)
        picks = np.where(picks == RET, RET0 + r, picks)
        d = np.unique(picks)
        row = _new_row(d[np.random.RandomState(len(ROWS)).permutation(d.size)])      # row order: neither id nor visit order
    assert np.isin(picks, ROWS[row]).all()
    CASES[name] = Case(name, row, W, L, sinks, picks, cuts, extra, want)
    return CASES[name]


def _interleave(*runs, seed=0):
    """a seeded shuffle of the multiset {id x count}"""
    seq = np.concatenate([np.full(n, i, dtype=np.int64) for i, n in runs])
    return seq[np.random.RandomState(seed).permutation(seq.size)]


def _tight(P, n_collide, seed, mod4=None, n=None, last=V - 1):
    """n (default P) distinct ids: n_collide with one home slot three below the end of the table (the chain wraps), id 0 and
    `last` (V - 1, or V - 4, whose walk reaches V - 1 at its third step), the rest spread"""
    n = P if n is None else n
    HS = 1 << hs_log2(P)
    ends = [0, last]
    col = ids_at_home(P, HS - 3, n_collide, mod4, skip=[0, V - 1, V - 4])
    rest = spread_ids(n - n_collide - 2, seed, mod4, skip=np.concatenate([col, [0, V - 1, V - 4]]))
    ids = np.concatenate([col, ends, rest])
    return ids[np.random.RandomState(seed + 1).permutation(n)]


def _build():
    one = lambda W, d=4000: np.full(W, d, dtype=np.int64)
    # ---- every NP instantiation, full and with lane 0 of the last slot only; count == W * L on every word the bitmap has
    _case("one_1", 1, 1, one(1), extra=(8,), maxcount=1)
    for P, bit0 in ((51, False), (64, True), (257, False), (1024, True), (1025, False), (2048, True), (4096, True)):
        _case(f"one_{P}", P, 1, one(P, 4000 + 4 * P), maxcount=P, bit0=bit0, words={P >> 5})
    for P in (64, 65, 128, 256, 257, 512, 1024, 1025, 2048, 4096):
        _case(f"distinct_{P}", P, 1, spread_ids(P, P), cuts="all" if P <= 128 else "edges", extra=(63, 64, 65, 100),
              cut_slots=2 if P > 64 else 1, cut_same_slot=True, maxcount=1, slots_used=(P + 63) // 64,
              **({"full": True} if P % 64 == 0 else {"lane0": True}))
    for P in (193, 449, 961, 1985, 4033):     # P = 64 NP - 63: lane 0 of the LAST slot of the instantiation (1 and 65 are above)
        _case(f"last_slot_lane0_{P}", P, 1, spread_ids(P, P), extra=(63, 64, 65, P - 64, P - 2, P - 1), maxcount=1, slots_used=n_slots(P),
              lane0=True, last_slot=True, cut_slots=2)
    # ---- counts on a bitmap word boundary
    a, b, c = 90_000, 50_000, 20_000          # first visits arrive in the order the shuffle gives, not in id order
    _case("c31_33_at_64", 64, 1, _interleave((a, 33), (b, 31), seed=1), words={0, 1})
    _case("c32_32_1_at_65", 65, 1, np.concatenate([_interleave((a, 32), (b, 32), seed=2), [c]]), cuts="all", bit0=True, lane0=True)
    _case("c31_32_33", 128, 1, np.concatenate([_interleave((a, 33), (b, 32), (c, 31), seed=3), spread_ids(32, 4)]), cuts="edges",
          bit0=True, words={0, 1})
    _case("c63_64_65", 256, 1, np.concatenate([spread_ids(64, 5), _interleave((c, 65), (a, 64), (b, 63), seed=6)]), cuts="edges",
          bit0=True, words={0, 1, 2}, cut_slots=1)
    _case("c1023_1", 1024, 1, np.concatenate([one(500, a), [b], one(523, a)]), words={0, 31})
    _case("c1024_1", 1025, 1, np.concatenate([[b], one(1024, a)]), bit0=True, words={0, 32})
    _case("c1024_1024", 2048, 1, _interleave((b, 1024), (a, 1024), seed=7), cuts="all", bit0=True, words={32})
    _case("c1056_1024_1023", 3276, 1, np.concatenate([_interleave((c, 1023), (a, 1024), (b, 1056), seed=8), spread_ids(173, 9)]),
          cuts="edges", bit0=True, words={0, 31, 32, 33})
    _case("c2048_1025_1023", 4096, 1, _interleave((a, 1023), (c, 2048), (b, 1025), seed=10), bit0=True, words={31, 32, 64})
    # ---- tie classes whose first-visit order is no other order; cut at every position
    for name, P, k, rep in (("shuffle_128", 128, 32, 4), ("shuffle_256", 256, 64, 4), ("shuffle_512", 512, 170, 3)):
        ids = spread_ids(k, P + 1)
        seq = _interleave(*[(i, rep) for i in ids], seed=P)
        seq = np.concatenate([seq, ids[:P - seq.size]])
        _case(name, P, 1, seq, cuts="all", order=("id", "last", "lane", "hash"), cut_slots=2 if P > 128 else 1, cut_same_slot=True)
    # ---- probe chains at the tightest load: 1.25 P just fits
    for P in (51, 102, 204, 409, 819, 1638, 3276):
        _case(f"tight_{P}_collide", P, 1, _tight(P, 40, P), cuts="all" if P <= 102 else "edges", wrap=True, chain=32, load=0.78,
              has_ids=(0, V - 1), order=("id", "hash"))
    for P, W, L in ((102, 51, 2), (204, 68, 3), (819, 273, 3), (1638, 819, 2), (3276, 1092, 3)):
        nc = min(40, W // 2, (V // 4 >> hs_log2(P)) - 2)                   # ids 0 mod 4 with one home slot: V / 4 / HS of them
        _case(f"tight_{P}_walk", W, L, _tight(P, nc, P + 7, mod4=0, n=W, last=V - 1 if L == 2 else V - 4), cuts="edges", wrap=True,
              chain=nc, load=0.78, has_ids=(0, V - 1))
    # ---- the reference's shape, W = 100, L = 2 (the destination-record kernels) and other walks of more than one step
    d100 = spread_ids(100, 100, mod4=0)
    _case("ref_distinct", 100, 2, d100, cuts="all", extra=(63, 64, 65, 150), cut_slots=2, cut_same_slot=True, maxcount=1)
    _case("ref_merge", 100, 2, np.concatenate([d100[:50], d100[:50] + 2])[np.random.RandomState(11).permutation(100)], cuts="edges",
          maxcount=2, cut_slots=2)
    _case("ref_one", 100, 2, one(100), cuts="all", maxcount=100)
    _case("ref_return", 100, 2, np.concatenate([d100[:15], np.full(60, RET), d100[15:40]]), cuts="edges", returns=True, maxcount=60)
    _case("walk_256_merge", 128, 2, np.concatenate([d100[:64], d100[:64] + 2])[np.random.RandomState(12).permutation(128)],
          cuts="edges", maxcount=2, cut_slots=2, full=True)
    _case("walk_512_one", 256, 2, one(256), maxcount=256, bit0=True, full=True)
    _case("walk_1024_return", 512, 2, np.concatenate([spread_ids(12, 13, mod4=0), np.full(500, RET)]), returns=True, maxcount=500)
    _case("walk_4096_cycle", 1024, 4, spread_ids(1024, 14, mod4=0), extra=(63, 64, 65, 1000, 1023, 1024, 1025, 2000, 3071, 3072),
          maxcount=2, cut_slots=2, full=True)
    # ---- fused rounds: one start row, three kinds of round (heavy collisions / one node / all distinct)
    for P, W, L in ((51, 51, 1), (200, 100, 2), (409, 409, 1)):
        m4 = None if L == 1 else 0
        heavy = _tight(P, 36 if P == 51 else 40, 3 * P, mod4=m4, n=W)
        plain = spread_ids(W, 5 * P, mod4=m4, skip=heavy)
        row = _new_row(np.concatenate([heavy, plain])[np.random.RandomState(P).permutation(2 * W)])
        _case(f"fused_{P}_heavy", W, L, heavy, row=row, wrap=True, chain=20, load=0.78)
        _case(f"fused_{P}_one", W, L, np.full(W, heavy[0]), row=row, maxcount=W)
        _case(f"fused_{P}_distinct", W, L, plain, row=row, maxcount=1)
    # ---- holes: the sink variant (8k -> 8k+1 stops there; 8k+1 stops at once; 8k+4 walks on)
    s8 = spread_ids(400, 15, mod4=0)
    s0, s4 = s8[(s8 & 7) == 0], s8[(s8 & 7) == 4]
    for W, L in ((100, 2), (68, 3)):
        t = f"{W}x{L}"
        _case(f"sink_all_die_{t}", W, L, _interleave(*[(i + 1, 2) for i in s0[:W // 2]], seed=16), sinks=True, cuts="edges", hole=True,
              all_die=True, maxcount=2)
        mixed = np.concatenate([s0[:W // 4], s0[:W // 4] + 2, s0[:W // 4] + 1, s4[:W - 3 * (W // 4)]])
        _case(f"sink_mixed_{t}", W, L, mixed[np.random.RandomState(17).permutation(W)], sinks=True, cuts="edges", hole=True)
        _case(f"sink_return_{t}", W, L, np.concatenate([s4[:W // 2], np.full(W - W // 2 - 5, RET), s0[:5] + 1]), sinks=True,
              hole=True, returns=True)
        _case(f"sink_whole_{t}", W, L, s4[:W], sinks=True, maxcount=1)
    _case("sink_lane0_65", 65, 1, np.concatenate([s0[:64] + 1, s4[:1]]), sinks=True, cuts="edges", lane0=True)


_build()
ISOLATED = START0 + 2 * np.arange(len(ROWS)) + 1          # isolated nodes, one beside every start node
SHAPES = sorted({(c.W, c.L, c.sinks) for c in CASES.values()})
FUSED = {(51, 1): "fused_51", (100, 2): "fused_200", (409, 1): "fused_409"}


def shape_cases(W, L, sinks=False):
    return [c for c in CASES.values() if (c.W, c.L, c.sinks) == (W, L, sinks)]


# ------------------------------------------------------------------------------------------------------------------ graph

def build_case_graph(sinks=False):
    """(edge_index int64[2, E], weights fp32[E]) in CSR order"""
    d = _ORD if not sinks else _ORD[~is_sink(_ORD)]
    src = [d, RET0 + np.arange(len(ROWS))] + [np.full(r.size, START0 + 2 * i) for i, r in enumerate(ROWS)]
    dst = [chain_next(d), START0 + 2 * np.arange(len(ROWS))] + list(ROWS)
    src, dst = np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64)
    return np.stack([src, dst]), np.ones(src.size, dtype=np.float32)


_cache = {}


def case_graph(sinks=False):
    """(host Graph of the C oracle, edge_index, weights), built once per process"""
    key = ("graph", sinks)
    if key not in _cache:
        from oracle import c_oracle as co
        ei, ew = build_case_graph(sinks)
        cg = co.Graph(ei, ew, num_nodes=V)
        assert cg.V == V
        _cache[key] = (cg, ei, ew)
    return _cache[key]


# --------------------------------------------------------------------------------------------------------------- planting

class Planted:
    """pos int64[W, L]: the node every step reached (-1: the walk had stopped); u fp64[W, L]; walks: python lists, start first"""


def plant(c):
    key = ("plant", c.name)
    if key in _cache:
        return _cache[key]
    cg = case_graph(c.sinks)[0]
    rowptr, col, cdf = cg.rowptr, cg.col, cg.cdf
    lo, hi = int(rowptr[c.start]), int(rowptr[c.start + 1])
    row = col[lo:hi].astype(np.int64)
    assert np.array_equal(row, ROWS[c.row])                                  # the CSR build kept the planted order
    order = np.argsort(row, kind="stable")
    j = order[np.searchsorted(row[order], c.picks)]
    assert np.array_equal(row[j], c.picks)
    below = np.concatenate([[0.0], cdf[lo:hi]])                              # cdf[-1] = 0
    p = Planted()
    p.u = np.full((c.W, c.L), 0.5)
    p.u[:, 0] = (below[j] + below[j + 1]) / 2
    p.pos = np.full((c.W, c.L), -1, dtype=np.int64)
    cur = np.full(c.W, c.start, dtype=np.int64)
    alive = np.ones(c.W, dtype=bool)
    for st in range(c.L):
        alive &= rowptr[cur + 1] > rowptr[cur]
        if not alive.any():
            break
        e = wc.searchsorted_rows(rowptr, cdf, cur[alive], p.u[alive, st])
        if st == 0:
            assert np.array_equal(e - lo, j), c.name                         # the midpoint picks the intended destination
        cur[alive] = col[e]
        p.pos[alive, st] = col[e]
    p.taken = p.pos >= 0
    p.walks = [[c.start] + [int(v) for v in w if v >= 0] for w in p.pos]
    _cache[key] = p
    return p


def restate(walks, T):
    """utils/random_walk.py sample_neighbors, padded: (ids[T], counts[T], nvalid)"""
    visit_counts = Counter()
    for walk in walks:
        for node in walk[1:]:
            visit_counts[node] += 1
    top = sorted(visit_counts.items(), key=lambda x: x[1], reverse=True)[:T]
    ids = [n for n, _ in top] + [-1] * (T - len(top))
    counts = [k for _, k in top] + [0] * (T - len(top))
    return ids, counts, min(T, len(visit_counts))


SLIPS = ("by_id", "by_last_visit", "lane_major", "ascending", "bit0_dropped", "saturate_1023", "start_excluded", "hole_ends",
         "pad_count", "nvalid_unclamped")


def select(pos, start, T, slip=None):
    """The same selection from the position buffer (pos flat, -1 = hole): equals `restate` with slip=None; with a slip, what a
    plausible mistake in the count / select phases would give."""
    pos = [int(v) for v in np.asarray(pos).reshape(-1)]
    if slip == "hole_ends" and -1 in pos:
        pos = pos[:pos.index(-1)]
    count, first, last = Counter(), {}, {}
    for p, v in enumerate(pos):
        if v < 0 or (slip == "start_excluded" and v == start):
            continue
        count[v] += 1
        first.setdefault(v, p)
        last[v] = p
    if slip == "saturate_1023":
        count = Counter({v: min(k, 1023) for v, k in count.items()})
    nodes = [v for v in first if not (slip == "bit0_dropped" and count[v] % 32 == 0)]
    tie = {"by_id": lambda v: v, "by_last_visit": lambda v: last[v],
           "lane_major": lambda v: (first[v] % SLOTS, first[v] // SLOTS)}.get(slip, lambda v: first[v])
    sign = 1 if slip == "ascending" else -1
    top = sorted(nodes, key=lambda v: (sign * count[v], tie(v)))[:T]
    pad = count[top[-1]] if (slip == "pad_count" and top) else 0
    ids = top + [-1] * (T - len(top))
    counts = [count[v] for v in top] + [pad] * (T - len(top))
    return ids, counts, len(nodes) if slip == "nvalid_unclamped" else min(T, len(nodes))


def expected(c, T):
    key = ("want", c.name, T)
    if key not in _cache:
        _cache[key] = restate(plant(c).walks, T)
    return _cache[key]


EMPTY = None                                                                 # a start node that does not walk


def expected_batch(cases, T):
    """(ids int64[B, T], counts int32[B, T], nvalid int32[B]); an entry of `cases` that is EMPTY gives a -1 / 0 / 0 row"""
    ids = np.full((len(cases), T), -1, dtype=np.int64)
    counts = np.zeros((len(cases), T), dtype=np.int32)
    nvalid = np.zeros(len(cases), dtype=np.int32)
    for i, c in enumerate(cases):
        if c is not EMPTY:
            ids[i], counts[i], nvalid[i] = expected(c, T)
    return ids, counts, nvalid


def stream(cases, sequential=False):
    """the planted uniforms of a batch laid end to end.  Sink-free layout: W * L per walking start node, step (w, st) at w * L + st;
    sequential (graphs with sinks): the steps really taken, in walk order"""
    parts = []
    for c in cases:
        if c is EMPTY:
            continue
        p = plant(c)
        assert sequential or p.taken.all(), c.name
        parts.append(p.u[p.taken] if sequential else p.u.reshape(-1))
    return np.concatenate(parts) if parts else np.zeros(0)


def oracle_batch(cases, nodes, T, sinks=False):
    """the C oracle on the same uniforms (in-range start nodes only: it rejects the others as the reference does)"""
    key = ("oracle", tuple(None if c is EMPTY else c.name for c in cases), tuple(int(n) for n in nodes), T)
    if key not in _cache:
        from oracle import c_oracle as co
        cg = case_graph(sinks)[0]
        live = [c for c in cases if c is not EMPTY]
        W, L = live[0].W, live[0].L
        u = stream(cases, sequential=sinks)
        nodes = np.asarray(nodes, dtype=np.int64)
        if sinks:
            o = co.walk_sample(cg, nodes, T, L, W, uniforms=u)
            assert o[4] == u.size
        else:
            uoff, n = cg.uniform_offsets(nodes, W, L)
            assert n == u.size
            o = co.walk_sample(cg, nodes, T, L, W, uniforms=u, uoff=uoff, threads=4)
        _cache[key] = o[:3]
    return _cache[key]


# ---------------------------------------------------------------------------------------------------------- classification

def classify(c):
    """What the kernel's count phase meets on this case, from the arithmetic restated above: the table filled by linear probing
    in position order p = j * 64 + lane, the bitmap words of the counts, the order of every tie class."""
    key = ("class", c.name)
    if key in _cache:
        return _cache[key]
    pos = plant(c).pos.reshape(-1)
    P = c.P
    h = hs_log2(P)
    HS = 1 << h
    table = np.full(HS, -1, dtype=np.int64)
    slot, count, first, last = {}, Counter(), {}, {}
    chain, wrapped = 0, False
    for p, v in enumerate(pos.tolist()):
        if v < 0:
            continue
        count[v] += 1
        last[v] = p
        if v in first:
            continue
        first[v] = p
        s = s0 = int(home_slot(v, h))
        n = 1
        while table[s] != -1:
            s = (s + 1) & (HS - 1)
            n += 1
        table[s] = v
        slot[v] = s
        chain = max(chain, n)
        wrapped |= s < s0
    ranked = sorted(first, key=lambda v: (-count[v], first[v]))
    live = np.flatnonzero(pos >= 0)
    holes = np.flatnonzero(pos < 0)
    out = {"P": P, "HS": HS, "chain": chain, "wrap": wrapped, "load": len(first) / HS, "distinct": len(first),
           "maxcount": max(count.values()), "words": {k >> 5 for k in count.values()},
           "bit0": any(k >= 32 and k % 32 == 0 for k in count.values()),
           "hole": bool(holes.size and live.size and holes.min() < live.max()),
           "all_die": c.L > 1 and bool((pos.reshape(c.W, c.L)[:, 1:] < 0).all()),
           "returns": c.start in count, "ids": set(first), "slots_used": int(live.max()) // SLOTS + 1,
           "full": P == n_slots(P) * SLOTS, "lane0": P % SLOTS == 1, "last_slot": P == n_slots(P) * SLOTS - 63,
           "ranked": ranked, "count": count, "first": first}
    assert max(out["words"]) < bitmap_words(P) and len(first) <= HS
    # the orders a tie class could come out in by mistake: which of them differ from first-visit order in some class
    differs = set()
    a = 0
    while a < len(ranked):
        b = a
        while b < len(ranked) and count[ranked[b]] == count[ranked[a]]:
            b += 1
        cls = ranked[a:b]
        for name, k in (("id", lambda v: v), ("last", lambda v: last[v]), ("lane", lambda v: (first[v] % SLOTS, first[v] // SLOTS)),
                        ("hash", lambda v: slot[v])):
            if sorted(cls, key=k) != cls:
                differs.add(name)
        a = b
    out["order"] = differs
    _cache[key] = out
    return out


def cut_info(c, T):
    """(the class T cuts, the slots j its members' first visits lie in, the cut falls between two members of one slot) or None"""
    k = classify(c)
    r, count, first = k["ranked"], k["count"], k["first"]
    if not (0 < T < len(r)) or count[r[T - 1]] != count[r[T]]:
        return None
    cls = [v for v in r if count[v] == count[r[T]]]
    return cls, {first[v] // SLOTS for v in cls}, first[r[T - 1]] // SLOTS == first[r[T]] // SLOTS


def case_T(c):
    """The T values a case is run at: 1, P, one above P, its extras, and the cut positions of its tie classes -- every one
    ('all'), or those around each change of position slot inside a class and around 64 ('edges')"""
    k = classify(c)
    r, count, first = k["ranked"], k["count"], k["first"]
    D = len(r)
    ts = {1, c.P, c.P + 7} | set(c.extra)
    if c.cuts == "all":
        ts |= set(range(1, D + 2))
    elif c.cuts == "edges":
        ts |= {63, 64, 65, D - 1, D, D + 1}
        for i in range(1, D):
            same = count[r[i - 1]] == count[r[i]]
            if not same or first[r[i - 1]] // SLOTS != first[r[i]] // SLOTS:
                ts |= {i - 1, i, i + 1}
    return sorted(t for t in ts if t >= 1)


def shape_T(W, L, sinks=False):
    key = ("T", W, L, sinks)
    if key not in _cache:
        _cache[key] = sorted(set().union(*[case_T(c) for c in shape_cases(W, L, sinks)]))
    return _cache[key]
