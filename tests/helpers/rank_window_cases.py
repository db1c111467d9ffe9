"""The case table of the rank-window tests (csrc/rank_window.hip: ps_rank_window) and numpy / plain-python restatements of what
include/pinsage_hip.h says about it.  numpy only; shared by tests/test_rank_window_cases.py (CPU), tests/test_hip_rank_window.py
(GPU) and tests/helpers/abi_cases_rank_window.py.

  restate   window / nwin from one lexsort on (-score, id) per row;
  brute     the same from python's sorted() over (-score, id) tuples -- a second, independent statement;
  pick      Floyd's subset sampling over the window's positions, as the header writes it;
  fill_short_rows   the host fill of pinsage_hip.negatives, restated.

Rows are built from bit patterns and rank lists so that every property a case is named after is planted, not hoped for:
`check_tag` states each property as a predicate over the brute-force ranking, and tests/test_rank_window_cases.py holds every
case to the tags it carries."""
import functools
import math

import numpy as np

MAX_WINDOW = 1 << 16          # ps_rank_window_max(), asserted against the library by the tests
MAX_PICKS = 64
VPS = (1, 63, 64, 65, 255, 256, 257, 1025, 70001)
INF_KEY = 0x7FF0000000000000
HUGE = 1.0e300                # planted where nothing may compete: columns in [limit, Vp) and the pad columns [Vp, ld)
U_MAX = 1.0 - 2.0 ** -53      # the largest double below 1
PAD = 5                       # ld - Vp of every case


def from_bits(keys):
    return np.asarray(keys, dtype=np.uint64).view(np.float64)


def limit_of(Vp, max_target):
    return max_target if 0 <= max_target < Vp else Vp


# ---- restatements -----------------------------------------------------------------------------------------------------------------
def candidates(row, limit, skip):
    """ascending ids t < limit with row[t] > 0 and t != skip (NaN, zeros of either sign and negatives fail `> 0`)"""
    with np.errstate(invalid="ignore"):
        ids = np.flatnonzero(row[:limit] > 0)
    return ids if skip is None else ids[ids != skip]


def restate(score, limit, skip, lo, hi):
    """(window int32[S, hi - lo], nwin int32[S]): ranks [lo, hi) of (score descending, id ascending), written in ascending id"""
    S = score.shape[0]
    window = np.full((S, hi - lo), -1, np.int32)
    nwin = np.zeros(S, np.int32)
    for s in range(S):
        ids = candidates(score[s], limit, None if skip is None else int(skip[s]))
        ranked = ids[np.lexsort((ids, -score[s, ids]))]
        members = np.sort(ranked[lo:hi])
        window[s, :len(members)] = members
        nwin[s] = len(members)
    return window, nwin


def ranking(row, limit, skip):
    """the whole ranking of one row by python's sorted()"""
    return sorted((int(t) for t in candidates(row, limit, skip)), key=lambda t: (-float(row[t]), t))


def brute(score, limit, skip, lo, hi):
    S = score.shape[0]
    window = np.full((S, hi - lo), -1, np.int32)
    nwin = np.zeros(S, np.int32)
    for s in range(S):
        members = sorted(ranking(score[s], limit, None if skip is None else int(skip[s]))[lo:hi])
        window[s, :len(members)] = members
        nwin[s] = len(members)
    return window, nwin


def pick_positions(m, u_row, n):
    """the positions p_0 .. p_{c-1} of Floyd's rule and, per step, whether t was taken already / whether the clamp acted"""
    c = min(n, m)
    pos, collided, clamped = [], [], []
    for i in range(c):
        j = m - c + i
        prod = float(u_row[i]) * float(j + 1)                # one fp64 product
        if not prod >= 0.0:                                  # negative or NaN
            t = 0
        elif prod >= j + 1:
            t = j
        else:
            t = min(int(math.floor(prod)), j)
        clamped.append(prod >= j + 1)
        collided.append(t in pos)
        pos.append(j if t in pos else t)
    return pos, collided, clamped


def pick(window, nwin, u, n):
    """picks int32[S, n]"""
    S = window.shape[0]
    out = np.full((S, n), -1, np.int32)
    for s in range(S):
        pos = pick_positions(int(nwin[s]), u[s], n)[0]
        out[s, :len(pos)] = window[s, pos]
    return out


def fill_short_rows(picks, queries, u2, num_movies):
    """a -1 slot gets min(floor(u2 * M), M - 1), moved on by (cand + 1) % M while it is the query or an earlier slot of the row"""
    out = np.array(picks, dtype=np.int64)
    M = int(num_movies)
    if M <= out.shape[1] + 1:
        raise ValueError("too few items")
    for b in range(out.shape[0]):
        for i in range(out.shape[1]):
            if out[b, i] < 0:
                cand = min(int(math.floor(float(u2[b, i]) * M)), M - 1)
                while cand == int(queries[b]) or cand in out[b, :i].tolist():
                    cand = (cand + 1) % M
                out[b, i] = cand
    return out


# ---- row builders -----------------------------------------------------------------------------------------------------------------
_JUNK = from_bits([0, 1 << 63, 0x7FF8000000000000, 0xBFF8000000000000, 0xFFF0000000000000, (1 << 63) | 5, 0xFFF8000000000001])
# +0.0, -0.0, NaN, -1.5, -inf, a negative denormal, a NaN with the sign bit: none of them competes


def distinct_keys(rs, n):
    """n distinct keys of positive finite doubles spread over twelve decades like PPR scores, descending"""
    keys = np.zeros(0, np.uint64)
    while len(keys) < n:
        v = rs.random_sample(2 * n + 8) * 10.0 ** rs.randint(-12, 0, 2 * n + 8)
        keys = np.unique(np.concatenate([keys, v[v > 0].view(np.uint64)]))
    return np.sort(rs.permutation(keys)[:n])[::-1].copy()


def row_from_keys(rs, Vp, limit, keys, salt=False):
    """a row of Vp doubles: `keys` (uint64, any order) on random ids below limit, junk that never competes on the other ids
    below limit (every kind in turn; zeros only without `salt`), HUGE in [limit, Vp)"""
    keys = np.asarray(keys, np.uint64)
    assert len(keys) <= limit
    row = np.zeros(Vp, np.float64)
    ids = rs.permutation(limit)
    row[ids[:len(keys)]] = from_bits(keys)
    if salt:
        row[ids[len(keys):]] = np.resize(_JUNK, limit - len(keys))
    row[limit:] = HUGE
    return row


def tie(keys, a, b):
    """ranks a .. b-1 of a descending key list share the key of rank a"""
    keys = np.array(keys, np.uint64)
    keys[a:b] = keys[a]
    return keys


def byte_keys(rs, b, n):
    """n keys that differ in byte b (0 = least significant) only"""
    shift = 8 * b
    base = 0x3FE5555555555555 & ~(0xFF << shift)
    vals = (rs.permutation(126) + 1 if b == 7 else rs.permutation(256))[:n]          # byte 7: 0x01 .. 0x7e, finite and positive
    return np.array([base | (int(v) << shift) for v in vals], np.uint64)


class Case:
    def __init__(self, name, rows, Vp, max_target, lo, hi, skip=None, n=0, u=None, tags=()):
        self.name, self.Vp, self.max_target, self.lo, self.hi, self.n = name, Vp, max_target, lo, hi, n
        self.ld = Vp + PAD
        self.limit = limit_of(Vp, max_target)
        self.score = np.full((len(rows), self.ld), HUGE, np.float64)                   # the pad columns hold HUGE
        for s, r in enumerate(rows):
            assert r.shape == (Vp,)
            self.score[s, :Vp] = r
        self.S = len(rows)
        self.skip = None if skip is None else np.ascontiguousarray(skip, np.int64)
        self.u = None if u is None else np.ascontiguousarray(u, np.float64)
        self.tags = tuple(tags)                                                        # (row or None, tag)
        assert 0 <= lo < hi and hi - lo <= MAX_WINDOW and 0 <= n <= MAX_PICKS
        assert (self.u is None) == (n == 0) and (n == 0 or self.u.shape == (self.S, n))
        assert self.skip is None or self.skip.shape == (self.S,)
        for a in (self.score, self.skip, self.u):
            if a is not None:
                a.setflags(write=False)

    def __repr__(self):
        return f"Case({self.name})"


def _uniforms(rs, S, n):
    return rs.random_sample((S, n)) if n else None


def _sizes(Vp):
    rs = np.random.RandomState(9100 + Vp % 9973)
    if Vp == 1:
        rows = [from_bits([0x3FF0000000000000]), np.zeros(1), from_bits([0x7FF8000000000000])]
        return Case("sizes-1", rows, 1, -1, 0, 1, n=1, u=_uniforms(rs, 3, 1), tags=[(0, "exact_hi"), (1, "zeros"), (2, "below_hi_nan")])
    limit = Vp - 3
    lo, hi = limit // 4, limit // 2
    counts = [("zeros", 0), ("below_lo", lo // 2 + 1), ("exact_lo", lo), ("between", (lo + hi) // 2), ("exact_hi", hi),
              ("above_hi", hi + 1), ("above_hi", limit - 8)]
    rows, tags = [], []
    for s, (tag, N) in enumerate(counts):
        keys = distinct_keys(rs, N)
        if tag == "above_hi" and N > hi + 1:                  # the full row: +inf and denormals among the candidates, junk around them
            keys[0] = INF_KEY
            keys[-3:] = [9, 2, 1]
            tags.append((s, "salted"))
        rows.append(row_from_keys(rs, Vp, limit, keys, salt=N > 0))
        tags.append((s, tag))
    tags.append((None, "planted_beyond_limit"))
    return Case(f"sizes-{Vp}", rows, Vp, limit, lo, hi, n=6, u=_uniforms(rs, len(rows), 6), tags=tags)


def _ties(Vp):
    rs = np.random.RandomState(9200 + Vp)
    lo, hi = Vp // 4, Vp // 2
    d = distinct_keys(rs, Vp)
    rows = [row_from_keys(rs, Vp, Vp, np.full(Vp, d[0])), row_from_keys(rs, Vp, Vp, tie(d, lo - 3, lo + 4)),
            row_from_keys(rs, Vp, Vp, tie(d, hi - 2, hi + 5)), row_from_keys(rs, Vp, Vp, tie(d, lo - 2, hi + 3))]
    return Case(f"ties-{Vp}", rows, Vp, -1, lo, hi, n=6, u=_uniforms(rs, 4, 6),
                tags=[(0, "one_value"), (1, "tie_lo_only"), (2, "tie_hi_only"), (3, "tie_both")])


def _bytes():
    rs = np.random.RandomState(9300)
    rows = [row_from_keys(rs, 257, 257, byte_keys(rs, b, 120), salt=True) for b in range(8)]
    return Case("bytes", rows, 257, -1, 30, 90, tags=[(b, f"byte_{b}") for b in range(8)])


def _windows():
    rs = np.random.RandomState(9400)
    out = []
    rows = [row_from_keys(rs, 256, 256, distinct_keys(rs, 200)), row_from_keys(rs, 256, 256, distinct_keys(rs, 5)), np.zeros(256)]
    out.append(Case("lo0", rows, 256, -1, 0, 10, n=6, u=_uniforms(rs, 3, 6), tags=[(0, "above_hi"), (1, "between"), (2, "zeros"), (None, "S3")]))
    out.append(Case("width1", rows, 256, -1, 7, 8, n=1, u=_uniforms(rs, 3, 1), tags=[(0, "above_hi"), (1, "below_lo"), (None, "S3")]))
    out.append(Case("single", [row_from_keys(rs, 65, 60, tie(distinct_keys(rs, 50), 8, 13), salt=True)], 65, 60, 10, 30,
                    tags=[(0, "tie_lo_only"), (None, "S1")]))
    Vp = VPS[-1]
    rows = [row_from_keys(rs, Vp, Vp, tie(distinct_keys(rs, Vp), 90, 120)), row_from_keys(rs, Vp, Vp, distinct_keys(rs, 30000))]
    out.append(Case("maxwin", rows, Vp, -1, 100, 100 + MAX_WINDOW, n=64, u=_uniforms(rs, 2, 64),
                    tags=[(0, "above_hi"), (0, "tie_lo_only"), (1, "between"), (None, "max_window")]))
    return out


def _rows70():
    """70 rows of every regime, each with a skip entry of some kind"""
    rs = np.random.RandomState(9500)
    Vp, limit, lo, hi = 257, 250, 40, 100
    rows, skip = [], []
    for s in range(70):
        N = (0, 17, lo, 77, hi, 101, limit, 180)[s % 8]
        keys = distinct_keys(rs, N)
        if N > hi and s % 3 == 0:
            keys = tie(keys, lo - 1 - s % 5, lo + 2)
        if N > hi and s % 3 == 1:
            keys = tie(keys, hi - 1, hi + 1 + s % 4)
        rows.append(row_from_keys(rs, Vp, limit, keys, salt=True))
        skip.append((-1, limit, limit + 3, int(rs.randint(0, limit)), int(rs.randint(0, limit)), 1 << 40)[s % 6])
    return Case("rows70", rows, Vp, limit, lo, hi, skip=skip, n=6, u=_uniforms(rs, 70, 6), tags=[(None, "S70")])


def _skip():
    rs = np.random.RandomState(9600)
    Vp, limit, lo, hi = 256, 250, 20, 60
    keys = tie(distinct_keys(rs, 240), lo - 4, lo + 5)
    base = row_from_keys(rs, Vp, limit, keys, salt=True)
    order = ranking(base, limit, None)
    skip = [order[0], order[(lo + hi) // 2], order[lo - 1], -1, limit, 1 << 40]
    tags = [(0, "skip_rank0"), (1, "skip_in_window"), (2, "skip_in_tie"), (3, "skip_minus1"), (4, "skip_beyond"), (5, "skip_beyond")]
    return Case("skip", [base] * 6, Vp, limit, lo, hi, skip=skip, n=6, u=_uniforms(rs, 6, 6), tags=tags)


def _picks(n):
    rs = np.random.RandomState(9700 + n)
    Vp, lo, hi = 256, 10, 110
    counts = (256, 13, 0, 256, 256, 256, 80, 256)        # nwin = 100, 3, 0, 100, 100, 100, 70, 100
    rows = [row_from_keys(rs, Vp, Vp, distinct_keys(rs, N)) for N in counts]
    u = rs.random_sample((len(rows), n))
    u[3] = 0.0
    u[4] = U_MAX
    u[5, 0::2] = -0.25
    u[5, 1::2] = np.nan
    u[7, 0::2] = 1.0                                     # outside [0, 1): what the clamp is for
    u[7, 1::2] = 1.0e300
    tags = [(2, "nwin0"), (3, "u0"), (4, "u_max"), (5, "u_neg_nan"), (7, "u_clamped")]
    if n > 3:
        tags.append((1, "n_above_nwin"))
    if n > 1:                                            # steps 0 and 1 of row 6 land on the same t: step 1 takes j
        m, c = 70, min(n, 70)
        t0 = (m - c + 1) // 2
        u[6, 0] = (t0 + 0.5) / (m - c + 1)
        u[6, 1] = (t0 + 0.5) / (m - c + 2)
        tags.append((6, "collision"))
    return Case(f"picks-n{n}", rows, Vp, -1, lo, hi, n=n, u=u, tags=tags)


@functools.lru_cache(maxsize=None)
def cases():
    out = [_sizes(Vp) for Vp in VPS] + [_ties(Vp) for Vp in (255, 256, 1025)] + [_bytes()] + _windows() + [_rows70(), _skip()]
    out += [_picks(n) for n in (1, 6, 64)]
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


NAMES = tuple(c.name for c in cases())


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(window, nwin, picks or None) of a case from the restatement: made once, shared, read-only"""
    c = case(name)
    window, nwin = restate(c.score, c.limit, c.skip, c.lo, c.hi)
    picks = pick(window, nwin, c.u, c.n) if c.n else None
    for a in (window, nwin, picks):
        if a is not None:
            a.setflags(write=False)
    return window, nwin, picks


# ---- the planted properties, as predicates over the brute-force ranking -------------------------------------------------------------
def check_tag(c, row, tag):
    """raises AssertionError unless case c (row `row`, or the case as a whole for row None) has the property `tag` names"""
    lo, hi, limit = c.lo, c.hi, c.limit
    if row is None:
        if tag in ("S1", "S3", "S70"):
            assert c.S == int(tag[1:])
        elif tag == "max_window":
            assert hi - lo == MAX_WINDOW
        elif tag == "planted_beyond_limit":
            assert limit < c.Vp < c.ld and (c.score[:, limit:] == HUGE).all()
        else:
            raise KeyError(tag)
        return
    x = c.score[row]
    sk = None if c.skip is None else int(c.skip[row])
    free = ranking(x, limit, None)                        # the ranking without the skip
    order = ranking(x, limit, sk)
    N = len(order)
    ks = [float(x[t]) for t in order]
    lo_tie = 0 < lo < N and ks[lo - 1] == ks[lo]
    hi_tie = hi < N and ks[hi - 1] == ks[hi]
    if tag == "zeros":
        assert N == 0 and not x[:limit].any()
    elif tag == "below_hi_nan":
        assert N == 0 and np.isnan(x[:limit]).all()
    elif tag == "below_lo":
        assert 0 < N < lo
    elif tag == "exact_lo":
        assert N == lo > 0
    elif tag == "between":
        assert lo < N < hi
    elif tag == "exact_hi":
        assert N == hi
    elif tag == "above_hi":
        assert N > hi
    elif tag == "salted":
        v = x[:limit]
        assert np.isnan(v).any() and (v < 0).any() and np.isinf(v[v > 0]).any() and (np.signbit(v) & (v == 0)).any()
        assert ((v > 0) & (v < 2.0 ** -1022)).any()       # positive denormals compete
    elif tag == "one_value":
        assert N == limit > hi and len(set(ks)) == 1
    elif tag == "tie_lo_only":
        assert lo_tie and not hi_tie
    elif tag == "tie_hi_only":
        assert hi_tie and not lo_tie
    elif tag == "tie_both":
        assert lo_tie and hi_tie and ks[lo] == ks[hi] and len(set(ks)) > 1
    elif tag.startswith("byte_"):
        b = int(tag[5:])
        keys = x[order].view(np.uint64)
        diff = np.bitwise_or.reduce(keys ^ keys[0])
        assert N > hi and len(set(keys.tolist())) == N and diff != 0 and diff & ~np.uint64(0xFF << (8 * b)) == 0
    elif tag == "skip_rank0":
        assert sk == free[0]
    elif tag == "skip_in_window":
        assert lo <= free.index(sk) < hi and x[sk] != x[free[lo]]
    elif tag == "skip_in_tie":
        r = free.index(sk)
        assert x[free[lo - 1]] == x[free[lo]] == x[sk] and r < lo          # one of the tied ids ahead of the boundary leaves
    elif tag == "skip_minus1":
        assert sk == -1 and order == free
    elif tag == "skip_beyond":
        assert sk >= limit and order == free
    elif tag in ("nwin0", "n_above_nwin", "u0", "u_max", "u_clamped", "u_neg_nan", "collision"):
        m = min(N, hi) - lo if N > lo else 0
        pos, collided, clamped = pick_positions(m, c.u[row], c.n)
        if tag == "nwin0":
            assert m == 0 and pos == []
        elif tag == "n_above_nwin":
            assert 0 < m < c.n and sorted(pos) == list(range(m))
        elif tag == "u0":
            assert (c.u[row] == 0).all() and m > c.n and pos[0] == 0 and (c.n == 1 or all(collided[1:]))
        elif tag == "u_max":
            # (1 - 2^-53)(j + 1) never rounds up to j + 1: the floor alone gives j, the largest position of every step
            assert (c.u[row] == U_MAX).all() and m > c.n and not any(clamped) and pos == list(range(m - c.n, m))
        elif tag == "u_clamped":
            assert (c.u[row] >= 1).all() and m > c.n and all(clamped) and pos == list(range(m - c.n, m))
        elif tag == "u_neg_nan":
            assert (c.u[row, 0::2] < 0).all() and (c.n == 1 or np.isnan(c.u[row, 1::2]).all()) and pos[0] == 0
        else:
            assert not collided[0] and collided[1] and pos[1] == m - min(c.n, m) + 1
    else:
        raise KeyError(tag)
