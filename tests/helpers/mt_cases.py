"""The device MT19937 generator (csrc/mt19937.hip) restated on the host, its numpy oracles, and the case table that
tests/test_mt_cases.py proves (which plan / scheme / writer every case reaches) and tests/test_hip_mt_stream.py runs.

Stream word w = 0 is the next 32-bit word numpy would output; uniform i is made of the words 2i and 2i + 1.  Window c is the 624
raw words from stream word 1 + c * CHUNK on; its forward workgroup stores the words [1 + c CHUNK, 1 + c CHUNK + HALF), its backward
workgroup the words [1 + c CHUNK - HALF, 1 + c CHUNK).  Everything below is plain integer arithmetic, host only.

What reaches what (case -> code in mt19937.hip):
  key_w == 0                          a-p0-s1-n1, a-p624-*         mt_final_state_kernel
  key_w < 0                           a-p1-s1-n1, a-p5-s1-n1       state copy + mt_set_pos_kernel
  r == 0 -> pos_out = 624             a-p0-s311-n1                 make_plan's fold
  state window over a half edge       b-half-*, b-half-c77-*       mt_chunk_kernel: forward workgroup of slot q, backward of q + 1
  ... over a window base              b-base-*, b-base-c79-*       both workgroups of one slot (after a base jump: slot 0 = window c0)
  w_lo < 2 skip, w_hi > 2 (skip + n)  b-*-lo / b-*-hi              make_plan's two extensions
  request ends on the geometry        c-*                          mt_chunk_kernel's chain loops, last / first block partial
  K = 32|33, 512|513, 1024|1025       d-K*                         combine | one round | two rounds | three radix levels
  every scheme, smallest and ragged   e-K*                         doubling, mt_combine_radix_kernel (1 and 2 levels), two rounds, one round
  schemes after a skipped prefix      f-*                          base jump, then each scheme; one round via mt_fold_kernel
  base jump levels >= 24              JUMP_CASE                    mt_expand_kernel + mt_combine_kernel at levels 17, 19, 30, 43
  ranged planner                      h-*                          mt_generate's `ranges` block, mt_chunk_kernel<true>, both fallbacks"""
import collections
import functools

import numpy as np

MT_N = 624
Geometry = collections.namedtuple("Geometry", "chunk_log2 n_window radix_lo two_round_max jump_levels radix_levels window_shift")
# the library's values (tests/test_hip_mt_stream.py::test_the_library_has_the_geometry_assumed_here holds them to it):
# 2^17-word chunks, 511 rows of one-round window polynomials, K > 32: matrix-core products, K - 1 <= 511: one round,
# K <= 1024: two rounds, 44 binary jump levels, 6 radix-32 levels, 17 blocks expanded before the first window
GEOM = Geometry(17, 511, 32, 1024, 44, 6, 17 * MT_N)
JP, SEQ_PAD, KS_TOTAL, JT = 24, 34 * MT_N, 320, 20
PLW, WSZ = SEQ_PAD // 32, JP * MT_N
FILL = 0xFFFFFFFF                                          # what the ranged tests pre-fill the caller's buffer with


# ---- the request planner -------------------------------------------------------------------------------------------------------
Plan = collections.namedtuple("Plan", "wa wb key_w pos_out w_lo w_hi c0 c1 K")


def make_plan(pos_in, skip, n, g=GEOM, fold_r0=True, extend_hi=True, half_shift=0):
    """make_plan of mt19937.hip.  Perturbations (test_mt_cases.py::test_teeth): fold_r0=False leaves pos_out = 0 where numpy says
    624, extend_hi=False keeps w_hi at the request's end, half_shift moves the half-chunk edge of the window arithmetic."""
    chunk = 1 << g.chunk_log2
    half = chunk // 2 + half_shift
    wa, wb = 2 * skip, 2 * (skip + n)
    q, r = divmod(pos_in + wb, MT_N)
    if fold_r0 and r == 0 and wb > 0:
        q, r = q - 1, MT_N
    key_w = q * MT_N - pos_in
    w_lo = key_w if 0 <= key_w < wa else wa
    w_hi = wb
    if extend_hi and key_w >= 0 and key_w + MT_N > w_hi:
        w_hi = key_w + MT_N
    first, last = max(w_lo, 1), w_hi - 1
    c0 = (first - 1 + half) // chunk
    c1 = (last - 1 + half) // chunk if last >= 1 else 0
    c1 = max(c1, c0)
    return Plan(wa, wb, key_w, r, w_lo, w_hi, c0, c1, c1 - c0 + 1)


def key_class(p):
    """which of the three hand-back forms the plan takes, and the sub-cases the issue names"""
    if p.key_w < 0:
        return "copy"                                      # state copied, only pos moves
    if p.key_w == 0:
        return "final_state_kernel"
    return "chunk_kernel"                                  # stored by whoever produces the words


def n_for_K(K, pos_in=0, skip=0, g=GEOM):
    """the smallest n whose plan has K chunk windows (K is monotone in n), by bisection"""
    lo, hi = 0, 1
    while make_plan(pos_in, skip, hi, g).K < K:
        hi *= 2
    while hi - lo > 1:                                     # K(lo) < K <= K(hi)
        mid = (lo + hi) // 2
        if make_plan(pos_in, skip, mid, g).K < K:
            lo = mid
        else:
            hi = mid
    assert make_plan(pos_in, skip, hi, g).K == K and hi >= 1
    return hi


# ---- the ranged planner ------------------------------------------------------------------------------------------------------------
Ranged = collections.namedtuple("Ranged", "ranged why words wins Kw")


def ranged_plan(pos_in, n, ranges, g=GEOM, one_round=True, radix=True, drop_key=False, chi_from_b=False, half_shift=0,
                extend_hi=True):
    """The `ranges` block of mt_generate behind the Python wrapper: (ranged?, why not, wanted word runs [a, b), window runs
    [first, last], window slots).  Not ranged = the whole stream is generated.  Perturbations: drop_key leaves the state's 624
    words out of the wanted set, chi_from_b takes a run's last window from its end instead of its last word."""
    chunk = 1 << g.chunk_log2
    half = chunk // 2 + half_shift
    p = make_plan(pos_in, 0, n, g, extend_hi=extend_hi)
    whole = Ranged(False, None, [(p.w_lo, p.w_hi)], [(1, p.K - 1)] if p.K > 1 else [], p.K)
    runs = [] if ranges is None else [tuple(r) for r in ranges]
    if not runs:
        return whole._replace(why="no runs")
    if len(runs) > 3:
        return whole._replace(why="more than three runs")             # the wrapper passes none on
    if not (radix and one_round) or p.c0 != 0:
        return whole._replace(why="no one-round table")
    ab = []
    for lo, hi in runs:
        lo, hi = max(lo, 0), min(hi, n)
        if lo < hi:
            ab.append((2 * lo, 2 * hi))
    if p.key_w >= 0 and not drop_key:
        ab.append((p.key_w, p.key_w + MT_N))
    ab.sort(key=lambda t: t[0])                            # (stable, as the insertion sort)
    words = []
    for a, b in ab:
        if words and a <= words[-1][1]:
            words[-1] = (words[-1][0], max(words[-1][1], b))
        else:
            words.append((a, b))
    wins, maxwin = [], 0
    for a, b in words:
        a1 = max(a, 1)
        if b <= a1:
            continue
        clo = (a1 - 1 + half) // chunk
        chi = ((b if chi_from_b else b - 2) + half) // chunk
        clo = max(clo, 1)                                  # window 0 is slot 0
        if chi < clo:
            continue
        if wins and clo <= wins[-1][1] + 1:
            wins[-1] = (wins[-1][0], max(wins[-1][1], chi))
        else:
            wins.append((clo, chi))
        maxwin = wins[-1][1]
    if not words:
        return whole._replace(why="nothing wanted")
    if maxwin > g.n_window:
        return whole._replace(why="beyond the window table")
    return Ranged(True, None, words, wins, 1 + sum(l - f + 1 for f, l in wins))


def window_list(p, rp=None):
    """window index (relative to c0) of every slot of the chunk launch"""
    if rp is None or not rp.ranged:
        return list(range(p.K))
    return [0] + [w for f, l in rp.wins for w in range(f, l + 1)]


# ---- the chunk generators' share of the words -------------------------------------------------------------------------------------------
Writer = collections.namedtuple("Writer", "window back wbase lo hi")


def writers(p, windows, wanted, g=GEOM):
    """mt_chunk_kernel's workgroups that store something: (absolute window, backwards?, window base, hull [lo, hi) of its wanted
    words).  Always the kernel's own geometry, whatever a perturbed planner asked for."""
    chunk = 1 << g.chunk_log2
    half = chunk // 2
    out = []
    for w in windows:
        wbase = 1 + (p.c0 + w) * chunk
        for back in (False, True):
            h_lo, h_hi = (wbase - half, wbase) if back else (wbase, wbase + half)
            h_lo = max(h_lo, 1)
            lo, hi = h_hi, h_lo
            for a, b in wanted:
                a, b = max(a, h_lo), min(b, h_hi)
                if a < b:
                    lo, hi = min(lo, a), max(hi, b)
            if lo < hi:
                out.append(Writer(p.c0 + w, back, wbase, lo, hi))
    return sorted(out, key=lambda w: w.lo)


def stored_runs(ws, wanted):
    """the stream words >= 1 that the workgroups `ws` store: sorted disjoint runs"""
    runs = []
    for w in ws:
        for a, b in wanted:
            a, b = max(a, w.lo, 1), min(b, w.hi)
            if a < b:
                runs.append((a, b))
    runs.sort()
    out = []
    for a, b in runs:
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def wanted_runs(wanted):
    """the wanted words >= 1 as sorted disjoint runs (word 0 is not a chunk word)"""
    out = []
    for a, b in sorted((max(a, 1), b) for a, b in wanted):
        if a >= b:
            continue
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def state_writers(p, ws):
    """the workgroups that store part of state_out (key_w >= 1 only)"""
    if p.key_w < 1:
        return []
    return [w for w in ws if w.lo < p.key_w + MT_N and w.hi > p.key_w]


def straddle(p, ws):
    """None, 'half' (forward workgroup of window q, backward one of q + 1) or 'base' (both workgroups of one window)"""
    sw = state_writers(p, ws)
    if len(sw) < 2:
        return None
    assert len(sw) == 2
    a, b = sw
    if a.window == b.window:
        return "base"
    assert b.window == a.window + 1 and not a.back and b.back
    return "half"


# ---- the scheme that makes the chunk windows ---------------------------------------------------------------------------------------
def _a256(x):
    return (x + 255) // 256 * 256


def _one_round_fits(K, Kw):
    Kc = max(K, 126)
    ngroups = (Kw - 1 + 31) // 32
    parts_w, best = 32, 1e30
    for parts in (4, 8, 16, 32):
        wgs = ngroups * 16 * parts
        cost = ((wgs + 511) // 512) * (KS_TOTAL // parts + 4)
        if wgs >= 256 and cost < best:
            best, parts_w = cost, parts
    q = _a256(SEQ_PAD * 4) + _a256(32 * PLW * 4) + _a256(ngroups * KS_TOTAL * 64 * 16) + _a256(Kw * MT_N * 4)
    return q <= _a256((Kc // 2 + 2) * SEQ_PAD * 4) and parts_w * ngroups * 32 * JT * 32 <= (Kc - 1) * WSZ


def _two_round_fits(K):
    nsrc = (K - 1) // 32 + 1
    q = _a256(nsrc * SEQ_PAD * 4) + _a256(nsrc * 32 * PLW * 4) + 2 * _a256(KS_TOTAL * 64 * 16) + _a256(K * MT_N * 4)
    room = (K - 1) * WSZ                                   # the parity planes live in the window store of windows 1 .. K - 1
    return q <= _a256((K // 2 + 2) * SEQ_PAD * 4) and 8 * nsrc * 32 * JT * 32 <= room and 32 * 32 * JT * 32 <= room


def scheme(K, c0=0, radix=True, one_round=True, n_window=None, ranged=False, Kw=None, g=GEOM):
    """which code makes the K chunk windows: 'none' (one window), 'doubling', 'combine<levels>' (radix-32 rounds of
    mt_combine_radix_kernel), 'two_round' (two radix rounds on the matrix cores), 'one_round', 'one_round_fold' (after a base
    jump), 'one_round_empty' (no product).  radix / one_round are the wrapper's flags: no radix table means no window table."""
    n_window = g.n_window if n_window is None else n_window
    Kw = K if Kw is None else Kw
    if radix and one_round and (ranged or (K > g.radix_lo and K - 1 <= n_window)) and _one_round_fits(K, Kw):
        return "one_round_empty" if Kw == 1 else "one_round_fold" if c0 > 0 else "one_round"
    if radix and g.radix_levels >= 2 and g.radix_lo < K <= g.two_round_max and _two_round_fits(K):
        return "two_round"
    if K == 1:
        return "none"
    if radix:
        lvl, have = 0, 1
        while have < K:
            have, lvl = have * 32, lvl + 1
        return "combine%d" % lvl
    return "doubling"


def takes_parallel_path(skip, n, parallel=True):
    return parallel and (skip > 0 or n >= (1 << 17))


# ---- numpy as the oracle ---------------------------------------------------------------------------------------------------------------------
def temper(y):
    y = np.asarray(y, dtype=np.uint32).copy()
    y ^= y >> np.uint32(11)
    y ^= (y << np.uint32(7)) & np.uint32(0x9d2c5680)
    y ^= (y << np.uint32(15)) & np.uint32(0xefc60000)
    y ^= y >> np.uint32(18)
    return y


def untemper(z):
    """the inverse of temper (a bijection on 32-bit words): every bit of a raw word is pinned by numpy's tempered output"""
    z = np.asarray(z, dtype=np.uint32).copy()
    z ^= z >> np.uint32(18)
    z ^= (z << np.uint32(15)) & np.uint32(0xefc60000)
    y = z.copy()
    for _ in range(5):                                     # 7 more bits right per round
        y = z ^ ((y << np.uint32(7)) & np.uint32(0x9d2c5680))
    x = y.copy()
    for _ in range(3):                                     # 11 more bits right per round
        x = y ^ (x >> np.uint32(11))
    return x


def untemper_torch(z):
    """untemper on a torch int32 tensor of tempered words (any device): int32 raw words.  For the requests whose stream is too long
    to untemper on the host in a test's time; held to `untemper` in test_mt_cases.py."""
    import torch
    M = 0xFFFFFFFF
    z = z.to(torch.int64) & M
    z = z ^ (z >> 18)
    z = z ^ ((z << 15) & 0xefc60000)
    y = z
    for _ in range(5):
        y = z ^ ((y << 7) & 0x9d2c5680)
    x = y
    for _ in range(3):
        x = y ^ (x >> 11)
    x = x & M
    return torch.where(x >= 2 ** 31, x - 2 ** 32, x).to(torch.int32)


def state_at(pos_in, seed=1234):
    """a RandomState whose position inside its 624-word block is pos_in"""
    rs = np.random.RandomState(seed)
    rs.random_sample(400)                                  # past the seeding block: pos = 800 - 624 = 176 into a generated block
    key = rs.get_state()[1].copy()
    rs.set_state(("MT19937", key, pos_in, 0, 0.0))
    return rs


def tempered_words(rs, m):
    """the next m 32-bit outputs of rs (one MT19937 word each)"""
    return rs.randint(0, 2 ** 32, size=m, dtype=np.uint32)


def doubles_of(words):
    """genrand_res53 of consecutive tempered word pairs"""
    w = np.asarray(words, dtype=np.uint32).astype(np.uint64)
    a, b = w[0::2] >> np.uint64(5), w[1::2] >> np.uint64(6)
    return (a.astype(np.float64) * 67108864.0 + b.astype(np.float64)) / 9007199254740992.0


def state_from_words(p, raw, base=0):
    """(624 state words, pos) the plan hands back, read from the raw stream words raw[w - base] (key_w >= 0)"""
    assert p.key_w >= 0
    return np.asarray(raw[p.key_w - base:p.key_w - base + MT_N], dtype=np.uint32), p.pos_out


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name why pos_in skip n radix one_round raw ranges seed")


def _case(name, why, pos_in, skip, n, radix=True, one_round=True, raw=False, ranges=None, seed=1234):
    return Case(name, why, pos_in, skip, n, radix, one_round, raw, None if ranges is None else tuple(ranges), seed)


CHUNK = 1 << GEOM.chunk_log2
HALF = CHUNK // 2
FORMS = (("doubling", dict(radix=False)), ("radix", dict(one_round=False)), ("default", dict()))
POS_EDGES = (0, 1, 623, 624)


def plan_of(c, **kw):
    return make_plan(c.pos_in, c.skip, c.n, **kw)


def writers_of(c):
    p = plan_of(c)
    rp = ranged_plan(c.pos_in, c.n, c.ranges, one_round=c.one_round, radix=c.radix) if c.raw else None
    wanted = rp.words if rp is not None else [(p.w_lo, p.w_hi)]
    return p, rp, writers(p, window_list(p, rp), wanted)


def scheme_of(c):
    p = plan_of(c)
    if c.raw and c.ranges is not None:
        rp = ranged_plan(c.pos_in, c.n, c.ranges, one_round=c.one_round, radix=c.radix)
        return scheme(p.K, p.c0, c.radix, c.one_round, ranged=rp.ranged, Kw=rp.Kw)
    return scheme(p.K, p.c0, c.radix, c.one_round)


def _straddle_skips(edge, pos_in):
    """the smallest and the largest skip for which the one-uniform request's state window has `edge` strictly inside"""
    hits = []
    for skip in range(max(edge // 2 - 700, 1), edge // 2 + 700):
        p = make_plan(pos_in, skip, 1)
        if p.key_w < edge <= p.key_w + MT_N - 1:
            hits.append(skip)
    return hits[0], hits[-1]


def _forward_end_case(res, extra):
    """(pos_in, n): skip = 0, the last workgroup runs forwards and its wanted words end `res` words past a block start"""
    n = 146000 + extra
    for pos_in in range(MT_N + 1):
        p = make_plan(pos_in, 0, n)
        w = writers(p, range(p.K), [(p.w_lo, p.w_hi)])[-1]
        if not w.back and (w.hi - w.wbase) % MT_N == res:
            return pos_in, n
    raise AssertionError(res)


def _backward_start_case(res, extra):
    """(pos_in, skip, n): the first workgroup runs backwards and its wanted words start `res` words before a block end.  The request's
    own first word 2 * skip can only be an odd distance from a (odd) window base; distance 0 mod 624 needs the state window to
    open the request (n = 1 and an odd pos_in)."""
    if res != 0:
        for skip in range(100000 + extra, 100000 + extra + MT_N):
            p = make_plan(2, skip, 70000)
            w = writers(p, range(p.K), [(p.w_lo, p.w_hi)])[0]
            if w.back and w.lo == 2 * skip and (w.wbase - w.lo) % MT_N == res:
                return 2, skip, 70000
    else:
        for pos_in in range(1, MT_N, 2):
            for skip in range(100000 + extra, 100000 + extra + MT_N):
                p = make_plan(pos_in, skip, 1)
                w = writers(p, range(p.K), [(p.w_lo, p.w_hi)])[0]
                if w.back and w.lo == p.key_w < 2 * skip and (w.wbase - w.lo) % MT_N == 0:
                    return pos_in, skip, 1
    raise AssertionError(res)


# g: the base jump's high levels.  c0 = 2^26 + 2^13 + 5 chunks; the request opens in the backward half of chunk c0
JUMP_C0 = (1 << 26) + (1 << 13) + 5
JUMP_CASE = _case("g-jump-high-levels", "base jump over levels 19, 30 and 43, then a backward half chunk", 3,
                  (JUMP_C0 * CHUNK - HALF) // 2 + 501, 70000)
BEYOND_TABLE_SKIP = (1 << (GEOM.jump_levels - GEOM.chunk_log2)) * CHUNK // 2      # c1 >= 2^27: no polynomial for it

RANGED_N = 41 * HALF                                        # h: 41 chunks of words
TABLE_FALLBACK_N = 514 * HALF


def ranged_sets(n=RANGED_N):
    """h: name -> (runs of uniform indices, why)"""
    c_h, c_b = 7, 9
    i_half = (c_h * CHUNK + HALF) // 2                      # words 2i, 2i + 1 lie in different half chunks
    i_base = c_b * HALF                                     # words 2i, 2i + 1 lie on either side of window c_b's base
    wb = 1 + 12 * CHUNK                                     # a window base for the one-word blocks
    fwd_last = (wb + 5 * MT_N + MT_N - 1) // 2              # its word 2i is the LAST word of forward block 5
    fwd_first = (wb + 5 * MT_N + 1) // 2                    # ends with word wb + 5 * 624, the FIRST word of forward block 5
    bwd_last = (wb - 4 * MT_N - 1) // 2                     # word 2i is the last word of backward block 5
    bwd_first = (wb - 5 * MT_N + 1) // 2                    # ends with the first word of backward block 5
    return collections.OrderedDict([
        ("four-window-runs", ([(3 * HALF + 1000, 3 * HALF + 1010), (10 * HALF + 5, 10 * HALF + 300), (25 * HALF, 25 * HALF + 700)],
                              "three far-apart runs and the key window: four window runs")),
        ("across-half-edge", ([(i_half, i_half + 1)], "one uniform whose words lie in different half chunks: two windows")),
        ("before-half-edge", ([(i_half - 1, i_half)], "a run that ends on the last word of a forward half chunk")),
        ("after-half-edge", ([(i_half + 1, i_half + 2)], "a run that begins one uniform after a half edge")),
        ("across-window-base", ([(i_base, i_base + 1)], "one uniform whose words lie on either side of a window base")),
        ("adjacent-windows", ([(5 * HALF + 10, 5 * HALF + 20), (6 * HALF + 10, 6 * HALF + 20)], "far-apart word runs whose window runs touch")),
        ("touching-overlapping", ([(100, 200), (200, 300), (250, 400)], "runs that touch and overlap merge into one")),
        ("into-key-window", ([(n - 100, n)], "a run that ends inside the key window merges into it")),
        ("clamped-and-empty", ([(-5, 10), (50, 50), (n - 3, n + 99)], "runs clamped at 0 and at n, and an empty one")),
        ("block-last-word", ([(fwd_last, fwd_last + 20), (bwd_last, bwd_last + 20)], "blocks of which only the last word is wanted")),
        ("block-first-word", ([(fwd_first - 20, fwd_first), (bwd_first - 20, bwd_first)], "blocks of which only the first word is wanted")),
        ("everything", ([(0, n)], "(0, n): one run over the whole request")),
        ("four-runs", ([(10, 20), (3000, 3010), (70000, 70010), (n - 10, n)], "more runs than the planner takes: whole stream")),
    ])


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case, in the issue's groups a .. h (g is JUMP_CASE)"""
    out = []
    # a. K = 1 on the parallel path: every hand-back form
    for pos_in in POS_EDGES:
        for skip in (1, 311, 700):
            for n in (1, 2, 311, 312, 313):
                out.append(_case("a-p%d-s%d-n%d" % (pos_in, skip, n), "K = 1 hand-back forms", pos_in, skip, n))
    out.append(_case("a-p5-s1-n1", "key_w < 0 with the state copy, pos moves", 5, 1, 1))
    # b. the state window across a half edge and across a window base, at the stream's start and after a base jump
    out.append(_case("b-half-issue", "the issue's example: key_w = 65520, w_hi = 66144, K = 2", 0, 32768, 1))
    for tag, edge in (("half", 1 + HALF), ("base", 1 + CHUNK), ("half-c77", 1 + 77 * CHUNK + HALF), ("base-c79", 1 + 79 * CHUNK)):
        for pos_in in (0, 623):
            lo, hi = _straddle_skips(edge, pos_in)
            for which, skip in (("lo", lo), ("hi", hi)):
                for form, kw in FORMS[::2]:
                    out.append(_case("b-%s-p%d-%s-%s" % (tag, pos_in, which, form), "state window split between two workgroups",
                                     pos_in, skip, 1, **kw))
    # c. the request's ends against the chunk geometry
    for tag, edge in (("half", 1 + CHUNK + HALF), ("base", 1 + 2 * CHUNK)):
        u = (edge - 1) // 2                                 # the uniform whose second word is the first word past the edge
        for d in (-1, 0, 1):
            out.append(_case("c-start-%s%+d" % (tag, d), "2 skip at an edge", 3, u + d, 70000))
            out.append(_case("c-end-%s%+d" % (tag, d), "2 (skip + n) at an edge", 3, 5, u + d - 5))
    for res in (MT_N - 1, 0, 1):
        for extra in (0, 312):
            pos_in, n = _forward_end_case(res, extra)
            out.append(_case("c-fwd-end-r%d-x%d" % (res, extra), "forward chain ends %d words into a block" % res, pos_in, 0, n))
            pos_in, skip, n = _backward_start_case(res, extra)
            out.append(_case("c-bwd-start-r%d-x%d" % (res, extra), "backward chain starts %d words before a block end" % res,
                             pos_in, skip, n))
    for tag, w_hi in (("fwd-last", 1 + 2 * CHUNK + HALF), ("back-first", 2 + 2 * CHUNK + HALF)):
        pos_in = (-w_hi) % MT_N                             # the state window, and with it the kept words, ends at w_hi
        out.append(_case("c-whi-%s" % tag, "the kept words end with the %s word of a half chunk" % tag.split("-")[1], pos_in, 0,
                         (w_hi - 100) // 2))
    # d. the scheme thresholds, default flags
    for K in (2, 32, 33, 34, 512, 513, 1024, 1025):
        out.append(_case("d-K%d" % K, "threshold", 0, 0, n_for_K(K)))
    # e. every scheme at its smallest and at a ragged K, as doubles and as raw words (K = 45: the smallest that fits two MFMA rounds).
    #    A request from the stream's start takes the parallel path from 2^17 doubles on, which are three chunk windows: K = 2 needs
    #    a skipped prefix, and so has no raw form.
    for K in (2, 3, 31, 32, 33, 45, 64, 65):
        skip = 2 if K == 2 else 0
        for form, kw in FORMS:
            for raw in ((False,) if K == 2 else (False, True)):
                out.append(_case("e-K%d-%s-%s" % (K, form, "raw" if raw else "dbl"), "scheme x form", 1, skip,
                                 max(n_for_K(K, 1, skip), 0 if skip else 1 << 17), raw=raw, **kw))
    # f. schemes after a skipped prefix, odd word position
    skip = 5_000_017
    for K, form in ((33, "doubling"), (32, "default"), (33, "radix"), (45, "radix"), (33, "default")):
        out.append(_case("f-K%d-%s" % (K, form), "scheme after a base jump", 311, skip, n_for_K(K, 311, skip), **dict(FORMS)[form]))
    # h. ranged requests
    for pos_in in (3, 624):
        for name, (runs, why) in ranged_sets().items():
            out.append(_case("h-p%d-%s" % (pos_in, name), why, pos_in, 0, RANGED_N, raw=True, ranges=runs))
    out.append(_case("h-table-fallback", "the key window lies beyond the 511-row table: whole stream", 3, 0, TABLE_FALLBACK_N,
                     raw=True, ranges=[(70000, 70050)]))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return collections.OrderedDict((c.name, c) for c in out)


def group(letter):
    return [c for c in cases().values() if c.name.startswith(letter + "-")]
