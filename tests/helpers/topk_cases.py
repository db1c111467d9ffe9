"""The case table of the top-k selection behind the three searches (csrc/dot_topk.hip: WaveSelect under row_topk_kernel<0> =
ps_dot_topk, row_topk_kernel<1> = ps_l2_topk plain and masked, ivf_row_topk_kernel = ps_ivf_topk), shared by
tests/test_topk_cases.py (CPU: the table proves its own coverage) and tests/test_hip_topk_matrix.py (GPU: every case bit for bit).
numpy only.  Four parts:

  exact data   small integers in fp32: every product, partial sum, squared norm and (|q|^2 + |x|^2) - 2 q.x stays below 2^24, so
               each value is exact in fp32 whatever the summation order and an int64 evaluation IS the answer (assert_exact).
               The pattern sits in column 0 of D = 4 (D = 3 where the scalar loads are wanted), zeros elsewhere.
  the oracle   the first k of a lexsort by (value descending / distance ascending, id ascending) over the visible items.
  the model    WaveSelect restated from the kernel: 64-lane offers in sweep order, one threshold, the 256-slot queue, the reduce
               trigger, the sweeps of 32 with `after` and `dry`; it returns what it emits and a Facts record per row.
  the table    cases(): one entry per launch, named after the situation it exists for.
"""
import functools
from collections import namedtuple

import numpy as np

SELQ = 256                # slots of a wave's queue                         (constexpr int SELQ = 256)
WAVE = 64                 # keys offered together; reduce when cnt > SELQ - WAVE
TOPK_SWEEP = 32           # keys emitted per sweep                           (constexpr int TOPK_SWEEP = 32)
LOAD_STEP = 512           # elements a flat sweep requests together          (j0 += 512)
PIECE = 256               # elements of one piece of an IVF segment          (off += 256)
ROUND = 64                # probe slots of one round of the IVF sweep        (pb += 64)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
FLT_MAX = np.float32(3.4028234663852886e38)
EXACT = 1 << 24
U32 = np.uint64(32)


# ---- keys ------------------------------------------------------------------------------------------------------------------------
def mono_u(v):
    """fp32 -> uint32, monotone increasing in the value (the `u` of desc_key)"""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def value_key(kind, v):
    """the high word of a key: desc_key(v) for the inner product (larger value = smaller key), ~desc_key(v) for a distance"""
    u = mono_u(v)
    return ~u if kind == "dot" else u


def key_value(kind, hi):
    hi = np.asarray(hi, dtype=np.uint32)
    u = ~hi if kind == "dot" else hi
    b = np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32)
    return b.view(np.float32)


def make_keys(kind, vals, ids):
    return (value_key(kind, np.asarray(vals, dtype=np.float32)).astype(np.uint64) << U32) | np.asarray(ids).astype(np.uint64)


def decode(kind, keys):
    """emitted keys (EMPTY = padding) -> (fp32 values, int64 ids)"""
    keys = np.asarray(keys, dtype=np.uint64)
    pad = keys == EMPTY
    vals = key_value(kind, (keys >> U32).astype(np.uint32)).copy()
    ids = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    vals[pad] = -np.inf if kind == "dot" else FLT_MAX
    ids[pad] = -1
    return vals, ids


# ---- the restated selection ------------------------------------------------------------------------------------------------------
Facts = namedtuple("Facts", "reductions admitted max_cnt boundary_in_tie thr_tie_smaller_id after_tie_smaller_id dry")
# reductions            in-sweep reductions, one count per sweep that ran
# admitted              keys that entered the queue, all sweeps
# max_cnt               the largest queue count reached (before the reduction it triggers)
# boundary_in_tie       one flag per sweep boundary: the last key of a sweep and the first of the next share their value word
# thr_tie_smaller_id    keys admitted whose value word equals the threshold's (their id is the smaller one)
# after_tie_smaller_id  keys of a later sweep turned away by `after` on the id alone (value word equal, id smaller)
# dry                   a sweep came up short, the remaining sweeps were skipped

VARIANTS = ("no_after", "after_ge", "after_value_only", "thr_value_only", "late_reduce", "thr_kk_minus_1")


def _reduce(q, kk, thr, variant):
    u = np.unique(q)[:kk]                                  # the kk smallest; equal keys (a list probed twice) fall together
    if len(u) == kk:
        thr = u[kk - 2] if (variant == "thr_kk_minus_1" and kk >= 2) else u[kk - 1]
    return u, thr


def wave_select(groups, k, variant=None):
    """groups: the valid keys (uint64 arrays, lane order) of every 64-lane offer of ONE sweep, in sweep order; every sweep
    offers the same sequence.  -> (k emitted keys, Facts)"""
    kcap = min(k, TOPK_SWEEP)
    out, after, first, dry = [], np.uint64(0), True, False
    reductions, admitted, max_cnt, boundary, thr_tie, after_tie = [], 0, 0, [], 0, 0
    for base in range(0, k, kcap):
        kk = min(k - base, kcap)
        q, thr = np.empty(0, dtype=np.uint64), EMPTY
        if not dry:
            nred = 0
            for keys in groups:
                if variant == "thr_value_only":
                    adm = (keys >> U32) < (thr >> U32)
                else:
                    adm = keys < thr
                if not first:
                    if variant == "no_after":
                        pass
                    elif variant == "after_ge":
                        adm &= keys >= after
                    elif variant == "after_value_only":
                        adm &= (keys >> U32) > (after >> U32)
                    else:
                        after_tie += int((adm & ((keys >> U32) == (after >> U32)) & (keys < after)).sum())
                        adm &= keys > after
                if not adm.any():
                    continue
                new = keys[adm]
                if thr != EMPTY:
                    thr_tie += int(((new >> U32) == (thr >> U32)).sum())
                admitted += len(new)
                q = np.concatenate([q, new])
                max_cnt = max(max_cnt, len(q))
                if variant == "late_reduce":               # reduces only once the queue is full; keys past slot 255 are lost
                    q = q[:SELQ]
                    trigger = len(q) >= SELQ
                else:
                    trigger = len(q) > SELQ - WAVE
                if trigger:
                    q, thr = _reduce(q, kk, thr, variant)
                    nred += 1
            reductions.append(nred)
        q, thr = _reduce(q, kk, thr, variant)
        if base:
            boundary.append(bool(len(q)) and bool(out[-1] != EMPTY) and (int(out[-1]) >> 32) == (int(q[0]) >> 32))
        out += list(q) + [EMPTY] * (kk - len(q))
        if len(q) < kk:
            dry = True
        else:
            after = q[kk - 1]
        first = False
    return np.array(out, dtype=np.uint64), Facts(tuple(reductions), admitted, max_cnt, tuple(boundary), thr_tie, after_tie, dry)


# ---- cases -----------------------------------------------------------------------------------------------------------------------
class Case:
    """one launch.  kind: "dot" (ps_dot_topk), "l2" (ps_l2_topk), "l2m" (ps_l2_topk with assign / probe), "ivf" (ps_ivf_topk).
    x: the column-0 integers of the item table (for "ivf": of the rows sorted by list); q: the queries' column-0 integers
    ("dot": qidx, row indices of the table)."""

    def __init__(self, name, kind, x, k, D=4, **kw):
        self.name, self.kind, self.k, self.D = name, kind, int(k), D
        self.x = np.asarray(x, dtype=np.int64)
        self.exclude_self = False
        self.__dict__.update(kw)
        self.N = len(self.x)
        self.nq = len(self.qidx) if kind == "dot" else len(self.q)

    @property
    def order(self):
        return "dot" if self.kind == "dot" else "l2"

    def table(self):
        """fp32 [N, D]: the pattern in column 0"""
        t = np.zeros((self.N, self.D), dtype=np.float32)
        t[:, 0] = self.x
        return t

    def queries(self):
        """fp32 [nq, D] (not for "dot", whose queries are table rows)"""
        t = np.zeros((self.nq, self.D), dtype=np.float32)
        t[:, 0] = self.q
        return t

    def qval(self, r):
        return int(self.x[self.qidx[r]]) if self.kind == "dot" else int(self.q[r])

    def row_values(self, r):
        """the planted slab row of query r as integers: E[q] . E^T (every kind) -- what dense.linear must return"""
        return self.qval(r) * self.x

    def values(self, r):
        """float64 [N]: what the selection orders for query r over ALL table rows (sorted rows for "ivf")"""
        c = self.qval(r)
        if self.kind == "dot":
            v = (c * self.x).astype(np.float64)
            if self.exclude_self:
                v[self.qidx[r]] = -np.inf
            return v
        return ((c * c + self.x * self.x) - 2 * (c * self.x)).astype(np.float64)

    def valid_probes(self, r, oob_as_list0=False):
        """the probe slots of query r that name a list, in slot order (None for a skipped slot)"""
        out = []
        for l in self.probes[r]:
            l = int(l)
            if 0 <= l < self.nlist:
                out.append(l)
            else:
                out.append(0 if oob_as_list0 else None)
        return out

    def visible(self, r):
        """(values fp32, ids int64) of the items query r may return, each once"""
        v = self.values(r).astype(np.float32)
        if self.kind in ("dot", "l2"):
            return v, np.arange(self.N, dtype=np.int64)
        lists = sorted({l for l in self.valid_probes(r) if l is not None})
        if self.kind == "l2m":
            m = np.isin(self.assign, lists)
            return v[m], np.flatnonzero(m).astype(np.int64)
        rows = np.concatenate([np.arange(self.list_ptr[l], self.list_ptr[l + 1]) for l in lists] + [np.empty(0, dtype=np.int64)])
        rows = rows.astype(np.int64)
        return v[rows], self.item_ids[rows]

    def groups(self, r, variant=None):
        """the 64-lane offers of one sweep over query r, as the kernel makes them: valid keys only, lane order"""
        v = self.values(r).astype(np.float32)
        if self.kind != "ivf":
            keys = make_keys(self.order, v, np.arange(self.N))
            ok = np.ones(self.N, dtype=bool)
            if self.kind == "l2m":
                ok = np.isin(self.assign, [l for l in self.valid_probes(r) if l is not None])
            out = []
            for j0 in range(0, self.N, LOAD_STEP):
                for u in range(LOAD_STEP // WAVE):
                    a = j0 + WAVE * u
                    out.append(keys[a:a + WAVE][ok[a:a + WAVE]])
            return out
        keys = make_keys("l2", v, self.item_ids)
        slots = self.valid_probes(r, oob_as_list0=(variant == "oob_as_list0"))
        out = []
        for pb in range(0, len(slots), ROUND):
            for l in slots[pb:pb + ROUND]:
                if l is None:
                    continue
                j0, n = int(self.list_ptr[l]), int(self.list_ptr[l + 1] - self.list_ptr[l])
                for off in range(0, n, PIECE):             # an empty segment has no piece
                    for u in range(PIECE // WAVE):
                        a, b = off + WAVE * u, min(off + WAVE * (u + 1), n)
                        out.append(keys[j0 + a:j0 + max(a, b)])
            if variant == "one_round":
                break
        return out


def assert_exact(c):
    """every number the kernels form for this case is an integer below 2^24 in magnitude"""
    xm = int(np.abs(c.x).max()) if c.N else 0
    qm = max((abs(c.qval(r)) for r in range(c.nq)), default=0)
    assert qm * xm < EXACT, c.name                         # the one non-zero product of a dot (the other columns are zeros)
    if c.kind != "dot":
        assert qm * qm + xm * xm + 2 * qm * xm < EXACT, c.name     # |q|^2, |x|^2, their sum, 2 q.x and the difference


def oracle_of(c):
    """the oracle of any Case object, in the table or not (computed on every call)"""
    vals = np.full((c.nq, c.k), -np.inf if c.kind == "dot" else FLT_MAX, dtype=np.float32)
    ids = np.full((c.nq, c.k), -1, dtype=np.int64)
    for r in range(c.nq):
        v, i = c.visible(r)
        v64 = v.astype(np.float64)
        o = np.lexsort((i, -v64 if c.kind == "dot" else v64))[:c.k]
        vals[r, :len(o)], ids[r, :len(o)] = v[o], i[o]
    vals.setflags(write=False)
    ids.setflags(write=False)
    return vals, ids


@functools.lru_cache(maxsize=None)
def _oracle(name):
    return oracle_of(cases()[name])


def oracle(c):
    """(fp32 [nq, k], int64 [nq, k]): the k best by (value, id) over the visible items, padded; computed once, read-only"""
    return _oracle(c.name)


def model(c, variant=None):
    """the restated kernel on every row -> (values, ids, [Facts per row])"""
    vals = np.empty((c.nq, c.k), dtype=np.float32)
    ids = np.empty((c.nq, c.k), dtype=np.int64)
    facts = []
    for r in range(c.nq):
        keys, f = wave_select(c.groups(r, variant), c.k, variant)
        vals[r], ids[r] = decode(c.order, keys)
        facts.append(f)
    return vals, ids, facts


def same(a, b):
    """bit for bit: floats compared as int32"""
    (va, ia), (vb, ib) = a[:2], b[:2]
    return np.array_equal(va.view(np.int32), vb.view(np.int32)) and np.array_equal(ia, ib)


def probe_bits(c):
    """uint32 [nq, words]: bit l set = list l is probed (skipped entries set no bit)"""
    words = (c.nlist + 31) // 32
    bits = np.zeros((c.nq, words), dtype=np.uint32)
    for r in range(c.nq):
        for l in c.valid_probes(r):
            if l is not None:
                bits[r, l >> 5] |= np.uint32(1 << (l & 31))
    return bits


def masked_form(c):
    """an "ivf" case as ps_l2_topk sees it: (table column in ORIGINAL id order, assign int32 [N])"""
    x = np.empty(c.N, dtype=np.int64)
    assign = np.empty(c.N, dtype=np.int32)
    x[c.item_ids] = c.x
    assign[c.item_ids] = np.repeat(np.arange(c.nlist), np.diff(c.list_ptr))
    return x, assign


# ---- the table -------------------------------------------------------------------------------------------------------------------
DOT_Q = (1, -1, 0, 2)     # the query items appended to an inner-product table: the row of query c is c * a


def _dot(name, a, k, cs=DOT_Q, sel=None, **kw):
    a = np.asarray(a, dtype=np.int64)
    x = np.concatenate([a, np.asarray(cs, dtype=np.int64)])
    sel = range(len(cs)) if sel is None else sel
    return Case("dot-" + name, "dot", x, k, qidx=np.array([len(a) + s for s in sel], dtype=np.int64), **kw)


def _l2(name, a, cs, k, **kw):
    kind = "l2m" if "assign" in kw else "l2"
    return Case(kind + "-" + name, kind, a, k, q=np.asarray(cs, dtype=np.int64), **kw)


def _both(name, a_dot, k, a_l2, cs_l2, cs=DOT_Q, sel=None, sel_l2=None):
    cs_l2 = list(cs_l2) if sel_l2 is None else [cs_l2[s] for s in sel_l2]
    return [_dot(name, a_dot, k, cs=cs, sel=sel), _l2(name, a_l2, cs_l2, k)]


def _tie_runs():
    """30 / 10 / 400 items of three values, best to worst, scattered over the row"""
    rank = np.repeat([0, 1, 2], [30, 10, 400])
    return rank[np.random.RandomState(3).permutation(len(rank))]


IVF_LENS = (513, 1, 255, 256, 257, 0, 0, 0, 2, 64, 65, 63, 300, 128, 192, 193) + tuple((l * 7) % 23 + 3 for l in range(16, 79)) + (0,)
IVF_NLIST = len(IVF_LENS)
IVF_EMPTY = tuple(l for l, n in enumerate(IVF_LENS) if n == 0)
IVF_Q = (30, 70, -5, 17, 44)


def _ivf(name, probes, k, D=4):
    lens = np.array(IVF_LENS, dtype=np.int64)
    N = int(lens.sum())
    x = np.random.RandomState(11).randint(0, 60, size=N)
    item_ids = np.random.RandomState(12).permutation(N).astype(np.int64)
    probes = np.array(probes, dtype=np.int64)
    q = [IVF_Q[r % len(IVF_Q)] for r in range(len(probes))]
    return Case("ivf-" + name, "ivf", x, k, D=D, q=np.asarray(q, dtype=np.int64), probes=probes.astype(np.int32), nlist=IVF_NLIST,
                list_ptr=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), item_ids=item_ids, max_list=int(lens.max()))


def _wide_probes(nprobe):
    """probe rows for nprobe around the 64-slot round"""
    rs = np.random.RandomState(nprobe)
    perm = rs.permutation(IVF_NLIST)[:nprobe]
    holes = perm.copy()
    holes[::5] = -1
    holes[2::7] = IVF_NLIST
    twice = perm.copy()
    twice[-1] = twice[0] = 12                                            # list 12 in the first and in the last slot
    last_only = np.array([IVF_EMPTY[i % len(IVF_EMPTY)] for i in range(nprobe)])
    last_only[-1] = 12                                                   # everything the query sees sits in the last slot
    tail = np.arange(IVF_NLIST - nprobe, IVF_NLIST)                      # ends with the empty list 79
    return [np.arange(nprobe), tail[::-1], perm, holes, twice, last_only, tail]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case"""
    out = []
    # flat scans, inner product and L2
    for N in (192, 193):                                   # queue count 192: no in-sweep reduction; 193: exactly one
        out += _both("improving-N%d" % N, np.arange(-(N - 2), 1), 32, np.arange(N), [N + 5], cs=(1,))
    a = np.arange(1500 - 4) - 750                          # both signs; the rows of 1 / -1 / 0 / 2: improving, worsening, equal, improving
    x = np.arange(1500)
    for k in (11, 100):
        out += _both("regimes-N1500-k%d" % k, a, k, x, [1600, -100, 750, 749])       # L2: improving, worsening, V on an item, V
    out.append(_l2("equal-N1500-k100", np.full(1500, 7), [3, 7], 100))
    for nq in (5, 6, 7):                                   # four regimes in one workgroup, a ragged last workgroup
        out += _both("regimes-N1500-nq%d" % nq, a, 40, x, [1600, -100, 750, 749], sel=[s % 4 for s in range(nq)],
                     sel_l2=[s % 4 for s in range(nq)])
    t = _tie_runs()                                        # both sweep boundaries (32, 64) inside tie runs
    out += _both("tie-runs-k70", np.array([50, 40, -70])[t], 70, np.array([12, 11, 10])[t], [13, 9])
    late = np.concatenate([300 - 2 * np.arange(256), [281]])                          # 281: between the 10th (282) and 11th (280)
    out += _both("late-odd-k11", late, 11, late, [700], cs=(1,))
    r600 = np.random.RandomState(5).randint(-40, 40, size=600)
    for k in (1, 31, 32, 33, 64, 65):
        out += _both("N600-k%d" % k, r600[:596], k, r600, [0, 50, -50])
    for n in (31, 32, 33):                                 # fewer items than k, straddling a sweep
        out += _both("short-N%d-k64" % n, r600[:n - 1], 64, r600[:n], [3], cs=(1,))
    out += _both("short-N1-k5", [], 5, [4], [6, 4], cs=(1,))
    for N in (63, 64, 65, 511, 512, 513):                  # the 512-element load step and the 64-lane group, improving rows
        out += _both("improving-N%d-k33" % N, np.arange(-(N - 2), 1), 33, np.arange(N), [N + 5, -3], cs=(1,))
    out += [_dot("d3-regimes-N600-k40", np.arange(596) - 300, 40, D=3)]
    # exclude_self: the queries are pattern items; 9 * 9 = 81 is the row's best (self inside the top k), 0 * 0 ties with everything
    # (item 9: rank 9, just inside k = 10; item 40: outside), item 5 has rank 10, just outside
    es = np.concatenate([np.arange(-9, 10), np.random.RandomState(8).randint(-6, 7, size=51)])
    for k in (10, 70):
        out.append(Case("dot-exclude-self-k%d" % k, "dot", es, k, qidx=np.array([18, 9, 0, 30, 69, 40, 5], dtype=np.int64), exclude_self=True))
    # masked L2: the visible items are a cut through an improving run
    for nlist in (70, 20):                                 # words = 3 and words = 1
        assign = ((np.arange(1500) // 7) % nlist).astype(np.int32)
        probes = np.full((6, 24), -1, dtype=np.int64)
        probes[0] = (np.arange(24) * 2) % nlist            # every other list: about a third / half of the run
        probes[1, 0] = nlist - 1                           # one list: fewer than k items
        probes[2, :3] = [0, nlist - 1, 33 % nlist]         # (row 3: nothing probed)
        probes[4] = (np.arange(24) * 3 + 1) % nlist
        probes[5, :2] = [31 % nlist, 32 % nlist]           # either side of a word boundary
        out.append(_l2("improving-N1500-nlist%d-k40" % nlist, x, [1600, 1600, -100, 750, 750, 1600], 40, assign=assign,
                       probes=probes.astype(np.int32), nlist=nlist))
    # the inverted-file scan
    out.append(_ivf("p1-k33", [[0], [5], [-1], [3], [1], [IVF_NLIST], [4], [2], [12]], 33))
    p3 = [[5, 12, 13], [12, 6, 13], [12, 13, 79], [5, 6, 7], [-1, 12, IVF_NLIST], [-1, IVF_NLIST, 1000], [-2 ** 31, 2 ** 31 - 1, 14],
          [12, 12, 13], [12, 13, 12], [3, 4, 0], [0, 3, 4], [4, 0, 3], [2, 15, 1], [20, 41, 38]]
    out.append(_ivf("p3-k40", p3, 40))
    out.append(_ivf("p3-k1", p3[:9], 1))
    out.append(_ivf("d3-p3-k40", p3[:11], 40, D=3))
    out.append(_ivf("p64-k100", _wide_probes(64), 100))
    out.append(_ivf("p65-k40", _wide_probes(65), 40))
    out.append(_ivf("p65-k1", _wide_probes(65)[:6], 1))
    out.append(_ivf("p70-k32", _wide_probes(70)[:5], 32))
    out.append(_ivf("p70-k100", _wide_probes(70), 100))
    d = {c.name: c for c in out}
    assert len(d) == len(out)
    return d
