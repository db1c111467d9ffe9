"""An exact numpy restatement of ps_spmm_csr_exact and ps_sddmm_csr (csrc/spmm_exact.hip, as include/pinsage_hip.h states them),
their float64 closed forms with derived bounds, and the case table both test files share: tests/test_spmm_cases.py (CPU: the
restatement against the closed forms and against torch autograd) and tests/test_hip_spmm_grad.py (GPU: the kernels against the
restatement, bit for bit).

Every fp32 product-and-add is oracle.pinsage_oracle._fmaf_vec (one rounding), every lane sum agg_cases.wave_sum; the slice length
S is read from the library (slice_len()), and the case table is written in terms of it."""
import functools

import numpy as np

from helpers import agg_cases as ac

U32 = 2.0 ** -24                            # unit roundoff of fp32
BIG = np.float32(2.0 ** 24)


def slice_len():
    """S = ps_spmm_exact_slice(): a compile-time constant of the library (no GPU needed to ask)"""
    from pinsage_hip import native
    return int(native.lib().ps_spmm_exact_slice())


def _f(a):
    return np.asarray(a, dtype=np.float32)


def _fma(a, b, c):
    from oracle.pinsage_oracle import _fmaf_vec
    a, b, c = np.broadcast_arrays(_f(a), _f(b), _f(c))
    return _fmaf_vec(a, b, c)


def gamma(k):
    """gamma_k = k u / (1 - k u): what k successive roundings can do to a term, relative to it"""
    k = np.asarray(k, dtype=np.float64)
    return k * U32 / (1.0 - k * U32)


# ---- the restatements ------------------------------------------------------------------------------------------------------
def pieces(rowptr, S):
    """per row, the lengths of the pieces the slices [k S, (k + 1) S) cut its slot range into"""
    out = []
    for r in range(len(rowptr) - 1):
        lo, hi = int(rowptr[r]), int(rowptr[r + 1])
        row = []
        while lo < hi:
            nxt = min(hi, (lo // S + 1) * S)
            row.append(nxt - lo)
            lo = nxt
        out.append(row)
    return out


def spmm_exact(rowptr, col, val, x, S):
    """ps_spmm_csr_exact: a piece is the chain acc = fmaf(val[e], x[col[e]], acc) over its slots ascending from +0.0 (val None = 1.0,
    a source id outside [0, N) skipped); a row is ((p_0 + p_1) + p_2) + ... over its pieces, +0.0 when it is empty."""
    x = _f(x)
    N, H = x.shape
    V = len(rowptr) - 1
    out = np.zeros((V, H), dtype=np.float32)
    one = np.float32(1.0)
    for r in range(V):
        lo, hi = int(rowptr[r]), int(rowptr[r + 1])
        total = None
        while lo < hi:
            nxt = min(hi, (lo // S + 1) * S)
            acc = np.zeros(H, dtype=np.float32)
            for e in range(lo, nxt):
                if 0 <= col[e] < N:
                    acc = _fma(one if val is None else val[e], x[col[e]], acc)
            total = acc if total is None else total + acc
            lo = nxt
        if total is not None:
            out[r] = total
    return out


def lane_dot(a, b, vec):
    """[..., H] x [..., H] -> [...]: lane l chains part = fmaf(a[c], b[c], part) over its columns c = 64 vec k + vec l + e (sweep k,
    element e ascending) from +0.0, columns past H entering as 0 * 0; the 64 lanes are added by ps_wave_sum_f32's tree"""
    a, b = np.broadcast_arrays(_f(a), _f(b))
    H = a.shape[-1]
    chunk = 64 * vec
    sweeps = -(-H // chunk)

    def pad(t):
        out = np.zeros(t.shape[:-1] + (sweeps * chunk,), dtype=np.float32)
        out[..., :H] = t
        return out.reshape(t.shape[:-1] + (sweeps, 64, vec))
    ap, bp = pad(a), pad(b)
    part = np.zeros(a.shape[:-1] + (64,), dtype=np.float32)
    for k in range(sweeps):
        for e in range(vec):
            part = _fma(ap[..., k, :, e], bp[..., k, :, e], part)
    return ac.wave_sum(part)


def sddmm_exact(rowptr, col, x, g, vec):
    """ps_sddmm_csr: d[e] = lane_dot(g[r], x[col[e]]) for slot e of row r; +0.0 for a source id outside [0, N)"""
    x, g = _f(x), _f(g)
    N = x.shape[0]
    col = np.asarray(col, dtype=np.int64)
    d = np.zeros(len(col), dtype=np.float32)
    for r in range(len(rowptr) - 1):
        lo, hi = int(rowptr[r]), int(rowptr[r + 1])
        if hi == lo:
            continue
        ids = col[lo:hi]
        ok = (ids >= 0) & (ids < N)
        if ok.any():
            d[lo:hi][ok] = lane_dot(g[r][None, :], x[ids[ok]], vec)
    return d


# ---- float64 closed forms and bounds ---------------------------------------------------------------------------------------
def spmm_64(rowptr, col, val, x, S):
    """(out, bound) in float64: out[r] = sum_e val[e] x[col[e]] over the row's slots with a source id inside [0, N).

    Bound.  A piece of m slots is m fmaf, each one rounding (the first, onto +0.0, included), so a term that enters a piece passes
    through at most m roundings; adding the row's p pieces in order passes it through at most p - 1 more.  With n slots in the row
    no term sees more than n + p - 1 roundings, each a factor (1 + d), |d| <= u = 2^-24, hence
        |fp32 - exact| <= gamma_(n + p - 1) sum_e |val[e] x[col[e]]|,    gamma_k = k u / (1 - k u)
    (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1).  It holds while nothing underflows, which the case data
    (magnitudes 2^-6 .. 2^24) keep far away."""
    x = np.asarray(x, dtype=np.float64)
    N, H = x.shape
    V = len(rowptr) - 1
    out, mag = np.zeros((V, H)), np.zeros((V, H))
    npieces = [len(p) for p in pieces(rowptr, S)]
    n = np.diff(np.asarray(rowptr, dtype=np.int64))
    for r in range(V):
        for e in range(int(rowptr[r]), int(rowptr[r + 1])):
            if 0 <= col[e] < N:
                t = (1.0 if val is None else float(val[e])) * x[col[e]]
                out[r] += t
                mag[r] += np.abs(t)
    k = np.maximum(n + np.asarray(npieces) - 1, 0)
    return out, gamma(k)[:, None] * mag


def sddmm_64(rowptr, col, x, g, vec):
    """(d, bound) in float64: d[e] = sum_c g[r, c] x[col[e], c].

    Bound.  A lane chains m = ceil(H / (64 vec)) vec fmaf (one rounding each, the padding columns add exact zeros), then its partial
    passes the six levels of the lane tree, one rounded addition each: no term sees more than m + 6 roundings, hence
        |fp32 - exact| <= gamma_(m + 6) sum_c |g[r, c] x[col[e], c]|."""
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    N, H = x.shape
    m = -(-H // (64 * vec)) * vec
    d, mag = np.zeros(len(col)), np.zeros(len(col))
    for r in range(len(rowptr) - 1):
        for e in range(int(rowptr[r]), int(rowptr[r + 1])):
            if 0 <= col[e] < N:
                t = g[r] * x[col[e]]
                d[e], mag[e] = t.sum(), np.abs(t).sum()
    return d, gamma(m + 6) * mag


# ---- the case table --------------------------------------------------------------------------------------------------------
def _table(S):
    """name -> dict(deg = slots per row, H, what = what the case is for, want = {row: its piece lengths}, and optionally
    offset (x / out start one float into their storage), val (False: NULL), N (rows of x, when fewer than the V nodes))"""
    short = [3, 0, 1, 0, 0, 7, 2, 0, 5, 1, 0, 0, 0, 9, 4, 0, 2, 6, 0, 1]
    tail = [1, 3, 0, 2, 4]                                    # more nodes, so that uncut rows name rows of x beyond the planted ones
    return {
        "single": dict(deg=[1], H=1, what="V = E = H = 1", want={0: [1]}),
        "short": dict(deg=short, H=4, what="one slice of many short rows with empty rows between them", want={}),
        "straddle": dict(deg=[S - 3, 8, 5, 2, 6] + tail, H=4, what="a row covering [S - 3, S + 5)", want={1: [3, 5]}),
        "abut": dict(deg=[S - 10, 10, 12, 3, 0, 4] + tail, H=4, what="a row ending exactly at S, the next starting at S: no cut",
                     want={0: [S - 10], 1: [10], 2: [12]}),
        "one-slice": dict(deg=[S, S, 5, 1, 2] + tail, H=4, what="a row that is exactly one slice", want={0: [S], 1: [S]}),
        "two-slices": dict(deg=[2 * S, 5, 3, 0, 1] + tail, H=4, what="a row that is exactly two slices", want={0: [S, S]}),
        "hub": dict(deg=[S - 1, 2 * S + 2, 4, 0, 3] + tail, H=8, what="a hub starting at S - 1 of length 2 S + 2", want={1: [1, S, S, 1]}),
        "meet": dict(deg=[S - 5, 45, S - 20, 7, 3] + tail, H=4,
                     what="two cut rows meeting inside one slice: one ends there, the next starts there and runs on",
                     want={1: [5, 40], 2: [S - 40, 20]}),
        "empties": dict(deg=[0, 0, 0, 20, 0, S, 0, 30, 0, 0], H=4, val=False,
                        what="leading and trailing empty rows, the last slice partial, val NULL", want={5: [S - 20, 20]}),
        "scalar": dict(deg=[S - 1, 2 * S + 2, 4, 0, 3] + tail, H=10, what="H = 10: the scalar sweep (VEC 1)", want={1: [1, S, S, 1]}),
        "two-sweeps": dict(deg=[S - 3, 8, 5, 2, 6] + tail, H=300, what="H = 300: 16-byte sweeps, the second one partial", want={1: [3, 5]}),
        "offset": dict(deg=[S - 5, 45, S - 20, 7, 3] + tail, H=8, offset=1, what="H = 8 with x / out one float off alignment (VEC 1)",
                       want={1: [5, 40], 2: [S - 40, 20]}),
        "no-val": dict(deg=[S - 3, 8, 5, 2, 6] + tail, H=8, val=False, what="val NULL across a cut", want={1: [3, 5]}),
        "outside": dict(deg=[7, 0, 3, S, 5, 9, 2, 4, 1, 6, 0, 8], H=4, N=7, what="N < V: source ids >= N are skipped",
                        want={3: [S - 10, 10]}),
    }


def names():
    return list(_table(slice_len()))


def vec_of(H, offset):
    return 4 if H % 4 == 0 and not offset else 1


def _mixed(rs, shape):
    """fp32 of mixed sign and magnitude: a normal deviate (kept away from 0) times 2^-6 .. 2^6"""
    a = rs.standard_normal(shape)
    a = np.where(np.abs(a) < 0.05, 0.05, a)
    return (a * 2.0 ** rs.randint(-6, 7, size=shape)).astype(np.float32)


def planted(rowptr, S):
    """[(row, b)]: for every cut row its first slice boundary b (a slot on either side of it and one more behind)"""
    out = []
    for r in range(len(rowptr) - 1):
        lo, hi = int(rowptr[r]), int(rowptr[r + 1])
        b = (lo // S + 1) * S
        if b < hi:
            assert b + 1 < hi, "a cut row of the table needs two slots behind its first boundary"
            out.append((r, b))
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs of a case (made once, shared, read-only): rowptr int64[V + 1], col int32[E] (edges grouped by target row),
    val fp32[E] or None, x fp32[N, H], g fp32[V, H] (a gradient of out), and the same edges grouped by source node: s_rowptr,
    s_col (= target), s_val, index (val[index] = s_val), built with a stable sort as ps_csr_build builds them.

    Nodes 0, 1, 2 carry the planted rows x = 2^24 + 2^22, 1, -3 * 2^22 in every column, and around the first slice boundary b
    inside a cut row the slots b - 1, b, b + 1 name them with val = 1.  Every other slot of a cut row names node 3 or 4, whose x
    are even integers of mixed sign and magnitude below 2^10, with val in {1, 2, -1, -2}: a piece's sum of those stays below
    2^22, so every partial sum of such a row is an integer that fp32 holds exactly -- except where the 1 meets a sum of 2^24 or
    more (spacing 2), which rounds it away.  With the pieces cut at multiples of S the 1 starts a piece, 1 - 3 * 2^22 + ... is
    exact and the row's value, 2^23 + 1 + an even number, is odd; any order that adds the 1 to the 2^24 + 2^22 (another slice
    length, one chain) gives an even value.  All other rows, val and g are floats of mixed sign and magnitude (a normal deviate
    times 2^-6 .. 2^6)."""
    S = slice_len()
    t = dict(_table(S)[name])
    rs = np.random.RandomState(4200 + names().index(name))
    deg = np.asarray(t["deg"], dtype=np.int64)
    V, H = len(deg), t["H"]
    N = t.get("N", V)
    rowptr = np.zeros(V + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    E = int(rowptr[V])
    col = rs.randint(3 if V > 3 else 0, V, size=E).astype(np.int32)
    val = _mixed(rs, E) if t.get("val", True) else None
    x = _mixed(rs, (N, H))
    g = _mixed(rs, (V, H))
    plants = planted(rowptr, S)
    if plants:
        x[0], x[1], x[2] = BIG + BIG / 4, np.float32(1.0), -3 * BIG / 4
        x[3:5] = rs.choice([-2.0, 2.0], size=(2, H)) * 2.0 ** rs.randint(0, 7, size=(2, H)) * rs.randint(1, 8, size=(2, H))
        for r, p in enumerate(pieces(rowptr, S)):
            if len(p) > 1:
                lo, hi = int(rowptr[r]), int(rowptr[r + 1])
                col[lo:hi] = rs.randint(3, 5, size=hi - lo)
                if val is not None:
                    val[lo:hi] = rs.choice([1.0, 2.0, -1.0, -2.0], size=hi - lo)
        for _, b in plants:
            col[b - 1:b + 2] = [0, 1, 2]
            if val is not None:
                val[b - 1:b + 2] = 1.0
    rows = np.repeat(np.arange(V), deg)
    index = np.argsort(col, kind="stable")
    s_rowptr = np.zeros(V + 1, dtype=np.int64)
    s_rowptr[1:] = np.cumsum(np.bincount(col, minlength=V))
    out = dict(name=name, what=t["what"], want=t["want"], S=S, V=V, N=N, E=E, H=H, offset=t.get("offset", 0),
               vec=vec_of(H, t.get("offset", 0)), rowptr=rowptr, col=col, val=val, x=x, g=g, rows=rows, plants=plants,
               s_rowptr=s_rowptr, s_col=rows[index].astype(np.int32), s_val=None if val is None else val[index], index=index)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement's results for a case (computed once): out (target CSR), dx (source CSR over g), dval"""
    c = case(name)
    return dict(out=spmm_exact(c["rowptr"], c["col"], c["val"], c["x"], c["S"]),
                dx=spmm_exact(c["s_rowptr"], c["s_col"], c["s_val"], c["g"], c["S"]),
                dval=sddmm_exact(c["rowptr"], c["col"], c["x"], c["g"], c["vec"]))
