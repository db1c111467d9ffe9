"""The case table of the ranking losses (csrc/loss.hip: hardest_rows_kernel, hinge_rows_kernel, mean_kernel, loss_bwd_rows_kernel,
loss_bwd_scatter_kernel; the shared-candidate arg-max is csrc/dense_mfma.hip's EPI 3), numpy only.

include/pinsage_hip.h states the bits: "every product and sum is one rounded fp32 operation in the order written; sums over rows
are taken in ascending row order by one wave", and the library is built with -ffp-contract=off.  Two restatements of that
sentence live here and must agree word for word (tests/test_loss_cases.py): the plain-C one (oracle.c_oracle.hardest_negative /
margin_loss / margin_loss_bwd) and a numpy-float32 one (np_forward / np_backward: every statement one operation on float32
arrays, which numpy rounds once).  tests/test_hip_loss_matrix.py holds the kernels to the C one, bit for bit.

The launcher is restated (facts) only to prove that each case reaches the branch it names and to word failure messages, never
to compute an expected value.

Data.  `unit`: Gaussian / sqrt(D) with magnitudes kept in [2^-10, 4], margin 0.1 -- everything rounds, so a summation order
shows.  `levels`: values in {-1, -1/2, 0, 1/2, 1}, Q live in its first four columns, margin 0.25 -- every operation of the
forward is exact, maxima tie and the hinge lands on 0 exactly; the second half of the candidates repeats the first, so a row's
maximum is attained twice.  Planted in both kinds:
  * HUB rows -- 0, 3, 6, ... below 600, and row 64 -- carry Q_0: with shared candidates they share one arg-max, in many 64-row
    groups and on both sides of the first ballot boundary (63 | 64, 66);
  * even rows (but 64) have P_b = pscale * Q_b and are mostly inactive, so the even hub rows are inactive rows that a wrong mask
    would add; row 64 has P = -Q and is active.  pscale is 1 unless the case says otherwise: where the candidates are many the
    largest similarity beats |q|^2 and the positives are scaled up until enough rows are inactive.
`levels` with B >= 63 also has row 1 with l == 0 exactly and row 5 with l == margin (_plant_hinge_edges); `unit` with shared
candidates repeats candidate 0 as the last one, which is then never the smallest index of a maximum: a dX row of +0.0.
"""
import functools
import os
import sys
import zlib
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

f32 = np.float32
SHARED, PER_QUERY, BATCH_HARD = 0, 1, 2                     # PS_LOSS_* of include/pinsage_hip.h
MODE_NAMES = {SHARED: "shared", PER_QUERY: "per-query", BATCH_HARD: "batch-hard"}
FORM = {SHARED: "shared", PER_QUERY: "perq", BATCH_HARD: "bh"}      # the closed form's names
MARGIN = {"unit": 0.1, "levels": 0.25}
THREADS = 8

# ------------------------------------------------------------------------------------------------------ the launcher, restated
BALLOT = 64                               # rows per ballot of loss_bwd_scatter_kernel's scan
ROW_STRIDE = 64                           # columns per stride of loss_bwd_rows_kernel (one wave per row)
COL_PASS = 256                            # columns per pass of loss_bwd_scatter_kernel (64 lanes x SCAT_KC = 4)
BWD_WAVES = 4096 * 4                      # both backward kernels: at most 4096 blocks of 4 waves, one row / candidate per wave
HARDEST_THREADS = 4096 * 256              # hardest_rows_kernel: one (b, n) per thread
HINGE_THREADS = 4096 * 64                 # hinge_rows_kernel: one row per thread
MEAN_THREADS = 1024                       # mean_kernel: one block


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------- cases
LossCase = namedtuple("LossCase", "name mode B N D kind pscale gos unaligned forward_only reaches")
GOS = (1.0, 0.3)


def _lc(mode, B, N, D, reaches, kinds=("unit", "levels"), pscale=1, gos=GOS, unaligned=False, forward_only=False):
    out = []
    for kind in kinds:
        ps = pscale[kind] if isinstance(pscale, dict) else pscale
        name = f"{MODE_NAMES[mode]}-B{B}-N{N}-D{D}-{kind}" + ("-unaligned" if unaligned else "") + ("-fwd" if forward_only else "")
        out.append(LossCase(name, mode, B, N, D, kind, ps, tuple(gos), unaligned, forward_only, reaches))
    return out


CASES = tuple(
    _lc(SHARED, 1, 1, 1, "minimum of everything", kinds=("unit",))
    + _lc(SHARED, 63, 7, 3, "ragged ballot, scalar chain")
    + _lc(SHARED, 64, 37, 4, "one full ballot, smallest vector chain")
    + _lc(SHARED, 65, 37, 36, "second ballot of one row; hub on rows 63 and 64")
    + _lc(SHARED, 130, 9, 64, "exactly one 64-column stride in the rows kernel")
    + _lc(SHARED, 300, 500, 65, "column 64 alone in a second stride", pscale={"unit": 1, "levels": 2})
    + _lc(SHARED, 1025, 33, 256, "mean_kernel thread 0 sums two elements; scatter: exactly one 256-column pass")
    + _lc(SHARED, 1030, 11, 257, "scatter second column pass of one column", gos=GOS + (-1.7,))
    + _lc(SHARED, 200, 50, 260, "vector chain, partial second pass")
    + _lc(SHARED, 77, 16, 516, "three column passes")
    + _lc(SHARED, 16389, 40, 8, "rows kernel's grid-stride second pass (4096 x 4 waves)", kinds=("unit",), pscale=2)
    + _lc(SHARED, 700, 16389, 8, "scatter kernel's grid-stride second pass", kinds=("unit",), pscale=2)
    + _lc(SHARED, 130, 37, 36, "Q, P, X each one float off a 16-byte boundary", unaligned=True)
    + _lc(SHARED, 262147, 3, 4, "hinge_rows_kernel second pass; 257 elements per mean_kernel thread", kinds=("unit",),
          forward_only=True)
    + _lc(PER_QUERY, 1, 1, 1, "minimum", kinds=("unit",))
    + _lc(PER_QUERY, 65, 7, 36, "dX zero fill around the hit")
    + _lc(PER_QUERY, 130, 1, 64, "N = 1: every hit is index 0")
    + _lc(PER_QUERY, 33, 9, 257, "scalar chain, ragged columns")
    + _lc(PER_QUERY, 2100, 500, 4, "hardest_rows_kernel second pass (B N > 1 048 576)", pscale={"unit": 2, "levels": 2})
    + _lc(PER_QUERY, 65, 7, 36, "unaligned bases: Q, P, X each one float off a 16-byte boundary", unaligned=True)
    + _lc(BATCH_HARD, 1, 1, 5, "no candidate: idx -1, sim -inf, every gradient a zero", kinds=("unit",))
    + _lc(BATCH_HARD, 2, 2, 4, "each row's only candidate is the other")
    + _lc(BATCH_HARD, 65, 65, 36, "ballot boundary", pscale={"unit": 1, "levels": 2})
    + _lc(BATCH_HARD, 130, 130, 64, "two full ballots and two rows, one 64-column stride")
    + _lc(BATCH_HARD, 1025, 1025, 257, "column passes + mean", pscale={"unit": 1, "levels": 2})
    + _lc(BATCH_HARD, 16389, 16389, 8, "both grid caps at once", kinds=("unit",), pscale=2)
)
BY_NAME = {c.name: c for c in CASES}
NULL_SUBSET_CASES = {SHARED: "shared-B65-N37-D36-unit", PER_QUERY: "per-query-B65-N7-D36-unit", BATCH_HARD: "batch-hard-B65-N65-D36-unit"}


def facts(c):
    """what the restated launcher says of case c"""
    B, N, D = c.B, c.N, c.D
    return dict(
        ballots=_cdiv(B, BALLOT), last_ballot_rows=B - (_cdiv(B, BALLOT) - 1) * BALLOT,
        row_strides=_cdiv(D, ROW_STRIDE), last_stride_cols=D - (_cdiv(D, ROW_STRIDE) - 1) * ROW_STRIDE,
        col_passes=_cdiv(D, COL_PASS), last_pass_cols=D - (_cdiv(D, COL_PASS) - 1) * COL_PASS,
        vector_chain=D % 4 == 0 and not c.unaligned,
        rows_second_pass=not c.forward_only and B > BWD_WAVES, scatter_second_pass=not c.forward_only and N > BWD_WAVES,
        hardest_second_pass=c.mode == PER_QUERY and B * N > HARDEST_THREADS,
        hinge_second_pass=B > HINGE_THREADS, mean_elements=_cdiv(B, MEAN_THREADS))


# ----------------------------------------------------------------------------------------------------------------------- data

def _seed(name):
    return zlib.crc32(name.encode()) & 0x7fffffff


def hub_rows(B):
    """the rows that carry Q_0"""
    h = set(range(0, min(B, 600), 3))
    if B > 64:
        h.add(64)
    return np.array(sorted(h), dtype=np.int64)


def near_rows(B):
    """the rows whose positive is pscale * Q_b"""
    r = np.arange(0, B, 2)
    return r[r != 64]


def _values(rs, shape, kind, D):
    if kind == "levels":
        return (rs.randint(-2, 3, size=shape) * 0.5).astype(f32)
    v = (rs.standard_normal(shape) / np.sqrt(D)).astype(f32)
    return np.where(v < 0, f32(-1), f32(1)) * np.clip(np.abs(v), f32(2.0 ** -10), f32(4.0))


LossData = namedtuple("LossData", "Q P X margin")
EDGE_ROWS = (1, 5)                        # levels, B >= 63: row 1 has l == 0 exactly, row 5 has l == margin


def _plant_hinge_edges(mode, Q, P, X):
    """levels data: rows 1 and 5 (odd, no hub rows) get Q = 1/2 in one column and P chosen in that column so that
    l = (margin + sim) - pos is exactly 0 (row 1: inactive, on the edge) and exactly margin (row 5: the first step above it).
    Every product and sum of levels is exact, so float64 gives the chain's similarity.  Row 5's positive lives in another column
    than row 1's query and is planted second, so as a batch-hard candidate it adds a similarity of 0 to row 1."""
    margin = MARGIN["levels"]
    for col, (r, l) in enumerate(zip(EDGE_ROWS, (0.0, margin))):
        Q[r] = 0.0
        Q[r, col] = 0.5
        P[r] = 0.0
        if mode == BATCH_HARD:
            s = np.delete(P.astype(np.float64) @ Q[r].astype(np.float64), r)
        else:
            s = (X[r] if mode == PER_QUERY else X).astype(np.float64) @ Q[r].astype(np.float64)
        P[r, col] = 2.0 * (margin + float(s.max()) - l)                    # pos = P / 2 = margin + sim - l
        assert abs(P[r, col]) <= 4.0


@functools.lru_cache(maxsize=3)
def loss_data(c):
    """Q [B, D], P [B, D], X ([N, D] shared, [B, N, D] per-query, None batch-hard), margin.  The unaligned twin of a case has the
    same name but for its suffix and so the same seed: equal data."""
    rs = np.random.RandomState(_seed("loss" + c.name.replace("-unaligned", "")))
    B, N, D, kind = c.B, c.N, c.D, c.kind
    Q, P = _values(rs, (B, D), kind, D), _values(rs, (B, D), kind, D)
    if kind == "levels":
        Q[:, 4:] = 0.0
    Q[hub_rows(B)] = Q[0]
    near = near_rows(B)
    P[near] = np.clip(f32(c.pscale) * Q[near], f32(-4.0), f32(4.0))
    if B > 64:
        P[64] = -Q[64]
    X = None
    if c.mode != BATCH_HARD:
        X = _values(rs, (N, D) if c.mode == SHARED else (B, N, D), kind, D)
        if kind == "levels" and N >= 2:
            h = N // 2
            X[..., h:2 * h, :] = X[..., :h, :]
        elif c.mode == SHARED and N >= 2:
            X[N - 1] = X[0]                                                # never the SMALLEST index of a maximum: its dX row is +0.0
    if kind == "levels" and B >= 63:
        _plant_hinge_edges(c.mode, Q, P, X)
    for a in (Q, P, X):
        if a is not None:
            a.setflags(write=False)
    return LossData(Q, P, X, MARGIN[kind])


# ------------------------------------------------------------------------------------------------------------ the C oracle's leg
Forward = namedtuple("Forward", "sim idx pos row_loss active loss")


def c_chain_rows(Q, P):
    """pos_b = the C fmaf chain of Q_b . P_b (orc_hardest_negative over one candidate per row)"""
    from oracle import c_oracle as co
    return co.hardest_negative(Q, P[:, None, :], per_query=True, threads=THREADS)[0]


@functools.lru_cache(maxsize=3)
def c_forward(c):
    from oracle import c_oracle as co
    d = loss_data(c)
    if c.mode == BATCH_HARD:
        sim, idx = co.hardest_negative(d.Q, d.P, exclude_diag=True, threads=THREADS)
    else:
        sim, idx = co.hardest_negative(d.Q, d.X, per_query=c.mode == PER_QUERY, threads=THREADS)
    row_loss, active, loss = co.margin_loss(d.Q, d.P, sim, d.margin)
    out = Forward(sim, idx, c_chain_rows(d.Q, d.P), row_loss, active, np.array([loss], dtype=f32))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=4)
def c_backward(c, go):
    """{dQ, dP, dX (not batch-hard)} of the C oracle for grad_out = float32(go)"""
    from oracle import c_oracle as co
    d, fw = loss_data(c), c_forward(c)
    out = co.margin_loss_bwd(d.Q, d.P, d.X, c.mode, fw.idx, fw.active, f32(go))
    for a in out.values():
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ the numpy-float32 restatement

def np_mean(v, sequential=False):
    """mean_kernel: 1024 strided partial sums from +0.0, the tree s[i] += s[i + w] for w = 512 .. 1, s[0] / (float)B.
    sequential=True is the plain left-to-right sum, which the teeth test must tell apart."""
    v = np.ascontiguousarray(v, dtype=f32)
    B = v.size
    if sequential:
        return np.array([np.add.accumulate(v, dtype=f32)[-1] / f32(B)], dtype=f32)
    s = np.zeros(MEAN_THREADS, dtype=f32)
    for r0 in range(0, B, MEAN_THREADS):
        chunk = v[r0:r0 + MEAN_THREADS]
        s[:chunk.size] = s[:chunk.size] + chunk
    w = MEAN_THREADS // 2
    while w > 0:
        s[:w] = s[:w] + s[w:2 * w]
        w //= 2
    return np.array([s[0] / f32(B)], dtype=f32)


def np_forward(sim, pos, margin, sequential_mean=False):
    """(row_loss, active, loss) from the C chain's sim and pos"""
    ms = f32(margin) + sim
    l = ms - pos
    neg = l <= 0
    row_loss = np.where(neg, f32(0), l).astype(f32)
    return row_loss, (~neg).astype(np.uint8), np_mean(row_loss, sequential_mean)


def _pairwise(terms):
    if len(terms) == 1:
        return terms[0]
    h = len(terms) // 2
    return _pairwise(terms[:h]) + _pairwise(terms[h:])


def feeders(idx, active, N, j):
    """the rows whose g Q_b the scatter sum of candidate j adds, ascending"""
    return np.flatnonzero((np.asarray(active) != 0) & (idx == j) & (idx >= 0) & (idx < N))


def np_backward(Q, P, X, mode, idx, active, go, order="ascending", g_form="quotient", drop=None):
    """{dQ, dP, dX}: the header's formulas, each statement one float32 operation.  order / g_form / drop are the deviations the
    teeth test plants: the scatter sum "descending" or as a pairwise "tree", g = go * (1.0f / B) ("reciprocal"), one feeding row
    left out."""
    B, D = Q.shape
    N = B if mode == BATCH_HARD else X.shape[1] if mode == PER_QUERY else X.shape[0]
    Bf = f32(B)
    g = f32(go) / Bf if g_form == "quotient" else f32(go) * (f32(1.0) / Bf)
    hit = (idx >= 0) & (idx < N)
    on = (np.asarray(active) != 0) & hit
    gb = np.where(on, g, f32(0)).astype(f32)[:, None]
    ng = -gb
    a = np.where(hit, idx, 0)
    cand = P if mode == BATCH_HARD else X
    xa = cand[np.arange(B), a] if mode == PER_QUERY else cand[a]
    t = np.where(hit[:, None], gb * xa, f32(0)).astype(f32)
    u = ng * P
    out = {"dQ": t + u}
    if mode != BATCH_HARD:
        out["dP"] = ng * Q
    if mode == PER_QUERY:
        dX = np.zeros((B, N, D), dtype=f32)
        rows = np.flatnonzero(hit)
        dX[rows, a[rows]] = (gb * Q)[rows]
        out["dX"] = dX
        return out
    GQ = (g * Q).astype(f32)
    acc = np.zeros((N, D), dtype=f32)
    rows = [int(b) for b in np.flatnonzero(on) if b != drop]
    if order == "tree":
        groups = {}
        for b in rows:
            groups.setdefault(int(idx[b]), []).append(GQ[b])
        for j, terms in groups.items():
            acc[j] = acc[j] + _pairwise(terms)
    else:
        for b in (rows if order == "ascending" else rows[::-1]):
            acc[idx[b]] = acc[idx[b]] + GQ[b]
    if mode == BATCH_HARD:
        out["dP"] = (ng * Q) + acc
    else:
        out["dX"] = acc
    assert all(v.dtype == f32 for v in out.values())
    return out


# -------------------------------------------------------------------------------------------------------- the fp64 closed form

def _closed_form(Q, P, X, idx, active, form, go=1.0):
    """the gradient of include/pinsage_hip.h in float64; X as the form takes it ([N, D], [B, H, D] or [B, D])"""
    Q, P = Q.astype(np.float64), P.astype(np.float64)
    B = Q.shape[0]
    rows = np.arange(B)
    g = np.where(active, go / B, 0.0)[:, None]
    if form == "bh":
        dP = -g * Q
        np.add.at(dP, idx, g * Q)
        return g * P[idx] + (-g * P), dP, None
    X = X.astype(np.float64)
    dX = np.zeros_like(X)
    if form == "shared":
        np.add.at(dX, idx, g * Q)
        return g * X[idx] + (-g * P), -g * Q, dX
    if form == "twod":
        dX[:] = g * Q
        return g * X + (-g * P), -g * Q, dX
    dX[rows, idx] = g * Q
    return g * X[rows, idx] + (-g * P), -g * Q, dX


def _closed_form_magnitude(Q, P, X, idx, active, form, go=1.0):
    """per gradient entry (sum of the magnitudes of its terms, number of terms): the closed form over absolute values"""
    aQ, aP = np.abs(Q), np.abs(P)
    ones = np.ones_like(Q)
    if form == "bh":                                  # dQ = g p_a - g p, dP = -g q + sum: every term with a plus sign
        g, a = np.where(active, go / Q.shape[0], 0.0)[:, None], active[:, None] * ones
        mP, cP = g * aQ, a.copy()
        np.add.at(mP, idx, g * aQ)
        np.add.at(cP, idx, a)
        return {"dQ": (g * (aP[idx] + aP), 2 * a), "dP": (mP, cP)}
    aX = np.abs(X)
    mags = _closed_form(aQ, -aP, aX, idx, active, form, go)                   # -(-g |p|): every term enters with a plus sign
    cnts = _closed_form(ones, -ones, np.ones_like(X), idx, active, form, float(Q.shape[0]))
    return {k: (np.abs(m), np.abs(c)) for k, m, c in zip(("dQ", "dP", "dX"), mags, cnts) if m is not None}


def closed_form_violations(c, go, grads, limit=4):
    """(tensor, row, col, got, want, tolerance) where a float32 gradient of case c leaves terms x ulp(magnitude sum) around the
    fp64 closed form over the oracle's indices and mask, or is zero where the closed form is not (tests/test_hip_loss.py's bound).

    The bound counts the roundings of an entry of n terms: n products and n - 1 sums (batch-hard dP: n sums), each at most half
    an ulp of a partial magnitude sum, n ulp together.  It has no room for the rounding of g = grad_out / B itself, which is
    RELATIVE (2^-24) and so reaches a whole ulp of an entry at the top of its binade: a single product g q can be 1.5 ulp from the
    fp64 value (seen on this table at grad_out 0.3: 1.02 ulp).  The header makes g one fp32 division, so the closed form is
    evaluated at that g -- computed here in numpy, never taken from the oracle, and required to be the correctly rounded fp64
    quotient -- and the bound then holds for what it counts."""
    d, fw = loss_data(c), c_forward(c)
    g32 = f32(go) / f32(c.B)
    exact = float(f32(go)) / c.B
    assert abs(float(g32) - exact) <= 0.5 * float(np.spacing(np.abs(g32)))
    gof = float(g32) * c.B                                                 # 24 x 18 bits: exact in fp64, and gof / B is g32 again
    assert gof / c.B == float(g32)
    form = FORM[c.mode]
    idx = np.where(fw.idx < 0, 0, fw.idx)                                  # a row without a candidate is inactive: g = 0
    act = (fw.active != 0) & (fw.idx >= 0)
    cf = dict(zip(("dQ", "dP", "dX"), _closed_form(d.Q, d.P, d.X, idx, act, form, gof)))
    mag = _closed_form_magnitude(d.Q, d.P, d.X, idx, act, form, abs(gof))
    bad = []
    for which, got in grads.items():
        want = cf[which]
        msum, terms = mag[which]
        tol = np.maximum(terms, 1) * np.spacing(np.abs(msum).astype(f32)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - want)
        wrong = (err > tol) | ((got == 0) != (want == 0))
        g2, w2, t2 = got.reshape(-1, c.D), want.reshape(-1, c.D), tol.reshape(-1, c.D)
        for r, k in np.argwhere(wrong.reshape(-1, c.D))[:limit]:
            bad.append((which, int(r), int(k), float(g2[r, k]), float(w2[r, k]), float(t2[r, k])))
    return bad


# ------------------------------------------------------------------------------------------------------------- the comparison
FILL = 0xFF                               # the byte every output buffer and guard band holds before a call
Mismatch = namedtuple("Mismatch", "row col got want what")


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def mismatches(got, want, limit=4):
    """first `limit` Mismatch(row, col, got, want, what) where two arrays differ in their BITS (-0.0 is not +0.0).  what is
    "not written" where the word still holds the fill pattern (and the oracle's does not), else "differs".  Arrays of one
    dimension are a column; three dimensions [B, N, D] report row b * N + n."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    cols = got.shape[-1] if got.ndim >= 2 else 1
    g, w = _words(got).reshape(-1, cols), _words(want).reshape(-1, cols)
    gv, wv = got.reshape(-1, cols), want.reshape(-1, cols)
    pattern = g.dtype.type(np.iinfo(g.dtype).max)
    return [Mismatch(int(r), int(k), gv[r, k].item(), wv[r, k].item(), "not written" if g[r, k] == pattern else "differs")
            for r, k in np.argwhere(g != w)[:limit]]


def report(c, tensor, got, want, idx=None, active=None, limit=4):
    """the failure lines of one tensor of case c (empty: equal bits).  For a scatter output (idx / active given) each line lists
    the rows that feed the entry."""
    lines = []
    for m in mismatches(got, want, limit):
        line = (f"case {c.name} ({c.reaches}): {tensor} row {m.row} column {m.col} {m.what}: got {m.got!r} want {m.want!r}")
        if idx is not None:
            fed = feeders(idx, active, want.shape[0], m.row)
            line += f"; fed by rows {fed.tolist()}" + (f" (ballots {sorted(set((fed // BALLOT).tolist()))})" if fed.size else "")
        lines.append(line)
    return lines


def scatter_tensor(mode):
    """the output loss_bwd_scatter_kernel writes, or None"""
    return {SHARED: "dX", BATCH_HARD: "dP"}.get(mode)
