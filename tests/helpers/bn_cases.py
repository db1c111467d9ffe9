"""The batch-norm kernels (csrc/batch_norm.hip: ps_bn_batch_stats, ps_bn_apply) held to their documented operation order: a case
table whose rows name the launcher gate they reach, a restatement of the launchers (`facts`: coverage proof and messages only,
never an expected value), and exact restatements of the two entry points.  numpy only: shared by tests/test_bn_cases.py (CPU)
and tests/test_hip_bn_matrix.py (GPU).

ps_bn_batch_stats, in fp64 (stats_exact)
  partition p = rows 128 p .. 128 p + 127; wave w of the partition's four adds (double) z and its square -- exact in fp64: 24-bit
  significands -- of rows r0 + w, r0 + w + 4, ... one after the other from +0.0; the partial is ((s0 + s1) + s2) + s3; the
  partitions are added in ascending order from 0.0; m = S / M; v = max(Q / M - m * m, 0) with the product and the difference
  rounded separately (-ffp-contract=off); scale = gamma / sqrt(v + (double)(float) eps); the running statistics become
  (1.0 - mom) old + mom new with mom = (double)(float) momentum, each product and the sum rounded, the variance entering as
  v * (M / (M - 1)).
  The sums are exact restatements: the workspace equals them bit for bit.  The three fp64 divisions (S / M and Q / M, the
  scale's, M / (M - 1)) are not: the instruction sequence the compiler emits for an fp64 `/` is faithful but not always
  correctly rounded (csrc/ps_common.h), so each quotient is carried as the interval of its two neighbours unless it is exact -- a
  faithful division returns an exact quotient as it is -- and, to be on the safe side, so is the square root.  An fp32 output is
  DECIDED when both ends of its interval round to the same fp32; the data is chosen so that every column of every case is
  (tests/test_bn_cases.py asserts it), and the GPU test demands equality without exceptions.
  The constant column is CONST = 3.703125 (8 significant bits) and not layers_cases' 3.7f: its squares have 16 bits, every sum
  of them is exact, so the mean is CONST and the variance +0.0 exactly.  With 3.7f the variance is the cancellation residue of
  a rounded sum, of the order of one fp64 ulp of Q / M, which no faithful division decides.

ps_bn_apply, in fp32 (apply_exact)
  t = fmaf(z - mean, scale, beta), the subtraction rounded; ReLU: t < 0 -> +0.0 (NaN and -0.0 pass); PS_L2NORM: lane l chains
  acc = fmaf(t, t, acc) over its columns k * 64 * VEC + l * VEC + e (sweep k, element e, ascending, past KEEP sweeps too), the
  64 lanes are added by ps_wave_sum_f32's balanced tree (wave_sum), nrm = max(sqrtf(sum), 1e-12f) -- a NaN sum stays NaN, as
  torch's clamp_min keeps it -- and y = t / nrm with fp32 sqrt and division correctly rounded."""
import functools
from fractions import Fraction

import numpy as np

BN_ROWS, BN_UNROLL, KEEP = 128, 8, 4        # csrc/col_sums.h: PS_BN_ROWS; csrc/batch_norm.hip
GRID_X_CAP = 65535                          # bn_partial_kernel's grid.x
ROW_GRID_CAP = 256 * 16                     # ps_row_grid() (csrc/ps_common.h): workgroups of four waves
EPS, MOMENTUM = 1e-5, 0.1                   # nn.BatchNorm1d's defaults
CONST = np.float32(3.703125)
OUTPUTS = ("mean", "var", "scale", "rm", "rv")


def _cdiv(a, b):
    return -(-a // b)


def _fmaf_vec(a, b, c):
    """fp32 fma with one rounding (oracle/pinsage_oracle.py)"""
    from oracle.pinsage_oracle import _fmaf_vec as f
    return f(np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32), np.asarray(c, dtype=np.float32))


# ---- case tables ---------------------------------------------------------------------------------------------------------------
# (name, M, N, z_off, gate): z_off = z starts that many floats past a 16-byte boundary
STATS_CASES = (
    ("min", 2, 1, 0, "minimum, VEC 1"),
    ("p127", 127, 4, 0, "one partition, one row short; VEC 4"),
    ("p128", 128, 4, 0, "exactly one partition"),
    ("p129", 129, 4, 0, "a one-row second partition"),
    ("ragged-steps", 161, 8, 0, "second partition of 33 rows: wave 0 needs a second unroll step, the others do not"),
    ("vec1-2blocks", 129, 65, 0, "aligned base, VEC 1, second column block of one column"),
    ("vec4-2blocks", 37, 260, 0, "VEC 4, second column block of one float4"),
    ("vec1-offset", 129, 256, 1, "VEC 1 from alignment, four column blocks"),
    ("finish-unroll", 4229, 8, 0, "P = 34: bn_finish_kernel's 32-deep unroll plus a remainder"),
    ("partial-second-pass", 8388609, 4, 0, "P = 65 537: blocks 0 and 1 take a second partition"),
)
# (name, M, N, z_off, vec_off, gate): vec_off = beta alone starts one float past a 16-byte boundary
APPLY_CASES = (
    ("min", 1, 1, 0, 0, "minimum"),
    ("v4-keep", 5, 1024, 0, 0, "VEC 4: exactly KEEP sweeps"),
    ("v4-keep+1", 5, 1028, 0, 0, "VEC 4: one float4 beyond KEEP sweeps"),
    ("v4-long", 3, 2052, 0, 0, "VEC 4: five sweeps beyond"),
    ("v1-keep", 5, 256, 1, 0, "VEC 1 from a one-float offset of z: exactly KEEP sweeps"),
    ("v1-keep+1", 5, 257, 0, 0, "VEC 1 by N % 4: one column beyond"),
    ("v1-long", 3, 515, 0, 0, "VEC 1 by N % 4: five sweeps beyond"),
    ("rows-second-pass", 16389, 8, 0, 0, "second grid-stride pass"),
    ("v1-by-beta", 9, 1028, 0, 1, "VEC 1 chosen by a column vector, 17 sweeps"),
)
STATS_NAMES = tuple(c[0] for c in STATS_CASES)
APPLY_NAMES = tuple(c[0] for c in APPLY_CASES)


def stats_case(name):
    return STATS_CASES[STATS_NAMES.index(name)]


def apply_case(name):
    return APPLY_CASES[APPLY_NAMES.index(name)]


# ---- the launchers, restated (csrc/batch_norm.hip: ps_bn_batch_stats, ps_bn_apply) ---------------------------------------------
def stats_facts(M, N, z_off=0):
    vec = 4 if N % 4 == 0 and z_off % 4 == 0 else 1
    P = _cdiv(M, BN_ROWS)
    gx = min(P, GRID_X_CAP)
    steps = []                                  # per partition length: unroll steps of waves 0..3
    for rows in {min(BN_ROWS, M - p * BN_ROWS) for p in (0, P - 1)}:
        steps.append(tuple(_cdiv(_cdiv(max(rows - w, 0), 4), BN_UNROLL) for w in range(4)))
    return dict(kernel="stats", vec=vec, P=P, grid=(gx, _cdiv(N, 64 * vec)), passes=_cdiv(P, gx), col_blocks=_cdiv(N, 64 * vec),
                last_rows=M - (P - 1) * BN_ROWS, wave_steps=tuple(sorted(steps)),
                ragged_steps=any(max(s) >= 2 and min(s) < max(s) for s in steps),
                finish_unrolled=P // 32, finish_rest=P % 32, workspace_bytes=P * 2 * N * 8)


def apply_facts(M, N, z_off=0, vec_off=0):
    vec = 4 if N % 4 == 0 and z_off % 4 == 0 and vec_off % 4 == 0 else 1
    chunk = 64 * vec
    sweeps = _cdiv(N, chunk)
    grid = min(_cdiv(M, 4), ROW_GRID_CAP)
    return dict(kernel="apply", vec=vec, sweeps=sweeps, fits=N <= KEEP * chunk, beyond=max(sweeps - KEEP, 0),
                tail_cols=N - (sweeps - 1) * chunk, grid=grid, passes=_cdiv(M, 4 * grid))


def facts(case):
    """the launcher's decisions for a row of STATS_CASES or APPLY_CASES"""
    if len(case) == 5:
        return stats_facts(*case[1:4])
    return apply_facts(*case[1:5])


# the gates tests/helpers/layers_cases.py's tables do not reach (tests/test_bn_cases.py proves both halves)
GATES = {
    "bn_apply_kernel<4>: long row": lambda f: f["kernel"] == "apply" and f["vec"] == 4 and not f["fits"],
    "bn_apply_kernel<1>: long row, two or more sweeps beyond KEEP": lambda f: f["kernel"] == "apply" and f["vec"] == 1 and f["beyond"] >= 2,
    "bn_apply_kernel: second grid-stride pass": lambda f: f["kernel"] == "apply" and f["passes"] >= 2,
    "bn_partial_kernel: second pass of the partition loop": lambda f: f["kernel"] == "stats" and f["passes"] >= 2,
    "bn_partial_kernel: unroll steps of unequal count": lambda f: f["kernel"] == "stats" and f["ragged_steps"],
}


# ---- inputs --------------------------------------------------------------------------------------------------------------------
LEVELS = 16                                 # the large case draws z from this many fp32 values per column
SEEDS = {"p127": 7001}                      # name -> seed, where the default leaves a column undecided (the planted column's
#                                             variance: kappa = 4e6 times the quotients' two ulps is 4 % of an fp32 half-ulp)


def _ro(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=2)
def stats_data(name):
    """Inputs of a STATS_CASES row (made once, shared, read-only), as layers_cases.stats_case: N(0.3, 1.5) columns; column 0
    has mean 100 and standard deviation 0.05 (E[z^2] / var = 4e6); for N >= 2 the last column is the constant CONST.  Above
    2^20 rows every column takes LEVELS fp32 values drawn that way (a table lookup: generation stays well under a second)."""
    _, M, N, _, _ = stats_case(name)
    rs = np.random.RandomState(SEEDS.get(name, 7000 + 1000 * N + M % 997))
    if M <= 1 << 20:
        z = (0.3 + 1.5 * rs.standard_normal((M, N))).astype(np.float32)
        z[:, 0] = (100.0 + 0.05 * rs.standard_normal(M)).astype(np.float32)
        if N >= 2:
            z[:, N - 1] = CONST
    else:
        table = (0.3 + 1.5 * rs.standard_normal((N, LEVELS))).astype(np.float32)
        table[0] = (100.0 + 0.05 * rs.standard_normal(LEVELS)).astype(np.float32)
        table[N - 1] = CONST
        z = np.empty((M, N), dtype=np.float32)
        for c in range(N):
            z[:, c] = table[c][rs.randint(0, LEVELS, size=M, dtype=np.uint8)]
    gamma = rs.uniform(0.5, 1.5, N).astype(np.float32)
    rm0 = rs.standard_normal(N).astype(np.float32)
    rv0 = rs.uniform(0.5, 2.0, N).astype(np.float32)
    return _ro(dict(M=M, N=N, z=z, gamma=gamma, rm0=rm0, rv0=rv0))


@functools.lru_cache(maxsize=None)
def apply_data(name):
    """Inputs of an APPLY_CASES row: z as above with two planted rows (M >= 3), a mean / positive scale / beta, and
      neg_row   a row so far below `mean` that fmaf(z - mean, scale, beta) < 0 in every column (layers_cases' all-negative row)
      nan_row   a row with a NaN in its last column (the last sweep)"""
    _, M, N, _, _, _ = apply_case(name)
    rs = np.random.RandomState(9000 + 1000 * N + M % 997)
    z = (0.3 + 1.5 * rs.standard_normal((M, N))).astype(np.float32)
    z[:, 0] = (100.0 + 0.05 * rs.standard_normal(M)).astype(np.float32)
    if N >= 2:
        z[:, N - 1] = CONST
    beta = (0.5 * rs.standard_normal(N)).astype(np.float32)
    mean = z.astype(np.float64).mean(axis=0).astype(np.float32)
    scale = rs.uniform(0.5, 2.0, N).astype(np.float32)
    neg_row = nan_row = None
    if M >= 3:
        neg_row, nan_row = M // 2, M // 2 + 1
        z[neg_row] = mean - (np.abs(beta) / scale + 1.0 + np.abs(rs.standard_normal(N))).astype(np.float32)
        z[nan_row, N - 1] = np.nan
    return _ro(dict(M=M, N=N, z=z, mean=mean, scale=scale, beta=beta, neg_row=neg_row, nan_row=nan_row))


# ---- ps_bn_batch_stats, exactly ------------------------------------------------------------------------------------------------
VARIANTS_STATS = ("waves added as (s0 + s1) + (s2 + s3)", "partitions of 64 rows", "a single-pass fp32 square")


def partials(z, variant=None):
    """double[P, 2, N]: what bn_partial_kernel leaves in the workspace"""
    z = np.asarray(z, dtype=np.float32)
    M, N = z.shape
    rows = 64 if variant == VARIANTS_STATS[1] else BN_ROWS
    P = _cdiv(M, rows)
    if P * rows == M:
        zp = z
    else:
        zp = np.zeros((P * rows, N), dtype=np.float32)       # a row past the end adds +0.0: no change (a sum from +0.0 is never -0.0)
        zp[:M] = z
    zp = zp.reshape(P, rows // 4, 4, N)
    s = np.zeros((P, 4, N), dtype=np.float64)
    q = np.zeros((P, 4, N), dtype=np.float64)
    for t in range(rows // 4):
        zt = zp[:, t]
        d = zt.astype(np.float64)
        s += d
        q += (zt * zt).astype(np.float64) if variant == VARIANTS_STATS[2] else d * d
    out = np.empty((P, 2, N), dtype=np.float64)
    for k, a in enumerate((s, q)):
        if variant == VARIANTS_STATS[0]:
            out[:, k] = (a[:, 0] + a[:, 1]) + (a[:, 2] + a[:, 3])
        else:
            out[:, k] = ((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]
    return out


def _is_exact_quotient(q, a, b):
    return np.array([Fraction(float(x)) == Fraction(float(y)) * Fraction(float(z)) for x, y, z in
                     np.broadcast(np.asarray(a, dtype=np.float64), np.asarray(q, dtype=np.float64), np.asarray(b, dtype=np.float64))],
                    dtype=bool).reshape(np.shape(q))


def _around(q, exact=None):
    """(lo, hi): the fp64 neighbours of q, q itself where `exact`"""
    lo, hi = np.nextafter(q, -np.inf), np.nextafter(q, np.inf)
    if exact is not None:
        lo, hi = np.where(exact, q, lo), np.where(exact, q, hi)
    return lo, hi


def _div(a, b):
    """a / b rounded to nearest, and the interval a faithful division may return"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    q = a / b
    return (q,) + _around(q, _is_exact_quotient(q, a, b))


def _span(*cands):
    c = np.stack([np.asarray(a, dtype=np.float64) for a in cands])
    return c.min(axis=0), c.max(axis=0)


def stats_exact(z, gamma, rm0=None, rv0=None, eps=EPS, momentum=MOMENTUM, variant=None):
    """ps_bn_batch_stats restated.  Returns a dict: part (double[P, 2, N]), the fp32 outputs mean / var / scale and, with running
    statistics, rm / rv, and decided[name] (bool[N]): the fp32 rounding does not depend on how the fp64 divisions (and the
    square root) round, see the module docstring."""
    z = np.asarray(z, dtype=np.float32)
    M, N = z.shape
    part = partials(z, variant)
    tot = np.cumsum(np.concatenate([np.zeros((1, 2, N)), part]), axis=0)[-1]           # ascending, from 0.0
    S, Q = tot[0], tot[1]
    Md = np.float64(M)
    eps, mom = np.float64(np.float32(eps)), np.float64(np.float32(momentum))
    g = np.asarray(gamma, dtype=np.float32).astype(np.float64)

    def var_of(e, m):
        return np.maximum(e - m * m, 0.0)

    m, m_lo, m_hi = _div(S, Md)
    e, e_lo, e_hi = _div(Q, Md)
    v = var_of(e, m)
    v_lo, v_hi = _span(*[var_of(ee, mm) for ee in (e_lo, e, e_hi) for mm in (m_lo, m, m_hi)])

    def scale_span(vv):
        r = np.sqrt(vv + eps)
        out = []
        for rr in (np.nextafter(r, -np.inf), r, np.nextafter(r, np.inf)):
            out.extend((g / rr,) + _around(g / rr))
        return out

    sc = g / np.sqrt(v + eps)
    sc_lo, sc_hi = _span(*(scale_span(v_lo) + scale_span(v_hi)))
    val = {"mean": (m, m_lo, m_hi), "var": (v, v_lo, v_hi), "scale": (sc, sc_lo, sc_hi)}
    if rm0 is not None:
        ratio, ratio_lo, ratio_hi = _div(Md, Md - 1.0)
        old_m, old_v = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (rm0, rv0))

        def blend(old, new):
            return (1.0 - mom) * old + mom * new
        val["rm"] = (blend(old_m, m),) + _span(blend(old_m, m_lo), blend(old_m, m_hi))
        val["rv"] = (blend(old_v, v * ratio),) + _span(*[blend(old_v, vv * rr) for vv in (v_lo, v_hi) for rr in (ratio_lo, ratio_hi)])
    out = {"part": part, "decided": {}}
    for k, (mid, lo, hi) in val.items():
        out[k] = mid.astype(np.float32)
        out["decided"][k] = (lo.astype(np.float32) == hi.astype(np.float32)) & (lo <= mid) & (mid <= hi)
    return out


@functools.lru_cache(maxsize=2)
def stats_expected(name):
    d = stats_data(name)
    return stats_exact(d["z"], d["gamma"], d["rm0"], d["rv0"])


# ---- ps_bn_apply, exactly ------------------------------------------------------------------------------------------------------
VARIANTS_APPLY = ("the L2 chain in column order", "a sequential wave sum")


def wave_sum(lanes):
    """ps_wave_sum_f32 of fp32 [..., 64]: the six DPP steps add, in turn, lanes one, two, four, eight apart and then the rows of
    sixteen -- a balanced binary tree over the lanes in their order (an fp32 addition commutes, so which side a lane adds its
    partner on does not matter)"""
    a = np.asarray(lanes, dtype=np.float32)
    assert a.shape[-1] == 64
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def prenorm_exact(z, mean, scale, beta, relu):
    z, mean, scale, beta = (np.asarray(a, dtype=np.float32) for a in (z, mean, scale, beta))
    with np.errstate(invalid="ignore"):
        t = _fmaf_vec(z - mean[None, :], np.broadcast_to(scale[None, :], z.shape), np.broadcast_to(beta[None, :], z.shape))
        if relu:
            t = np.where(t < 0, np.float32(0.0), t)
    return t.astype(np.float32)


def sum_squares_exact(t, vec, variant=None):
    """fp32 [M]: the kernel's sum of squares of the rows of t"""
    M, N = t.shape
    chunk = 64 * vec
    sweeps = _cdiv(N, chunk)
    with np.errstate(invalid="ignore"):
        if variant == VARIANTS_APPLY[0]:
            acc = np.zeros(M, dtype=np.float32)
            for c in range(N):
                acc = _fmaf_vec(t[:, c], t[:, c], acc)
            return acc
        tp = np.zeros((M, sweeps * chunk), dtype=np.float32)     # a column past N: fmaf(0, 0, acc) = acc (acc is never -0.0)
        tp[:, :N] = t
        tp = tp.reshape(M, sweeps, 64, vec)
        acc = np.zeros((M, 64), dtype=np.float32)
        for k in range(sweeps):
            for e in range(vec):
                acc = _fmaf_vec(tp[:, k, :, e], tp[:, k, :, e], acc)
        if variant == VARIANTS_APPLY[1]:
            s = acc[:, 0]
            for lane in range(1, 64):
                s = s + acc[:, lane]
            return s
        return wave_sum(acc)


def apply_exact(z, mean, scale, beta, relu, l2, vec, variant=None):
    """ps_bn_apply restated: fp32 [M, N]"""
    t = prenorm_exact(z, mean, scale, beta, relu)
    if not l2:
        return t
    with np.errstate(invalid="ignore"):
        nrm = np.maximum(np.sqrt(sum_squares_exact(t, vec, variant)), np.float32(1e-12))          # np.maximum keeps a NaN
        return (t / nrm[:, None]).astype(np.float32)


def mismatches(got, want, limit=8):
    """first `limit` (row, col, got, want) where two fp32 arrays differ in their bits (-0 is not +0); a NaN equals any NaN"""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    return [(int(r), int(c), float(got[r, c]), float(want[r, c])) for r, c in np.argwhere(~same)[:limit]]
