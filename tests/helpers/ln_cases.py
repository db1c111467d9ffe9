"""Exact numpy restatements of ps_layer_norm and ps_layer_norm_bwd (csrc/layer_norm.hip, as include/pinsage_hip.h states them), their
float64 closed forms with derived bounds, a restatement of the launchers (`facts`: coverage proof and messages only, never an
expected value) and the case table both test files share: tests/test_ln_cases.py (CPU: the restatements against the closed forms
and the closed forms against torch float64 autograd) and tests/test_hip_layer_norm.py (GPU: the kernels against the restatements,
bit for bit).  numpy only.

The restatements (ln_fwd_exact, ln_bwd_exact) are ONE function per direction, parametrised only by VEC.  Every fp32
product-and-add is spmm_cases._fma, every lane sum bn_cases.wave_sum, the fp64 column sums bn_bwd_cases.col_sums; numpy's fp32
sqrt, division, subtraction and product are correctly rounded, as the kernel's are.  A dead row (live <= 0) is never read: its y,
mean, rstd and gx are +0.0 and it adds (+0.0, +0.0) to the columns, whatever x and gy hold there.

Closed forms, in float64 from the same fp32 operands.  ln_fwd_64: mean = sum_c x / N, var = sum_c (x - mean)^2 / N, rstd = 1 /
sqrt(var + eps), xh = (x - mean) rstd, y = xh gamma + beta.  ln_bwd_64 (mean and rstd given, the kernel's own inputs): gg = gy
gamma, k1 = sum_c gg / N, k2 = sum_c gg xh / N, gx = rstd (gg - k1 - xh k2), dbeta = sum_r gy, dgamma = sum_r gy xh over the live
rows.  With the exact mean and rstd this is the gradient of F.layer_norm followed by the torch.where (tests/test_ln_cases.py holds
it to torch's autograd).

Bounds (u = 2^-24, first order with a factor 1.01 for the second-order terms).  A row sum is 64 lane chains of at most n = sweeps
VEC terms, one rounding each, and a tree of 6 additions: a term passes at most a = n + 6 roundings.
 forward (ln_fwd_bound), per row, A = sum_c |x|:
  mean  the sum: a u A; the division by (float)N (exact: N < 2^24) rounds once: Em = a u A / N + u |mean|
  d     the subtraction rounds once from a moved mean: Ed = Em + u |d|
  Q     every term d^2 moves by 2 |d| Ed; the fmaf chain and the tree: a u Q.  EQ = sum_c 2 |d| Ed + a u Q
  var   Ev = EQ / N + u var;  w = var + eps rounds once: Ew = Ev + u w
  rstd  the root and the division round once each, w moves by Ew: Er = rstd (Ew / (2 w) + 2 u)
  xh    Ex = rstd Ed + |d| Er + u |xh|
  y     the fmaf rounds once: Ey = |gamma| Ex + u |y|
 backward (ln_bwd_bound), from the given mean and rstd:
  xh    d and the product round once each: Ex = 2 u |xh|;  gg rounds once: Eg = u |gg|
  c1    Ec1 = (1 + a) u sum_c |gg|;  c2: a term gg xh moves by 3 u |gg xh|: Ec2 = (3 + a) u sum_c |gg xh|
  k     the division rounds once: Ek1 = Ec1 / N + u |k1|, Ek2 = Ec2 / N + u |k2|
  gx    w = gg - k1 rounds once, fmaf(-xh, k2, w) once, the product with rstd once:
        Egx = rstd (Eg + Ek1 + Ex |k2| + |xh| Ek2 + 3 u (|gg| + |k1| + |xh k2|))
  S1    gy is exact; the fp64 sums add at most M 2^-52 sum_r |gy|; dbeta = fp32(S1): Edb = u |S1| + M 2^-52 sum_r |gy|
  S2    Edg = sum_r |gy| Ex + u |S2| + M 2^-52 sum_r |gy xh|
The planted rows (below) are outside every bound: they exist for the bit-for-bit comparison."""
import functools

import numpy as np

from helpers import bn_bwd_cases as bb
from helpers import bn_cases as bc
from helpers.spmm_cases import _fma

U32 = 2.0 ** -24
BN_ROWS, LN_UNROLL, KEEP = 128, 4, 4        # csrc/col_sums.h: PS_BN_ROWS; csrc/layer_norm.hip: LN_UNROLL; csrc/row_sweep.h: PS_LN_KEEP
EPS = 1e-5                                  # nn.LayerNorm's default
CONST = bc.CONST                            # 3.703125: N copies of it add without rounding


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _cdiv(a, b):
    return -(-a // b)


# ---- the launchers, restated ---------------------------------------------------------------------------------------------------
def facts(M, N, x_off=0):
    """ps_layer_norm's and ps_layer_norm_bwd's decisions (csrc/layer_norm.hip); x_off = x starts that many floats past a 16-byte
    boundary"""
    vec = 4 if N % 4 == 0 and x_off % 4 == 0 else 1
    chunk = 64 * vec
    P = _cdiv(M, BN_ROWS)
    steps = []                                  # per partition length: unroll steps of waves 0..3 in ln_bwd_partial_kernel
    for rows in {min(BN_ROWS, M - p * BN_ROWS) for p in (0, P - 1)}:
        steps.append(tuple(_cdiv(_cdiv(max(rows - w, 0), 4), LN_UNROLL) for w in range(4)))
    return dict(vec=vec, P=P, col_blocks=_cdiv(N, chunk), sweeps=_cdiv(N, chunk), tail_cols=N - (_cdiv(N, chunk) - 1) * chunk,
                last_rows=M - (P - 1) * BN_ROWS, ragged_steps=any(max(s) >= 2 and min(s) < max(s) for s in steps),
                finish_unrolled=P // 32, finish_rest=P % 32, row_blocks=_cdiv(M, 4), aligned=x_off % 4 == 0,
                workspace_bytes=P * 2 * N * 8)


GATES = {
    "minimum": lambda f: f["P"] == 1 and f["last_rows"] == 1 and f["col_blocks"] == 1 and f["tail_cols"] == 1,
    "VEC 1, one partial sweep": lambda f: f["vec"] == 1 and f["sweeps"] == 1 and 1 < f["tail_cols"] < 64,
    "one partition, one row short": lambda f: f["P"] == 1 and f["last_rows"] == BN_ROWS - 1,
    "exactly one partition": lambda f: f["P"] == 1 and f["last_rows"] == BN_ROWS,
    "a one-row second partition": lambda f: f["P"] == 2 and f["last_rows"] == 1,
    "unroll steps of unequal count": lambda f: f["ragged_steps"],
    "VEC 1 by N, second column block": lambda f: f["vec"] == 1 and f["aligned"] and f["col_blocks"] >= 2,
    "VEC 4, second sweep and second column block": lambda f: f["vec"] == 4 and f["sweeps"] >= 2 and f["col_blocks"] >= 2,
    "VEC 1 by alignment": lambda f: f["vec"] == 1 and not f["aligned"],
    "VEC 4: exactly KEEP sweeps": lambda f: f["vec"] == 4 and f["sweeps"] == KEEP,
    "VEC 4: one beyond KEEP": lambda f: f["vec"] == 4 and f["sweeps"] == KEEP + 1,
    "VEC 1: exactly KEEP sweeps": lambda f: f["vec"] == 1 and f["sweeps"] == KEEP,
    "VEC 1: one beyond KEEP": lambda f: f["vec"] == 1 and f["sweeps"] == KEEP + 1,
    "long rows": lambda f: f["sweeps"] >= KEEP + 2,
    "finish: unroll plus a remainder": lambda f: f["finish_unrolled"] >= 1 and f["finish_rest"] >= 1,
}

# (name, M, N, x_off, gates).  Every row has a wave of its own in both directions: there is no grid-stride pass to open.
CASES = (
    ("min", 1, 1, 0, ("minimum",)),
    ("vec1-partial", 3, 3, 0, ("VEC 1, one partial sweep",)),
    ("p127", 127, 4, 0, ("one partition, one row short",)),
    ("p128", 128, 4, 0, ("exactly one partition",)),
    ("p129", 129, 4, 0, ("a one-row second partition",)),
    ("ragged-steps", 161, 8, 0, ("unroll steps of unequal count",)),
    ("vec1-2blocks", 129, 65, 0, ("VEC 1 by N, second column block", "a one-row second partition")),
    ("vec4-2blocks", 37, 260, 0, ("VEC 4, second sweep and second column block",)),
    ("vec1-offset", 129, 256, 1, ("VEC 1 by alignment", "VEC 1: exactly KEEP sweeps")),
    ("v4-keep", 5, 1024, 0, ("VEC 4: exactly KEEP sweeps",)),
    ("v4-keep+1", 5, 1028, 0, ("VEC 4: one beyond KEEP",)),
    ("v1-keep", 5, 256, 1, ("VEC 1: exactly KEEP sweeps", "VEC 1 by alignment")),
    ("v1-keep+1", 5, 257, 0, ("VEC 1: one beyond KEEP",)),
    ("long", 3, 2052, 0, ("long rows",)),
    ("finish-unroll", 4229, 8, 0, ("finish: unroll plus a remainder",)),
)
NAMES = tuple(c[0] for c in CASES)
MASKS = ("none", "all dead", "first row dead", "last row of a partition dead", "a wholly dead partition")


def case(name):
    return CASES[NAMES.index(name)]


def mask(which, M):
    """int32 [M] or None: the `live` vector of a MASKS entry (live rows carry 1 or 7, dead rows 0 or -1)"""
    if which == "none":
        return None
    live = np.where(np.arange(M) % 3 == 0, 7, 1).astype(np.int32)
    dead = {"all dead": np.arange(M), "first row dead": np.array([0]),
            "last row of a partition dead": np.array([min(BN_ROWS, M) - 1]),
            "a wholly dead partition": np.arange(min(BN_ROWS, M))}[which]
    live[dead] = np.where(dead % 2 == 0, 0, -1)
    live.setflags(write=False)
    return live


def alive_rows(live, M):
    return np.ones(M, dtype=bool) if live is None else np.asarray(live) > 0


def poison(a, live):
    """a copy of a [M, N] whose dead rows hold NaN and Inf: the kernels do not read them"""
    a = np.array(a, dtype=np.float32)
    dead = ~alive_rows(live, a.shape[0])
    fill = np.where(np.arange(a.shape[1]) % 2 == 0, np.float32(np.nan), np.float32(np.inf)).astype(np.float32)
    a[dead] = fill[None, :]
    return a


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _ro(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def data(name, plants=True):
    """Inputs of a CASES row (made once, shared, read-only): x N(0.3, 1.5), gy N(0, 1), gamma U(0.5, 1.5), beta N(0, 0.5).
    plants=True adds, for M >= 5 (rows M // 2 ...):
      const_row    every element CONST: the sum is exact, var == 0, rstd = 1 / sqrtf(eps), y = beta
      hundred_row  100 +- 0.05: the row a single-pass variance loses
      zero_row     zeros
    and, for N >= 8 and M >= 69, order_cols: two columns of gy that are zero but for 2^53, 1, 1, -2^53 in rows chosen so that the
    column's fp64 sum depends on the order of the waves and on the partition length (bn_bwd_cases.data).  nan_row names the row
    with_nan() plants a NaN in."""
    _, M, N, _, _ = case(name)
    rs = np.random.RandomState(9100 + 1000 * N + M % 997)
    x = (0.3 + 1.5 * rs.standard_normal((M, N))).astype(np.float32)
    gy = rs.standard_normal((M, N)).astype(np.float32)
    gamma = rs.uniform(0.5, 1.5, N).astype(np.float32)
    beta = (0.5 * rs.standard_normal(N)).astype(np.float32)
    rows = dict(const_row=None, hundred_row=None, zero_row=None, nan_row=None, order_cols=None)
    if plants and M >= 5:
        r = M // 2
        rows.update(const_row=r, hundred_row=r + 1, zero_row=r - 1, nan_row=r - 2)
        x[r] = CONST
        x[r + 1] = (100.0 + 0.05 * rs.standard_normal(N)).astype(np.float32)
        x[r - 1] = 0.0
    if plants and N >= 8 and M >= 69:
        B = np.float32(2.0 ** 53)
        gy[:, 3:5] = 0.0
        gy[[0, 1, 2, 3], 3] = (B, 1.0, 1.0, -B)         # one row per wave: ((B + 1) + 1) - B = 0, but (B + 1) + (1 - B) = 1
        gy[[0, 4, 64, 68], 4] = (B, 1.0, 1.0, -B)       # wave 0 of partition 0: 0 in one chain, 1 when row 64 opens a new partition
        rows.update(order_cols=(3, 4))
    return _ro(dict(M=M, N=N, x=x, gy=gy, gamma=gamma, beta=beta, **rows))


def with_nan(d):
    """x of data(...) with one NaN, in the last column of nan_row"""
    x = np.array(d["x"])
    x[d["nan_row"], d["N"] - 1] = np.nan
    return x


# ---- the kernels, exactly --------------------------------------------------------------------------------------------------------
VARIANTS = ("a sequential wave sum", "the chains in plain column order", "single-pass E[x^2] - mean^2",
            "waves added as (s0 + s1) + (s2 + s3)", "k1 and k2 from fp64")


def row_sum(a, b, vec, variant=None):
    """fp32 [M]: the wave sum of the lane chains acc = acc + a (b None) or acc = fmaf(a, b, acc) over the columns 64 VEC k + VEC
    lane + e, sweep k and element e ascending, from +0.0.  A column past N adds +0.0 (no change: a chain from +0.0 never is -0.0)."""
    M, N = a.shape

    def step(acc, p, q):
        return (acc + p).astype(np.float32) if q is None else _fma(p, q, acc)
    with np.errstate(invalid="ignore", over="ignore"):
        if variant == VARIANTS[1]:
            acc = np.zeros(M, dtype=np.float32)
            for c in range(N):
                acc = step(acc, a[:, c], None if b is None else b[:, c])
            return acc
        chunk = 64 * vec
        sweeps = _cdiv(N, chunk)

        def lanes(t):
            tp = np.zeros((M, sweeps * chunk), dtype=np.float32)
            tp[:, :N] = t
            return tp.reshape(M, sweeps, 64, vec)
        ap, bp = lanes(a), (None if b is None else lanes(b))
        acc = np.zeros((M, 64), dtype=np.float32)
        for k in range(sweeps):
            for e in range(vec):
                acc = step(acc, ap[:, k, :, e], None if bp is None else bp[:, k, :, e])
        if variant == VARIANTS[0]:
            s = acc[:, 0]
            for lane in range(1, 64):
                s = (s + acc[:, lane]).astype(np.float32)
            return s
        return bc.wave_sum(acc)


def ln_fwd_exact(x, gamma, beta, eps, live, vec, variant=None):
    """ps_layer_norm restated: dict(y fp32 [M, N], mean fp32 [M], rstd fp32 [M])"""
    x, gamma, beta = _f(x), _f(gamma), _f(beta)
    M, N = x.shape
    alive = alive_rows(live, M)
    x = np.where(alive[:, None], x, np.float32(0.0)).astype(np.float32)          # a dead row is not read
    Nf = np.float32(N)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mean = (row_sum(x, None, vec, variant) / Nf).astype(np.float32)
        d = (x - mean[:, None]).astype(np.float32)
        if variant == VARIANTS[2]:
            ex2 = (row_sum(x, x, vec) / Nf).astype(np.float32)
            var = (ex2 - (mean * mean).astype(np.float32)).astype(np.float32)
        else:
            var = (row_sum(d, d, vec, variant) / Nf).astype(np.float32)
        rstd = (np.float32(1.0) / np.sqrt((var + np.float32(eps)).astype(np.float32))).astype(np.float32)
        xh = (d * rstd[:, None]).astype(np.float32)
        y = _fma(xh, gamma[None, :], beta[None, :])
    zero = np.float32(0.0)
    return dict(y=_f(np.where(alive[:, None], y, zero)), mean=_f(np.where(alive, mean, zero)), rstd=_f(np.where(alive, rstd, zero)))


def ln_bwd_exact(x, gy, mean, rstd, gamma, live, vec, variant=None):
    """ps_layer_norm_bwd restated: dict(gx fp32 [M, N], dgamma fp32 [N], dbeta fp32 [N])"""
    x, gy, mean, rstd, gamma = (_f(a) for a in (x, gy, mean, rstd, gamma))
    M, N = x.shape
    alive = alive_rows(live, M)
    x = np.where(alive[:, None], x, np.float32(0.0)).astype(np.float32)          # a dead row is not read
    gy = np.where(alive[:, None], gy, np.float32(0.0)).astype(np.float32)
    Nf = np.float32(N)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = (x - mean[:, None]).astype(np.float32)
        xh = (d * rstd[:, None]).astype(np.float32)
        gg = (gy * gamma[None, :]).astype(np.float32)
        k1 = (row_sum(gg, None, vec, variant) / Nf).astype(np.float32)
        k2 = (row_sum(gg, xh, vec, variant) / Nf).astype(np.float32)
        if variant == VARIANTS[4]:
            k1 = (gg.astype(np.float64).sum(axis=1) / N).astype(np.float32)
            k2 = ((gg.astype(np.float64) * xh.astype(np.float64)).sum(axis=1) / N).astype(np.float32)
        w = (gg - k1[:, None]).astype(np.float32)
        gx = (rstd[:, None] * _fma(-xh, k2[:, None], w)).astype(np.float32)
        gx = np.where(alive[:, None], gx, np.float32(0.0))
        cv = bb.VARIANTS[0] if variant == VARIANTS[3] else None
        a64 = np.where(alive[:, None], gy.astype(np.float64), 0.0)               # a dead row adds (+0.0, +0.0)
        b64 = np.where(alive[:, None], gy.astype(np.float64) * xh.astype(np.float64), 0.0)
        S1, S2 = bb.col_sums(a64, cv), bb.col_sums(b64, cv)
    return dict(gx=_f(gx), dgamma=_f(S2.astype(np.float32)), dbeta=_f(S1.astype(np.float32)))


@functools.lru_cache(maxsize=None)
def expected(name, which="none", plants=True, nan=False):
    """dict(y, mean, rstd, gx, dgamma, dbeta) of a CASES row under a MASKS entry; the backward from the forward's mean and rstd"""
    d = data(name, plants)
    vec = facts(d["M"], d["N"], case(name)[3])["vec"]
    live = mask(which, d["M"])
    x = with_nan(d) if nan else d["x"]
    out = ln_fwd_exact(x, d["gamma"], d["beta"], EPS, live, vec)
    out.update(ln_bwd_exact(x, d["gy"], out["mean"], out["rstd"], d["gamma"], live, vec))
    return _ro(out)


# ---- the closed forms and their bounds ---------------------------------------------------------------------------------------------
def ln_fwd_64(x, gamma, beta, eps, live):
    """dict(y, mean, rstd and the intermediates d, xh, var) in float64 (module docstring); eps as the kernel receives it"""
    x, gamma, beta = (np.asarray(a, dtype=np.float64) for a in (x, gamma, beta))
    alive = alive_rows(live, x.shape[0])
    x = np.where(alive[:, None], x, 0.0)
    mean = x.mean(axis=1)
    d = x - mean[:, None]
    var = (d * d).mean(axis=1)
    rstd = 1.0 / np.sqrt(var + np.float64(np.float32(eps)))
    xh = d * rstd[:, None]
    y = xh * gamma + beta
    return dict(y=np.where(alive[:, None], y, 0.0), mean=np.where(alive, mean, 0.0), rstd=np.where(alive, rstd, 0.0), d=d, xh=xh,
                var=var, x=x)


def _depth(N, vec):
    return _cdiv(N, 64 * vec) * vec + 6


def ln_fwd_bound(x, gamma, beta, eps, live, vec):
    """dict(y, mean, rstd): fp64 bounds on |ln_fwd_exact - ln_fwd_64| (module docstring); zero in dead rows"""
    r = ln_fwd_64(x, gamma, beta, eps, live)
    alive = alive_rows(live, r["x"].shape[0])
    N = r["x"].shape[1]
    a = _depth(N, vec)
    g = np.abs(np.asarray(gamma, dtype=np.float64))
    d, xh = np.abs(r["d"]), np.abs(r["xh"])
    rstd_full = 1.0 / np.sqrt(r["var"] + np.float64(np.float32(eps)))
    Em = a * U32 * np.abs(r["x"]).sum(axis=1) / N + U32 * np.abs(r["x"].mean(axis=1))
    Ed = Em[:, None] + U32 * d
    Q = (d * d).sum(axis=1)
    EQ = (2.0 * d * Ed).sum(axis=1) + a * U32 * Q
    w = r["var"] + np.float64(np.float32(eps))
    Ew = EQ / N + U32 * r["var"] + U32 * w
    Er = rstd_full * (Ew / (2.0 * w) + 2.0 * U32)
    Ex = rstd_full[:, None] * Ed + d * Er[:, None] + U32 * xh
    Ey = g[None, :] * Ex + U32 * np.abs(xh * g[None, :] + np.asarray(beta, dtype=np.float64)[None, :])
    return dict(y=1.01 * np.where(alive[:, None], Ey, 0.0), mean=1.01 * np.where(alive, Em, 0.0), rstd=1.01 * np.where(alive, Er, 0.0))


def ln_bwd_64(x, gy, mean, rstd, gamma, live):
    """dict(gx, dgamma, dbeta and the intermediates xh, gg, k1, k2) in float64 (module docstring) for the given mean and rstd"""
    x, gy, mean, rstd, gamma = (np.asarray(a, dtype=np.float64) for a in (x, gy, mean, rstd, gamma))
    alive = alive_rows(live, x.shape[0])
    x, gy = np.where(alive[:, None], x, 0.0), np.where(alive[:, None], gy, 0.0)
    N = x.shape[1]
    xh = (x - mean[:, None]) * rstd[:, None]
    gg = gy * gamma[None, :]
    k1, k2 = gg.sum(axis=1) / N, (gg * xh).sum(axis=1) / N
    gx = rstd[:, None] * (gg - k1[:, None] - xh * k2[:, None])
    xh, gx = np.where(alive[:, None], xh, 0.0), np.where(alive[:, None], gx, 0.0)
    return dict(gx=gx, dgamma=(gy * xh).sum(axis=0), dbeta=gy.sum(axis=0), xh=xh, gg=gg, k1=k1, k2=k2, gy=gy, rstd=rstd)


def ln_bwd_bound(x, gy, mean, rstd, gamma, live, vec):
    """dict(gx, dgamma, dbeta): fp64 bounds on |ln_bwd_exact - ln_bwd_64| (module docstring)"""
    r = ln_bwd_64(x, gy, mean, rstd, gamma, live)
    M, N = r["gy"].shape
    a = _depth(N, vec)
    xh, gg, gyb, rs = np.abs(r["xh"]), np.abs(r["gg"]), np.abs(r["gy"]), np.abs(r["rstd"])
    k1, k2 = np.abs(r["k1"]), np.abs(r["k2"])
    Ex, Eg = 2.0 * U32 * xh, U32 * gg
    Ek1 = (1 + a) * U32 * gg.sum(axis=1) / N + U32 * k1
    Ek2 = (3 + a) * U32 * (gg * xh).sum(axis=1) / N + U32 * k2
    Egx = rs[:, None] * (Eg + Ek1[:, None] + Ex * k2[:, None] + xh * Ek2[:, None] + 3.0 * U32 * (gg + k1[:, None] + xh * k2[:, None]))
    Edb = U32 * np.abs(r["dbeta"]) + M * 2.0 ** -52 * gyb.sum(axis=0)
    Edg = (gyb * Ex).sum(axis=0) + U32 * np.abs(r["dgamma"]) + M * 2.0 ** -52 * (gyb * xh).sum(axis=0)
    return dict(gx=1.01 * Egx, dgamma=1.01 * Edg, dbeta=1.01 * Edb)


def autograd_64(x, gy, gamma, beta, eps, live):
    """torch CPU float64 autograd of F.layer_norm followed by the torch.where over the live rows: dict(y, gx, dgamma, dbeta)"""
    import torch
    import torch.nn.functional as F
    xt, gt, bt = (torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True) for a in (x, gamma, beta))
    y = F.layer_norm(xt, (xt.size(1),), gt, bt, float(np.float32(eps)))
    if live is not None:
        y = torch.where(torch.tensor(np.asarray(live) > 0)[:, None], y, torch.zeros_like(y))
    y.backward(torch.tensor(np.asarray(gy, dtype=np.float64)))
    return dict(y=y.detach().numpy(), gx=xt.grad.numpy(), dgamma=gt.grad.numpy(), dbeta=bt.grad.numpy())


mismatches = bb.mismatches
outside = bb.outside
