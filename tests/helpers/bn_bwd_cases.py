"""An exact numpy restatement of ps_bn_bwd (csrc/batch_norm_bwd.hip, as include/pinsage_hip.h states it), its float64 closed form
with a derived bound, a restatement of the launcher (`facts`: coverage proof and messages only, never an expected value) and the
case table both test files share: tests/test_bn_bwd_cases.py (CPU: the restatement against the closed form and against torch
float64 autograd) and tests/test_hip_bn_bwd.py (GPU: the kernels against the restatement, bit for bit).  numpy only.

The restatement (bn_bwd_exact) is ONE function, parametrised only by VEC.  Every
fp32 product-and-add is spmm_cases._fma; t is bn_cases.prenorm_exact (ps_bn_apply's bits), ga is
linear_bwd_cases.epilogue_bwd_exact(t, gy); numpy's fp32 sqrt, division, subtraction and product are correctly rounded, as the
kernel's are.  The fp64 column sums are exact restatements of the summation order (partitions of 128 rows, four strided row subsets
per partition added as ((s0 + s1) + s2) + s3, partitions ascending from 0.0); unlike ps_bn_batch_stats there is no fp64 division
behind them, so every output is decided.

Closed form (bn_bwd_64), in float64 from the same fp32 operands: d = z - mean, a = d scale + beta, t = relu(a), xh = d / sqrt(var +
eps), ga = linear_bwd_cases.epilogue_bwd_64(t, gy), S1 = sum_r ga, S2 = sum_r ga xh, dbeta = S1, dgamma = S2,
gz = scale (ga - S1 / M - xh S2 / M).  With mean, var, scale the exact batch statistics this is the gradient of
F.normalize(F.relu(F.batch_norm(z, training=True))) (tests/test_bn_bwd_cases.py holds it to torch's autograd).

Bound (bn_bwd_bound; u = 2^-24, first order with a factor 1.01 for the second-order terms):
  t     d carries one rounding, the fmaf another: |a32 - a| <= u (|d scale| + |a|) =: et.  The data keeps every |a| at least 1e-4
        (far beyond et, asserted), so the ReLU masks the same elements.
  ga    linear_bwd_cases.epilogue_bound(t, gy) for the computation from a given t, plus -- with the norm -- what moving t by et does
        to it: at most 3 |gy|_2 |et|_2 / c^2 per element of the row (linear_bwd_cases' docstring, `layer`).  Without the norm ga is
        gy or a mask of it: exact.  =: Eg
  xh    var + eps, its root, the reciprocal and the product round once each, d once: |xh32 - xh| <= 5 u |xh| =: Ex
  S1    the fp64 sums add at most M 2^-52 sum |ga| (nothing beside u); dbeta = fp32(S1): Edb = sum_r Eg + u |S1|
  S2    Edg = sum_r (Eg |xh| + |ga| Ex) + u |S2|
  k     k1 = dbeta / fp32(M): Ek1 = Edb / M + 2 u |k1| (M rounded to fp32, the division); k2 likewise
  gz    w = ga - k1 rounds once, fmaf(-xh, k2, w) once, the product with scale once:
        Egz = |scale| (Eg + Ek1 + Ex |k2| + |xh| Ek2 + 3 u (|ga| + |k1| + |xh k2|))
Rows that the ReLU masks entirely are exact zeros on both sides (Eg = 0 there).  The planted rows (below) are outside every bound:
they exist for the bit-for-bit comparison."""
import functools

import numpy as np

from helpers import bn_cases as bc
from helpers import linear_bwd_cases as lb
from helpers.spmm_cases import _fma

U32 = 2.0 ** -24
BN_ROWS, BN_UNROLL = 128, 4                 # csrc/col_sums.h: PS_BN_ROWS; csrc/batch_norm_bwd.hip
KEEP = bc.KEEP                              # ps_bn_apply keeps this many sweeps of a row in registers: where the forward changes path
EPS = bc.EPS
FLAGSETS = lb.FLAGSETS                      # (relu, l2norm)
MIN_PRE = 1e-4                              # every float64 pre-activation outside the planted rows is at least this far from zero


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _cdiv(a, b):
    return -(-a // b)


# ---- the launcher, restated ------------------------------------------------------------------------------------------------------
def facts(M, N, z_off=0):
    """bn_bwd_launch's decisions (csrc/batch_norm_bwd.hip); z_off = z starts that many floats past a 16-byte boundary"""
    vec = 4 if N % 4 == 0 and z_off % 4 == 0 else 1
    chunk = 64 * vec
    P = _cdiv(M, BN_ROWS)
    steps = []                                  # per partition length: unroll steps of waves 0..3 in bn_bwd_partial_kernel
    for rows in {min(BN_ROWS, M - p * BN_ROWS) for p in (0, P - 1)}:
        steps.append(tuple(_cdiv(_cdiv(max(rows - w, 0), 4), BN_UNROLL) for w in range(4)))
    return dict(vec=vec, P=P, col_blocks=_cdiv(N, chunk), sweeps=_cdiv(N, chunk),
                last_rows=M - (P - 1) * BN_ROWS, ragged_steps=any(max(s) >= 2 and min(s) < max(s) for s in steps),
                finish_unrolled=P // 32, finish_rest=P % 32, row_blocks=_cdiv(M, 4), aligned=z_off % 4 == 0,
                workspace_bytes=P * 2 * N * 8 + 16 + 3 * _cdiv(N, 4) * 4 * 4 + M * 8)


GATES = {
    "minimum": lambda f: f["P"] == 1 and f["last_rows"] == 2 and f["col_blocks"] == 1,
    "one partition, one row short": lambda f: f["P"] == 1 and f["last_rows"] == BN_ROWS - 1,
    "exactly one partition": lambda f: f["P"] == 1 and f["last_rows"] == BN_ROWS,
    "a one-row second partition": lambda f: f["P"] == 2 and f["last_rows"] == 1,
    "unroll steps of unequal count": lambda f: f["ragged_steps"],
    "VEC 1 by N, second column block": lambda f: f["vec"] == 1 and f["aligned"] and f["col_blocks"] >= 2,
    "VEC 4, second column block": lambda f: f["vec"] == 4 and f["col_blocks"] >= 2,
    "VEC 1 by alignment": lambda f: f["vec"] == 1 and not f["aligned"],
    "VEC 4: exactly KEEP sweeps": lambda f: f["vec"] == 4 and f["sweeps"] == KEEP,
    "VEC 4: one beyond KEEP": lambda f: f["vec"] == 4 and f["sweeps"] == KEEP + 1,
    "VEC 1: exactly KEEP sweeps": lambda f: f["vec"] == 1 and f["sweeps"] == KEEP,
    "VEC 1: one beyond KEEP": lambda f: f["vec"] == 1 and f["sweeps"] == KEEP + 1,
    "long rows": lambda f: f["sweeps"] >= KEEP + 2,
    "finish: unroll plus a remainder": lambda f: f["finish_unrolled"] >= 1 and f["finish_rest"] >= 1,
}

# (name, M, N, z_off, gates).  No row-per-wave grid is capped (every row has a wave of its own), so there is no second stride pass
# for a 16 389-row case to open.
CASES = (
    ("min", 2, 1, 0, ("minimum",)),
    ("p127", 127, 4, 0, ("one partition, one row short",)),
    ("p128", 128, 4, 0, ("exactly one partition",)),
    ("p129", 129, 4, 0, ("a one-row second partition",)),
    ("ragged-steps", 161, 8, 0, ("unroll steps of unequal count",)),
    ("vec1-2blocks", 129, 65, 0, ("VEC 1 by N, second column block", "a one-row second partition")),
    ("vec4-2blocks", 37, 260, 0, ("VEC 4, second column block",)),
    ("vec1-offset", 129, 256, 1, ("VEC 1 by alignment", "VEC 1: exactly KEEP sweeps")),
    ("v4-keep", 5, 1024, 0, ("VEC 4: exactly KEEP sweeps",)),
    ("v4-keep+1", 5, 1028, 0, ("VEC 4: one beyond KEEP",)),
    ("v1-keep", 5, 256, 1, ("VEC 1: exactly KEEP sweeps", "VEC 1 by alignment")),
    ("v1-keep+1", 5, 257, 0, ("VEC 1: one beyond KEEP",)),
    ("long", 3, 2052, 0, ("long rows",)),
    ("finish-unroll", 4229, 8, 0, ("finish: unroll plus a remainder",)),
)
NAMES = tuple(c[0] for c in CASES)


def case(name):
    return CASES[NAMES.index(name)]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _ro(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _stats(z, gamma):
    """the batch statistics of z in float64, rounded to fp32 as ps_bn_batch_stats leaves them (not its bits: inputs only)"""
    z64 = z.astype(np.float64)
    mean, var = z64.mean(axis=0), z64.var(axis=0)
    return mean.astype(np.float32), var.astype(np.float32), (gamma.astype(np.float64) / np.sqrt(var + np.float64(np.float32(EPS)))).astype(np.float32)


def pre64(z, mean, scale, beta):
    z, mean, scale, beta = (np.asarray(a, dtype=np.float64) for a in (z, mean, scale, beta))
    return (z - mean) * scale + beta


@functools.lru_cache(maxsize=None)
def data(name, plants=True, seed=0):
    """Inputs of a CASES row (made once, shared, read-only), as bn_cases.stats_data: N(0.3, 1.5) columns; column 0 has mean 100
    and standard deviation 0.05; for N >= 2 the last column is the constant bn_cases.CONST, whose variance is exactly 0.  For
    N >= 4 column 1 has gamma = 0 (scale = 0, a negative beta).  mean / var / scale are the float64 statistics of z rounded to fp32.
    Offending z are nudged until every float64 pre-activation is at least MIN_PRE from zero (the statistics made again after
    every nudge: they are z's own).
    plants=True adds, for N >= 4 and M >= 5, AFTER the statistics are made (the kernel takes them as inputs; these rows serve the
    bit-for-bit comparison only):
      clamp_col  column 2 gets mean 0 and beta 0, so that a = fmaf(z, scale, 0) can be planted
      gy0_row    gy = 0
      neg_row    z so far below the mean that every pre-activation is negative: under the ReLU t = 0, the norm is below the clamp
                 and every element is masked
      above_row  neg_row's z with a = 2^-39 in clamp_col (under the ReLU nrm = 1.8e-12, just above the clamp)
      below_row  the same with 2^-41 (4.5e-13, just below)
    and, for N >= 8 and M >= 69, order_cols: two columns of gy that are zero but for 2^53, 1, 1, -2^53 in rows chosen so that the
    column's fp64 sum depends on the order of the waves and on the partition length"""
    _, M, N, _, _ = case(name)
    rs = np.random.RandomState(8000 + 1000 * N + M % 997 + 17 * seed)
    z = (0.3 + 1.5 * rs.standard_normal((M, N))).astype(np.float32)
    z[:, 0] = (100.0 + 0.05 * rs.standard_normal(M)).astype(np.float32)
    if N >= 2:
        z[:, N - 1] = bc.CONST
    gamma = rs.uniform(0.5, 1.5, N).astype(np.float32)
    beta = (0.5 * rs.standard_normal(N)).astype(np.float32)
    beta = np.where(np.abs(beta) < 1e-2, np.float32(1e-2), beta).astype(np.float32)
    if N >= 4:
        gamma[1] = 0.0
        beta[1] = -np.abs(beta[1])
    gy = rs.standard_normal((M, N)).astype(np.float32)
    for _ in range(32):
        mean, var, scale = _stats(z, gamma)
        a = pre64(z, mean, scale, beta)
        bad = (np.abs(a) < 2 * MIN_PRE) & (scale != 0)[None, :]
        if N >= 2:
            bad[:, N - 1] = False                                       # the constant column: a = beta
        if not bad.any():
            break
        z = np.where(bad, z + np.float32(0.01) * np.where(a >= 0, 1, -1).astype(np.float32), z).astype(np.float32)
    else:
        raise AssertionError("no data without a pre-activation near zero")
    rows = dict(gy0_row=None, neg_row=None, above_row=None, below_row=None, clamp_col=None, gamma0_col=1 if N >= 4 else None,
                order_cols=None)
    if plants and N >= 4 and M >= 5:
        mean, beta = mean.copy(), beta.copy()
        mean[2] = 0.0
        beta[2] = 0.0
        a = pre64(z, mean, scale, beta)
        bad = np.abs(a[:, 2]) < 2 * MIN_PRE
        z[bad, 2] = np.float32(0.01)
        neg = M // 2
        rows.update(gy0_row=neg - 1, neg_row=neg, above_row=neg + 1, below_row=neg + 2, clamp_col=2)
        gy[neg - 1] = 0.0
        safe = np.where(scale > 0, scale, np.float32(1.0))
        z[neg] = mean - (np.abs(beta) / safe + 1.0 + np.abs(rs.standard_normal(N))).astype(np.float32)
        z[neg + 1] = z[neg]
        z[neg + 2] = z[neg]
        z[neg + 1, 2] = np.float32(2.0 ** -39) / scale[2]
        z[neg + 2, 2] = np.float32(2.0 ** -41) / scale[2]
    if plants and N >= 8 and M >= 69:
        # the order of the fp64 sums, visible in dbeta without flags (ga = gy): B + 1 is a tie that rounds back to B, 1 - B is exact
        B = np.float32(2.0 ** 53)
        gy[:, 3:5] = 0.0
        gy[[0, 1, 2, 3], 3] = (B, 1.0, 1.0, -B)         # one row per wave: ((B + 1) + 1) - B = 0, but (B + 1) + (1 - B) = 1
        gy[[0, 4, 64, 68], 4] = (B, 1.0, 1.0, -B)       # wave 0 of partition 0: 0 in one chain, 1 when row 64 opens a new partition
        rows.update(order_cols=(3, 4))
    return _ro(dict(M=M, N=N, z=z, gy=gy, gamma=gamma, beta=beta, mean=mean, var=var, scale=scale, **rows))


def planted_rows(d):
    return [d[k] for k in ("gy0_row", "neg_row", "above_row", "below_row") if d[k] is not None]


# ---- ps_bn_bwd, exactly ----------------------------------------------------------------------------------------------------------
VARIANTS = ("waves added as (s0 + s1) + (s2 + s3)", "k1 and k2 from the fp64 sums", "xh through scale / gamma",
            "partitions of 64 rows", "gz without the fmaf")


def col_sums(a64, variant=None):
    """fp64 [N]: the column sums of a float64 [M, N] array in bn_partial_kernel's order"""
    M, N = a64.shape
    rows = 64 if variant == VARIANTS[3] else BN_ROWS
    P = _cdiv(M, rows)
    ap = np.zeros((P * rows, N), dtype=np.float64)              # a row past the end adds +0.0: no change (a sum from +0.0 is never -0.0)
    ap[:M] = a64
    ap = ap.reshape(P, rows // 4, 4, N)
    s = np.zeros((P, 4, N), dtype=np.float64)
    for t in range(rows // 4):
        s += ap[:, t]
    if variant == VARIANTS[0]:
        part = (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])
    else:
        part = ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]
    tot = np.zeros(N, dtype=np.float64)
    for p in range(P):
        tot = tot + part[p]
    return tot


def bn_bwd_exact(z, gy, mean, var, scale, beta, eps, relu, l2, vec, variant=None, gamma=None):
    """ps_bn_bwd restated: dict(gz fp32 [M, N], dgamma fp32 [N], dbeta fp32 [N])"""
    z, gy, mean, var, scale, beta = (_f(a) for a in (z, gy, mean, var, scale, beta))
    M = z.shape[0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rstd = (np.float32(1.0) / np.sqrt(var + np.float32(eps))).astype(np.float32)
        if variant == VARIANTS[2]:
            rstd = (scale / _f(gamma)).astype(np.float32)
        d = (z - mean[None, :]).astype(np.float32)
        t = bc.prenorm_exact(z, mean, scale, beta, relu)
        xh = (d * rstd[None, :]).astype(np.float32)
        ga = lb.epilogue_bwd_exact(t, gy, relu, l2, vec) if (relu or l2) else gy
        S1 = col_sums(ga.astype(np.float64), variant)
        S2 = col_sums(ga.astype(np.float64) * xh.astype(np.float64), variant)
        dbeta, dgamma = S1.astype(np.float32), S2.astype(np.float32)
        Mf = np.float32(M)
        k1, k2 = (dbeta / Mf).astype(np.float32), (dgamma / Mf).astype(np.float32)
        if variant == VARIANTS[1]:
            k1, k2 = (S1 / M).astype(np.float32), (S2 / M).astype(np.float32)
        w = (ga - k1[None, :]).astype(np.float32)
        if variant == VARIANTS[4]:
            inner = (w - (xh * k2[None, :]).astype(np.float32)).astype(np.float32)
        else:
            inner = _fma(-xh, k2[None, :], w)
        gz = (scale[None, :] * inner).astype(np.float32)
    return dict(gz=_f(gz), dgamma=_f(dgamma), dbeta=_f(dbeta))


@functools.lru_cache(maxsize=None)
def expected(name, relu, l2, plants=True):
    d = data(name, plants)
    return bn_bwd_exact(d["z"], d["gy"], d["mean"], d["var"], d["scale"], d["beta"], EPS, relu, l2, facts(d["M"], d["N"], case(name)[3])["vec"])


# ---- the closed form and its bound -----------------------------------------------------------------------------------------------
def bn_bwd_64(z, gy, mean, var, scale, beta, eps, relu, l2):
    """dict(gz, dgamma, dbeta, and the intermediates a, t, xh, ga) in float64 (module docstring); eps as the kernel receives it"""
    z, gy, mean, var, scale, beta = (np.asarray(a, dtype=np.float64) for a in (z, gy, mean, var, scale, beta))
    M = z.shape[0]
    d = z - mean
    a = d * scale + beta
    t = np.maximum(a, 0.0) if relu else a
    xh = d / np.sqrt(var + np.float64(np.float32(eps)))
    ga = lb.epilogue_bwd_64(t, gy, relu, l2)
    S1, S2 = ga.sum(axis=0), (ga * xh).sum(axis=0)
    gz = scale * (ga - S1 / M - xh * (S2 / M))
    return dict(gz=gz, dgamma=S2, dbeta=S1, a=a, t=t, xh=xh, ga=ga, d=d)


def bn_bwd_bound(z, gy, mean, var, scale, beta, eps, relu, l2, vec):
    """dict(gz, dgamma, dbeta): fp64 bounds on |bn_bwd_exact - bn_bwd_64| (module docstring), and et (the bound on the
    pre-activation, for the mask condition)"""
    r = bn_bwd_64(z, gy, mean, var, scale, beta, eps, relu, l2)
    sc = np.abs(np.asarray(scale, dtype=np.float64))
    g = np.abs(np.asarray(gy, dtype=np.float64))
    M = g.shape[0]
    a, t, xh, ga = np.abs(r["a"]), r["t"], np.abs(r["xh"]), np.abs(r["ga"])
    et = 1.01 * U32 * (np.abs(r["d"]) * sc + a)
    live = (t > 0) if relu else np.ones(t.shape, dtype=bool)
    Eg = lb.epilogue_bound(t, gy, relu, l2, vec)
    if l2:
        c = np.maximum(np.sqrt((t * t).sum(axis=1)), 1e-12)
        etl = np.where(live, et, 0.0)
        move = 1.01 * 3.0 * np.sqrt((g * g).sum(axis=1)) * np.sqrt((etl * etl).sum(axis=1)) / (c * c)
        Eg = Eg + np.where(live, move[:, None], 0.0)
    Ex = 1.01 * 5.0 * U32 * xh
    S1, S2 = np.abs(r["dbeta"]), np.abs(r["dgamma"])
    Edb = 1.01 * (Eg.sum(axis=0) + U32 * S1) + M * 2.0 ** -52 * ga.sum(axis=0)
    Edg = 1.01 * ((Eg * xh + ga * Ex).sum(axis=0) + U32 * S2) + M * 2.0 ** -52 * (ga * xh).sum(axis=0)
    k1, k2 = S1 / M, S2 / M
    Ek1, Ek2 = Edb / M + 2.0 * U32 * k1, Edg / M + 2.0 * U32 * k2
    Egz = 1.01 * sc * (Eg + Ek1 + Ex * k2 + xh * Ek2 + 3.0 * U32 * (ga + k1 + xh * k2))
    return dict(gz=Egz, dgamma=Edg, dbeta=Edb, et=et)


def autograd_64(z, gy, gamma, beta, eps, relu, l2):
    """torch CPU float64 autograd of F.normalize(F.relu(F.batch_norm(z, training=True))): dict(gz, dgamma, dbeta)"""
    import torch
    import torch.nn.functional as F
    zt, gt, bt = (torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True) for a in (z, gamma, beta))
    y = F.batch_norm(zt, None, None, gt, bt, training=True, eps=float(np.float32(eps)))
    if relu:
        y = F.relu(y)
    if l2:
        y = F.normalize(y, p=2, dim=1)
    y.backward(torch.tensor(np.asarray(gy, dtype=np.float64)))
    return dict(gz=zt.grad.numpy(), dgamma=gt.grad.numpy(), dbeta=bt.grad.numpy())


def exact_stats_64(z, gamma, eps):
    z64 = np.asarray(z, dtype=np.float64)
    mean, var = z64.mean(axis=0), z64.var(axis=0)
    return mean, var, np.asarray(gamma, dtype=np.float64) / np.sqrt(var + np.float64(np.float32(eps)))


mismatches = lb.mismatches
outside = lb.outside
