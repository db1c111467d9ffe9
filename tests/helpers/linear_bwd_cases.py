"""An exact numpy restatement of ps_linear_wgrad and ps_linear_epilogue_bwd (csrc/linear_bwd.hip, as include/pinsage_hip.h states
them), their float64 closed forms with derived bounds, and the case table both test files share: tests/test_linear_bwd_cases.py
(CPU: the restatements against the closed forms and against torch float64 autograd) and tests/test_hip_linear_bwd.py (GPU: the
kernels against the restatements, bit for bit).

Every fp32 product-and-add is spmm_cases._fma (one rounding); the row norm and the lane layout of the epilogue are bn_cases'
sum_squares_exact / wave_sum.  The partition size P is an argument of the restatements: the GPU tests read it from the library
(partition()), partition_rule() restates the header's rule.

Bounds (u = 2^-24, gamma_n = n u / (1 - n u)):
  wgrad     s_p is a chain of at most r = min(P, M) fused multiply-adds from +0.0, the p = ceil(M / P) partials are added one after
            the other: every product passes through at most r + p - 1 roundings, so
            |dW - sum_m g x| <= gamma_{r+p-1} sum_m |g x|            (wgrad_bound; db: the same with x = 1).
  epilogue  (epilogue_bound) with L = sweeps * vec the length of a lane's chain and six levels of the wave sum:
            the sum of squares has relative error gamma_{L+6}, its root half of that and one rounding more, so c carries at most
            ec = gamma_{L+8} (generous); y = t / c carries ey = ec + u; s = sum g y is off by at most ds = (gamma_{L+6} + ey) sum |g y|;
            the numerator fmaf(-y, s, g) is off by |y| ds + ey |y s| + u (|g| + |y s|), and the quotient by c adds (ec + u) of
            (|g| + |y s|) / c.  Second-order terms are covered by a factor 1.01.  Below the clamp gt = g / c: one rounding.
            Without the norm the epilogue is a copy or a mask: exact.
  layer     (layer_grad_bounds) against float64 autograd of the whole layer the saved activation itself differs: the fp32
            pre-activation is a chain of K + K2 fmafs and the bias addition, |dt| <= gamma_{K+K2+1} (sum |x W| + |b|) =: et.
            With y = t / c, gz = (G - y (y . G)) / c (masked by the ReLU) has d gz / d t of norm at most 3 |G| / c^2 (two terms
            from dy = (I - y y^T) dt / c, one from d(1 / c) = -(y . dt) / c^2), so every element of a row's gz moves by at most
            3 |G|_2 |et|_2 / c^2 (first order; the factor 1.01 again); without the norm gz does not depend on t (the data keeps
            every pre-activation 1e-4 away from zero, far beyond et, so the mask is the same).  That and epilogue_bound give
            E = |gz - gz64|; then |dW - dW64| <= sum_m E |x| + wgrad_bound(|gz|, x), |dx - dx64| <= sum_n E |W| + gamma_N sum_n |gz W|."""
import functools

import numpy as np

from helpers import bn_cases as bc
from helpers.spmm_cases import _fma, gamma

U32 = 2.0 ** -24
CLAMP = np.float32(1e-12)
PART, MAX_PARTS = 512, 256                  # csrc/linear_bwd.hip: WG_PART, WG_MAX_PARTS
PLANT = (np.float32(2.0 ** 24 + 2.0 ** 22), np.float32(1.0), np.float32(-3.0 * 2.0 ** 22))


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _cdiv(a, b):
    return -(-a // b)


def partition_rule(M):
    """ps_linear_wgrad_partition restated: 512 rows, doubled while there would be more than 256 partitions"""
    P = PART
    while _cdiv(M, P) > MAX_PARTS:
        P *= 2
    return P


def partition(M):
    """P = ps_linear_wgrad_partition(M), asked of the library (no GPU needed)"""
    from pinsage_hip import native
    return int(native.lib().ps_linear_wgrad_partition(int(M)))


# ---- ps_linear_wgrad, exactly ---------------------------------------------------------------------------------------------------
def _partials(g, x, P):
    """fp32 [parts, N, K]: s_p = the chain acc = fmaf(g[m, n], x[m, k], acc) over the rows of partition p ascending from +0.0.
    All partitions advance together, one row each per step; the last one stops where the rows end."""
    g, x = _f(g), _f(x)
    M, N = g.shape
    K = x.shape[1]
    parts = _cdiv(M, P)
    acc = np.zeros((parts, N, K), dtype=np.float32)
    last = M - (parts - 1) * P
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(min(P, M)):
            live = parts if r < last else parts - 1
            rows = np.arange(live) * P + r
            acc[:live] = _fma(g[rows][:, :, None], x[rows][:, None, :], acc[:live])
    return acc


def _add_partials(acc):
    out = acc[0].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(1, acc.shape[0]):
            out = out + acc[p]
    return out


def wgrad_exact(g, x, P):
    """dW fp32 [N, K] of ps_linear_wgrad: ((s_0 + s_1) + s_2) + ... in partition order; zeros for M == 0"""
    g, x = _f(g), _f(x)
    if g.shape[0] == 0:
        return np.zeros((g.shape[1], x.shape[1]), dtype=np.float32)
    return _add_partials(_partials(g, x, P))


def bias_grad_exact(g, P):
    """db fp32 [N]: the same form with x = 1, the chain acc = acc + g[m, n]"""
    g = _f(g)
    M, N = g.shape
    if M == 0:
        return np.zeros(N, dtype=np.float32)
    parts = _cdiv(M, P)
    acc = np.zeros((parts, N), dtype=np.float32)
    last = M - (parts - 1) * P
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(min(P, M)):
            live = parts if r < last else parts - 1
            acc[:live] = acc[:live] + g[np.arange(live) * P + r]
    return _add_partials(acc)


def wgrad_64(g, x):
    g64, x64 = np.asarray(g, dtype=np.float64), np.asarray(x, dtype=np.float64)
    return g64.T @ x64, np.abs(g64).T @ np.abs(x64)


def wgrad_bound(g, x, P):
    """fp64 [N, K]: gamma_{r+p-1} sum_m |g x| (module docstring)"""
    M = np.shape(g)[0]
    if M == 0:
        return np.zeros((np.shape(g)[1], np.shape(x)[1]))
    return gamma(min(P, M) + _cdiv(M, P) - 1) * wgrad_64(g, x)[1]


# ---- ps_linear_epilogue_bwd, exactly --------------------------------------------------------------------------------------------
def vec_of(N, offset=0):
    """VEC of the epilogue kernel: 4 when N % 4 == 0 and t, g, gz start on 16-byte boundaries (offset: floats past one)"""
    return 4 if N % 4 == 0 and offset % 4 == 0 else 1


def _lanes(a, vec):
    """[M, N] -> [M, sweeps, 64, vec]: column 64 vec k + vec l + e at [k, l, e], zeros past N"""
    M, N = a.shape
    chunk = 64 * vec
    sweeps = _cdiv(N, chunk)
    p = np.zeros((M, sweeps * chunk), dtype=np.float32)
    p[:, :N] = a
    return p.reshape(M, sweeps, 64, vec)


def epilogue_bwd_exact(t, g, relu, l2, vec):
    """gz fp32 [M, N] of ps_linear_epilogue_bwd"""
    t, g = _f(t), _f(g)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        gt = g
        if l2:
            nrm = np.sqrt(bc.sum_squares_exact(t, vec))
            c = np.maximum(nrm, CLAMP)                                  # np.maximum keeps a NaN
            below = nrm < CLAMP
            y = (t / c[:, None]).astype(np.float32)
            gp, yp = _lanes(g, vec), (_lanes(t, vec) / c[:, None, None, None]).astype(np.float32)
            acc = np.zeros((t.shape[0], 64), dtype=np.float32)
            for k in range(gp.shape[1]):
                for e in range(vec):
                    acc = _fma(gp[:, k, :, e], yp[:, k, :, e], acc)
            s = bc.wave_sum(acc)
            full = (_fma(-y, s[:, None], g) / c[:, None]).astype(np.float32)
            gt = np.where(below[:, None], (g / c[:, None]).astype(np.float32), full)
        if relu:
            gt = np.where(t > 0, gt, np.float32(0.0))
    return _f(gt)


def epilogue_bwd_64(t, g, relu, l2):
    """the same in float64 from the same fp32 operands"""
    t64, g64 = np.asarray(t, dtype=np.float64), np.asarray(g, dtype=np.float64)
    gt = g64
    if l2:
        nrm = np.sqrt((t64 * t64).sum(axis=1))
        c = np.maximum(nrm, 1e-12)[:, None]
        y = t64 / c
        gt = np.where((nrm < 1e-12)[:, None], g64 / c, (g64 - y * (y * g64).sum(axis=1)[:, None]) / c)
    if relu:
        gt = np.where(t64 > 0, gt, 0.0)
    return gt


def epilogue_bound(t, g, relu, l2, vec):
    """fp64 [M, N] (module docstring); rows above the clamp"""
    t64, g64 = np.abs(np.asarray(t, dtype=np.float64)), np.abs(np.asarray(g, dtype=np.float64))
    if not l2:
        return np.zeros_like(t64)
    L = _cdiv(t64.shape[1], 64 * vec) * vec
    c = np.maximum(np.sqrt((t64 * t64).sum(axis=1)), 1e-12)[:, None]
    y = t64 / c
    sabs = (g64 * y).sum(axis=1)[:, None]                               # sum |g y| >= |s|
    ec = gamma(L + 8)
    ey = ec + U32
    ds = (gamma(L + 6) + ey) * sabs
    b = 1.01 * ((y * ds + ey * y * sabs + U32 * (g64 + y * sabs)) / c + (ec + U32) * (g64 + y * sabs) / c)
    return np.where(t64 > 0, b, 0.0) if relu else b


# ---- a whole layer: y = normalize(relu(x W^T + x2 W2^T + b)) and its gradients ------------------------------------------------------
def layer_exact(x, W, b, x2, W2, G, relu, l2, P, vec=None, need=("x", "W", "b", "x2", "W2")):
    """The fp32 values LinearFn computes: t (the C oracle's ps_linear chain), gz, and the gradients named in `need`."""
    from oracle import c_oracle as co
    x, W, G = _f(x), _f(W), _f(G)
    t = co.linear(x, W, None if b is None else _f(b), x2=None if x2 is None else _f(x2), W2=None if W2 is None else _f(W2), relu=relu)
    N = W.shape[0]
    gz = epilogue_bwd_exact(t, G, relu, l2, vec_of(N) if vec is None else vec) if (relu or l2) else G
    out = {"t": t, "gz": gz}
    if "W" in need:
        out["W"] = wgrad_exact(gz, x, P)
    if "b" in need and b is not None:
        out["b"] = bias_grad_exact(gz, P)
    if "x" in need:
        out["x"] = co.linear(gz, _f(W.T))
    if x2 is not None:
        if "W2" in need:
            out["W2"] = wgrad_exact(gz, _f(x2), P)
        if "x2" in need:
            out["x2"] = co.linear(gz, _f(np.asarray(W2).T))
    return out


def layer_autograd_64(x, W, b, x2, W2, G, relu, l2):
    """torch CPU float64 autograd of F.normalize(F.relu(F.linear(x, W, b) + F.linear(x2, W2))) on the same leaves: the
    gradients by name, and the float64 pre-norm activation"""
    import torch
    import torch.nn.functional as F
    leaves = {k: torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True)
              for k, v in (("x", x), ("W", W), ("b", b), ("x2", x2), ("W2", W2)) if v is not None}
    t = F.linear(leaves["x"], leaves["W"], leaves.get("b"))
    if x2 is not None:
        t = t + F.linear(leaves["x2"], leaves["W2"])
    if relu:
        t = F.relu(t)
    y = F.normalize(t, p=2, dim=1) if l2 else t
    y.backward(torch.tensor(np.asarray(G, dtype=np.float64)))
    out = {k: v.grad.numpy() for k, v in leaves.items()}
    out["t"] = t.detach().numpy()
    return out


def layer_grad_bounds(x, W, b, x2, W2, G, relu, l2, P, vec=None):
    """{leaf: fp64 bound on |fp32 gradient - float64 autograd|} (module docstring: layer)"""
    a = {k: (None if v is None else np.abs(np.asarray(v, dtype=np.float64))) for k, v in
         (("x", x), ("W", W), ("b", b), ("x2", x2), ("W2", W2), ("G", G))}
    N, K = a["W"].shape
    K2 = 0 if x2 is None else a["W2"].shape[1]
    pre = a["x"] @ a["W"].T + (0.0 if b is None else a["b"][None, :]) + (0.0 if x2 is None else a["x2"] @ a["W2"].T)
    et = gamma(K + K2 + 1) * pre
    ref = layer_autograd_64(x, W, b, x2, W2, G, relu, l2)
    t64 = ref["t"]
    E = epilogue_bound(t64, G, relu, l2, vec_of(N) if vec is None else vec)
    gz = np.abs(epilogue_bwd_64(t64, G, relu, l2))
    if l2:
        c = np.maximum(np.sqrt((t64 * t64).sum(axis=1)), 1e-12)
        move = 1.01 * 3.0 * np.sqrt((a["G"] ** 2).sum(axis=1)) * np.sqrt((et ** 2).sum(axis=1)) / (c * c)
        E = E + move[:, None]
    gz = gz + E
    M = gz.shape[0]
    gw = gamma(min(P, max(M, 1)) + _cdiv(max(M, 1), P) - 1)
    out = {"x": E @ a["W"] + gamma(N) * (gz @ a["W"]), "W": E.T @ a["x"] + gw * (gz.T @ a["x"])}
    if b is not None:
        out["b"] = E.sum(axis=0) + gw * gz.sum(axis=0)
    if x2 is not None:
        out["x2"] = E @ a["W2"] + gamma(N) * (gz @ a["W2"])
        out["W2"] = E.T @ a["x2"] + gw * (gz.T @ a["x2"])
    return out, ref


# ---- case tables and data ---------------------------------------------------------------------------------------------------------
WGRAD_SHAPES = ((1, 1), (33, 31), (64, 64), (130, 36), (257, 300))           # (N, K)
EPILOGUE_N = (1, 4, 63, 64, 65, 256, 300)
FLAGSETS = ((False, False), (True, False), (False, True), (True, True))     # (relu, l2norm)


def wgrad_rows(P):
    """the row counts of the wgrad cases for a partition size P"""
    return (1, 2, 3, P - 1, P, P + 1, 2 * P + 3)


def doubling_rows():
    """the first M whose partition is 2 * PART: one row more than MAX_PARTS partitions of PART rows"""
    return PART * MAX_PARTS + 1


def wrong_partitions(M, P):
    """the partition sizes the plant has to tell from P: one row less, one more, twice as many, one single chain.  (Half as many
    it cannot: that cuts at every boundary of P as well, and the cuts it adds fall among small integers, whose sums are exact.)"""
    return tuple(q for q in (P - 1, P + 1, 2 * P, M) if q >= 1 and q != P)


def plant_value(col, P):
    """the planted element of dW (= of db): the column of g against the column of ones, fmaf(g, 1, acc) = acc + g"""
    return bias_grad_exact(np.asarray(col, dtype=np.float32)[:, None], P)[0]


def plant_works(col, P):
    want = plant_value(col, P)
    return all(plant_value(col, q) != want for q in wrong_partitions(len(col), P))


@functools.lru_cache(maxsize=8)
def wgrad_data(M, N, K, P, seed=0):
    """g [M, N], x [M, K]: N(0, 1) floats, with the plant (M >= P + 2: with a single row behind the boundary, adding that partial
    IS the next step of the single chain): column N // 2 of g holds small even integers and column K // 2 of x ones, and at
    every partition boundary b = j P (0 < b < M) the rows b - 1, b, b + 1 of that column of g hold 2^24 + 2^22, 1, -3 * 2^22.
    Cut at b, the 1 opens a chain and 1 - 3 * 2^22 is exact; in a chain that runs through b it meets 2^24 + 2^22 + (an even
    integer) and is rounded away.  Further roundings follow where the column's total passes 2^24, so the small integers are
    drawn until the element does differ for every partitioning of wrong_partitions() (the restatement alone decides that)."""
    rs = np.random.RandomState(4000 + 7 * N + 13 * K + M % 1009 + seed)
    g = rs.standard_normal((M, N)).astype(np.float32)
    x = rs.standard_normal((M, K)).astype(np.float32)
    x[:, K // 2] = 1.0
    for _ in range(64):
        g[:, N // 2] = 2.0 * rs.randint(-4, 5, M)
        for b in range(P, M, P):
            for d, v in zip((-1, 0, 1), PLANT):
                if 0 <= b + d < M:
                    g[b + d, N // 2] = v
        if M < P + 2 or plant_works(g[:, N // 2], P):
            break
    else:
        raise AssertionError("no plant that tells the partitionings apart")
    g.setflags(write=False)
    x.setflags(write=False)
    return g, x


@functools.lru_cache(maxsize=None)
def epilogue_data(N, M=9, seed=0):
    """t (after a ReLU: a third of the entries +0.0, the rest at least 1e-4), g, and the planted rows
      zero_row    t all +0.0: below the clamp, gz = g / 1e-12 and all +0 under the ReLU
      above_row   one entry 2^-39 (nrm = 1.8e-12, just above the clamp)
      below_row   one entry 2^-41 (nrm = 4.5e-13, just below)
      nan_row     a NaN in the last column"""
    rs = np.random.RandomState(5000 + N + seed)
    t = np.abs(rs.standard_normal((M, N))).astype(np.float32) + np.float32(1e-4)
    t[rs.random_sample((M, N)) < 1.0 / 3.0] = 0.0
    g = rs.standard_normal((M, N)).astype(np.float32)
    rows = dict(zero_row=2, above_row=3, below_row=4, nan_row=6)
    t[rows["zero_row"]] = 0.0
    t[rows["above_row"]] = 0.0
    t[rows["above_row"], N - 1] = 2.0 ** -39
    t[rows["below_row"]] = 0.0
    t[rows["below_row"], 0] = 2.0 ** -41
    t[rows["nan_row"], N - 1] = np.nan
    t.setflags(write=False)
    g.setflags(write=False)
    return t, g, rows


def plain_rows(rows, M):
    """the rows of epilogue_data that carry no plant"""
    return np.array([r for r in range(M) if r not in rows.values()])


@functools.lru_cache(maxsize=None)
def layer_data(M, K, N, K2, bias=True, seed=0):
    """x, W, b, x2, W2, G of one layer; drawn again until no pre-activation lies within 1e-4 of zero and no row's
    activation is near the clamp"""
    rs = np.random.RandomState(6000 + M + 3 * K + 5 * N + 7 * K2 + seed)
    for _ in range(64):
        x = rs.standard_normal((M, K)).astype(np.float32)
        W = (rs.standard_normal((N, K)) / np.sqrt(K + K2)).astype(np.float32)
        b = rs.standard_normal(N).astype(np.float32) if bias else None
        x2 = rs.standard_normal((M, K2)).astype(np.float32) if K2 else None
        W2 = (rs.standard_normal((N, K2)) / np.sqrt(K + K2)).astype(np.float32) if K2 else None
        pre = x.astype(np.float64) @ W.astype(np.float64).T + (0.0 if b is None else b.astype(np.float64))
        if K2:
            pre = pre + x2.astype(np.float64) @ W2.astype(np.float64).T
        if np.abs(pre).min() > 1e-4 and (np.maximum(pre, 0.0) ** 2).sum(axis=1).min() > 1e-6:
            break
    else:
        raise AssertionError("no data without a pre-activation near zero")
    G = rs.standard_normal((M, N)).astype(np.float32)
    out = dict(x=x, W=W, b=b, x2=x2, W2=W2, G=G)
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


def mismatches(got, want, limit=8):
    """first `limit` (row, col, got, want) where two fp32 arrays differ in their bits (-0 is not +0); a NaN equals any NaN"""
    return bc.mismatches(np.atleast_2d(got), np.atleast_2d(want), limit)


def outside(got, ref64, bound, limit=8):
    """first `limit` (index, got, want, bound) where |got - ref64| > bound"""
    got, ref64, bound = np.atleast_2d(got).astype(np.float64), np.atleast_2d(ref64), np.atleast_2d(bound)
    bad = ~(np.abs(got - ref64) <= bound)
    return [(tuple(int(i) for i in ix), float(got[tuple(ix)]), float(ref64[tuple(ix)]), float(bound[tuple(ix)])) for ix in np.argwhere(bad)[:limit]]
