"""Special values through the dense layers (csrc/dense_mfma.hip: ps_linear), numpy only: NaN, infinities, overflow and signed
zeros planted into the operands of helpers/gemm_cases.py, the oracle's answer to them, and the comparison that holds a kernel to
it -- every output as a uint32 word, a NaN of any payload and sign where the oracle holds a NaN.

Which cases.  For every instantiation of gemm_cases.INSTANTIATIONS the smallest case of the table (by M N (K + K2)) that reaches
it -- by the launcher's own choice or, failing that, under one of gemm_cases.switch_runs -- and has room for the plantings: M >=
MIN_M rows and N >= MIN_N columns (the table's M = 1 and N = 1 cases have no second row or column to keep ordinary).

What is planted (`data`), in rows and columns the table leaves ordinary (it uses rows 0, 1 and the last, k = 0, the last column).
Every planted row lies in rows 0 .. 15, the first 32-row MFMA block, between ordinary rows.  Each is order-free: at most one
non-finite or overflowing term per output, so the summation order -- held by the ordinary cases -- decides no class here.
  variant "rows" (and "rows_nobias": the same with b = NULL), every flag set of the case:
    R_NAN      x[R_NAN, K - 1] = NaN (inside the last, ragged K step): the whole output row is NaN.  M >= 64: a second such row,
               M - 2, the last row but one, in another row tile.
    R_NAN2     K2 > 0: x2[R_NAN2, K2 - 1] = NaN, x ordinary: the same.
    R_INF      x[R_INF, K_INF] = +Inf against W[:, K_INF] of both signs: +Inf / -Inf, with ReLU +Inf / +0; the norm is Inf:
               Inf / Inf = NaN, 0 / Inf = +0.
    R_INFINF   x[R_INFINF, K_INF] = +Inf and -Inf in x2[R_INFINF, K_INF] (K2 > 0) or x[R_INFINF, K_INF2] (K2 = 0): Inf - Inf = NaN
               in any order where the two weights have one sign, +-Inf elsewhere.  The only rows with NaN and non-NaN columns
               side by side: the norm is NaN, and the clamp must leave it.
    R_OVF      zero but x[R_OVF, K_OVF] = 3e38, W[C_OVP, K_OVF] = 1.5, W[C_OVN, K_OVF] = -1.5: +Inf and -Inf from finite
               operands; every other |w| < 1.13 stays finite.
    R_NEG0     zero but -1e-30 at the last k of the chain (of x2 where K2 > 0), the weight of column C_NEG0 there 1e-30 and
               b[C_NEG0] = -0.0: fmaf(-1e-30, 1e-30, +0.0) = -0.0, + -0.0 = -0.0.  Without ReLU -0.0 is stored, with it +0.0;
               the norm divides it and keeps the sign.  rows_nobias: + 0.0f gives +0.0.  Where the last chain's length is no
               multiple of 32 (`neg0_survives` is false) the header lets terms +0.0 * +0.0 follow it -- the kernel's K step is
               padded with zeros -- and the chain ends in +0.0; the oracle restates that, and the planting then pins +0.0.
  variant "w_nan": W[C_WNAN, K - 1] = NaN; variant "b_nan": b[C_BNAN] = NaN; nothing else planted.  Column n is NaN in every row,
    the all-zero row included.  Flag sets without the norm only (NO_NORM): with it every row is poisoned and shows nothing more.

References.  `expected` is oracle/c_oracle.linear (orc_linear: the definitions of include/pinsage_hip.h).  `torch_classes` is
F.normalize(F.relu(x @ W.T + x2 @ W2.T + b)) on the CPU in fp64; it must agree with the oracle on every output's class (`classes`)
up to two deviations: NEG0 -- ps_linear's definition turns -0.0 into +0.0 where torch keeps it (relu(-0.0), + 0.0f) -- and OVERFLOW
-- fp64 does not overflow where fp32 does, so with the norm row R_OVF is held to the same expression in fp32."""
import functools

import numpy as np

import gemm_cases as gc

MIN_M, MIN_N = 16, 8
R_NAN, R_NAN2, R_INF, R_INFINF, R_OVF, R_NEG0 = 3, 5, 6, 9, 10, 12
C_OVP, C_NEG0, C_WNAN, C_OVN, C_BNAN = 2, 3, 4, 5, 6
K_INF, K_OVF, K_INF2 = 1, 2, 3
BIG, TINY = np.float32(3e38), np.float32(1e-30)
NO_NORM = (gc.NONE, gc.RELU)
VARIANTS = ("rows", "rows_nobias", "w_nan", "b_nan")

NAN, PINF, NINF, FINITE, PZERO, NZERO = range(6)
CLASS_NAMES = ("NaN", "+Inf", "-Inf", "finite", "+0", "-0")


def classes(a):
    """int8 array: NAN, PINF, NINF, FINITE (nonzero), PZERO or NZERO per element"""
    a = np.asarray(a)
    out = np.full(a.shape, FINITE, dtype=np.int8)
    out[np.isnan(a)] = NAN
    out[a == np.inf] = PINF
    out[a == -np.inf] = NINF
    zero = a == 0
    out[zero & ~np.signbit(a)] = PZERO
    out[zero & np.signbit(a)] = NZERO
    return out


# ------------------------------------------------------------------------------------------------------------------ the cases

def _runs(c):
    """(env, staged) of every run the GPU test makes of base case c: the launcher's default, then the switches for FAST cases"""
    return [((), False)] + (gc.switch_runs(c) if c in gc.FAST_CASES else [])


@functools.lru_cache(maxsize=None)
def reached_by(c):
    """{instantiation: (env, staged, l2) of the first run of c that reaches it}"""
    out = {}
    for env, staged in _runs(c):
        for (_, l2) in c.flagsets:
            for k in gc.kernels_of(gc.launcher_choice(c.M, c.K, c.N, c.K2, c.layout, l2, env=env, staged=staged)):
                out.setdefault(k, (env, staged, l2))
    return out


def eligible(c):
    return c.M >= MIN_M and c.N >= MIN_N


def _size(c):
    return c.M * c.N * (c.K + c.K2)


def _choose():
    chosen = {}
    for inst in sorted(gc.INSTANTIATIONS):
        default = [c for c in gc.CASES if eligible(c) and inst in reached_by(c) and reached_by(c)[inst][0] == () and
                   not reached_by(c)[inst][1]]
        pool = default or [c for c in gc.CASES if eligible(c) and inst in reached_by(c)]
        chosen[inst] = min(pool, key=lambda c: (_size(c), c.name))
    return chosen


CHOSEN = _choose()                                         # instantiation -> base case
BASES = tuple(c for c in gc.CASES if c in set(CHOSEN.values()))
FAST_BASES = tuple(c for c in BASES if c in gc.FAST_CASES)
NORM_ROWS_BASE = CHOSEN["l2norm_rows_kernel"]              # N > 256: the GEMM without the norm, then l2norm_rows_kernel


def neg0_survives(c):
    """does the chain that ends in -0.0 end the K loop (no padding term +0.0 * +0.0 behind it)?"""
    return (c.K2 or c.K) % 32 == 0


def flagsets_of(c, variant):
    return c.flagsets if variant.startswith("rows") else NO_NORM


# ------------------------------------------------------------------------------------------------------------------- operands

def planted_rows(c):
    """{name: row} of variant "rows" in case c"""
    rows = dict(nan=R_NAN, inf=R_INF, infinf=R_INFINF, ovf=R_OVF, neg0=R_NEG0)
    if c.K2:
        rows["nan2"] = R_NAN2
    if c.M >= 64:
        rows["nan_tail"] = c.M - 2
    return rows


@functools.lru_cache(maxsize=None)
def data(c, variant):
    """gemm_cases.Data of base case c with the variant's plantings (b is None for rows_nobias)"""
    assert eligible(c) and variant in VARIANTS and c.K > K_INF2
    d = gc.case_data(c)
    x, b, Wbig = d.x.copy(), d.b.copy(), d.Wbig.copy()
    x2 = None if d.x2 is None else d.x2.copy()
    W2big = None if d.W2big is None else d.W2big.copy()
    W = gc.view_of(Wbig, c.K, c.layout)                    # writes go through to the matrix the kernel is given
    W2 = None if W2big is None else gc.view_of(W2big, c.K2, c.layout)
    if variant == "w_nan":
        W[C_WNAN, c.K - 1] = np.nan
    elif variant == "b_nan":
        b[C_BNAN] = np.nan
    else:
        rows = planted_rows(c)
        for r in (rows["nan"], rows.get("nan_tail")):
            if r is not None:
                x[r, c.K - 1] = np.nan
        x[R_INF, K_INF] = np.inf
        x[R_INFINF, K_INF] = np.inf
        if c.K2:
            x2[R_NAN2, c.K2 - 1] = np.nan
            x2[R_INFINF, K_INF] = -np.inf
        else:
            x[R_INFINF, K_INF2] = -np.inf
        x[R_OVF] = 0.0
        x[R_OVF, K_OVF] = BIG
        W[C_OVP, K_OVF], W[C_OVN, K_OVF] = 1.5, -1.5
        x[R_NEG0] = 0.0
        if c.K2:
            x2[R_OVF] = 0.0
            x2[R_NEG0] = 0.0
            x2[R_NEG0, c.K2 - 1] = -TINY
            W2[C_NEG0, c.K2 - 1] = TINY
        else:
            x[R_NEG0, c.K - 1] = -TINY
            W[C_NEG0, c.K - 1] = TINY
        b[C_NEG0] = -0.0
        if variant == "rows_nobias":
            b = None
    Wc = np.ascontiguousarray(W)
    W2c = None if W2 is None else np.ascontiguousarray(W2)
    for a in (x, Wc, b, x2, W2c, Wbig, W2big):
        if a is not None:
            a.setflags(write=False)
    return gc.Data(x, Wc, b, x2, W2c, Wbig, W2big)


# ----------------------------------------------------------------------------------------------------------------- references

@functools.lru_cache(maxsize=None)
def expected(c, variant, relu, l2):
    """fp32 [M, N]: the oracle's output"""
    from oracle import c_oracle as co
    d = data(c, variant)
    y = co.linear(d.x, d.W, d.b, x2=d.x2, W2=d.W2, relu=relu, l2norm=l2, threads=8)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def expected_ref64(c, variant, relu):
    """fp64 [M, N]: the rows of the oracle's fp32 pre-norm output over their norm in fp64 (gemm_cases.ref_normed); what a
    normalised finite output is held to, within gemm_cases.norm_bound(N)"""
    with np.errstate(invalid="ignore", over="ignore"):
        r = gc.ref_normed(expected(c, variant, relu, False))
    r.setflags(write=False)
    return r


def mismatches(got, want, ref64=None, limit=8):
    """first `limit` (row, col, got, want) where fp32 `got` is not the oracle's `want`: a NaN where want is NaN, else the same
    uint32 word.  With ref64 (a normalised output): where want is finite and not zero, got within norm_bound(N) of ref64 instead
    -- the bound gemm_cases derives; nothing else has a tolerance."""
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    ok = got.view(np.uint32) == want.view(np.uint32)
    wnan = np.isnan(want)
    ok[wnan] = np.isnan(got[wnan])
    if ref64 is not None:
        fin = np.isfinite(want) & (want != 0)
        with np.errstate(invalid="ignore"):
            within = np.abs(got.astype(np.float64) - ref64) <= gc.norm_bound(got.shape[1]) * np.abs(ref64) + 2.0 ** -149
        ok[fin] = within[fin]
    bad = np.argwhere(~ok)
    return [(int(r), int(c), float(got[r, c]), float(want[r, c])) for r, c in bad[:limit]]


def torch_classes(c, variant, relu, l2, dtype="float64"):
    """classes of F.normalize(F.relu(x @ W.T + x2 @ W2.T + b)) on the CPU in `dtype`, the result rounded to fp32 (what the fp32 chain
    rounds to +-Inf or +-0.0 in its one special term, fp64 carries on as 4.5e38 or -1e-60)"""
    import torch
    import torch.nn.functional as F
    d = data(c, variant)
    dt = getattr(torch, dtype)
    t = lambda a: torch.tensor(a, dtype=dt)                # noqa: E731
    v = t(d.x) @ t(d.W).T
    if d.x2 is not None:
        v = v + t(d.x2) @ t(d.W2).T
    if d.b is not None:
        v = v + t(d.b)
    if relu:
        v = F.relu(v)
    if l2:
        v = F.normalize(v, p=2.0, dim=1, eps=1e-12)
    with np.errstate(over="ignore"):
        return classes(v.numpy().astype(np.float32))


# ------------------------------------------------------------------------------------------- the slip: the kernel before the fix

def slipped(c, variant, relu, l2):
    """orc_linear with the two selects the GEMM's epilogue had: v > 0 ? v : 0 and nrm > 1e-12f ? nrm : 1e-12f -- both drop a NaN"""
    from oracle import c_oracle as co
    d = data(c, variant)
    v = co.linear(d.x, d.W, d.b, x2=d.x2, W2=d.W2, relu=False, l2norm=False, threads=8)
    with np.errstate(invalid="ignore", over="ignore"):
        if d.b is None:
            v = v + np.float32(0.0)
        if relu:
            v = np.where(v > 0, v, np.float32(0.0))
        if l2:
            ss = np.zeros(v.shape[0], dtype=np.float32)
            for n in range(v.shape[1]):
                ss = ss + v[:, n] * v[:, n]
            nrm = np.sqrt(ss)
            nrm = np.where(nrm > np.float32(1e-12), nrm, np.float32(1e-12))
            v = v / nrm[:, None]
    return v.astype(np.float32)


# ------------------------------------------------------------------------------------ the backward of the epilogue (csrc/linear_bwd.hip)

EPI_N = (4, 65, 300)                                       # the set of test_epilogue_bwd_planted_rows
EPI_ROWS = dict(inf_row=5, neg0_row=7, gnan_row=8)         # beside linear_bwd_cases.epilogue_data's zero / above / below / nan rows


@functools.lru_cache(maxsize=None)
def epilogue_special(N):
    """t, g, rows: linear_bwd_cases.epilogue_data(N) -- activations after a ReLU with an all-zero row, rows just above and below
    the 1e-12 clamp and a row with a NaN -- and three more plants in rows that were plain: inf_row (t = +Inf in column 0),
    neg0_row (t = -0.0 in column 1 where N > 1) and gnan_row (an ordinary t, positive in the last column, under a NaN of g)"""
    from helpers import linear_bwd_cases as lb
    t, g, rows = lb.epilogue_data(N)
    t, g, rows = t.copy(), g.copy(), dict(rows, **EPI_ROWS)
    assert len(set(rows.values())) == len(rows) and max(rows.values()) < t.shape[0]
    t[rows["inf_row"], 0] = np.inf
    t[rows["neg0_row"], min(1, N - 1)] = -0.0
    t[rows["gnan_row"], N - 1] = 1.0
    g[rows["gnan_row"], N - 1] = np.nan
    t.setflags(write=False)
    g.setflags(write=False)
    return t, g, rows


def epilogue_torch_classes(t, g, relu, l2):
    """classes of torch autograd's gradient of F.normalize(F.relu(z)) at z = t under g, fp64 on the CPU, rounded to fp32"""
    import torch
    import torch.nn.functional as F
    z = torch.tensor(t, dtype=torch.float64, requires_grad=True)
    y = F.relu(z) if relu else z
    if l2:
        y = F.normalize(y, p=2.0, dim=1, eps=1e-12)
    y.backward(torch.tensor(g, dtype=torch.float64))
    with np.errstate(over="ignore"):
        return classes(z.grad.numpy().astype(np.float32))


def epilogue_class_mismatches(gz, t, g, relu, l2, limit=8):
    """first (row, col, class of gz, class torch gives) where the two differ.  One named deviation, MASK_NAN: under PS_RELU the
    header masks with t > 0, so the gradient at a NaN activation is +0.0, where torch's threshold_backward (which zeroes only
    where the result <= 0) passes it on."""
    got, want = classes(gz), epilogue_torch_classes(t, g, relu, l2)
    if relu:
        want[np.isnan(t)] = PZERO                          # MASK_NAN
    bad = np.argwhere(got != want)
    return [(int(r), int(c), CLASS_NAMES[got[r, c]], CLASS_NAMES[want[r, c]]) for r, c in bad[:limit]]
