"""The dense GEMM's case table (csrc/dense_mfma.hip: ps_linear, ps_lsh_encode), numpy only.

launch_gemm / launch_gemm_v pick among a dozen kernel instantiations by M, N, the flags, the operands' alignment and three
environment switches.  This module lists the smallest shapes that reach every one of them with a ragged last tile, builds their
operands (seeded by the case's name, with planted rows), restates the launcher's choice as a string (`launcher_choice`: for the
coverage proof in tests/test_gemm_cases.py and for failure messages, never to compute an expected value) and holds the two
references: the C oracle's k-ordered fmaf chain before the norm (`ref_prenorm`), and the row norm of THAT fp32 matrix evaluated
in fp64 (`ref_normed`) with a derived bound (`norm_bound`).

Planted in every case: W's column 0 is |w| + 0.5 (ordinary data, but positive); row 0 of x (and x2) is all zero when M >= 2, so
its output is the bias alone; when M >= 3, row 1 is x = (-100, 0, ...), x2 = 0: every pre-activation is b[n] - 100 W[n, 0] <= b[n] - 50
< 0, so with ReLU the whole row is +0 and the norm takes its 1e-12 clamp -- in a tile whose other rows are ordinary, which is
what sends ONE wave of the fused epilogue down its division path.  The last row and the last column are ordinary data.  (M = 1:
the single row is ordinary data; a zero row there would leave nothing of the product to check.)"""
import functools
import zlib
from collections import namedtuple

import numpy as np

# (relu, l2norm)
NONE, RELU, RELU_L2, L2 = (False, False), (True, False), (True, True), (False, True)
ALL_THREE = (NONE, RELU, RELU_L2)

Case = namedtuple("Case", "name M K N K2 layout flagsets kernel")

LAYOUTS = ("plain", "w_off1", "ld33")
# W as the kernel sees it: (first column of the view inside its matrix, columns the matrix has beyond K)
_LAYOUT_GEOMETRY = {"plain": (0, 0), "w_off1": (1, 4), "ld33": (0, 1)}

# ------------------------------------------------------------------------------------------------------ the launcher, restated
SH_BM, SH_BN, SHARD_TILES_RING3, SHARD_TILES_RING2 = 32, 256, 256, 512      # gemm_shard_kernel's tile and launch_gemm's thresholds
MANY_ROWS = 64 * 384                                                        # launch_gemm_v: 64 x 256 tiles from here on
NORM_TAIL = " + l2norm_rows_kernel"


def is_fast(K, K2, layout):
    """aligned_operand() for every operand: 16-byte pointers, K % 32 == 0, ld % 4 == 0 (x / x2 are contiguous allocations)"""
    return layout == "plain" and K % 32 == 0 and K2 % 32 == 0


def launcher_choice(M, K, N, K2, layout, l2, env=(), staged=False, lsh=False):
    """The kernel launch_gemm<EPI> picks, as a string.  env: the PS_GEMM_* switches set; staged: image-order weights (PS_WPERM);
    lsh: ps_lsh_encode (EPI 1: never sharded by size, no norm).  N > 256 with the norm: ps_linear clears the flag and appends
    l2norm_rows_kernel."""
    env = dict(env)
    fast = is_fast(K, K2, layout) or (staged and K % 32 == 0 and K2 % 32 == 0)     # a staged weight is a fresh contiguous matrix
    tail = NORM_TAIL if (l2 and N > 256) else ""
    l2 = l2 and N <= 256 and not lsh
    mode = int(env.get("PS_GEMM_SHARD", -1))
    tiles = -(-M // SH_BM) * -(-N // SH_BN)
    by_size = (not lsh) and l2 and tiles <= SHARD_TILES_RING2
    if fast and N > 128 and mode != 0 and (mode > 0 or by_size):
        ring = 3 if (mode == 3 or (mode < 0 and tiles <= SHARD_TILES_RING3)) else 2
        return f"gemm_shard_kernel<ring {ring}, {'WPERM' if staged else 'plain'}>" + tail
    if fast and "PS_GEMM_DMA" in env and not staged and N % 256 == 0 and M >= MANY_ROWS:
        return "gemm_dma_kernel" + tail
    persist = int(env.get("PS_GEMM_PERSIST", 1)) != 0
    if fast and N > 128 and persist:
        if not l2:
            return "gemm_f32_pkernel<2,2,1,2>" + tail
        if M < MANY_ROWS:
            return "gemm_f32_pkernel<1,4,1,2>"
    f = "FAST" if fast else "general"
    if N <= 64:
        return f"gemm_f32_kernel<2,2,1,1,{f}>"
    if N <= 128:
        return f"gemm_f32_kernel<2,2,1,2,{f}> one column tile"
    if not l2:
        return f"gemm_f32_kernel<2,2,1,2,{f}> several column tiles" + tail
    if M < MANY_ROWS:
        return f"gemm_f32_kernel<1,4,1,2,{f}>"
    return f"gemm_f32_kernel<1,4,2,2,{f}>"


# Every instantiation the launcher can pick for ps_linear / ps_lsh_encode (tests/test_gemm_cases.py holds the runs of the GPU
# tests against this set)
INSTANTIATIONS = frozenset(
    [f"gemm_f32_kernel<2,2,1,1,{f}>" for f in ("FAST", "general")] +
    [f"gemm_f32_kernel<2,2,1,2,{f}> {t}" for f in ("FAST", "general") for t in ("one column tile", "several column tiles")] +
    [f"gemm_f32_kernel<1,4,1,2,{f}>" for f in ("FAST", "general")] +
    [f"gemm_f32_kernel<1,4,2,2,{f}>" for f in ("FAST", "general")] +
    ["gemm_f32_pkernel<2,2,1,2>", "gemm_f32_pkernel<1,4,1,2>"] +
    [f"gemm_shard_kernel<ring {r}, {w}>" for r in (2, 3) for w in ("WPERM", "plain")] +
    ["gemm_dma_kernel", "l2norm_rows_kernel"])


# ------------------------------------------------------------------------------------------------------------------ the table

def _case(M, K, N, K2, layout, flagsets, kernel):
    return Case(f"{M}x{K}x{N}+{K2}-{layout}", M, K, N, K2, layout, tuple(flagsets), kernel)


def _table():
    t = []
    # N <= 64
    t += [_case(65, 32, 64, 0, "plain", ALL_THREE, "gemm_f32_kernel<2,2,1,1,FAST>"),
          _case(63, 32, 1, 0, "plain", ALL_THREE, "gemm_f32_kernel<2,2,1,1,FAST>"),
          _case(64, 32, 64, 32, "w_off1", ALL_THREE, "gemm_f32_kernel<2,2,1,1,general>"),
          _case(130, 31, 33, 5, "plain", ALL_THREE, "gemm_f32_kernel<2,2,1,1,general>"),
          _case(70, 36, 40, 4, "plain", ALL_THREE, "gemm_f32_kernel<2,2,1,1,general>")]
    # 64 < N <= 128
    t += [_case(65, 64, 65, 0, "plain", ALL_THREE, "gemm_f32_kernel<2,2,1,2,FAST> one column tile"),
          _case(129, 64, 128, 32, "plain", ALL_THREE, "gemm_f32_kernel<2,2,1,2,FAST> one column tile"),
          _case(70, 36, 100, 4, "plain", ALL_THREE, "gemm_f32_kernel<2,2,1,2,general> one column tile"),
          _case(70, 37, 127, 3, "plain", ALL_THREE, "gemm_f32_kernel<2,2,1,2,general> one column tile"),
          _case(66, 32, 96, 0, "ld33", ALL_THREE, "gemm_f32_kernel<2,2,1,2,general> one column tile")]
    # N > 128 without the norm
    t += [_case(130, 32, 129, 0, "plain", (NONE, RELU), "gemm_f32_pkernel<2,2,1,2>"),
          _case(200, 64, 300, 32, "plain", (NONE, RELU), "gemm_f32_pkernel<2,2,1,2>"),
          _case(64, 32, 512, 0, "plain", (NONE, RELU), "gemm_f32_pkernel<2,2,1,2>"),
          _case(130, 33, 257, 0, "plain", (NONE, RELU), "gemm_f32_kernel<2,2,1,2,general> several column tiles"),
          _case(90, 32, 257, 0, "w_off1", (NONE, RELU), "gemm_f32_kernel<2,2,1,2,general> several column tiles"),
          _case(90, 32, 200, 32, "ld33", (NONE, RELU), "gemm_f32_kernel<2,2,1,2,general> several column tiles")]
    # fused norm, 128 < N <= 256, aligned operands: the ring of three (<= 256 tiles), of two (<= 512), the persistent 32 x 256 tile
    # (16 384 < M < 24 576), the 64 x 256 tile
    for M in (1, 31, 33):
        for N in (129, 200, 256):
            for K2 in (0, 32):
                t.append(_case(M, 64, N, K2, "plain", (RELU_L2, L2), "gemm_shard_kernel<ring 3, plain>"))
    t += [_case(8193, 32, 200, 0, "plain", (RELU_L2, L2), "gemm_shard_kernel<ring 2, plain>"),
          _case(16417, 32, 129, 32, "plain", (RELU_L2, L2), "gemm_f32_pkernel<1,4,1,2>"),
          _case(24577, 32, 200, 0, "plain", (RELU_L2, L2), "gemm_f32_kernel<1,4,2,2,FAST>"),
          _case(24577, 32, 256, 32, "plain", (RELU_L2, L2), "gemm_f32_kernel<1,4,2,2,FAST>")]
    # fused norm, unaligned operands
    t += [_case(33, 36, 130, 0, "plain", (RELU_L2,), "gemm_f32_kernel<1,4,1,2,general>"),
          _case(33, 33, 255, 7, "plain", (RELU_L2,), "gemm_f32_kernel<1,4,1,2,general>"),
          _case(24577, 36, 130, 4, "plain", (RELU_L2,), "gemm_f32_kernel<1,4,2,2,general>"),
          _case(24577, 33, 255, 0, "plain", (RELU_L2,), "gemm_f32_kernel<1,4,2,2,general>"),
          _case(24577, 32, 200, 0, "w_off1", (RELU_L2,), "gemm_f32_kernel<1,4,2,2,general>")]
    # N > 256 with the norm: the GEMM without it, then l2norm_rows_kernel with more rows than its 16 384 waves
    t += [_case(16500, 32, 257, 0, "plain", (RELU_L2,), "gemm_f32_pkernel<2,2,1,2>" + NORM_TAIL),
          _case(16500, 33, 300, 0, "plain", (RELU_L2,), "gemm_f32_kernel<2,2,1,2,general> several column tiles" + NORM_TAIL)]
    return tuple(t)


CASES = _table()
FAST_CASES = tuple(c for c in CASES if is_fast(c.K, c.K2, c.layout))
DMA_CASE = "24577x32x256+32-plain"

# test_linear_matrix_under_every_launcher_switch: the switches, each with plain and image-order weights (the LDS-DMA kernel takes
# no image-order weights and serves whole 256-column tiles of many rows only: one case)
SWITCHES = ((("PS_GEMM_SHARD", "0"),), (("PS_GEMM_SHARD", "2"),), (("PS_GEMM_SHARD", "3"),),
            (("PS_GEMM_PERSIST", "0"), ("PS_GEMM_SHARD", "0")))
DMA_SWITCH = (("PS_GEMM_DMA", "1"),)


def switch_runs(c):
    """(env, staged) of every run test_linear_matrix_under_every_launcher_switch makes of FAST case c"""
    runs = [((), True)]                                                   # the launcher's own choice with image-order weights
    runs += [(env, staged) for env in SWITCHES for staged in (False, True)]
    if c.name == DMA_CASE:
        runs.append((DMA_SWITCH, False))
    return runs


def kernels_of(choice):
    """the instantiations a launcher_choice string names"""
    return {choice[:-len(NORM_TAIL)], "l2norm_rows_kernel"} if choice.endswith(NORM_TAIL) else {choice}


# ------------------------------------------------------------------------------------------------------------------- operands

def _seed(name):
    return zlib.crc32(name.encode()) & 0x7fffffff


def embed(W, layout, rs):
    """W [N, K] inside the matrix its layout names, the rest of which is ordinary data too (a kernel that read the wrong
    columns would see plausible numbers): plain -> W itself; w_off1 -> [N, K + 4], W at columns 1 .. K; ld33 -> [N, K + 1], W at
    columns 0 .. K - 1."""
    first, extra = _LAYOUT_GEOMETRY[layout]
    if extra == 0:
        return np.ascontiguousarray(W)
    big = rs.standard_normal((W.shape[0], W.shape[1] + extra)).astype(np.float32)
    big[:, first:first + W.shape[1]] = W
    return big


def view_of(big, K, layout):
    """the [N, K] view of embed()'s matrix: numpy array or torch tensor alike, no copy"""
    first = _LAYOUT_GEOMETRY[layout][0]
    return big if layout == "plain" else big[:, first:first + K]


def claimed_alignment(K, layout):
    """(byte offset of the view's first element from a 16-byte boundary, leading dimension)"""
    first, extra = _LAYOUT_GEOMETRY[layout]
    return 4 * first, K + extra


Data = namedtuple("Data", "x W b x2 W2 Wbig W2big")


@functools.lru_cache(maxsize=None)
def case_data(c):
    """Data of case c: x [M, K], W [N, K] (contiguous copies for the oracle), b [N], x2 / W2 or None, and the matrices that
    hold W / W2 in the case's layout (view_of() gives the operand the kernel gets)"""
    rs = np.random.RandomState(_seed(c.name))
    Kt = c.K + c.K2
    x = rs.standard_normal((c.M, c.K)).astype(np.float32)
    Wfull = (rs.standard_normal((c.N, Kt)) / np.sqrt(Kt)).astype(np.float32)
    b = rs.standard_normal(c.N).astype(np.float32)
    x2 = rs.standard_normal((c.M, c.K2)).astype(np.float32) if c.K2 else None
    Wfull[:, 0] = np.abs(Wfull[:, 0]) + np.float32(0.5)
    if c.M >= 2:
        x[0] = 0.0
        if c.K2:
            x2[0] = 0.0
    if c.M >= 3:
        x[1] = 0.0
        x[1, 0] = -100.0
        if c.K2:
            x2[1] = 0.0
    W = np.ascontiguousarray(Wfull[:, :c.K])
    W2 = np.ascontiguousarray(Wfull[:, c.K:]) if c.K2 else None
    Wbig = embed(W, c.layout, rs)
    W2big = embed(W2, c.layout, rs) if c.K2 else None
    for a in (x, W, b, x2, W2, Wbig, W2big):
        if a is not None:
            a.setflags(write=False)
    return Data(x, W, b, x2, W2, Wbig, W2big)


# ----------------------------------------------------------------------------------------------------------------- references

@functools.lru_cache(maxsize=None)
def ref_prenorm(c, relu):
    """fp32 [M, N]: the C oracle's fmaf chain (k ascending from +0, x then x2, + bias, ReLU), from contiguous operands.  The
    kernels compute the same chain per output: bit-identical."""
    from oracle import c_oracle as co
    d = case_data(c)
    y = co.linear(d.x, d.W, d.b, x2=d.x2, W2=d.W2, relu=relu, l2norm=False, threads=8)
    y.setflags(write=False)
    return y


def ref_normed(v):
    """fp64: rows of the fp32 matrix v over max(their norm, 1e-12) (F.normalize), every operation in fp64"""
    v64 = v.astype(np.float64)
    return v64 / np.maximum(np.sqrt((v64 ** 2).sum(1)), 1e-12)[:, None]


@functools.lru_cache(maxsize=None)
def ref_normed_of(c, relu):
    r = ref_normed(ref_prenorm(c, relu))
    r.setflags(write=False)
    return r


def norm_bound(N):
    """Relative bound on an fp32 row normalisation of N columns against ref_normed of the SAME fp32 pre-norm values, u = 2^-24:
    an fp32 sum of N non-negative squares -- each square rounded once, or fused into the addition -- has relative error at most
    N u in any summation order (every term passes through at most N roundings, all terms have one sign, so the errors cannot be
    amplified by cancellation); the square root halves a relative error and adds its own rounding u; the division is correctly
    rounded (tests/test_hip_model.py::test_fused_norm_quotient_is_the_ieee_division) and adds u.  (N / 2 + 2) u to first order;
    one more u covers the second-order terms (N^2 u^2 / 8 < 1e-10 at N = 512).  Elementwise:
        |y - ref| <= (N / 2 + 3) 2^-24 |ref| + 2^-149
    (the absolute term: a quotient in the subnormal range is rounded to a multiple of 2^-149).  7.8e-6 at N = 256."""
    return (N / 2.0 + 3.0) * 2.0 ** -24


def mismatches_exact(got, want, limit=8):
    """first `limit` (row, col, got, want) where two fp32 matrices differ in their BITS (-0 is not +0)"""
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    return [(int(r), int(c), float(got[r, c]), float(want[r, c])) for r, c in bad[:limit]]


def mismatches_normed(got, prenorm, ref64, limit=8):
    """first `limit` (row, col, got, want) where the normalised fp32 matrix `got` leaves norm_bound(N) around ref64, or where a
    row that is all zero before the norm (prenorm) is not +0 bits"""
    assert got.dtype == np.float32 and got.shape == ref64.shape, (got.dtype, got.shape, ref64.shape)
    N = got.shape[1]
    with np.errstate(invalid="ignore"):
        ok = np.abs(got.astype(np.float64) - ref64) <= norm_bound(N) * np.abs(ref64) + 2.0 ** -149      # NaN: not ok
    zero_rows = ~prenorm.any(axis=1)
    ok[zero_rows] &= got.view(np.uint32)[zero_rows] == 0
    bad = np.argwhere(~ok)
    return [(int(r), int(c), float(got[r, c]), float(ref64[r, c])) for r, c in bad[:limit]]


# ------------------------------------------------------------------------------------------------------------------ LSH encode

LshCase = namedtuple("LshCase", "name n D nbits layout")
LSH_CASES = tuple(LshCase(f"{n}x{D}x{nbits}-{layout}", n, D, nbits, layout) for n, D, nbits, layout in (
    (65, 32, 32, "plain"), (130, 33, 64, "plain"), (70, 36, 96, "plain"), (129, 64, 128, "plain"), (33, 37, 160, "plain"),
    (200, 32, 512, "plain"), (8193, 32, 256, "plain"), (90, 32, 160, "w_off1"), (90, 32, 64, "ld33")))
LSH_FAST_CASES = tuple(c for c in LSH_CASES if is_fast(c.D, 0, c.layout))
LSH_SWITCHES = ((("PS_GEMM_SHARD", "0"),), (("PS_GEMM_SHARD", "2"),), (("PS_GEMM_SHARD", "3"),))

LshData = namedtuple("LshData", "x A x_call A_store A_first D_call")


@functools.lru_cache(maxsize=None)
def lsh_data(c):
    """x [n, D], A [nbits, D]: what the oracle encodes.  x_call [n, D_call], A_store (flat fp32), A_first: what ps_lsh_encode gets
    -- A as A_store[A_first : A_first + nbits * D_call], rows D_call apart.  ps_lsh_encode has no leading dimension of its own
    (rows of A are D apart), so a strided A is legal only as a whole matrix:
      plain:  A itself.
      w_off1: A stored from element 1 of a buffer: every row starts 4 bytes off a 16-byte boundary, D_call = D.
      ld33:   A is the first D columns of a [nbits, D + 1] matrix; the call passes D_call = D + 1 -- the whole matrix, ld % 4 == 1
              -- and x with one more column of zeros.  fmaf(+0, a, acc) == acc for finite a, except that acc = -0 becomes +0,
              which `>= 0` does not see: the codes are those of (x, A).
    Planted: x row 0 all zero (every bit 1: +0 >= 0); x row 1 = (1, -1, 0, ...) against A row 0 = (1, 1, 0, ...) and
    A row 1 = -(1, 1, 0, ...): dots of exactly +0, bit 1."""
    rs = np.random.RandomState(_seed("lsh" + c.name))
    x = rs.standard_normal((c.n, c.D)).astype(np.float32)
    A = rs.standard_normal((c.nbits, c.D)).astype(np.float32)
    x[0] = 0.0
    x[1] = 0.0
    x[1, 0], x[1, 1] = 1.0, -1.0
    A[0] = 0.0
    A[0, 0], A[0, 1] = 1.0, 1.0
    A[1] = -A[0]
    if c.layout == "plain":
        x_call, store, first, D_call = x, A.reshape(-1).copy(), 0, c.D
    elif c.layout == "w_off1":
        store = rs.standard_normal(c.nbits * c.D + 4).astype(np.float32)
        store[1:1 + A.size] = A.reshape(-1)
        x_call, first, D_call = x, 1, c.D
    else:
        big = rs.standard_normal((c.nbits, c.D + 1)).astype(np.float32)
        big[:, :c.D] = A
        x_call = np.concatenate([x, np.zeros((c.n, 1), dtype=np.float32)], axis=1)
        store, first, D_call = big.reshape(-1).copy(), 0, c.D + 1
    for a in (x, A, x_call, store):
        a.setflags(write=False)
    return LshData(x, A, x_call, store, first, D_call)


@functools.lru_cache(maxsize=None)
def lsh_ref(c):
    from oracle import c_oracle as co
    d = lsh_data(c)
    codes = co.lsh_encode(d.x, d.A, threads=8)
    codes.setflags(write=False)
    return codes
