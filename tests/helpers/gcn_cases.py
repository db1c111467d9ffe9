"""The case table of the fused GCN layer (csrc/dense_mfma.hip: ps_gcn_layer = gcn_count_kernel + gcn_order_kernel +
gemm_f32_kernel<1,4,2,2,32,0,true,GCN=1>) and of the neighbour pooling (csrc/importance_pool.hip, csrc/pool_row.h), numpy only.

It restates the launcher (gcn_chunk_rows, the served-shape test, the stable partition of the rows into those that keep a
neighbour -- "heavy" -- and the rest), lists the smallest served shapes with the class boundary PLANTED where the kernels can go
wrong, builds their operands (seeded by the case's name) and holds the references: oracle.c_oracle.pool_ex, the plain-C
restatement of the pooling arithmetic bit for bit, fed into c_oracle.linear's fmaf chain (the bits before the norm), and
gemm_cases.ref_normed / norm_bound / mismatches_normed after it.  tests/test_gcn_cases.py proves on the CPU that every case
produces the situation it names and that the oracle meets the bound derived below; tests/test_hip_gcn_matrix.py holds the
kernels to it.  The restatement is used to prove coverage and to word failure messages, never to compute an expected value.

The one-wave-per-row kernel (PS_POOL_ROWS_PER_WAVE=1, T > 64, or H % 4 != 0) sums the weights in another order than the
four-rows-per-wave kernel: entry e in lane e % 64, ps_wave_sum_f32 (csrc/ps_common.h: the 16-lane butterfly per DPP row, then
row_bcast:15 into rows 1 and 3, row_bcast:31 into row 3, lane 63 read: (R3 + R2) + (R1 + R0)).  CHOSEN: the oracle takes that
order as a second documented one (pool_ex(..., lanes=64)) and the kernel is held to its bits, not to the fp64 bound: the order
is as fixed by the code as the 16-lane one, and a bit-exact check also sees a wrong rounding of a weight, which a bound does not.

pool_bound -- the oracle against the fp64 restatement of ImportancePooling.forward (ref_pool64: every operation in fp64, the
weights count / tot unrounded), u = 2^-24, S = sum_j |w_j x_j| over the kept entries with the reference's final weights:
  * a weight (float)((double)c / (double)tot) is rounded once: relative error u (given fp32 weights: none);
  * the tree adds non-negative weights (asserted for every row that is renormalised; rows planted with a zero or negative sum
    are not divided): a term passes through at most D additions, D = (pages - 1) + log2(lanes) with pages = ceil(T / lanes), so
    the sum has relative error at most D u from its additions and u from its terms' own rounding;
  * the fp32 division adds u: a final weight is off by at most (1 + D + 1 + 1) u = (D + 3) u relatively;
  * the fma chain rounds once per entry, k <= T entries (a dropped entry's fmaf(+0, +0, acc) is exact): at most T u S.
  To first order (T + D + 3) u S; one more u covers the second-order terms ((T + D + 3)^2 u^2 < 1e-10 at T = 100).  Elementwise:
        |out - ref| <= (T + D + 4) 2^-24 S + 2^-149
  1.5e-6 S at T = 16 (D = 4).  The existing orc_importance_pool (sequential sum, mul + add) is compared with pool_ex under the
  same figure, as the issue sets it."""
import functools
import os
import sys
import zlib
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_cases import mismatches_normed, norm_bound, ref_normed  # noqa: E402,F401  (the fused layer's acceptance, not restated)

# ------------------------------------------------------------------------------------------------------ the launcher, restated
GCN_MAX_CHUNKS = 1024
MANY_ROWS = 64 * 384                      # ps_gcn_layer serves M >= 24 576
TILE = 64                                 # rows of a GEMM tile; ord[64 t .. 64 t + 63] is tile t
PASS = 256                                # rows gcn_order_kernel places per pass of its loop
N_OUT = 256


def _cdiv(a, b):
    return -(-a // b)


def gcn_chunk_rows(M):
    return max(_cdiv(_cdiv(M, GCN_MAX_CHUNKS), 256) * 256, 256)


def gcn_served(M, K, N, H, T, relu=True, l2=True, env=(), w_first=0, ldw=None, w2_first=0, ldw2=None):
    """does ps_gcn_layer serve the call (else PS_EUNSUPPORTED and the caller runs ps_importance_pool + ps_linear)?  w_first /
    w2_first: the first column of the W / W2 view inside its 16-byte aligned matrix; ld: its leading dimension"""
    env = dict(env)
    ldw = K if ldw is None else ldw
    ldw2 = H if ldw2 is None else ldw2
    if env.get("PS_GCN_FUSED") is not None and int(env["PS_GCN_FUSED"]) == 0:
        return False
    if int(env.get("PS_GEMM_SHARD", 0)) > 0 or env.get("PS_GEMM_DMA") or int(env.get("PS_POOL_ROWS_PER_WAVE", 0)) == 1:
        return False
    if N != 256 or not (relu and l2) or M < MANY_ROWS or M > 0x7fffffff - 64 or T > 16:
        return False
    aligned = lambda first, k, ld: (4 * first) % 16 == 0 and k % 32 == 0 and ld % 4 == 0       # noqa: E731
    return aligned(0, K, K) and aligned(w_first, K, ldw) and aligned(w2_first, H, ldw2) and aligned(0, H, H)


def row_keeps(ids, nvalid, T, max_idx):
    """bool[M]: does row i keep a neighbour (j < min(nvalid[i], T), 0 <= ids[i, j] <= max_idx)?  pool_row_keeps."""
    k = np.minimum(nvalid, T)
    return ((np.arange(T)[None, :] < k[:, None]) & (ids >= 0) & (ids <= max_idx)).any(axis=1)


def partition(keeps):
    """(ord, nheavy): the heavy rows ascending, then the rest ascending"""
    return np.concatenate([np.flatnonzero(keeps), np.flatnonzero(~keeps)]).astype(np.int64), int(keeps.sum())


def order_by_passes(keeps, carry=True):
    """gcn_count_kernel + gcn_order_kernel step by step: per chunk the count of heavy rows, the prefix over the chunks, then passes of
    256 rows that place each class behind what the earlier passes placed (hoff / eoff).  Returns ord with -1 where nothing was
    written.  carry=False forgets to advance hoff between the passes: what the case with two passes per chunk exists to catch."""
    M = keeps.size
    chunk = gcn_chunk_rows(M)
    starts = np.arange(0, M, chunk)
    cnt = np.array([int(keeps[r0:r0 + chunk].sum()) for r0 in starts])
    total = int(cnt.sum())
    ord_ = np.full(M, -1, dtype=np.int64)
    for r0, before in zip(starts, np.concatenate([[0], np.cumsum(cnt)[:-1]])):
        r1 = min(r0 + chunk, M)
        hoff, eoff = int(before), total + (int(r0) - int(before))
        for base in range(int(r0), r1, PASS):
            f = keeps[base:min(base + PASS, r1)]
            i = np.arange(base, base + f.size)
            ord_[hoff + np.arange(int(f.sum()))] = i[f]
            ord_[eoff + np.arange(int((~f).sum()))] = i[~f]
            hoff += int(f.sum()) if carry else 0
            eoff += int((~f).sum())
    return ord_, total


# ---------------------------------------------------------------------------------------------------------------- row metadata

def _seed(name):
    return zlib.crc32(name.encode()) & 0x7fffffff


Rows = namedtuple("Rows", "ids counts wts nvalid kind")
# what a row is there for (Rows.kind)
ORDINARY, NV_ABOVE_T, AT_MAX_IDX, LAST_SLOT_ONLY, ZERO_SUM, NEG_SUM, NV_FULL, NV_ZERO, ALL_DROPPED, NV_NEGATIVE = range(10)
HEAVY_KINDS = (ORDINARY, NV_ABOVE_T, AT_MAX_IDX, LAST_SLOT_ONLY, ZERO_SUM, NEG_SUM, NV_FULL, ORDINARY)
EMPTY_KINDS = (NV_ZERO, ALL_DROPPED, NV_ZERO, ALL_DROPPED, NV_NEGATIVE)


def make_rows(want, T, max_idx, id_end, rs):
    """ids / counts / wts / nvalid of rows that keep a neighbour exactly where `want` says (max_idx: the effective bound;
    ids in (max_idx, id_end) are the ones too large).  Every slot holds ordinary data -- valid ids beyond nvalid, positive counts
    and weights under dropped ids -- and every row cycles through a kind:
      heavy: ORDINARY (random nvalid, -1 pads and too-large ids inside j < k), NV_ABOVE_T (nvalid = T + 1 .. or INT32_MAX),
             AT_MAX_IDX (a kept id == max_idx), LAST_SLOT_ONLY (nvalid = T, only slot T - 1 kept), ZERO_SUM / NEG_SUM (given weights
             (0.5, -0.5) / (0.25, -0.75) on the two kept slots, or 0 / -0.5 at T = 1: heavy, never renormalised; ordinary rows in
             the counts form), NV_FULL (nvalid = T);
      empty: NV_ZERO (nvalid = 0 over valid ids), ALL_DROPPED (nvalid >= 1, every slot inside it -1 or too large, valid ids
             beyond it), NV_NEGATIVE (nvalid = -3).
    counts has zeros among positive ones (slot 0 is positive: no row has tot == 0 with nvalid >= 1)."""
    B = want.size
    rows = np.arange(B)
    kind = np.where(want, np.array(HEAVY_KINDS)[rows % len(HEAVY_KINDS)], np.array(EMPTY_KINDS)[rows % len(EMPTY_KINDS)])
    valid = lambda n: rs.randint(0, max_idx + 1, size=n).astype(np.int32)                       # noqa: E731
    large = lambda n: rs.randint(max_idx + 1, id_end, size=n).astype(np.int32)                  # noqa: E731
    ids = valid((B, T))
    r = rs.random_sample((B, T))
    ids[r < 0.15] = -1
    ids[(r >= 0.15) & (r < 0.30)] = large(int(((r >= 0.15) & (r < 0.30)).sum()))
    nvalid = rs.randint(1, T + 1, size=B).astype(np.int32)
    counts = rs.randint(1, 40, size=(B, T)).astype(np.int32)
    counts[rs.random_sample((B, T)) < 0.1] = 0
    counts[:, 0] = np.maximum(counts[:, 0], 1)
    wts = (rs.random_sample((B, T)) + 0.05).astype(np.float32)
    nvalid[kind == NV_FULL] = T
    m = kind == NV_ABOVE_T
    nvalid[m] = np.where(rows[m] % 3 == 0, 2 ** 31 - 1, T + 1 + rows[m] % 50)
    m = kind == LAST_SLOT_ONLY
    nvalid[m] = T
    drop = np.where(rs.random_sample((int(m.sum()), T)) < 0.5, -1, large((int(m.sum()), T)))
    ids[m] = drop
    ids[m, T - 1] = valid(int(m.sum()))
    for knd, (w0, w1) in ((ZERO_SUM, (0.5, -0.5)), (NEG_SUM, (0.25, -0.75))):
        m = kind == knd
        n = int(m.sum())
        if T == 1:
            nvalid[m] = 1
            ids[m, 0] = valid(n)
            wts[m, 0] = 0.0 if knd == ZERO_SUM else -0.5
        else:
            nvalid[m] = min(T, 3)
            ids[m, 0], ids[m, 1] = valid(n), valid(n)
            ids[m, 2:min(T, 3)] = -1
            wts[m, 0], wts[m, 1] = w0, w1
    # heavy rows of the remaining kinds: one slot inside k certainly kept (AT_MAX_IDX: at max_idx itself)
    m = np.isin(kind, (ORDINARY, NV_ABOVE_T, AT_MAX_IDX, NV_FULL))
    k = np.minimum(nvalid, T)
    slot = np.minimum((rs.random_sample(B) * k).astype(np.int64), k - 1)
    ids[rows[m], slot[m]] = np.where(kind[m] == AT_MAX_IDX, max_idx, valid(int(m.sum())))
    # empty rows
    nvalid[kind == NV_ZERO] = 0
    nvalid[kind == NV_NEGATIVE] = -3
    m = kind == ALL_DROPPED
    inside = m[:, None] & (np.arange(T)[None, :] < nvalid[:, None])
    ids[inside] = np.where(rs.random_sample(int(inside.sum())) < 0.5, -1, large(int(inside.sum())))
    assert np.array_equal(row_keeps(ids, nvalid, T, max_idx), want)
    return Rows(ids, counts, wts, nvalid, kind)


# ----------------------------------------------------------------------------------------------------------- fused-layer cases

GcnCase = namedtuple("GcnCase", "name M K H T form renorms pattern extra max_idx_above h_is_x wslice served situation")
RAGGED = MANY_ROWS + 37
BIG_M = 1024 * 256 + 256 + 5


def _pattern(c):
    """bool[M]: the rows that keep a neighbour"""
    M = c.M
    rs = np.random.RandomState(_seed("pattern" + c.name))
    want = np.zeros(M, dtype=bool)
    if c.pattern == "none":
        pass
    elif c.pattern == "last_only":
        want[M - 1] = True
    elif c.pattern in ("64j", "64j+1"):
        n = 64 * 191 + (c.pattern == "64j+1")
        want[rs.permutation(M)[:n]] = True
    elif c.pattern == "all_but_row0":
        want[1:] = True
    elif c.pattern == "all":
        want[:] = True
    elif c.pattern == "mixed":
        want = rs.random_sample(M) < 0.45
        if want.sum() % 64 == 0:
            want[np.flatnonzero(~want)[-1]] = True
    elif c.pattern == "two_pass":
        # chunks of 512 rows = two passes of 256: chunk % 3 == 0 mixes both classes in both passes, 1 is an empty first and a
        # heavy second pass, 2 the reverse
        chunk = gcn_chunk_rows(M)
        ch, ps = np.arange(M) // chunk, (np.arange(M) % chunk) // PASS
        want = np.where(ch % 3 == 0, rs.random_sample(M) < 0.5, np.where(ch % 3 == 1, ps == 1, ps == 0))
    else:
        raise ValueError(c.pattern)
    return want


def _gc(name, M, K, H, T, form, pattern, situation, renorms=(1, 0), extra=64 + 5, above=False, h_is_x=False, wslice=False,
        served=True):
    return GcnCase(name, M, K, H, T, form, tuple(renorms), pattern, extra, above, h_is_x, wslice, served, situation)


FUSED_CASES = (
    _gc("k256h256-T16-mixed-counts-hx", RAGGED, 256, 256, 16, "counts", "mixed", h_is_x=True, extra=0,
        situation="the benchmark's form (h_full is x, K == H == 256) at T = 16, ragged M whose last tile keeps nothing, a tile "
                  "that mixes both classes with x rows of -0.0 among its empty rows, kmax from every lane group"),
    _gc("k128h256-T5-mixed-wts", MANY_ROWS, 128, 256, 5, "wts", "mixed",
        situation="K != H (a swap of K / K2 or ldw / ldw2 shows), given weights with zero-sum and negative-sum rows, T = 5: a "
                  "gather batch with one live entry; h_full has more rows than M and is not x"),
    _gc("k32h64-T1-none-counts", MANY_ROWS, 32, 64, 1, "counts", "none", renorms=(1,),
        situation="nheavy = 0: no tile pools, T = 1"),
    _gc("k32h64-T4-last-only-counts", RAGGED, 32, 64, 4, "counts", "last_only", renorms=(1,),
        situation="nheavy = 1, the heavy row is row M - 1: tile 0 pools one heavy row and 63 empty ones"),
    _gc("k32h64-T4-64j-wts", MANY_ROWS, 32, 64, 4, "wts", "64j", renorms=(1,),
        situation="nheavy = 64 * 191: the class boundary on a tile boundary, no mixed tile"),
    _gc("k32h64-T5-64j+1-counts", RAGGED, 32, 64, 5, "counts", "64j+1", renorms=(1,),
        situation="nheavy = 64 * 191 + 1: one heavy row in the mixed tile"),
    _gc("k32h64-T16-all-but-row0-counts", MANY_ROWS, 32, 64, 16, "counts", "all_but_row0", renorms=(0,),
        situation="nheavy = M - 1, the empty row is row 0: it is the last row of the last tile"),
    _gc("k32h64-T4-all-wts", RAGGED, 32, 64, 4, "wts", "all", renorms=(0,),
        situation="nheavy = M with ragged M: the partial last tile is heavy (the M - 1 clamp of sOrd and rok in the pooling)"),
    _gc("k64h288-T5-mixed-counts", RAGGED, 64, 288, 5, "counts", "mixed",
        situation="H = 288: pool4_row's second sweep is partly beyond H"),
    _gc("k32h512-T4-mixed-wts", MANY_ROWS, 32, 512, 4, "wts", "mixed",
        situation="H = 512: two full sweeps"),
    _gc("k32h64-T4-mixed-counts-slices-above", MANY_ROWS, 32, 64, 4, "counts", "mixed", wslice=True, above=True,
        situation="W and W2 are column slices of one [256, K + H] matrix (ld = K + H, no copy), also run with image-order "
                  "weights; the max_idx argument is above n_full - 1"),
    _gc("k32h32-T2-two-pass-counts", BIG_M, 32, 32, 2, "counts", "two_pass", renorms=(1,),
        situation="M = 1024 * 256 + 256 + 5: 512-row chunks, two passes of gcn_order_kernel per chunk with hoff / eoff carried, "
                  "heavy and empty rows in both passes, a heavy second pass after an empty first, a partial last chunk"),
)

# dense.gcn_layer where ps_gcn_layer does not serve: the pair ps_importance_pool + ps_linear, held to the same oracle
UNSERVED_CASES = (
    _gc("unserved-M1000-T10", 1000, 32, 64, 10, "counts", "mixed", renorms=(1,), served=False, situation="M = 1000 < 64 * 384"),
    _gc("unserved-T17", MANY_ROWS, 32, 64, 17, "counts", "mixed", renorms=(1,), served=False, situation="T = 17 > 16"),
    _gc("unserved-T50-wts", RAGGED, 32, 64, 50, "wts", "mixed", renorms=(1,), served=False, situation="T = 50 > 16"),
)
SWITCHED_OFF_CASE = "k32h64-T5-64j+1-counts"          # a served case again under PS_GCN_FUSED=0

GcnData = namedtuple("GcnData", "x W b h_full rows W2 Wbig n_full max_idx max_idx_arg keeps planted")


@functools.lru_cache(maxsize=2)
def gcn_data(c):
    """Operands of case c.  x [M, K]; h_full [n_full, H] (x itself when c.h_is_x, else n_full = M + c.extra rows); W [256, K] and
    W2 [256, H]: contiguous copies for the oracle; Wbig [256, K + H] holds both (W = Wbig[:, :K], W2 = Wbig[:, K:]: the views the
    kernel gets when c.wslice).  The effective max_idx is n_full - 41, so the last 40 rows of h_full are ordinary rows no id may
    reach; ids go up to n_full + 8.  max_idx_arg is what the call passes: n_full - 41, or -- c.max_idx_above -- the rows are built
    for max_idx = n_full - 1 and the call passes n_full + 1000.
    planted: up to three rows of x set to -0.0 among the empty rows of the tile that mixes both classes (b[0] = 0: their
    pre-activation in column 0 is a signed zero)."""
    rs = np.random.RandomState(_seed(c.name))
    M, K, H, T = c.M, c.K, c.H, c.T
    n_full = M if c.h_is_x else M + c.extra
    max_idx = n_full - 1 if c.max_idx_above else n_full - 41
    max_idx_arg = n_full + 1000 if c.max_idx_above else max_idx
    x = rs.standard_normal((M, K)).astype(np.float32)
    h_full = x if c.h_is_x else rs.standard_normal((n_full, H)).astype(np.float32)
    Wbig = (rs.standard_normal((N_OUT, K + H)) / np.sqrt(K + H)).astype(np.float32)
    b = (rs.standard_normal(N_OUT) * 0.1).astype(np.float32)
    b[0] = 0.0
    keeps = _pattern(c)
    rows = make_rows(keeps, T, max_idx, n_full + 9, rs)
    ord_, nheavy = partition(keeps)
    planted = ()
    if nheavy % TILE and nheavy < M:
        planted = tuple(int(i) for i in ord_[nheavy:min(nheavy + 3, _cdiv(nheavy, TILE) * TILE, M)])
        x[list(planted)] = -0.0
    W, W2 = np.ascontiguousarray(Wbig[:, :K]), np.ascontiguousarray(Wbig[:, K:])
    for a in (x, h_full, W, W2, b, Wbig, keeps) + tuple(rows):
        a.setflags(write=False)
    return GcnData(x, W, b, h_full, rows, W2, Wbig, n_full, max_idx, max_idx_arg, keeps, planted)


def form_args(rows, form):
    """(counts, wts) of the form: the other one is None"""
    return (rows.counts, None) if form == "counts" else (None, rows.wts)


@functools.lru_cache(maxsize=4)
def gcn_ref(c, renorm):
    """(pooled fp32 [M, H], prenorm fp32 [M, 256]): pool_ex in the 16-lane order, then the fmaf chain x W^T + pooled W2^T + b,
    ReLU.  The kernels compute the same chain per output: the bits before the norm."""
    from oracle import c_oracle as co
    d = gcn_data(c)
    counts, wts = form_args(d.rows, c.form)
    pooled = co.pool_ex(d.h_full, d.rows.ids, counts, wts, d.rows.nvalid, max_idx=d.max_idx_arg, renorm=renorm, threads=8)
    pre = co.linear(d.x, d.W, d.b, x2=pooled, W2=d.W2, relu=True, l2norm=False, threads=8)
    pooled.setflags(write=False)
    pre.setflags(write=False)
    return pooled, pre


def gcn_mismatches(got, c, renorm):
    """gemm_cases.mismatches_normed of a ps_gcn_layer / dense.gcn_layer output against the oracle of case c"""
    pre = gcn_ref(c, renorm)[1]
    return mismatches_normed(got, pre, ref_normed(pre))


def facts(c):
    """What the restated launcher says of case c: a dict of the situations the table exists for (tests/test_gcn_cases.py asserts
    them per case; the GPU test prints them on failure)."""
    d = gcn_data(c)
    M, T = c.M, c.T
    ord_, nheavy = partition(d.keeps)
    ntiles = _cdiv(M, TILE)
    chunk = gcn_chunk_rows(M)
    k = np.clip(d.rows.nvalid, 0, T)
    # the wave that pools tile rows 4 q .. 4 q + 3 of a heavy tile: which lane group holds the strictly largest k?
    pad = np.full(ntiles * TILE, -1, dtype=np.int64)
    pad[:M] = k[ord_]
    quads = pad.reshape(-1, 4)[:_cdiv(nheavy, TILE) * (TILE // 4)]
    top = quads.max(axis=1)
    strict = (quads == top[:, None]).sum(axis=1) == 1
    groups = sorted(set(int(g) for g in quads[strict].argmax(axis=1)))
    f = dict(nheavy=nheavy, ntiles=ntiles, chunk=chunk, nchunks=_cdiv(M, chunk), passes=chunk // PASS,
             mixed_tile=nheavy // TILE if (nheavy % TILE and nheavy < M) else None,
             last_tile_rows=M - (ntiles - 1) * TILE, last_tile_heavy=(ntiles - 1) * TILE < nheavy,
             kmax_groups=groups, sweeps=_cdiv(c.H, 256), last_sweep_cols=c.H - (_cdiv(c.H, 256) - 1) * 256)
    return f


# --------------------------------------------------------------------------------------------------------------- pooling cases

PoolCase = namedtuple("PoolCase", "name kernel T H B N env")
POOL_ENV_ONE_ROW = (("PS_POOL_ROWS_PER_WAVE", "1"),)


def _pc(kernel, T, H, B, N=90, env=()):
    return PoolCase(f"{kernel}-T{T}-H{H}-B{B}", kernel, T, H, B, N, tuple(env))


# "four": importance_pool4_kernel<1> (T <= 16) / <4> (T <= 64); "wave": importance_pool_kernel<4> (by the switch, or T > 64) or
# <1> (H % 4 != 0).  B is no multiple of 4; every launch has several blocks.
POOL_CASES = (
    _pc("four", 1, 4, 37), _pc("four", 16, 260, 131), _pc("four", 17, 32, 70), _pc("four", 33, 512, 37), _pc("four", 64, 256, 70),
    _pc("wave", 10, 256, 37, env=POOL_ENV_ONE_ROW), _pc("wave", 64, 32, 70, env=POOL_ENV_ONE_ROW), _pc("wave", 65, 260, 37),
    _pc("wave", 100, 512, 41), _pc("wave", 10, 7, 37), _pc("wave", 16, 4, 131, env=POOL_ENV_ONE_ROW),
)
POOL_RUNS = (("counts", 1), ("counts", 0), ("wts", 1), ("wts", 0))


def pool_kernel(T, H, env=()):
    """the kernel ps_importance_pool launches for contiguous fp32 operands from the allocator (16-byte aligned)"""
    if H % 4 != 0:
        return "wave"
    return "four" if T <= 64 and int(dict(env).get("PS_POOL_ROWS_PER_WAVE", 0)) != 1 else "wave"


def lanes_of(kernel):
    return 16 if kernel == "four" else 64


PoolData = namedtuple("PoolData", "x rows max_idx keeps")


@functools.lru_cache(maxsize=None)
def pool_data(c):
    """x [N, H]; rows of every kind (the last row has nvalid above T); max_idx = N - 4 cuts x short, ids go up to N + 20"""
    rs = np.random.RandomState(_seed("pool" + c.name))
    x = rs.standard_normal((c.N, c.H)).astype(np.float32)
    want = rs.random_sample(c.B) < 0.7
    want[-1] = True
    max_idx = c.N - 4
    rows = make_rows(want, c.T, max_idx, c.N + 21, rs)
    if rows.kind[-1] in (ZERO_SUM, NEG_SUM):
        rows.ids[-1, min(c.T, 3):] = -1                                    # the planted sum stays what it is under a larger nvalid
    rows.nvalid[-1] = c.T + 7                                              # the last row: entries beyond it are beyond the buffers
    assert np.array_equal(row_keeps(rows.ids, rows.nvalid, c.T, max_idx), want)
    for a in (x, want) + tuple(rows):
        a.setflags(write=False)
    return PoolData(x, rows, max_idx, want)


@functools.lru_cache(maxsize=None)
def pool_ref(c, form, renorm, lanes):
    from oracle import c_oracle as co
    d = pool_data(c)
    counts, wts = form_args(d.rows, form)
    out = co.pool_ex(d.x, d.rows.ids, counts, wts, d.rows.nvalid, max_idx=d.max_idx, renorm=renorm, lanes=lanes, threads=8)
    out.setflags(write=False)
    return out


def tree_depth(T, lanes):
    """additions a weight passes through on its way into wsum: the lane's pages, then the butterfly"""
    return (_cdiv(T, lanes) - 1) + {16: 4, 64: 6}[lanes]


def pool_bound(T, lanes):
    """relative to S = sum_j |w_j x_j| (module docstring)"""
    return (T + tree_depth(T, lanes) + 4) * 2.0 ** -24


def ref_pool64(x, ids, counts, wts, nvalid, max_idx, renorm):
    """(out fp64 [B, H], S fp64 [B, H], renormalised bool[B], nonneg bool[B]): ImportancePooling.forward in fp64 throughout --
    k = min(nvalid, T), the weights count / tot unrounded (or the given fp32 values), dropped entries 0, divided by their sum when
    renorm and it is positive -- and S = sum_j |w_j x_j| with those final weights.  nonneg: no kept weight of the row is negative."""
    B, T = ids.shape
    max_idx = min(max_idx, x.shape[0] - 1)
    k = np.clip(nvalid, 0, T)
    inside = np.arange(T)[None, :] < k[:, None]
    keep = inside & (ids >= 0) & (ids <= max_idx)
    if wts is None:
        tot = (counts * inside).sum(axis=1, dtype=np.int64).astype(np.float64)
        w = counts.astype(np.float64) / np.where(tot > 0, tot, 1.0)[:, None]
    else:
        w = wts.astype(np.float64)
    w = np.where(keep, w, 0.0)
    s = w.sum(axis=1)
    div = (s > 0) & bool(renorm)
    w = w / np.where(div, s, 1.0)[:, None]
    g = x.astype(np.float64)[np.where(keep, ids, 0)]                       # [B, T, H]
    out = (g * w[:, :, None]).sum(axis=1)
    S = (np.abs(g) * np.abs(w)[:, :, None]).sum(axis=1)
    return out, S, div, (w >= 0).all(axis=1)


def pool_mismatches_bound(got, ref64, S, T, lanes, limit=8):
    """first `limit` (row, col, got, want) where fp32 `got` leaves pool_bound(T, lanes) * S + 2^-149 around the fp64 reference"""
    with np.errstate(invalid="ignore"):
        ok = np.abs(got.astype(np.float64) - ref64) <= pool_bound(T, lanes) * S + 2.0 ** -149
    return [(int(r), int(c), float(got[r, c]), float(ref64[r, c])) for r, c in np.argwhere(~ok)[:limit]]
