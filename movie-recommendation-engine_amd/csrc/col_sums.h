// Two fp64 sums per column of an [M, N] matrix without atomics (ps_bn_batch_stats: z and z^2; ps_bn_bwd: ga and ga xh;
// ps_layer_norm_bwd: gy and gy xh over the live rows, a dead row inside its partition adding (+0.0, +0.0)).
// The rows are cut into partitions of PS_BN_ROWS consecutive rows (a function of M only).  ps_col_sums_partition is one
// workgroup's work on partition p and its 64 VEC columns: wave w takes the rows r0 + w, r0 + w + 4, ... ascending, every lane
// adds its columns' two addends in fp64, and the four waves' sums are added in wave order through LDS into part[p, 0 / 1, col].
// ps_col_sums_finish adds a column's partitions in ascending order.  Every word of part that is read was written by the same
// call: equal inputs give equal bits.
//
// A row past the partition adds nothing.  Under SKIP_DEAD it is skipped by a wave-uniform branch and its addends are never
// formed (ps_bn_bwd: what `terms` makes of a masked load is not zero).  Without SKIP_DEAD it goes through `terms` like a live
// row, and the caller promises that `terms` of a masked load is (+0.0, +0.0) (ps_bn_batch_stats: z and z * z of z = +0.0; no
// branch in the add loop, which measured 0.7 % faster at 59 047 x 256).  The two give the same bits: x + (+0.0) differs from x
// only for x = -0.0, and a sum that starts at +0.0 never is -0.0 (only -0.0 + -0.0 gives that).  A masked COLUMN of a live row
// goes through `terms` either way; its sums are never stored.
#pragma once
#include "ps_common.h"

constexpr int PS_BN_ROWS = 128;                // rows per partition
static inline int64_t ps_bn_partitions(int64_t M) { return ps_cdiv(M, PS_BN_ROWS); }

// load(rr, live) requests what row rr contributes (nothing when !live) and returns it; UNROLL rows are in flight.
// terms(row, e, a, b) sets the two addends of element e of a row.
// All 256 threads of the workgroup call it together; a caller that loops over partitions puts a __syncthreads() between calls.
template <int VEC, int UNROLL, bool SKIP_DEAD, typename LOAD, typename TERMS>
__device__ __forceinline__ void ps_col_sums_partition(int64_t M, int N, int64_t p, int col, LOAD load, TERMS terms,
                                                      double *__restrict__ part) {
    __shared__ double sh[3][2][64 * VEC];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r0 = p * PS_BN_ROWS;
    const int64_t r1 = (r0 + PS_BN_ROWS < M) ? r0 + PS_BN_ROWS : M;
    double s[2][VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) { s[0][e] = 0.0; s[1][e] = 0.0; }
    for (int64_t r = r0 + wave; r < r1; r += 4 * UNROLL) {
        decltype(load(r, true)) rows[UNROLL];
#pragma unroll
        for (int t = 0; t < UNROLL; ++t) rows[t] = load(r + 4 * t, r + 4 * t < r1);
#pragma unroll
        for (int t = 0; t < UNROLL; ++t) {
            if (SKIP_DEAD && r + 4 * t >= r1) continue;                  // wave-uniform
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                double a, b;
                terms(rows[t], e, a, b);
                s[0][e] += a;
                s[1][e] += b;
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            sh[wave - 1][0][lane * VEC + e] = s[0][e];
            sh[wave - 1][1][lane * VEC + e] = s[1][e];
        }
    }
    __syncthreads();
    if (wave == 0 && col < N) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            double a = s[0][e], b = s[1][e];
#pragma unroll
            for (int w = 0; w < 3; ++w) {
                a += sh[w][0][lane * VEC + e];
                b += sh[w][1][lane * VEC + e];
            }
            part[(p * 2 + 0) * N + col + e] = a;
            part[(p * 2 + 1) * N + col + e] = b;
        }
    }
}

// (S0, S1) of column c: the P partitions added in ascending order from 0.0, two chains
__device__ __forceinline__ double2 ps_col_sums_finish(const double *__restrict__ part, int64_t P, int N, int c) {
    double S0 = 0.0, S1 = 0.0;
#pragma unroll 32                                                        // the loads of 32 partitions in flight ahead of the two add chains
    for (int64_t p = 0; p < P; ++p) {
        S0 += part[(p * 2 + 0) * N + c];
        S1 += part[(p * 2 + 1) * N + c];
    }
    return make_double2(S0, S1);
}
