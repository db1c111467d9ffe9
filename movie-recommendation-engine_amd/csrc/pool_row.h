// pool_row.h -- the per-row math of the four-rows-per-wave importance pooling (csrc/importance_pool.hip), shared with the fused
// layer GEMM of csrc/dense_mfma.hip (ps_gcn_layer), so that both compute a pooled row with the same instructions in the same order.
#pragma once
#include "ps_common.h"

namespace {

template <int CTRL>
__device__ __forceinline__ int row_bcast_i32(int v) { return ps_dpp_step<CTRL, 0xf, false>(v, 0); }
// Does row i keep at least one neighbour (j < nvalid[i], 0 <= ids[i, j] <= max_idx)?  The keep test of pool4_row below: a row that
// keeps none is pooled to +0.0 in every column without touching x.
__device__ __forceinline__ bool pool_row_keeps(const int32_t *__restrict__ ids, const int32_t *__restrict__ nvalid, int64_t i, int T,
                                               int64_t max_idx) {
    // sixteen entries per round trip, requested together with nvalid (an early exit per entry measured one round trip per entry)
    int k = nvalid[i];
    k = k < T ? k : T;
    bool keep = false;
    for (int j0 = 0; j0 < T; j0 += 16) {
        int32_t v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = j0 + u < T ? ids[i * T + j0 + u] : -1;
#pragma unroll
        for (int u = 0; u < 16; ++u) keep |= j0 + u < k && v[u] >= 0 && (int64_t)v[u] <= max_idx;
        if (keep || j0 + 16 >= k) break;
    }
    return keep;
}

// The final weights of row i in the four-rows-per-wave layout: entry e = p * 16 + l of the row sits in lane l of the row's 16-lane
// group, page p.  On return id[p] is the entry's id (-1: not kept), w[p] the weight its gathered row is multiplied by (+0.0: not
// kept) and k = min(nvalid[i], T).  All 64 lanes of the wave must call it together (DPP across the group).  Shared by pool4_row
// below and by ps_pool_weights (csrc/neigh_agg_bwd.hip), whose backward needs the very weights the forward applied.
template <int PAGES>
__device__ __forceinline__ void pool4_weights(const int32_t *__restrict__ ids, const int32_t *__restrict__ counts,
                                              const float *__restrict__ wts, const int32_t *__restrict__ nvalid, int64_t i, bool rok,
                                              int T, int64_t max_idx, int renorm, int32_t (&id)[PAGES], float (&w)[PAGES], int &k) {
    const int l = threadIdx.x & 15;
    // ---- one round trip: nvalid, ids, counts / weights of the wave's four rows ----
    k = rok ? nvalid[i] : 0;
    int32_t cn[PAGES];
#pragma unroll
    for (int p = 0; p < PAGES; ++p) {
        const int e = p * 16 + l;
        const bool in = rok && e < T;
        id[p] = in ? ids[i * T + e] : -1;
        cn[p] = (in && counts) ? counts[i * T + e] : 0;
        w[p] = (in && wts) ? wts[i * T + e] : 0.f;
    }
    k = k < T ? k : T;
    // ---- weights: count / sum of the row's kept counts in fp64 -> fp32 (utils/random_walk.py:113-115 -> pinsage.py:140),
    // ids beyond max_idx dropped (:123-129), renormalised by their fp32 sum when it is positive (:141-143) ----
    int tot = 0;
#pragma unroll
    for (int p = 0; p < PAGES; ++p) tot += (p * 16 + l < k) ? cn[p] : 0;
    tot = ps_row16_sum_i32(tot);
    float wsum = 0.f;
#pragma unroll
    for (int p = 0; p < PAGES; ++p) {
        const bool keep = (p * 16 + l < k) && id[p] >= 0 && (int64_t)id[p] <= max_idx;
        w[p] = keep ? (wts ? w[p] : (float)((double)cn[p] / (double)tot)) : 0.f;
        id[p] = keep ? id[p] : -1;
        wsum += w[p];
    }
    wsum = ps_row16_sum_f32(wsum);
    if (renorm && wsum > 0.f) {
#pragma unroll
        for (int p = 0; p < PAGES; ++p) w[p] = id[p] >= 0 ? w[p] / wsum : 0.f;
    }
}

// One pooled row per 16-lane group, four rows per wave: the group (lane >> 4) pools row i of ids / counts / wts / nvalid into orow
// (nothing is read or written when !rok).  All 64 lanes of the wave must call it together (DPP across the group, the entry loop
// bound is the wave's largest k).  See importance_pool4_kernel for the layout.
template <int PAGES>
__device__ __forceinline__ void pool4_row(const float *__restrict__ x, int H, const int32_t *__restrict__ ids,
                                          const int32_t *__restrict__ counts, const float *__restrict__ wts,
                                          const int32_t *__restrict__ nvalid, int64_t i, bool rok, int T, int64_t max_idx, int renorm,
                                          float *__restrict__ orow) {
    constexpr int TU = 4;                                     // entries gathered per batch
    const int lane = threadIdx.x & 63, l = lane & 15;
    int k;
    int32_t id[PAGES];
    float w[PAGES];
    pool4_weights<PAGES>(ids, counts, wts, nvalid, i, rok, T, max_idx, renorm, id, w, k);
    // entries to walk: the largest k of the four rows (wave-uniform)
    int kmax = __builtin_amdgcn_readlane(k, 0);
    { const int k1 = __builtin_amdgcn_readlane(k, 16), k2 = __builtin_amdgcn_readlane(k, 32), k3 = __builtin_amdgcn_readlane(k, 48);
      kmax = kmax > k1 ? kmax : k1; kmax = kmax > k2 ? kmax : k2; kmax = kmax > k3 ? kmax : k3; }
    // ---- gather + reduce: 256 columns (four sweeps) at a time ----
    for (int cb = 0; cb < H; cb += 256) {
        float4 acc[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
#define PS_POOL_ENTRY(P, TT, U)                                                                            \
        {                                                                                                  \
            nid[U] = row_bcast_i32<0x150 + (TT)>(id[P]);                                                   \
            nw[U] = __builtin_bit_cast(float, row_bcast_i32<0x150 + (TT)>(__builtin_bit_cast(int, w[P]))); \
            _Pragma("unroll") for (int s = 0; s < 4; ++s) {                                                \
                const int col = cb + s * 64 + l * 4;                                                       \
                r[U][s] = make_float4(0.f, 0.f, 0.f, 0.f);                                                 \
                if (nid[U] >= 0 && col < H) r[U][s] = *reinterpret_cast<const float4 *>(x + (int64_t)nid[U] * H + col); \
            }                                                                                              \
        }
#define PS_POOL_BATCH(P, T0)                                                                               \
        if ((P) * 16 + (T0) < kmax) {                                                                      \
            int32_t nid[TU];                                                                               \
            float nw[TU];                                                                                  \
            float4 r[TU][4];                                                                               \
            PS_POOL_ENTRY(P, (T0) + 0, 0) PS_POOL_ENTRY(P, (T0) + 1, 1) PS_POOL_ENTRY(P, (T0) + 2, 2) PS_POOL_ENTRY(P, (T0) + 3, 3) \
            _Pragma("unroll") for (int u = 0; u < TU; ++u)                                                 \
                _Pragma("unroll") for (int s = 0; s < 4; ++s) {                                            \
                    acc[s].x = fmaf(r[u][s].x, nw[u], acc[s].x); acc[s].y = fmaf(r[u][s].y, nw[u], acc[s].y); \
                    acc[s].z = fmaf(r[u][s].z, nw[u], acc[s].z); acc[s].w = fmaf(r[u][s].w, nw[u], acc[s].w); \
                }                                                                                          \
        }
#define PS_POOL_PAGE(P) PS_POOL_BATCH(P, 0) PS_POOL_BATCH(P, 4) PS_POOL_BATCH(P, 8) PS_POOL_BATCH(P, 12)
        PS_POOL_PAGE(0)
        if constexpr (PAGES > 1) { PS_POOL_PAGE(1) }
        if constexpr (PAGES > 2) { PS_POOL_PAGE(2) }
        if constexpr (PAGES > 3) { PS_POOL_PAGE(3) }
#undef PS_POOL_PAGE
#undef PS_POOL_BATCH
#undef PS_POOL_ENTRY
        if (rok) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int col = cb + s * 64 + l * 4;
                if (col < H) *reinterpret_cast<float4 *>(orow + col) = acc[s];
            }
        }
    }
}

}  // namespace
