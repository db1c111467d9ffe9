// importance_pool.hip -- weighted sparse neighbour gather on gfx950 (HBM/L2-bound row gather).
//
// Replaces ImportancePooling.forward (reference model/pinsage.py:101-150) and the gather +
// weighted-reduce part of WeightedAggregator / MeanAggregator / ImportanceAggregator
// (model/aggregators.py:13-91, 233-287).  Two kernels: importance_pool4_kernel (T <= 64, 16-byte aligned rows: four output
// rows per wave, below) and importance_pool_kernel (any shape: one wave per output row; every neighbour row one coalesced
// 16 B-per-lane sweep, up to UNROLL rows in flight); accumulation in fp32 in neighbour order in both.
#include "ps_common.h"
#include "pool_row.h"
#include "row_sweep.h"

namespace {

constexpr int UNROLL = 8;

template <int VEC>   // floats per lane per chunk (4 -> float4 path, 1 -> scalar path)
__global__ __launch_bounds__(256) void importance_pool_kernel(const float *__restrict__ x, int H,
                                                              const int32_t *__restrict__ ids,
                                                              const int32_t *__restrict__ counts,
                                                              const float *__restrict__ wts,
                                                              const int32_t *__restrict__ nvalid, int64_t B, int T,
                                                              int64_t max_idx, int renorm,
                                                              float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int nwaves = (int)((gridDim.x * blockDim.x) >> 6);
    const int chunk = 64 * VEC;
    for (int64_t i = wave; i < B; i += nwaves) {
        // the row's metadata is requested at once (T <= 64: one id / count / weight per lane, kept in registers), so the
        // chain before the row gathers is one global round trip, not one per quantity
        const bool small = T <= 64;
        int32_t id0 = -1, cnt0 = 0;
        float wt0 = 0.f;
        if (small && lane < T) {
            id0 = ids[i * T + lane];
            if (counts) cnt0 = counts[i * T + lane];
            if (wts) wt0 = wts[i * T + lane];
        }
        int k = __builtin_amdgcn_readfirstlane(nvalid[i]);
        k = k < T ? k : T;                                // nvalid[i] above T means T (as pool4_row): nothing is read beyond row i
        // ---- weights: total of the kept counts (reference: weights = count / sum(top counts)) ----
        int tot = 0;
        if (small) {
            tot = lane < k ? cnt0 : 0;
        } else {
            for (int j0 = 0; j0 < k; j0 += 64) {
                const int j = j0 + lane;
                tot += (counts && j < k) ? counts[i * T + j] : 0;
            }
        }
        tot = ps_wave_sum_i32(tot);
        float wsum = 0.f;
        if (small) {
            if (lane < k && id0 >= 0 && (int64_t)id0 <= max_idx) wsum = wts ? wt0 : (float)((double)cnt0 / (double)tot);
        } else {
            for (int j0 = 0; j0 < k; j0 += 64) {
                const int j = j0 + lane;
                float wj = 0.f;
                if (j < k) {
                    const int32_t id = ids[i * T + j];
                    if (id >= 0 && (int64_t)id <= max_idx)
                        wj = wts ? wts[i * T + j] : (float)((double)counts[i * T + j] / (double)tot);
                }
                wsum += wj;
            }
        }
        wsum = ps_wave_sum_f32(wsum);
        const bool do_norm = renorm && wsum > 0.f;        // w /= w.sum() only if sum > 0 (pinsage.py:141-143)
        // ---- gather + reduce ----
        for (int c0 = 0; c0 < H; c0 += chunk) {
            const int col = c0 + lane * VEC;
            const bool cact = col < H;
            float acc[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
            for (int j0 = 0; j0 < k; j0 += 64) {
                const int jj = j0 + lane;
                int32_t myid = -1;
                float myw = 0.f;
                if (jj < k) {
                    myid = small ? id0 : ids[i * T + jj];
                    if (myid >= 0 && (int64_t)myid <= max_idx) {
                        if (small) myw = wts ? wt0 : (float)((double)cnt0 / (double)tot);
                        else myw = wts ? wts[i * T + jj] : (float)((double)counts[i * T + jj] / (double)tot);
                        if (do_norm) myw = myw / wsum;
                    } else {
                        myid = -1;
                    }
                }
                const int kk = (k - j0) < 64 ? (k - j0) : 64;
                for (int t0 = 0; t0 < kk; t0 += UNROLL) {
                    float r[UNROLL][VEC];
                    float wv[UNROLL];
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) {
                        const int t = t0 + u;
                        const int32_t id = (t < kk) ? __builtin_amdgcn_readlane(myid, t < 64 ? t : 0) : -1;
                        wv[u] = (t < kk) ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, myw), t < 64 ? t : 0)) : 0.f;
                        const bool ok = id >= 0 && cact;
                        load_vec<VEC>(x + (int64_t)id * H + col, ok, r[u]);
                    }
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u)
#pragma unroll
                        for (int v = 0; v < VEC; ++v) acc[v] = fmaf(r[u][v], wv[u], acc[v]);
                }
            }
            if (cact) store_vec<VEC>(out + i * H + col, acc);
        }
    }
}

// ---- four output rows per wave (r04) ------------------------------------------------------------------------------------
// On the catalogue graphs most of a start item's top-T neighbours are USERS, which the reference drops when x holds item rows only
// (model/pinsage.py:123-129): SYN-25M at T = 10 keeps 0.85 neighbours per row on average, so the one-wave-per-row kernel above spent a
// whole wave and two dependent round trips on copying <= 1 row.  Here a 16-lane group owns an output row (16 lanes x 16 B = 256 B per
// sweep, four sweeps per 1 KiB row), a wave four rows: their ids / counts come in ONE round trip (entry e of a row in lane e & 15 of
// its group, T <= 16 * PAGES), the per-row sums are DPP reductions over the group's 16 lanes (quad_perm, row_half_mirror,
// row_mirror -- for T <= 16 the same butterfly as ps_wave_sum over a wave whose other lanes hold zeros: identical bits), an entry is
// broadcast to its group by DPP row_newbcast, and the gathers of four entries x four sweeps x four rows are in flight together
// (16 KiB per wave; masked lanes request nothing, so dropped neighbours cost an instruction slot, not traffic).  Rows that keep no
// neighbour are stored as zeros without touching x.  Same operation order per output element as the kernel above (fp32 fma in
// neighbour order).
// The per-row math is pool4_row (csrc/pool_row.h), which the fused layer GEMM (ps_gcn_layer) calls too.
template <int PAGES>
__global__ __launch_bounds__(256) void importance_pool4_kernel(const float *__restrict__ x, int H, const int32_t *__restrict__ ids,
                                                               const int32_t *__restrict__ counts, const float *__restrict__ wts,
                                                               const int32_t *__restrict__ nvalid, int64_t B, int T, int64_t max_idx,
                                                               int renorm, float *__restrict__ out) {
    const int lane = threadIdx.x & 63, g = lane >> 4;
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t i0 = wave0 * 4; i0 < B; i0 += nwaves * 4) {
        const int64_t i = i0 + g;
        pool4_row<PAGES>(x, H, ids, counts, wts, nvalid, i, i < B, T, max_idx, renorm, out + i * H);    // csrc/pool_row.h
    }
}

}  // namespace

extern "C" int ps_importance_pool(const float *x, int64_t N, int H, const int32_t *ids, const int32_t *counts,
                                  const float *wts, const int32_t *nvalid, int64_t B, int T, int64_t max_idx,
                                  int renorm, float *out, ps_stream_t stream) {
    if (B < 0 || H <= 0 || T <= 0 || N < 0) return PS_EINVAL;
    if (B == 0) return PS_OK;
    if (!x || !ids || !nvalid || !out || (!counts && !wts)) return PS_EINVAL;
    if (max_idx > N - 1) max_idx = N - 1;
    hipStream_t st = ps_stream(stream);
    const bool vec4 = (H % 4 == 0) && ps_aligned16({x, out});
    const char *pe = getenv("PS_POOL_ROWS_PER_WAVE");         // 1: the one-row-per-wave kernel (experiments / cross-check)
    const bool four = vec4 && T <= 64 && !(pe && atoi(pe) == 1);
    if (four) {
        const dim3 grid4(ps_row4_grid(B));
        if (T <= 16)
            hipLaunchKernelGGL(importance_pool4_kernel<1>, grid4, dim3(256), 0, st, x, H, ids, counts, wts, nvalid, B, T, max_idx, renorm,
                               out);
        else
            hipLaunchKernelGGL(importance_pool4_kernel<4>, grid4, dim3(256), 0, st, x, H, ids, counts, wts, nvalid, B, T, max_idx, renorm,
                               out);
    } else {
        PS_LAUNCH_VEC(importance_pool_kernel<VEC>, vec4, dim3(ps_row_grid(B)), dim3(256), st, x, H, ids, counts, wts, nvalid, B, T,
                      max_idx, renorm, out);
    }
    PS_CHECK_LAUNCH();
    return PS_OK;
}
