// neigh_agg.hip -- the neighbour gathers of AttentionAggregator and MaxPoolingAggregator on gfx950 (L2/HBM-bound row gathers).
//
// Replaces the per-node loops of the reference's model/aggregators.py:131-158 (attention scores + softmax) and :195-209 (max over
// the neighbours' transformed rows).  The sweep of importance_pool_kernel (csrc/importance_pool.hip), from row_sweep.h: one wave per
// output row, a neighbour row is one coalesced 16 B-per-lane sweep (scalar sweep for H % 4 != 0 or unaligned pointers), up to UNROLL neighbour
// rows in flight, grid-stride over the rows, no atomics, no LDS.  A slot is kept iff j < min(nvalid[i], T) and 0 <= ids[i,j] < N.
#include "ps_common.h"
#include "row_sweep.h"

namespace {

constexpr int UNROLL = 8;

// ---- attention weights ------------------------------------------------------------------------------------------------------
// attn[i, j] = softmax_j( sum_c w2[c] * relu(u[i, c] + v[ids[i, j], c]) ) over the kept slots of row i, +0.0 elsewhere.
// Slot j0 + l of a 64-slot block belongs to lane l: that lane holds the slot's id, and after the block's gathers its score.
// Per slot: every lane runs acc = fmaf(w2[c], relu(u[c] + v[c]), acc) over its columns (ascending), then the wave sums the lanes
// (ps_wave_sum_f32).  T <= 64: the scores stay in registers.  T > 64: they are parked in attn[i, :] (each lane reads back only
// what it wrote itself) for the two further passes of the softmax (sum of exponentials, division).
template <int VEC>
__global__ __launch_bounds__(256) void attention_weights_kernel(const float *__restrict__ u, const float *__restrict__ v, int64_t N,
                                                                int Hd, const float *__restrict__ w2,
                                                                const int32_t *__restrict__ ids,
                                                                const int32_t *__restrict__ nvalid, int64_t B, int T,
                                                                float *__restrict__ attn) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int nwaves = (int)((gridDim.x * blockDim.x) >> 6);
    const int chunk = 64 * VEC;
    const float ninf = __int_as_float((int)0xff800000u);
    const bool small = T <= 64;
    // the first sweep's share of w2 is the same for every row
    float w0[VEC];
    load_vec<VEC>(w2 + lane * VEC, lane * VEC < Hd, w0);
    for (int64_t i = wave; i < B; i += nwaves) {
        int k = __builtin_amdgcn_readfirstlane(nvalid[i]);
        k = k < T ? k : T;
        float u0[VEC];
        load_vec<VEC>(u + i * Hd + lane * VEC, lane * VEC < Hd, u0);
        float m = ninf, s0 = ninf;
        for (int j0 = 0; j0 < k; j0 += 64) {
            const int32_t myid = kept_id(ids, i, T, j0 + lane, k, N);
            const int kk = (k - j0) < 64 ? (k - j0) : 64;
            float mys = ninf;
            for (int t0 = 0; t0 < kk; t0 += UNROLL) {
                int32_t id[UNROLL];
                float part[UNROLL];
#pragma unroll
                for (int q = 0; q < UNROLL; ++q) {
                    const int t = t0 + q;
                    id[q] = (t < kk) ? __builtin_amdgcn_readlane(myid, t < 64 ? t : 0) : -1;
                    part[q] = 0.f;
                }
                for (int c0 = 0; c0 < Hd; c0 += chunk) {
                    const int col = c0 + lane * VEC;
                    const bool cact = col < Hd;
                    float r[UNROLL][VEC];
#pragma unroll
                    for (int q = 0; q < UNROLL; ++q) load_vec<VEC>(v + (int64_t)id[q] * Hd + col, id[q] >= 0 && cact, r[q]);
                    float uu[VEC], ww[VEC];
                    if (c0 == 0) {
#pragma unroll
                        for (int e = 0; e < VEC; ++e) { uu[e] = u0[e]; ww[e] = w0[e]; }
                    } else {
                        load_vec<VEC>(u + i * Hd + col, cact, uu);
                        load_vec<VEC>(w2 + col, cact, ww);
                    }
#pragma unroll
                    for (int q = 0; q < UNROLL; ++q)
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            const float h = uu[e] + r[q][e];
                            part[q] = fmaf(ww[e], h < 0.f ? 0.f : h, part[q]);      // relu that keeps a NaN, as torch's does
                        }
                }
#pragma unroll
                for (int q = 0; q < UNROLL; ++q) {
                    if (t0 + q < kk) {                                                // wave-uniform
                        const float s = ps_wave_sum_f32(part[q]);
                        if (lane == t0 + q) mys = s;
                    }
                }
            }
            if (myid < 0) mys = ninf;
            m = fmaxf(m, mys);
            if (small) s0 = mys;
            else if (j0 + lane < k) attn[i * T + j0 + lane] = mys;
        }
        m = ps_wave_max_f32(m);
        // softmax over the kept slots: exp(s - max) / sum; a row that keeps nothing has sum 0 and is written as zeros
        if (small) {
            const bool kept = lane < k && kept_id(ids, i, T, lane, k, N) >= 0;
            const float e = kept ? expf(s0 - m) : 0.f;
            const float sum = ps_wave_sum_f32(e);
            if (lane < T) attn[i * T + lane] = kept ? e / sum : 0.f;
        } else {
            float sum = 0.f;
            for (int j0 = 0; j0 < k; j0 += 64) {
                const int jj = j0 + lane;
                const bool kept = kept_id(ids, i, T, jj, k, N) >= 0;
                sum += kept ? expf(attn[i * T + jj] - m) : 0.f;
            }
            sum = ps_wave_sum_f32(sum);
            for (int j0 = 0; j0 < T; j0 += 64) {
                const int jj = j0 + lane;
                const bool kept = kept_id(ids, i, T, jj, k, N) >= 0;
                if (jj < T) attn[i * T + jj] = kept ? expf(attn[i * T + jj] - m) / sum : 0.f;
            }
        }
    }
}

// ---- gather + max -----------------------------------------------------------------------------------------------------------
// out[i, c] = max over the kept slots of x[ids[i, j], c]; +0.0 in every column when the row keeps nothing.  The running maximum
// starts from -inf (never from 0: all-negative rows keep their sign) and a NaN, once met, stays -- torch.max's result.
template <int VEC>
__global__ __launch_bounds__(256) void gather_max_kernel(const float *__restrict__ x, int64_t N, int H,
                                                         const int32_t *__restrict__ ids, const int32_t *__restrict__ nvalid,
                                                         int64_t B, int T, float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int nwaves = (int)((gridDim.x * blockDim.x) >> 6);
    const int chunk = 64 * VEC;
    const float ninf = __int_as_float((int)0xff800000u);
    const bool small = T <= 64;
    for (int64_t i = wave; i < B; i += nwaves) {
        int k = __builtin_amdgcn_readfirstlane(nvalid[i]);
        k = k < T ? k : T;
        const int32_t id0 = small ? kept_id(ids, i, T, lane, k, N) : -1;
        // does the row keep anything?
        bool any = false;
        if (small) {
            any = __builtin_amdgcn_ballot_w64(id0 >= 0) != 0;
        } else {
            for (int j0 = 0; j0 < k && !any; j0 += 64) any = __builtin_amdgcn_ballot_w64(kept_id(ids, i, T, j0 + lane, k, N) >= 0) != 0;
        }
        for (int c0 = 0; c0 < H; c0 += chunk) {
            const int col = c0 + lane * VEC;
            const bool cact = col < H;
            float acc[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] = any ? ninf : 0.f;
            for (int j0 = 0; j0 < k && any; j0 += 64) {
                const int32_t myid = small ? id0 : kept_id(ids, i, T, j0 + lane, k, N);
                const int kk = (k - j0) < 64 ? (k - j0) : 64;
                for (int t0 = 0; t0 < kk; t0 += UNROLL) {
                    float r[UNROLL][VEC];
                    bool ok[UNROLL];
#pragma unroll
                    for (int q = 0; q < UNROLL; ++q) {
                        const int t = t0 + q;
                        const int32_t id = (t < kk) ? __builtin_amdgcn_readlane(myid, t < 64 ? t : 0) : -1;
                        ok[q] = id >= 0;
                        load_vec<VEC>(x + (int64_t)id * H + col, ok[q] && cact, r[q]);
                    }
#pragma unroll
                    for (int q = 0; q < UNROLL; ++q)
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            const float a = ok[q] ? r[q][e] : ninf;
                            acc[e] = (a > acc[e] || a != a) ? a : acc[e];
                        }
                }
            }
            if (cact) store_vec<VEC>(out + i * H + col, acc);
        }
    }
}

}  // namespace

extern "C" int ps_attention_weights(const float *u, const float *v, int64_t N, int Hd, const float *w2, const int32_t *ids,
                                    const int32_t *nvalid, int64_t B, int T, float *attn, ps_stream_t stream) {
    if (B < 0 || Hd <= 0 || T <= 0 || N < 0) return PS_EINVAL;
    if (B == 0) return PS_OK;                                 // before the pointers: an empty tensor's base is NULL
    if (!u || !v || !w2 || !ids || !nvalid || !attn) return PS_EINVAL;
    hipStream_t st = ps_stream(stream);
    const bool vec4 = (Hd % 4 == 0) && ps_aligned16({u, v, w2});
    PS_LAUNCH_VEC(attention_weights_kernel<VEC>, vec4, dim3(ps_row_grid(B)), dim3(256), st, u, v, N, Hd, w2, ids, nvalid, B, T, attn);
    PS_CHECK_LAUNCH();
    return PS_OK;
}

extern "C" int ps_gather_max(const float *x, int64_t N, int H, const int32_t *ids, const int32_t *nvalid, int64_t B, int T,
                             float *out, ps_stream_t stream) {
    if (B < 0 || H <= 0 || T <= 0 || N < 0) return PS_EINVAL;
    if (B == 0) return PS_OK;                                 // before the pointers: an empty tensor's base is NULL
    if (!x || !ids || !nvalid || !out) return PS_EINVAL;
    hipStream_t st = ps_stream(stream);
    const bool vec4 = (H % 4 == 0) && ps_aligned16({x, out});
    PS_LAUNCH_VEC(gather_max_kernel<VEC>, vec4, dim3(ps_row_grid(B)), dim3(256), st, x, N, H, ids, nvalid, B, T, out);
    PS_CHECK_LAUNCH();
    return PS_OK;
}
