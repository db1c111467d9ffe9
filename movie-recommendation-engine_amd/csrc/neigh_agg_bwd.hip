// neigh_agg_bwd.hip -- the backward of the neighbour gathers (csrc/importance_pool.hip, csrc/neigh_agg.hip) on gfx950.
//
// The backward of a gather is a scatter; here it is a second gather over the TRANSPOSED index, so that no float is ever added
// atomically and every output bit is a function of the inputs.  A slot is s = i * T + j; the slot lists of a padded batch are
// rptr int64[N + 1] / slots int32[nnz]: S(r) = slots[rptr[r] .. rptr[r + 1]) holds the kept slots whose id is r, ascending.  One wave
// owns a destination row (or one SEG-slot segment of a hub row) and sweeps the source rows its slots name exactly as the forward
// kernels sweep theirs: 16 bytes per lane (a scalar sweep for H % 4 != 0 or unaligned pointers), UNROLL rows in flight, no LDS.
// include/pinsage_hip.h states the arithmetic; tests/helpers/agg_bwd_cases.py restates it bit for bit.
#include "ps_common.h"
#include "pool_row.h"
#include "row_sweep.h"

namespace {

constexpr int UNROLL = 8;
constexpr int SEG = 128;                       // slots per segment of S(r): ps_gather_bwd_segment()
constexpr int DW_ROWS = 128;                   // target rows per partition of the dw2 sum

// ---- the weights ps_importance_pool applies ----------------------------------------------------------------------------------
// 16-lane layout (T <= 64): pool4_weights, the code of the forward itself
template <int PAGES>
__global__ __launch_bounds__(256) void pool_weights4_kernel(const int32_t *__restrict__ ids, const int32_t *__restrict__ counts,
                                                            const float *__restrict__ wts, const int32_t *__restrict__ nvalid,
                                                            int64_t B, int T, int64_t max_idx, int renorm, float *__restrict__ w_eff) {
    const int lane = threadIdx.x & 63, g = lane >> 4, l = lane & 15;
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t i0 = wave0 * 4; i0 < B; i0 += nwaves * 4) {
        const int64_t i = i0 + g;
        int k;
        int32_t id[PAGES];
        float w[PAGES];
        pool4_weights<PAGES>(ids, counts, wts, nvalid, i, i < B, T, max_idx, renorm, id, w, k);
#pragma unroll
        for (int p = 0; p < PAGES; ++p)
            if (i < B && p * 16 + l < T) w_eff[i * T + p * 16 + l] = id[p] >= 0 ? w[p] : 0.f;
    }
}

// wave layout (entry e in lane e % 64): the weight arithmetic of importance_pool_kernel
__global__ __launch_bounds__(256) void pool_weights_kernel(const int32_t *__restrict__ ids, const int32_t *__restrict__ counts,
                                                           const float *__restrict__ wts, const int32_t *__restrict__ nvalid,
                                                           int64_t B, int T, int64_t max_idx, int renorm, float *__restrict__ w_eff) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int nwaves = (int)((gridDim.x * blockDim.x) >> 6);
    for (int64_t i = wave; i < B; i += nwaves) {
        int k = __builtin_amdgcn_readfirstlane(nvalid[i]);
        k = k < T ? k : T;
        int tot = 0;
        for (int j0 = 0; j0 < k; j0 += 64) {
            const int j = j0 + lane;
            tot += (counts && j < k) ? counts[i * T + j] : 0;
        }
        tot = ps_wave_sum_i32(tot);
        float wsum = 0.f;
        for (int j0 = 0; j0 < k; j0 += 64) {
            const int j = j0 + lane;
            float wj = 0.f;
            if (j < k) {
                const int32_t id = ids[i * T + j];
                if (id >= 0 && (int64_t)id <= max_idx) wj = wts ? wts[i * T + j] : (float)((double)counts[i * T + j] / (double)tot);
            }
            wsum += wj;
        }
        wsum = ps_wave_sum_f32(wsum);
        const bool do_norm = renorm && wsum > 0.f;
        for (int j0 = 0; j0 < T; j0 += 64) {
            const int j = j0 + lane;
            if (j >= T) continue;
            float wj = 0.f;
            if (j < k) {
                const int32_t id = ids[i * T + j];
                if (id >= 0 && (int64_t)id <= max_idx) {
                    wj = wts ? wts[i * T + j] : (float)((double)counts[i * T + j] / (double)tot);
                    if (do_norm) wj = wj / wsum;
                }
            }
            w_eff[i * T + j] = wj;
        }
    }
}

// ---- the transposed gathers ----------------------------------------------------------------------------------------------------
// MODE 0  gx[r, c] = chain fmaf(coef[s], g[s / T, c], acc)                                      (pool, attention sum)
// MODE 1  gx[r, c] = chain acc + g[i, c] over the slots with arg[i, c] == j                     (max)
// MODE 2  gx[r, c] = chain fmaf(coef[s], (g[i, c] + v[r, c] > 0 ? w2[c] : 0), acc)              (attention scores; g = u, coef = ds)
struct TArgs {
    const int64_t *rptr;
    const int32_t *slots;
    int64_t N;
    int T;
    const float *coef;
    const int32_t *arg;
    const float *g;
    int64_t B;
    int H;
    const float *v;
    const float *w2;
    float *gx;
    float *part;                               // [2 * nblk, H]: the segment chains of the rows with more than SEG slots
    int64_t nblk;
};

// the bounds of S(r), clamped to what a well-formed transposition can hold
__device__ __forceinline__ void row_bounds(const TArgs &a, int64_t r, int64_t &lo, int64_t &hi) {
    const int64_t cap = a.B * a.T;
    lo = a.rptr[r];
    hi = a.rptr[r + 1];
    lo = lo < 0 ? 0 : (lo > cap ? cap : lo);
    hi = hi < lo ? lo : (hi > cap ? cap : hi);
}

// The partial of the segment that starts at position p: entry 2 * (p / SEG) for a row's first segment, 2 * (p / SEG) + 1 for a
// later one.  Rows that are cut have more than SEG slots, so a SEG-aligned block of positions holds at most one start of each kind.
__device__ __forceinline__ int64_t part_index(int64_t p, bool first) { return 2 * (p / SEG) + (first ? 0 : 1); }

// acc += the chain over slots[p0, p1) for the columns col .. col + VEC - 1 of destination row r
template <int VEC, int MODE>
__device__ __forceinline__ void slot_chain(const TArgs &a, int64_t r, int64_t p0, int64_t p1, int col, bool cact, float (&acc)[VEC]) {
    const int lane = threadIdx.x & 63;
    const int64_t BT = a.B * a.T;
    float vv[VEC], ww[VEC];
    if (MODE == 2) {
        load_vec<VEC>(a.v + r * a.H + col, cact, vv);
        load_vec<VEC>(a.w2 + col, cact, ww);
    }
    for (int64_t q0 = p0; q0 < p1; q0 += 64) {
        const int kk = (p1 - q0) < 64 ? (int)(p1 - q0) : 64;
        int32_t myi = -1, myj = 0;
        float myc = 0.f;
        if (lane < kk) {
            const int32_t s = a.slots[q0 + lane];
            if (s >= 0 && (int64_t)s < BT) {                   // a slot outside the batch names nothing
                myi = s / a.T;
                myj = s - myi * a.T;
                if (MODE != 1) myc = a.coef[s];
            }
        }
        for (int t0 = 0; t0 < kk; t0 += UNROLL) {
            int32_t ii[UNROLL], jj[UNROLL];
            float cf[UNROLL];
            float rr[UNROLL][VEC];
            int32_t ar[UNROLL][VEC];
#pragma unroll
            for (int q = 0; q < UNROLL; ++q) {
                const int t = t0 + q;
                ii[q] = (t < kk) ? __builtin_amdgcn_readlane(myi, t < 64 ? t : 0) : -1;
                jj[q] = __builtin_amdgcn_readlane(myj, t < 64 ? t : 0);
                cf[q] = lane_f32(myc, t < 64 ? t : 0);
                load_vec<VEC>(a.g + (int64_t)ii[q] * a.H + col, ii[q] >= 0 && cact, rr[q]);
                if (MODE == 1) load_veci<VEC>(a.arg + (int64_t)ii[q] * a.H + col, ii[q] >= 0 && cact, ar[q]);
            }
#pragma unroll
            for (int q = 0; q < UNROLL; ++q) {
                if (ii[q] < 0) continue;                       // wave-uniform
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    if (MODE == 0) {
                        acc[e] = fmaf(cf[q], rr[q][e], acc[e]);
                    } else if (MODE == 1) {
                        acc[e] = (ar[q][e] == jj[q]) ? acc[e] + rr[q][e] : acc[e];
                    } else {
                        const float h = rr[q][e] + vv[e];
                        acc[e] = fmaf(cf[q], h > 0.f ? ww[e] : 0.f, acc[e]);
                    }
                }
            }
        }
    }
}

// Items 0 .. N - 1: destination row r with at most SEG slots, written to gx.  Items N + 2 m + t: the segment of a longer row that
// starts in positions [m SEG, (m + 1) SEG) -- t = 0 the row's first segment, t = 1 a later one --, written to part[2 m + t].
template <int VEC, int MODE>
__global__ __launch_bounds__(256) void transposed_kernel(TArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int64_t nwaves = (int64_t)((gridDim.x * blockDim.x) >> 6);
    const int chunk = 64 * VEC;
    const int64_t items = a.N + 2 * a.nblk;
    for (int64_t it = wave; it < items; it += nwaves) {
        int64_t r, p0, p1;
        float *dst;
        if (it < a.N) {
            r = it;
            row_bounds(a, r, p0, p1);
            if (p1 - p0 > SEG) continue;
            dst = a.gx + r * a.H;
        } else {
            const int64_t m = (it - a.N) >> 1;
            const bool first = ((it - a.N) & 1) == 0;
            // a cut row has more than SEG slots: the one that starts in block m reaches position (m + 1) SEG - 1, the one that
            // continues into block m holds position m SEG
            const int64_t probe = first ? (m + 1) * SEG - 1 : m * SEG;
            int64_t lo = 0, hi = a.N;                          // the last r in [0, N) with rptr[r] <= probe
            while (hi - lo > 1) {
                const int64_t mid = (lo + hi) >> 1;
                if (a.rptr[mid] <= probe) lo = mid; else hi = mid;
            }
            r = lo;
            int64_t b0, b1;
            row_bounds(a, r, b0, b1);
            if (b1 - b0 <= SEG || probe >= b1 || probe < b0) continue;
            if (first) {
                if (b0 < m * SEG) continue;
                p0 = b0;
            } else {
                if (b0 >= m * SEG) continue;
                p0 = b0 + (m * SEG - b0 + SEG - 1) / SEG * SEG;
                if (p0 >= b1) continue;
            }
            p1 = p0 + SEG < b1 ? p0 + SEG : b1;
            dst = a.part + (it - a.N) * a.H;
        }
        for (int c0 = 0; c0 < a.H; c0 += chunk) {
            const int col = c0 + lane * VEC;
            const bool cact = col < a.H;
            float acc[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
            slot_chain<VEC, MODE>(a, r, p0, p1, col, cact, acc);
            if (cact) store_vec<VEC>(dst + col, acc);
        }
    }
}

// the rows with more than SEG slots: their segment partials, first to last
template <int VEC>
__global__ __launch_bounds__(256) void combine_kernel(TArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int64_t nwaves = (int64_t)((gridDim.x * blockDim.x) >> 6);
    const int chunk = 64 * VEC;
    for (int64_t r = wave; r < a.N; r += nwaves) {
        int64_t b0, b1;
        row_bounds(a, r, b0, b1);
        if (b1 - b0 <= SEG) continue;
        const int64_t nseg = (b1 - b0 + SEG - 1) / SEG;
        for (int c0 = 0; c0 < a.H; c0 += chunk) {
            const int col = c0 + lane * VEC;
            const bool cact = col < a.H;
            float acc[VEC];
            load_vec<VEC>(a.part + part_index(b0, true) * a.H + col, cact, acc);
            for (int64_t q0 = 1; q0 < nseg; q0 += UNROLL) {
                float rr[UNROLL][VEC];
#pragma unroll
                for (int q = 0; q < UNROLL; ++q)
                    load_vec<VEC>(a.part + part_index(b0 + (q0 + q) * SEG, false) * a.H + col, q0 + q < nseg && cact, rr[q]);
#pragma unroll
                for (int q = 0; q < UNROLL; ++q) {
                    if (q0 + q >= nseg) continue;
#pragma unroll
                    for (int e = 0; e < VEC; ++e) acc[e] = acc[e] + rr[q][e];
                }
            }
            if (cact) store_vec<VEC>(a.gx + r * a.H + col, acc);
        }
    }
}

inline int64_t seg_blocks(int64_t B, int T) { return B * T / SEG + 1; }
inline size_t transposed_bytes(int64_t B, int T, int H) { return 256 + ps_align256((size_t)(2 * seg_blocks(B, T)) * H * sizeof(float)); }

template <int MODE>
int launch_transposed(TArgs a, bool vec4, hipStream_t st) {
    PS_LAUNCH_VEC((transposed_kernel<VEC, MODE>), vec4, dim3(ps_row_grid(a.N + 2 * a.nblk)), dim3(256), st, a);
    PS_CHECK_LAUNCH();
    PS_LAUNCH_VEC(combine_kernel<VEC>, vec4, dim3(ps_row_grid(a.N)), dim3(256), st, a);
    PS_CHECK_LAUNCH();
    return PS_OK;
}

// ---- gather + max with its arg-max ---------------------------------------------------------------------------------------------
// gather_max_kernel (csrc/neigh_agg.hip) with the slot that supplied the result: the first kept slot, then every slot that
// raises the maximum, then the first NaN (a later NaN replaces the value's bits, as in the forward, but not the slot).
template <int VEC>
__global__ __launch_bounds__(256) void gather_max_arg_kernel(const float *__restrict__ x, int64_t N, int H,
                                                             const int32_t *__restrict__ ids, const int32_t *__restrict__ nvalid,
                                                             int64_t B, int T, float *__restrict__ out, int32_t *__restrict__ arg) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int nwaves = (int)((gridDim.x * blockDim.x) >> 6);
    const int chunk = 64 * VEC;
    const float ninf = __int_as_float((int)0xff800000u);
    for (int64_t i = wave; i < B; i += nwaves) {
        int k = __builtin_amdgcn_readfirstlane(nvalid[i]);
        k = k < T ? k : T;
        bool any = false;
        for (int j0 = 0; j0 < k && !any; j0 += 64) any = __builtin_amdgcn_ballot_w64(kept_id(ids, i, T, j0 + lane, k, N) >= 0) != 0;
        for (int c0 = 0; c0 < H; c0 += chunk) {
            const int col = c0 + lane * VEC;
            const bool cact = col < H;
            float acc[VEC];
            int32_t aj[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) { acc[e] = any ? ninf : 0.f; aj[e] = -1; }
            for (int j0 = 0; j0 < k && any; j0 += 64) {
                const int32_t myid = kept_id(ids, i, T, j0 + lane, k, N);
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
                    for (int q = 0; q < UNROLL; ++q) {
                        if (!ok[q]) continue;                  // wave-uniform
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            const float v = r[q][e];
                            // one select per element (no short-circuit: the branchy form lost its NaN arm in the compiler)
                            const bool take = (aj[e] < 0) | (v > acc[e]) | ((v != v) & (acc[e] == acc[e]));
                            aj[e] = take ? j0 + t0 + q : aj[e];
                            acc[e] = (v > acc[e] || v != v) ? v : acc[e];
                        }
                    }
                }
            }
            if (cact) {
                store_vec<VEC>(out + i * H + col, acc);
                store_veci<VEC>(arg + i * H + col, aj);
            }
        }
    }
}

// ---- attention, the per-target-row half ----------------------------------------------------------------------------------------
// One wave per target row i.  Pass 1: da_ij per kept slot (lane j - j0 of a 64-slot block holds it, as the forward holds its
// score) and dot_i; pass 2: ds; pass 3: du and the row's share of dw2, a sweep over the same rows of v the forward read.
// T > 64: da is parked in ds[i, :] between the passes (each lane reads back only what it wrote itself).
template <int VEC>
__global__ __launch_bounds__(256) void attention_bwd_rows_kernel(const float *__restrict__ x, int64_t N, int H,
                                                                 const float *__restrict__ u, const float *__restrict__ v, int Hd,
                                                                 const float *__restrict__ w2, const int32_t *__restrict__ ids,
                                                                 const int32_t *__restrict__ nvalid, const float *__restrict__ attn,
                                                                 const float *__restrict__ g, int64_t B, int T, float *ds,
                                                                 float *__restrict__ du, float *__restrict__ share) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int nwaves = (int)((gridDim.x * blockDim.x) >> 6);
    const int chunk = 64 * VEC;
    const bool small = T <= 64;
    for (int64_t i = wave; i < B; i += nwaves) {
        int k = __builtin_amdgcn_readfirstlane(nvalid[i]);
        k = k < T ? k : T;
        float dot = 0.f, da0 = 0.f, at0 = 0.f;
        int32_t id0 = -1;
        for (int j0 = 0; j0 < k; j0 += 64) {
            const int32_t myid = kept_id(ids, i, T, j0 + lane, k, N);
            const int kk = (k - j0) < 64 ? (k - j0) : 64;
            float myda = 0.f;
            for (int t0 = 0; t0 < kk; t0 += UNROLL) {
                int32_t id[UNROLL];
                float part[UNROLL];
#pragma unroll
                for (int q = 0; q < UNROLL; ++q) {
                    const int t = t0 + q;
                    id[q] = (t < kk) ? __builtin_amdgcn_readlane(myid, t < 64 ? t : 0) : -1;
                    part[q] = 0.f;
                }
                for (int c0 = 0; c0 < H; c0 += chunk) {
                    const int col = c0 + lane * VEC;
                    const bool cact = col < H;
                    float r[UNROLL][VEC], gg[VEC];
#pragma unroll
                    for (int q = 0; q < UNROLL; ++q) load_vec<VEC>(x + (int64_t)id[q] * H + col, id[q] >= 0 && cact, r[q]);
                    load_vec<VEC>(g + i * H + col, cact, gg);
#pragma unroll
                    for (int q = 0; q < UNROLL; ++q)
#pragma unroll
                        for (int e = 0; e < VEC; ++e) part[q] = fmaf(gg[e], r[q][e], part[q]);
                }
#pragma unroll
                for (int q = 0; q < UNROLL; ++q) {
                    if (t0 + q < kk) {                          // wave-uniform
                        const float s = ps_wave_sum_f32(part[q]);
                        if (lane == t0 + q) myda = s;
                    }
                }
            }
            const float myat = (j0 + lane < k) ? attn[i * T + j0 + lane] : 0.f;
            for (int t = 0; t < kk; ++t)
                if (__builtin_amdgcn_readlane(myid, t) >= 0) dot = fmaf(lane_f32(myat, t), lane_f32(myda, t), dot);
            if (small) { da0 = myda; at0 = myat; id0 = myid; }
            else if (j0 + lane < k) ds[i * T + j0 + lane] = myda;
        }
        float ds0 = 0.f;
        if (small) {
            ds0 = id0 >= 0 ? at0 * (da0 - dot) : 0.f;
            if (lane < T) ds[i * T + lane] = ds0;
        } else {
            for (int j0 = 0; j0 < T; j0 += 64) {
                const int jj = j0 + lane;
                const bool kept = kept_id(ids, i, T, jj, k, N) >= 0;
                if (jj < T) ds[i * T + jj] = kept ? attn[i * T + jj] * (ds[i * T + jj] - dot) : 0.f;
            }
        }
        for (int c0 = 0; c0 < Hd; c0 += chunk) {
            const int col = c0 + lane * VEC;
            const bool cact = col < Hd;
            float uu[VEC], ww[VEC], adu[VEC], adw[VEC];
            load_vec<VEC>(u + i * Hd + col, cact, uu);
            load_vec<VEC>(w2 + col, cact, ww);
#pragma unroll
            for (int e = 0; e < VEC; ++e) adu[e] = adw[e] = 0.f;
            for (int j0 = 0; j0 < k; j0 += 64) {
                const int32_t myid = small ? id0 : kept_id(ids, i, T, j0 + lane, k, N);
                const float myds = small ? ds0 : (j0 + lane < k ? ds[i * T + j0 + lane] : 0.f);
                const int kk = (k - j0) < 64 ? (k - j0) : 64;
                for (int t0 = 0; t0 < kk; t0 += UNROLL) {
                    int32_t id[UNROLL];
                    float dsv[UNROLL];
                    float r[UNROLL][VEC];
#pragma unroll
                    for (int q = 0; q < UNROLL; ++q) {
                        const int t = t0 + q;
                        id[q] = (t < kk) ? __builtin_amdgcn_readlane(myid, t < 64 ? t : 0) : -1;
                        dsv[q] = lane_f32(myds, t < 64 ? t : 0);
                        load_vec<VEC>(v + (int64_t)id[q] * Hd + col, id[q] >= 0 && cact, r[q]);
                    }
#pragma unroll
                    for (int q = 0; q < UNROLL; ++q) {
                        if (id[q] < 0) continue;               // wave-uniform
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            const float h = uu[e] + r[q][e];
                            adu[e] = fmaf(dsv[q], h > 0.f ? ww[e] : 0.f, adu[e]);
                            adw[e] = fmaf(dsv[q], h < 0.f ? 0.f : h, adw[e]);
                        }
                    }
                }
            }
            if (cact) {
                store_vec<VEC>(du + i * Hd + col, adu);
                store_vec<VEC>(share + i * Hd + col, adw);
            }
        }
    }
}

// dw2: the row shares of DW_ROWS consecutive target rows added in ascending order from +0 (one partition per workgroup row),
// then the partitions in ascending order from +0
__global__ __launch_bounds__(256) void dw2_partition_kernel(const float *__restrict__ share, int64_t B, int Hd, float *__restrict__ parts) {
    const int c = blockIdx.y * blockDim.x + threadIdx.x;
    if (c >= Hd) return;
    const int64_t r0 = (int64_t)blockIdx.x * DW_ROWS;
    const int64_t r1 = r0 + DW_ROWS < B ? r0 + DW_ROWS : B;
    float acc = 0.f;
    for (int64_t q0 = r0; q0 < r1; q0 += UNROLL) {
        float t[UNROLL];
#pragma unroll
        for (int q = 0; q < UNROLL; ++q) t[q] = q0 + q < r1 ? share[(q0 + q) * Hd + c] : 0.f;
#pragma unroll
        for (int q = 0; q < UNROLL; ++q)
            if (q0 + q < r1) acc = acc + t[q];
    }
    parts[(int64_t)blockIdx.x * Hd + c] = acc;
}
__global__ __launch_bounds__(256) void dw2_final_kernel(const float *__restrict__ parts, int64_t P, int Hd, float *__restrict__ dw2) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= Hd) return;
    float acc = 0.f;
    for (int64_t p = 0; p < P; ++p) acc = acc + parts[p * Hd + c];
    dw2[c] = acc;
}

}  // namespace

extern "C" int ps_pool_weights(const int32_t *ids, const int32_t *counts, const float *wts, const int32_t *nvalid, int64_t B, int T,
                               int64_t max_idx, int renorm, int lanes, float *w_eff, ps_stream_t stream) {
    if (B < 0 || T <= 0 || (lanes != 16 && lanes != 64)) return PS_EINVAL;
    if (B == 0) return PS_OK;
    if (!ids || !nvalid || !w_eff || (!counts && !wts)) return PS_EINVAL;
    hipStream_t st = ps_stream(stream);
    const char *pe = getenv("PS_POOL_ROWS_PER_WAVE");         // ps_importance_pool's switch: 1 = the wave layout everywhere
    const bool four = lanes == 16 && T <= 64 && !(pe && atoi(pe) == 1);
    if (four) {
        const dim3 grid4(ps_row4_grid(B));
        if (T <= 16)
            hipLaunchKernelGGL(pool_weights4_kernel<1>, grid4, dim3(256), 0, st, ids, counts, wts, nvalid, B, T, max_idx, renorm, w_eff);
        else
            hipLaunchKernelGGL(pool_weights4_kernel<4>, grid4, dim3(256), 0, st, ids, counts, wts, nvalid, B, T, max_idx, renorm, w_eff);
    } else {
        hipLaunchKernelGGL(pool_weights_kernel, dim3(ps_row_grid(B)), dim3(256), 0, st, ids, counts, wts, nvalid, B, T, max_idx, renorm,
                           w_eff);
    }
    PS_CHECK_LAUNCH();
    return PS_OK;
}

extern "C" int ps_gather_bwd_segment(void) { return SEG; }

extern "C" size_t ps_gather_bwd_workspace_bytes(int64_t B, int T, int H) {
    if (B <= 0 || T <= 0 || H <= 0) return 0;
    return transposed_bytes(B, T, H);
}

extern "C" int ps_gather_bwd(const int64_t *rptr, const int32_t *slots, int64_t N, int T, const float *coef, const int32_t *arg,
                             const float *g, int64_t B, int H, float *gx, void *workspace, size_t workspace_bytes,
                             ps_stream_t stream) {
    if (N < 0 || B < 0 || T <= 0 || H <= 0 || B * (int64_t)T >= ((int64_t)1 << 31)) return PS_EINVAL;
    if (N == 0) return PS_OK;
    if (!gx) return PS_EINVAL;
    hipStream_t st = ps_stream(stream);
    if (B == 0) {                                             // nothing points at any row: every element is +0.0
        if (ps_fill_async(gx, 0, (size_t)N * H * sizeof(float), st) != hipSuccess) return PS_ELAUNCH;
        return PS_OK;
    }
    if (!rptr || !slots || !g || (coef != nullptr) == (arg != nullptr) || !workspace) return PS_EINVAL;
    if (workspace_bytes < transposed_bytes(B, T, H)) return PS_EINVAL;
    TArgs a{rptr, slots, N, T, coef, arg, g, B, H, nullptr, nullptr, gx, reinterpret_cast<float *>(ps_ws_base(workspace)),
            seg_blocks(B, T)};
    const bool vec4 = H % 4 == 0 && ps_aligned16({g, gx, arg});
    return coef ? launch_transposed<0>(a, vec4, st) : launch_transposed<1>(a, vec4, st);
}

extern "C" int ps_gather_max_arg(const float *x, int64_t N, int H, const int32_t *ids, const int32_t *nvalid, int64_t B, int T,
                                 float *out, int32_t *arg, ps_stream_t stream) {
    if (B < 0 || H <= 0 || T <= 0 || N < 0) return PS_EINVAL;
    if (B == 0) return PS_OK;
    if (!x || !ids || !nvalid || !out || !arg) return PS_EINVAL;
    hipStream_t st = ps_stream(stream);
    const bool vec4 = H % 4 == 0 && ps_aligned16({x, out, arg});
    PS_LAUNCH_VEC(gather_max_arg_kernel<VEC>, vec4, dim3(ps_row_grid(B)), dim3(256), st, x, N, H, ids, nvalid, B, T, out, arg);
    PS_CHECK_LAUNCH();
    return PS_OK;
}

extern "C" size_t ps_attention_bwd_rows_workspace_bytes(int64_t B, int Hd) {
    if (B <= 0 || Hd <= 0) return 0;
    return 256 + ps_align256((size_t)(B + ps_cdiv(B, DW_ROWS)) * Hd * sizeof(float));
}

extern "C" int ps_attention_bwd_rows(const float *x, int64_t N, int H, const float *u, const float *v, int Hd, const float *w2,
                                     const int32_t *ids, const int32_t *nvalid, const float *attn, const float *g, int64_t B, int T,
                                     float *ds, float *du, float *dw2, void *workspace, size_t workspace_bytes, ps_stream_t stream) {
    if (B < 0 || H <= 0 || Hd <= 0 || T <= 0 || N < 0) return PS_EINVAL;
    if (B == 0) return PS_OK;
    if (!x || !u || !v || !w2 || !ids || !nvalid || !attn || !g || !ds || !du || !dw2 || !workspace) return PS_EINVAL;
    if (workspace_bytes < ps_attention_bwd_rows_workspace_bytes(B, Hd)) return PS_EINVAL;
    hipStream_t st = ps_stream(stream);
    float *share = reinterpret_cast<float *>(ps_ws_base(workspace));
    float *parts = share + B * Hd;
    const int64_t P = ps_cdiv(B, DW_ROWS);
    const bool vec4 = H % 4 == 0 && Hd % 4 == 0 && ps_aligned16({x, u, v, w2, g, du});
    PS_LAUNCH_VEC(attention_bwd_rows_kernel<VEC>, vec4, dim3(ps_row_grid(B)), dim3(256), st, x, N, H, u, v, Hd, w2, ids, nvalid, attn, g,
                  B, T, ds, du, share);
    PS_CHECK_LAUNCH();
    hipLaunchKernelGGL(dw2_partition_kernel, dim3((unsigned)P, (unsigned)ps_cdiv(Hd, 256)), dim3(256), 0, st, share, B, Hd, parts);
    PS_CHECK_LAUNCH();
    hipLaunchKernelGGL(dw2_final_kernel, dim3((unsigned)ps_cdiv(Hd, 256)), dim3(256), 0, st, parts, P, Hd, dw2);
    PS_CHECK_LAUNCH();
    return PS_OK;
}

extern "C" int ps_attention_bwd_cols(const int64_t *rptr, const int32_t *slots, int64_t N, int T, const float *ds, const float *u,
                                     const float *v, int Hd, const float *w2, int64_t B, float *dv, void *workspace,
                                     size_t workspace_bytes, ps_stream_t stream) {
    if (N < 0 || B < 0 || T <= 0 || Hd <= 0 || B * (int64_t)T >= ((int64_t)1 << 31)) return PS_EINVAL;
    if (N == 0) return PS_OK;
    if (!dv) return PS_EINVAL;
    hipStream_t st = ps_stream(stream);
    if (B == 0) {
        if (ps_fill_async(dv, 0, (size_t)N * Hd * sizeof(float), st) != hipSuccess) return PS_ELAUNCH;
        return PS_OK;
    }
    if (!rptr || !slots || !ds || !u || !v || !w2 || !workspace) return PS_EINVAL;
    if (workspace_bytes < transposed_bytes(B, T, Hd)) return PS_EINVAL;
    TArgs a{rptr, slots, N, T, ds, nullptr, u, B, Hd, v, w2, dv, reinterpret_cast<float *>(ps_ws_base(workspace)), seg_blocks(B, T)};
    const bool vec4 = Hd % 4 == 0 && ps_aligned16({u, v, w2, dv});
    return launch_transposed<2>(a, vec4, st);
}
