// cooc_mfma.hip -- the item co-occurrence graph of GraphBuilder.build_item_similarity_graph (reference
// data/graph_builder.py:59-116) as an EXACT integer contraction on the gfx950 matrix cores.
//
// With m_ua the number of rows (user u, item a), the reference's count of the unordered pair {a, b}, a != b, is
//     count(a, b) = sum_u m_ua m_ub
// i.e. one element of the symmetric GEMM A A^T with K = users.  The multiplicities are stored once as K-major operand
// planes in fragment order (the idea of hamming_mfma.hip's sign planes) and contracted over the upper triangle of 64 x 64
// item blocks only (one wave per block = 2 x 2 tiles of 32 x 32; a diagonal block also computes its lower 32 x 32 tile, whose
// elements the epilogue's i < j test drops):
//   fp4  (every m <= 4): e2m1 codes 0 -> 0x0, 1 -> 0x2, 2 -> 0x4, 3 -> 0x5, 4 -> 0x6, v_mfma_scale_f32_32x32x64_f8f6f4 with
//        both block scales 2^0.  Every product and partial sum is a non-negative integer <= sum_u m_ua^2 (Cauchy-Schwarz),
//        so the f32 accumulator is exact while that bound is below 2^24.
//   int8 (5 <= max m <= 127): v_mfma_i32_32x32x32_i8, exact while the bound is below 2^31.
// Planes: for a tile of 32 items and a K step s, one 1 KiB block; lane `lane`'s 16 bytes hold the codes of item
// 32 tile + (lane & 31) for the users  64 s + 32 (lane >> 5) + j, j = 0..31, low nibble first  (fp4)  or
// 32 s + 16 (lane >> 5) + j, j = 0..15 (int8).  A and B use the same (lane, byte) -> user map, so the contraction is over
// matching users whatever order the hardware applies inside a step; a step always covers the same 64 / 32 users.
//
// The first common user (the reference's dict insertion order is keyed on it) comes out of the contraction almost for
// free: products are >= 0, so the accumulator is monotone in K.  After every window of PS_COOC_WINDOW users each element
// adds 1 to a counter when its accumulator is still 0; at the end that counter is the window that holds the first user
// with m_ua m_ub > 0.  ps_cooc_keys then resolves the user inside the window from the per-item user lists.
#include "ps_common.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int WINDOW = PS_COOC_WINDOW;

struct Fmt {
    int step;   // users per K step
    bool fp4;
};
inline Fmt fmt_of(int max_mult) { return max_mult <= 4 ? Fmt{64, true} : Fmt{32, false}; }

inline int64_t plane_steps(int64_t U, Fmt f) { return ps_cdiv(U, f.step); }
inline int64_t plane_tiles(int64_t M) { return ps_cdiv(M, 64) * 2; }            // items padded to whole 64-item blocks

__global__ void cooc_planes_kernel(const int32_t *__restrict__ user, const int32_t *__restrict__ item,
                                   const int32_t *__restrict__ mult, int64_t n, int64_t KS, int fp4,
                                   uint32_t *__restrict__ planes, int64_t *__restrict__ item_stats, int64_t M,
                                   int32_t *__restrict__ max_seen) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t u = user[e], a = item[e];
        const int m = mult[e];
        const int64_t t = a >> 5, r = a & 31;
        uint32_t code;
        int64_t byte;
        int shift;
        if (fp4) {
            const int64_t s = u >> 6, k = u & 63;
            const int64_t lane = ((k >> 5) << 5) + r, j = k & 31;
            byte = ((t * KS + s) * 64 + lane) * 16 + (j >> 1);
            shift = 4 * (int)(j & 1);
            code = m <= 0 ? 0u : m == 1 ? 0x2u : m == 2 ? 0x4u : m == 3 ? 0x5u : 0x6u;
        } else {
            const int64_t s = u >> 5, k = u & 31;
            const int64_t lane = ((k >> 4) << 5) + r, j = k & 15;
            byte = ((t * KS + s) * 64 + lane) * 16 + j;
            shift = 0;
            code = (uint32_t)m & 0xffu;
        }
        atomicOr(planes + (byte >> 2), code << (8 * (int)(byte & 3) + shift));
        atomicMax(max_seen, m);
        atomicAdd(reinterpret_cast<unsigned long long *>(item_stats + a), (unsigned long long)((int64_t)m * (m - 1) / 2));
        atomicAdd(reinterpret_cast<unsigned long long *>(item_stats + M + a), (unsigned long long)((int64_t)m * m));
        if (m >= 2) atomicMin(reinterpret_cast<unsigned long long *>(item_stats + 2 * M + a), (unsigned long long)u);
    }
}

// one wave = one 64 x 64 block of item pairs (2 x 2 tiles); a workgroup of 4 waves = 4 blocks of one block row
template <bool FP4>
__device__ __forceinline__ void cooc_step(const v4i &a0, const v4i &a1, const v4i &b0, const v4i &b1, v16f (&acc)[4]) {
    if constexpr (FP4) {
        const v8i A0 = {a0[0], a0[1], a0[2], a0[3], 0, 0, 0, 0}, A1 = {a1[0], a1[1], a1[2], a1[3], 0, 0, 0, 0};
        const v8i B0 = {b0[0], b0[1], b0[2], b0[3], 0, 0, 0, 0}, B1 = {b1[0], b1[1], b1[2], b1[3], 0, 0, 0, 0};
        acc[0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A0, B0, acc[0], 4, 4, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
        acc[1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A0, B1, acc[1], 4, 4, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
        acc[2] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A1, B0, acc[2], 4, 4, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
        acc[3] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A1, B1, acc[3], 4, 4, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
    } else {
        // int32 accumulators carried in the float vectors by bit pattern (no arithmetic touches them as floats)
        acc[0] = __builtin_bit_cast(v16f, __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, __builtin_bit_cast(v16i, acc[0]), 0, 0, 0));
        acc[1] = __builtin_bit_cast(v16f, __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b1, __builtin_bit_cast(v16i, acc[1]), 0, 0, 0));
        acc[2] = __builtin_bit_cast(v16f, __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, __builtin_bit_cast(v16i, acc[2]), 0, 0, 0));
        acc[3] = __builtin_bit_cast(v16f, __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, __builtin_bit_cast(v16i, acc[3]), 0, 0, 0));
    }
}

template <bool FP4>
__device__ __forceinline__ int acc_count(float v) {
    if constexpr (FP4) return (int)v;
    else return __builtin_bit_cast(int, v);
}

template <bool FP4>
__global__ __launch_bounds__(256) void cooc_pairs_kernel(const v4i *__restrict__ planes, int64_t KS, int64_t nb, int64_t M,
                                                        int64_t thr, int4 *__restrict__ rec, int64_t cap,
                                                        unsigned long long *__restrict__ count) {
    constexpr int C = WINDOW / (FP4 ? 64 : 32);              // K steps per window
    const int lane = ps_lane();
    const int64_t bi = blockIdx.y;
    const int64_t bj = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (bj < bi || bj >= nb) return;                          // lower triangle / past the end: wave-uniform exit
    const v4i *pa0 = planes + (2 * bi) * KS * 64 + lane, *pa1 = pa0 + KS * 64;
    const v4i *pb0 = planes + (2 * bj) * KS * 64 + lane, *pb1 = pb0 + KS * 64;
    v16f acc[4];
    int zc[4][16];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[t][r] = 0.0f; zc[t][r] = 0; }
    v4i a0 = pa0[0], a1 = pa1[0], b0 = pb0[0], b1 = pb1[0];
    for (int64_t w0 = 0; w0 < KS; w0 += C) {
        const int64_t end = w0 + C < KS ? w0 + C : KS;
        for (int64_t s = w0; s < end; ++s) {
            const int64_t o = (s + 1 < KS ? s + 1 : s) * 64;   // next step's fragments under this step's MFMAs
            const v4i na0 = pa0[o], na1 = pa1[o], nb0 = pb0[o], nb1 = pb1[o];
            cooc_step<FP4>(a0, a1, b0, b1, acc);
            a0 = na0; a1 = na1; b0 = nb0; b1 = nb1;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) zc[t][r] += acc_count<FP4>(acc[t][r]) == 0;
    }
    // 32 x 32 result layout: register r of lane l is row 8 (r >> 2) + 4 (l >> 5) + (r & 3) (A: items of tile row),
    // column l & 31 (B: items of tile column)
    const int64_t rbase = 64 * bi + 4 * (lane >> 5), cbase = 64 * bj + (lane & 31);
    auto item_i = [&](int t, int r) { return rbase + 32 * (t >> 1) + 8 * (r >> 2) + (r & 3); };
    auto item_j = [&](int t) { return cbase + 32 * (t & 1); };
    int mine = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t i = item_i(t, r), j = item_j(t);
            mine += (i < j && j < M && (int64_t)acc_count<FP4>(acc[t][r]) >= thr);
        }
    // wave-exclusive prefix of the survivors, one atomic per wave
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int v = __shfl_up(incl, d, 64);
        if (lane >= d) incl += v;
    }
    const int total = __shfl(incl, 63, 64);
    if (total == 0) return;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(count, (unsigned long long)total);
    base = __shfl(base, 0, 64);
    int64_t at = (int64_t)base + incl - mine;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t i = item_i(t, r), j = item_j(t);
            const int c = acc_count<FP4>(acc[t][r]);
            if (i < j && j < M && (int64_t)c >= thr) {
                if (at < cap) rec[at] = make_int4((int)i, (int)j, c, zc[t][r]);
                ++at;
            }
        }
}

// self pairs (a, a): count sum_u m(m-1)/2, first user = the first with m >= 2 (from the planes pass)
__global__ void cooc_self_kernel(const int64_t *__restrict__ item_stats, int64_t M, int64_t thr, int4 *__restrict__ rec,
                                 int64_t cap, unsigned long long *__restrict__ count) {
    const int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (a >= M) return;
    const int64_t c = item_stats[a];
    if (c <= 0 || c < thr) return;
    const int64_t at = (int64_t)atomicAdd(count, 1ull);
    if (at < cap) rec[at] = make_int4((int)a, (int)a, (int)c, (int)(item_stats[2 * M + a] / WINDOW));
}

__device__ __forceinline__ int64_t lower_bound_i32(const int32_t *__restrict__ v, int64_t lo, int64_t hi, int32_t x) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (v[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one thread per record: the first common user inside the record's window, then the first positions of a and b in that
// user's group by binary search; key = (uptr[u] + p) * R + (uptr[u] + q)  ==  the order of (u, p, q)
__global__ void cooc_keys_kernel(const int4 *__restrict__ rec, int64_t n, const int64_t *__restrict__ iptr,
                                 const int32_t *__restrict__ iuser, const int32_t *__restrict__ imult,
                                 const int64_t *__restrict__ uptr, const int32_t *__restrict__ uitem,
                                 const int32_t *__restrict__ upos, int64_t R, int64_t U, int64_t M, int64_t *__restrict__ keys) {
    const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int4 e = rec[k];
    if (e.x < 0 || e.x > e.y || e.y >= M || e.w < 0 || e.w > (U - 1) / WINDOW) { keys[k] = -1; return; }   // not a record of ps_cooc_pairs
    const int32_t a = e.x, b = e.y, w0 = e.w * WINDOW, w1 = w0 + WINDOW;
    int64_t ia = lower_bound_i32(iuser, iptr[a], iptr[a + 1], w0);
    const int64_t ea = iptr[a + 1];
    int64_t u = -1;
    if (a == b) {
        for (; ia < ea && iuser[ia] < w1; ++ia)
            if (imult[ia] >= 2) { u = iuser[ia]; break; }
    } else {
        int64_t ib = lower_bound_i32(iuser, iptr[b], iptr[b + 1], w0);
        const int64_t eb = iptr[b + 1];
        while (ia < ea && ib < eb) {
            const int32_t x = iuser[ia], y = iuser[ib];
            if (x >= w1 || y >= w1) break;
            if (x == y) { u = x; break; }
            if (x < y) ++ia;
            else ++ib;
        }
    }
    if (u < 0) { keys[k] = -1; return; }                      // not reached for a record of ps_cooc_pairs (checked by the caller)
    const int64_t g0 = uptr[u], g1 = uptr[u + 1];
    const int64_t xa = lower_bound_i32(uitem, g0, g1, a);
    const int64_t xb = a == b ? xa + 1 : lower_bound_i32(uitem, g0, g1, b);
    if (xa >= g1 || xb >= g1 || uitem[xa] != a || uitem[xb] != b) { keys[k] = -1; return; }
    int64_t p = upos[xa], q = upos[xb];
    if (q < p) { const int64_t t = p; p = q; q = t; }
    keys[k] = (g0 + p) * R + (g0 + q);
}

// record perm[k] -> columns 2k, 2k + 1 of both edge_index rows ([a -> b, b -> a]) and of edge_weight
__global__ void cooc_emit_kernel(const int4 *__restrict__ rec, const int64_t *__restrict__ perm, int64_t n,
                                 int64_t *__restrict__ edge_index, float *__restrict__ edge_weight) {
    const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int64_t j = perm[k];
    const int4 e = j >= 0 && j < n ? rec[j] : make_int4(-1, -1, -1, -1);    // -1 edges: perm was not a permutation of 0..n-1
    edge_index[2 * k] = e.x;
    edge_index[2 * k + 1] = e.y;
    edge_index[2 * n + 2 * k] = e.y;
    edge_index[2 * n + 2 * k + 1] = e.x;
    edge_weight[2 * k] = (float)e.z;
    edge_weight[2 * k + 1] = (float)e.z;
}

}  // namespace

extern "C" size_t ps_cooc_planes_bytes(int64_t U, int64_t M, int max_mult) {
    if (U <= 0 || M <= 0 || max_mult < 1 || max_mult > 127 || U >= ((int64_t)1 << 31) || M >= ((int64_t)1 << 31) - 64) return 0;
    const Fmt f = fmt_of(max_mult);
    return (size_t)(plane_tiles(M) * plane_steps(U, f) * 1024);
}

extern "C" int ps_cooc_planes(const int32_t *user, const int32_t *item, const int32_t *mult, int64_t n, int64_t U, int64_t M,
                              int max_mult, void *planes, size_t planes_bytes, int64_t *item_stats, int32_t *max_seen,
                              ps_stream_t stream) {
    if (n < 0 || U <= 0 || M <= 0 || max_mult < 1) return PS_EINVAL;
    if (max_mult > 127) return PS_EUNSUPPORTED;
    const size_t need = ps_cooc_planes_bytes(U, M, max_mult);
    if (need == 0) return PS_EINVAL;
    if (!planes || !item_stats || !max_seen || (n > 0 && (!user || !item || !mult))) return PS_EINVAL;
    if (reinterpret_cast<size_t>(planes) % 16 != 0) return PS_EINVAL;
    if (planes_bytes < need) return PS_EWORKSPACE;
    const Fmt f = fmt_of(max_mult);
    hipStream_t s = ps_stream(stream);
    if (ps_fill_async(planes, 0, need, s) != hipSuccess) return PS_ELAUNCH;
    if (ps_fill_async(item_stats, 0, (size_t)(2 * M) * sizeof(int64_t), s) != hipSuccess) return PS_ELAUNCH;
    if (ps_fill_async(item_stats + 2 * M, 0x7f, (size_t)M * sizeof(int64_t), s) != hipSuccess) return PS_ELAUNCH;
    if (ps_fill_async(max_seen, 0, sizeof(int32_t), s) != hipSuccess) return PS_ELAUNCH;
    if (n == 0) return PS_OK;
    int64_t grid = ps_cdiv(n, 256);
    if (grid > 256 * 64) grid = 256 * 64;
    hipLaunchKernelGGL(cooc_planes_kernel, dim3((unsigned)grid), dim3(256), 0, s, user, item, mult, n, plane_steps(U, f),
                       f.fp4 ? 1 : 0, reinterpret_cast<uint32_t *>(planes), item_stats, M, max_seen);
    PS_CHECK_LAUNCH();
    return PS_OK;
}

extern "C" int ps_cooc_pairs(const void *planes, int64_t U, int64_t M, int max_mult, int64_t max_sq, const int64_t *item_stats,
                             int64_t thr, ps_cooc_record *records, int64_t capacity, int64_t *count, int64_t *h_count,
                             ps_stream_t stream) {
    if (U <= 0 || M <= 0 || max_mult < 1 || thr < 1 || capacity < 0 || max_sq < 0) return PS_EINVAL;
    if (max_mult > 127) return PS_EUNSUPPORTED;
    const Fmt f = fmt_of(max_mult);
    if (max_sq >= (f.fp4 ? ((int64_t)1 << 24) : ((int64_t)1 << 31))) return PS_EUNSUPPORTED;   // a count could be inexact
    if (ps_cooc_planes_bytes(U, M, max_mult) == 0) return PS_EINVAL;
    if (!planes || !item_stats || !count || !h_count || (capacity > 0 && !records)) return PS_EINVAL;
    if (plane_tiles(M) / 2 > 65535) return PS_EUNSUPPORTED;             // one grid row per 64-item block row
    hipStream_t s = ps_stream(stream);
    if (ps_fill_async(count, 0, sizeof(int64_t), s) != hipSuccess) return PS_ELAUNCH;
    int4 *rec = reinterpret_cast<int4 *>(records);
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(count);
    hipLaunchKernelGGL(cooc_self_kernel, dim3((unsigned)ps_cdiv(M, 256)), dim3(256), 0, s, item_stats, M, thr, rec, capacity, cnt);
    PS_CHECK_LAUNCH();
    const int64_t KS = plane_steps(U, f), nb = plane_tiles(M) / 2;
    const dim3 grid((unsigned)ps_cdiv(nb, 4), (unsigned)nb);
    if (f.fp4)
        hipLaunchKernelGGL(cooc_pairs_kernel<true>, grid, dim3(256), 0, s, reinterpret_cast<const v4i *>(planes), KS, nb, M, thr,
                           rec, capacity, cnt);
    else
        hipLaunchKernelGGL(cooc_pairs_kernel<false>, grid, dim3(256), 0, s, reinterpret_cast<const v4i *>(planes), KS, nb, M, thr,
                           rec, capacity, cnt);
    PS_CHECK_LAUNCH();
    if (hipMemcpyAsync(h_count, count, sizeof(int64_t), hipMemcpyDeviceToHost, s) != hipSuccess) return PS_ELAUNCH;
    if (hipStreamSynchronize(s) != hipSuccess) return PS_ELAUNCH;
    return *h_count > capacity ? PS_EWORKSPACE : PS_OK;
}

extern "C" int ps_cooc_keys(const ps_cooc_record *records, int64_t n, int64_t U, int64_t M, const int64_t *iptr, const int32_t *iuser,
                            const int32_t *imult, const int64_t *uptr, const int32_t *uitem, const int32_t *upos, int64_t R,
                            int64_t *keys, ps_stream_t stream) {
    if (n < 0 || U <= 0 || M <= 0 || R < 0 || R >= ((int64_t)1 << 31)) return PS_EINVAL;
    if (n == 0) return PS_OK;
    if (!records || !iptr || !iuser || !imult || !uptr || !uitem || !upos || !keys) return PS_EINVAL;
    hipLaunchKernelGGL(cooc_keys_kernel, dim3((unsigned)ps_cdiv(n, 256)), dim3(256), 0, ps_stream(stream),
                       reinterpret_cast<const int4 *>(records), n, iptr, iuser, imult, uptr, uitem, upos, R, U, M, keys);
    PS_CHECK_LAUNCH();
    return PS_OK;
}

extern "C" int ps_cooc_emit(const ps_cooc_record *records, const int64_t *perm, int64_t n, int64_t *edge_index, float *edge_weight,
                            ps_stream_t stream) {
    if (n < 0) return PS_EINVAL;
    if (n == 0) return PS_OK;
    if (!records || !perm || !edge_index || !edge_weight) return PS_EINVAL;
    hipLaunchKernelGGL(cooc_emit_kernel, dim3((unsigned)ps_cdiv(n, 256)), dim3(256), 0, ps_stream(stream),
                       reinterpret_cast<const int4 *>(records), perm, n, edge_index, edge_weight);
    PS_CHECK_LAUNCH();
    return PS_OK;
}
