// lsh_filter.hip -- ps_lsh_encode over a STAGED rotation (flag PS_LSH_STAGED): the sign of x . A[j] decided by a split-bf16
// estimate on v_mfma_f32_32x32x16_bf16 wherever that estimate is beyond doubt, and by the oracle's own fp32 fmaf chain
// (oracle/pinsage_oracle.c: orc_lsh_encode) everywhere else.  Codes are bit-identical to the fp32 path of dense_mfma.hip.
//
//   estimate   f = sum_k xh ah + xl ah + xh al,   xh = bf16(x), xl = bf16(x - xh), ah / al likewise (round to nearest even),
//              f32 accumulator.  |f - chain| <= 2^-12.9 ||x|| ||a|| at D = 256 (DESIGN.md section 4 has the derivation).
//   rule       the sign of f is taken ONLY IF |f| > c nx_i na_j, c = 2^-12 max(1, D / 256), nx / na upper bounds of the row
//              norms.  The comparison is strict; a NaN, an infinite bound (norm not finite, zero, or outside [2^-30, 2^30])
//              and f = 0 all fail it.  Such a dot is FLAGGED and gets its exact chain: acc = fmaf(x[k], A[j][k], acc) from
//              +0.0f, k ascending, bit = acc >= 0.
//
// The staged image (ps_lsh_stage, made once per matrix):
//   [0, 64)        header: magic, nbits, D, 0; uint64 dots seen @16, uint64 dots flagged @24 (both only move under PS_LSH_STATS=1)
//   [64, ..)       A as fp32 [nbits, D], natural order (the chain reads it)
//   then nbits/32 slabs of KS * 2048 + 128 bytes, KS = D / 16: per k step s the A operand fragments of the 32 rotation rows,
//                  hi then lo, one 16-byte piece per lane (lane = 32 h + r holds row r, k = 16 s + 8 (e >> 2) + 4 h + (e & 3)
//                  in element e -- the k order in which the kernel's float4 loads of x fill ITS fragments: a sum over k may
//                  pair the operands in any order as long as both sides use the same one); then na[32] floats.
//
// One workgroup = 4 waves = one tile of 128 rows (JS = 1) or 64 rows (JS = 2: the waves split the slabs of an iteration among
// themselves, for launches of too few rows to fill the CUs with 128-row tiles).  A wave keeps the fragments of its 32 rows for
// the whole of D in registers (D <= 256: 128 VGPRs), the slabs pass through LDS once per tile (512 KiB of L2 reads per 128
// rows = 21 B/clk/CU at the MFMA rate), the next slab is prefetched into registers under the MFMAs of the current one.  Sign and
// flag words collect in LDS; after the last slab the flagged dots are compacted into an LDS list and drained by all 256
// threads, round after round until no flag is left (the list's size bounds a round, never the number of flagged dots).
#include "ps_common.h"

#ifndef PS_LSHF_DEBUG
#define PS_LSHF_DEBUG 0    // 1: every estimate f is also written to the [N, nbits] float buffer given to ps_debug_lsh_dump
#endif                     // (tools/lsh_filter_error.py measures |f - chain| / (nx na) with it; not part of the product build)
                           // 2: the buffer takes 16 s_memtime stamps / sums per workgroup instead (tools/lsh_filter_phases.py)

#if PS_LSHF_DEBUG
__device__ float *ps_lshf_dump_buf;
extern "C" int ps_debug_lsh_dump(float *buf) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(ps_lshf_dump_buf), &buf, sizeof buf); }
#endif

#if PS_LSHF_DEBUG == 2
#define LSHF_STAMP(slot) do { if (threadIdx.x == 0 && ps_lshf_dump_buf != nullptr) \
    reinterpret_cast<unsigned long long *>(ps_lshf_dump_buf)[(size_t)blockIdx.x * 16 + (slot)] = __builtin_readcyclecounter(); } while (0)
#define LSHF_NOW() __builtin_readcyclecounter()
#define LSHF_PUT(slot, v) do { if (threadIdx.x == 0 && ps_lshf_dump_buf != nullptr) \
    reinterpret_cast<unsigned long long *>(ps_lshf_dump_buf)[(size_t)blockIdx.x * 16 + (slot)] = (v); } while (0)
#else
#define LSHF_STAMP(slot) do {} while (0)
#define LSHF_NOW() 0ull
#define LSHF_PUT(slot, v) do {} while (0)
#endif

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t LSHF_MAGIC = 0x4653484cu;      // "LHSF"
constexpr int HEADER_BYTES = 64;
constexpr int LIST_CAP = 2048;
constexpr int MAX_NBITS = 1024;                   // sign + flag words of a 128-row tile: 32 KiB of LDS at most

__host__ __device__ constexpr int slab_f4(int KS) { return KS * 128 + 8; }       // float4s per slab

struct StageLayout {
    size_t a32, slabs, total;
};
inline StageLayout stage_layout(int nbits, int D) {
    StageLayout l;
    l.a32 = HEADER_BYTES;
    l.slabs = l.a32 + (size_t)nbits * D * 4;
    l.total = l.slabs + (size_t)(nbits / 32) * slab_f4(D / 16) * 16;
    return l;
}
inline bool served(int nbits, int D) {
    return (D == 32 || D == 64 || D == 128 || D == 256) && nbits > 0 && nbits % 32 == 0 && nbits <= MAX_NBITS;
}

__global__ __launch_bounds__(256) void lsh_stage_kernel(const float *__restrict__ A, int nbits, int D, unsigned char *__restrict__ img,
                                                        size_t off_a32, size_t off_slabs) {
    const int KS = D / 16, W = nbits / 32;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (t0 == 0) {
        uint32_t *h = reinterpret_cast<uint32_t *>(img);
        h[0] = LSHF_MAGIC;
        h[1] = (uint32_t)nbits;
        h[2] = (uint32_t)D;
        for (int i = 3; i < HEADER_BYTES / 4; ++i) h[i] = 0u;
    }
    float *a32 = reinterpret_cast<float *>(img + off_a32);
    for (int64_t i = t0; i < (int64_t)nbits * D; i += step) a32[i] = A[i];
    // fragments: one (slab, k step, lane) per thread
    for (int64_t i = t0; i < (int64_t)W * KS * 64; i += step) {
        const int lane = (int)(i & 63), s = (int)((i >> 6) % KS), jt = (int)((i >> 6) / KS);
        const int r = lane & 31, h = lane >> 5;
        const float *row = A + (size_t)(jt * 32 + r) * D + 16 * s + 4 * h;
        bf16x8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float a = row[8 * (e >> 2) + (e & 3)];
            hi[e] = (__bf16)a;
            lo[e] = (__bf16)(a - (float)hi[e]);
        }
        bf16x8 *dst = reinterpret_cast<bf16x8 *>(img + off_slabs + (size_t)jt * slab_f4(KS) * 16);
        dst[(2 * s) * 64 + lane] = hi;
        dst[(2 * s + 1) * 64 + lane] = lo;
    }
    // na_j: sqrt of the fp64 sum of squares, inflated by (1 + 2^-10); +inf where the filter must not be trusted
    for (int64_t j = t0; j < nbits; j += step) {
        double ss = 0.0;
        for (int k = 0; k < D; ++k) {
            const double a = (double)A[(size_t)j * D + k];
            ss += a * a;
        }
        const double nrm = sqrt(ss);
        float na = __builtin_inff();
        if (nrm >= 0x1p-30 && nrm <= 0x1p30) na = (float)(nrm * (1.0 + 0x1p-10));
        float *dst = reinterpret_cast<float *>(img + off_slabs + ((size_t)(j / 32) * slab_f4(KS) + KS * 128) * 16);
        dst[j % 32] = na;
    }
}

struct FilterArgs {
    const float *x;
    int64_t N;
    const float *a32;
    const f32x4 *slabs;
    int nbits;
    uint32_t *codes;
    unsigned long long *counters;       // nullptr: no statistics
    float c;
};

template <int KS, int JS>
__global__ __launch_bounds__(256, JS == 1 ? 2 : 1) void lsh_filter_kernel(const FilterArgs g) {
    constexpr int D = KS * 16, ROWS = 128 / JS, RG = 4 / JS, SF4 = slab_f4(KS), NQ = KS / 2;
    extern __shared__ f32x4 lds[];
    __shared__ uint32_t cnt, more;
    const int W = g.nbits / 32;
    f32x4 *slabL = lds;                                                       // JS slabs
    uint32_t *codesL = reinterpret_cast<uint32_t *>(lds + JS * SF4);           // [W][ROWS] sign words
    uint32_t *flagsL = codesL + W * ROWS;                                      // [W][ROWS] flag words
    uint32_t *listL = flagsL + W * ROWS;                                       // [LIST_CAP]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int rg = wave % RG, ph = wave / RG;
    const int64_t row0 = (int64_t)blockIdx.x * ROWS;
    const int64_t row = row0 + rg * 32 + r;
    const bool live = row < g.N;

    LSHF_STAMP(0);
    // ---- this lane's half of its row: fp32 -> (hi, lo) fragments, sum of squares
    bf16x8 xh[KS], xl[KS];
    float ss = 0.f;
    {
        const float4 *xr = reinterpret_cast<const float4 *>(g.x + (live ? row : 0) * D);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                float4 v = xr[4 * s + 2 * t + h];
                if (!live) v = make_float4(0.f, 0.f, 0.f, 0.f);
                const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const __bf16 hi = (__bf16)e[q];
                    xh[s][4 * t + q] = hi;
                    xl[s][4 * t + q] = (__bf16)(e[q] - (float)hi);
                    ss = fmaf(e[q], e[q], ss);
                }
            }
        }
    }
    ss += __shfl_xor(ss, 32);
    float thr = __builtin_inff();                                              // c * nx_i
    if (ss >= 0x1p-60f && ss <= 0x1p60f) thr = g.c * (sqrtf(ss) * (1.f + 0x1p-10f));

    // ---- slabs: prefetch (registers) -> LDS -> MFMA
    const int iters = (W + JS - 1) / JS;
    f32x4 pre[JS][NQ], pna[JS];
#define LSHF_PREFETCH(it_)                                                             \
    _Pragma("unroll") for (int sl = 0; sl < JS; ++sl) {                                \
        const int jt_ = (it_) * JS + sl;                                                \
        if (jt_ < W) {                                                                  \
            const f32x4 *src = g.slabs + (size_t)jt_ * SF4;                            \
            _Pragma("unroll") for (int q = 0; q < NQ; ++q) pre[sl][q] = src[tid + 256 * q]; \
            if (tid < 8) pna[sl] = src[KS * 128 + tid];                                 \
        }                                                                               \
    }
    LSHF_PREFETCH(0)
    LSHF_STAMP(1);
    [[maybe_unused]] unsigned long long t_stage = 0ull, t_mfma = 0ull, t_epi = 0ull;    // PS_LSHF_DEBUG == 2 only
    for (int it = 0; it < iters; ++it) {
        const unsigned long long c0 = LSHF_NOW();
        __syncthreads();                                                       // the previous slab's readers are done
#pragma unroll
        for (int sl = 0; sl < JS; ++sl) {
            if (it * JS + sl < W) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) slabL[sl * SF4 + tid + 256 * q] = pre[sl][q];
                if (tid < 8) slabL[sl * SF4 + KS * 128 + tid] = pna[sl];
            }
        }
        __syncthreads();
        const unsigned long long c1 = LSHF_NOW();
        t_stage += c1 - c0;
        if (it + 1 < iters) { LSHF_PREFETCH(it + 1) }
        const int jt = it * JS + ph;
        if (jt < W) {                                                          // wave-uniform
            const f32x4 *sb = slabL + ph * SF4;
            // two accumulators, even and odd k steps: a lone wave on its SIMD (64-row tiles) issues a dependent MFMA only every
            // 58 cycles, not 32
            f32x16 acc, acc1;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = acc1[e] = 0.f;
            // the fragments of k step s + 2 are requested before the MFMAs of step s (left to itself the compiler reads each
            // pair right in front of its MFMAs and waits out the LDS latency 2 KS times per slab: 5.5 k cycles against 1.5 k)
            f32x4 fh[3], fl[3];
            fh[0] = sb[lane];
            fl[0] = sb[64 + lane];
            if (KS > 1) {
                fh[1] = sb[2 * 64 + lane];
                fl[1] = sb[3 * 64 + lane];
            }
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                if (s + 2 < KS) {
                    fh[(s + 2) % 3] = sb[(2 * s + 4) * 64 + lane];
                    fl[(s + 2) % 3] = sb[(2 * s + 5) * 64 + lane];
                }
                __builtin_amdgcn_sched_barrier(0);
                const bf16x8 ah = __builtin_bit_cast(bf16x8, fh[s % 3]), al = __builtin_bit_cast(bf16x8, fl[s % 3]);
                if (s % 2 == 0) {
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, xh[s], acc, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, xl[s], acc1, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, xh[s], acc, 0, 0, 0);
                } else {
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, xh[s], acc1, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, xl[s], acc, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, xh[s], acc1, 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            acc += acc1;
            const unsigned long long c2 = LSHF_NOW();
            t_mfma += c2 - c1;
            // register e of lane (r, h) = dot(x row r, rotation row 8 (e >> 2) + 4 h + (e & 3))
            uint32_t sm = 0u, fm = 0u;
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const f32x4 na = sb[KS * 128 + 2 * gq + h];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float f = acc[4 * gq + q];
#if PS_LSHF_DEBUG == 1
                    if (ps_lshf_dump_buf != nullptr && live) ps_lshf_dump_buf[row * g.nbits + jt * 32 + 8 * gq + 4 * h + q] = f;
#endif
                    const bool trusted = __builtin_fabsf(f) > thr * na[q];
                    sm |= (trusted && f >= 0.f ? 1u : 0u) << (8 * gq + q);
                    fm |= (trusted ? 0u : 1u) << (8 * gq + q);
                }
            }
            sm <<= 4 * h;
            fm <<= 4 * h;
            if (!live) fm = 0u;                                                // rows past N: no chain, nothing stored
            sm |= (uint32_t)__shfl_xor((int)sm, 32);
            fm |= (uint32_t)__shfl_xor((int)fm, 32);
            if (h == 0) {
                codesL[jt * ROWS + rg * 32 + r] = sm;
                flagsL[jt * ROWS + rg * 32 + r] = fm;
            }
            t_epi += LSHF_NOW() - c2;
        }
    }

#undef LSHF_PREFETCH
    LSHF_STAMP(2);
    LSHF_PUT(6, t_stage);
    LSHF_PUT(7, t_mfma);
    LSHF_PUT(8, t_epi);

    // ---- the flagged dots: compact up to LIST_CAP of them, run their chains, repeat until no flag is left
    const int nwords = W * ROWS;
    unsigned long long nflag = 0ull;
    for (;;) {
        __syncthreads();
        if (tid == 0) {
            cnt = 0u;
            more = 0u;
        }
        __syncthreads();
        // a thread counts the flags of its words, reserves that many list slots with ONE atomic and fills those below LIST_CAP;
        // flags that found no slot stay set for the next round
        int mine = 0;
#pragma unroll 4
        for (int idx = tid; idx < nwords; idx += 256) mine += __builtin_popcount(flagsL[idx]);
        if (mine > 0) {
            uint32_t pos = atomicAdd(&cnt, (uint32_t)mine);
            if (pos + (uint32_t)mine > (uint32_t)LIST_CAP) more = 1u;
            for (int idx = tid; idx < nwords && pos < (uint32_t)LIST_CAP; idx += 256) {
                uint32_t m = flagsL[idx];
                if (m == 0u) continue;
                while (m != 0u && pos < (uint32_t)LIST_CAP) {
                    listL[pos++] = (uint32_t)idx * 32u + (uint32_t)__builtin_ctz(m);
                    m &= m - 1u;
                }
                flagsL[idx] = m;
            }
        }
        __syncthreads();
        LSHF_STAMP(3);
        const int n = cnt < (uint32_t)LIST_CAP ? (int)cnt : LIST_CAP;
        const bool again = more != 0u;
        for (int e = tid; e < n; e += 256) {
            const uint32_t ent = listL[e];
            const int idx = (int)(ent >> 5), b = (int)(ent & 31u);
            const int jt = idx / ROWS, rl = idx % ROWS;
            const float4 *xr = reinterpret_cast<const float4 *>(g.x + (row0 + rl) * D);
            const float4 *ar = reinterpret_cast<const float4 *>(g.a32 + (size_t)(jt * 32 + b) * D);
            float acc = 0.f;
#pragma unroll 16
            for (int k = 0; k < D / 4; ++k) {
                const float4 u = xr[k], v = ar[k];
                acc = fmaf(u.x, v.x, acc);
                acc = fmaf(u.y, v.y, acc);
                acc = fmaf(u.z, v.z, acc);
                acc = fmaf(u.w, v.w, acc);
            }
            if (acc >= 0.f) atomicOr(&codesL[idx], 1u << b);
        }
        nflag += (unsigned long long)n;
        if (!again) break;
    }
    __syncthreads();
    LSHF_STAMP(4);

    // ---- codes of the tile's rows, LSB first
    for (int i = tid; i < nwords; i += 256) {
        const int rl = i / W, w = i % W;
        if (row0 + rl < g.N) g.codes[(row0 + rl) * W + w] = codesL[w * ROWS + rl];
    }
    if (g.counters != nullptr && tid == 0) {
        const int64_t rows = g.N - row0 < ROWS ? g.N - row0 : ROWS;
        atomicAdd(g.counters, (unsigned long long)rows * (unsigned long long)g.nbits);
        atomicAdd(g.counters + 1, nflag);
    }
    LSHF_STAMP(5);
}

template <int KS, int JS>
size_t filter_lds(int nbits) {
    return (size_t)JS * slab_f4(KS) * 16 + (size_t)(nbits / 32) * (128 / JS) * 8 + (size_t)LIST_CAP * 4;
}

template <int KS, int JS>
int launch_filter(const FilterArgs &g, hipStream_t st) {
    const int64_t grid = ps_cdiv(g.N, 128 / JS);
    if (grid > 0x7fffffff) return PS_EUNSUPPORTED;
    const size_t lds = filter_lds<KS, JS>(g.nbits);
    hipLaunchKernelGGL((lsh_filter_kernel<KS, JS>), dim3((unsigned)grid), dim3(256), lds, st, g);
    PS_CHECK_LAUNCH();
    return PS_OK;
}

template <int KS, int JS>
bool allow_lds() {
    return ps_allow_lds(lsh_filter_kernel<KS, JS>, filter_lds<KS, JS>(MAX_NBITS));
}

}  // namespace

extern "C" size_t ps_lsh_stage_bytes(int nbits, int D) { return served(nbits, D) ? stage_layout(nbits, D).total : 0; }

extern "C" int ps_lsh_stage(const float *A, int nbits, int D, void *staged, size_t staged_bytes, ps_stream_t stream) {
    if (nbits <= 0 || D <= 0 || !A || !staged) return PS_EINVAL;
    if (!served(nbits, D) || (reinterpret_cast<size_t>(A) | reinterpret_cast<size_t>(staged)) % 16 != 0) return PS_EUNSUPPORTED;
    const StageLayout l = stage_layout(nbits, D);
    if (staged_bytes < l.total) return PS_EINVAL;
    int64_t grid = ps_cdiv((int64_t)nbits * D, 256);
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(lsh_stage_kernel, dim3((unsigned)grid), dim3(256), 0, ps_stream(stream), A, nbits, D,
                       static_cast<unsigned char *>(staged), l.a32, l.slabs);
    PS_CHECK_LAUNCH();
    return PS_OK;
}

// ps_lsh_encode with PS_LSH_STAGED (csrc/dense_mfma.hip checks N, D, nbits, the pointers and the flag combination)
int psi_lsh_encode_staged(const float *x, int64_t N, int D, const void *staged, int nbits, uint8_t *codes, ps_stream_t stream) {
    if (!served(nbits, D) || (reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(staged)) % 16 != 0) return PS_EUNSUPPORTED;
    static PsPerDevice cus;                                                    // attributes set, CU count known
    int dv = 0;
    if (!ps_device_index(&dv)) return PS_ELAUNCH;
    int ncu = cus.get(dv);
    if (ncu == 0) {
        if (!(allow_lds<2, 1>() && allow_lds<4, 1>() && allow_lds<8, 1>() && allow_lds<16, 1>() && allow_lds<2, 2>() &&
              allow_lds<4, 2>() && allow_lds<8, 2>() && allow_lds<16, 2>()))
            return PS_ELAUNCH;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dv) != hipSuccess || ncu <= 0) return PS_ELAUNCH;
        cus.set(dv, ncu);
    }
    const StageLayout l = stage_layout(nbits, D);
    const unsigned char *img = static_cast<const unsigned char *>(staged);
    const char *se = getenv("PS_LSH_STATS"), *re = getenv("PS_LSH_ROWS");
    FilterArgs g;
    g.x = x;
    g.N = N;
    g.a32 = reinterpret_cast<const float *>(img + l.a32);
    g.slabs = reinterpret_cast<const f32x4 *>(img + l.slabs);
    g.nbits = nbits;
    g.codes = reinterpret_cast<uint32_t *>(codes);
    g.counters = se && atoi(se) != 0 ? reinterpret_cast<unsigned long long *>(const_cast<unsigned char *>(img) + 16) : nullptr;
    g.c = 0x1p-12f * (D > 256 ? (float)D / 256.f : 1.f);
    // 64-row tiles while 128-row tiles would leave half the CUs without one: twice the workgroups, each half as long.
    // PS_LSH_ROWS=64 / 128 forces a tile (tests run both)
    const int rows = re ? atoi(re) : 0;
    const bool half = rows == 64 || (rows != 128 && ps_cdiv(N, 128) * 2 <= ncu);
    hipStream_t st = ps_stream(stream);
    switch (D / 16) {
        case 2: return half ? launch_filter<2, 2>(g, st) : launch_filter<2, 1>(g, st);
        case 4: return half ? launch_filter<4, 2>(g, st) : launch_filter<4, 1>(g, st);
        case 8: return half ? launch_filter<8, 2>(g, st) : launch_filter<8, 1>(g, st);
        default: return half ? launch_filter<16, 2>(g, st) : launch_filter<16, 1>(g, st);
    }
}
