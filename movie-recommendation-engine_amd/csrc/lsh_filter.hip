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
// flag words collect in LDS, and every wave notes which of its flag words have a bit set; after the last slab the noted words
// become the list of flagged dots without a pass over all flag words, and all 256 threads drain it (128-row tiles: operands
// through LDS in coalesced pieces of 16 k).  Scan rounds over the flag words follow only while flags are left (the list's size
// bounds a round, never the number of flagged dots).  ps_lsh_encode_planes also writes the sign planes of the tile's rows
// (csrc/hamming_mfma.hip: ps_lsh_expand) from the words in LDS.
#include "ps_common.h"
#include "lsh_planes.h"

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
    uint4 *planes;                      // nullptr: codes only; else the sign planes of the codes (layout: csrc/hamming_mfma.hip)
    int64_t plane_pieces;               // 16-byte pieces of the plane table, padding tiles included
};

// float4s of the first LDS area: the slabs of an iteration during the sweep; in the 128-row form (JS = 1) then the piece
// buffer of the chains, 256 entries x 2 operands x 64 bytes = 32 KiB whatever D is, so the area is at least that there (D < 256:
// the slab alone is smaller).  The 64-row form has no piece buffer and keeps its two slabs.
__host__ __device__ constexpr int area_f4(int KS, int JS) {
    return JS == 1 && slab_f4(KS) < 2048 ? 2048 : JS * slab_f4(KS);
}

template <int KS, int JS>
__global__ __launch_bounds__(256, JS == 1 ? 2 : 1) void lsh_filter_kernel(const FilterArgs g) {
    constexpr int D = KS * 16, ROWS = 128 / JS, RG = 4 / JS, SF4 = slab_f4(KS), NQ = KS / 2;
    constexpr int PF = KS >= 16 ? 4 : 2;                                      // chain pieces in flight
    extern __shared__ f32x4 lds[];
    constexpr int SEG = LIST_CAP / 4;                                          // flagged words a wave notes during the sweep
    __shared__ uint32_t cnt, more, segn[4];
    const int W = g.nbits / 32;
    f32x4 *slabL = lds;                                                       // JS slabs
    uint32_t *codesL = reinterpret_cast<uint32_t *>(lds + area_f4(KS, JS));    // [W][ROWS] sign words
    uint32_t *flagsL = codesL + W * ROWS;                                      // [W][ROWS] flag words
    uint32_t *listL = flagsL + W * ROWS;                                       // [LIST_CAP]
    uint16_t *wordL = reinterpret_cast<uint16_t *>(listL + LIST_CAP);          // [4][SEG] flag words with a bit set, per wave

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
    if (tid == 0) {                                                            // published by the barrier at the top of the sweep
        cnt = 0u;
        more = 0u;
    }
    int wcnt = 0;                                                              // flag words with a bit set, this wave (uniform)
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
            // a word with a flag set is noted as it is found, in the wave's own run of wordL and counted in a register: a
            // handful of instructions per slab, no atomic, nothing to wait for (the sweep is bound by instruction issue, and
            // an LDS round trip in front of its barriers costs more than the scan it saves).  Words beyond the run stay for
            // the scan rounds after the sweep.
            const bool fw = h == 0 && fm != 0u;
            const unsigned long long wm = __ballot(fw);
            if (fw) {
                const int at = wcnt + (int)__builtin_amdgcn_mbcnt_lo((uint32_t)wm, 0u);
                if (at < SEG) wordL[wave * SEG + at] = (uint16_t)(jt * ROWS + rg * 32 + r);
                else more = 1u;
            }
            wcnt += __builtin_popcountll(wm);
            if (h == 0) {
                codesL[jt * ROWS + rg * 32 + r] = sm;
                flagsL[jt * ROWS + rg * 32 + r] = fm;
            }
            t_epi += LSHF_NOW() - c2;
        }
    }

#undef LSHF_PREFETCH
    if (lane == 0) segn[wave] = (uint32_t)(wcnt < SEG ? wcnt : SEG);
    LSHF_STAMP(2);
    LSHF_PUT(6, t_stage);
    LSHF_PUT(7, t_mfma);
    LSHF_PUT(8, t_epi);

    // ---- the flagged dots.  The sweep has noted the words that hold them: one thread per noted word lists its first flag at
    // the word's own place in the list (no reservation) and, rarely, appends further ones behind all first flags with an atomic.
    // Their chains run now; only if a wave noted more words than its run takes, or the list more dots than LIST_CAP, do scan
    // rounds over all flag words follow, until no flag is left.
    //
    // A round of chains takes 256 list entries, one per thread, and moves the operands in pieces of 16 consecutive k: four
    // adjacent lanes load the four float4s of ONE entry's x piece (then of its A piece), so a wave load touches 16 runs of
    // 64 bytes and not 64 cache lines; the pieces pass through LDS (the slab area, dead by now) to the thread that owns the
    // chain, which runs acc = fmaf(x[k], A[j][k], acc) in k order as before.  PF pieces are in flight ahead of the fmas.
    // Entry e keeps float4 q of a piece at 4 e + (q ^ ((e >> 2) & 3)): conflict-free for the loaders' stores and for the
    // owners' reads.  Slots past the round's last entry repeat its first one: no address outside the listed rows is formed,
    // and the loads stay unconditional, so that the compiler counts them (vmcnt) and a store waits for its own piece only.
    // The 64-row form (JS = 2) keeps one thread per chain reading its own rows: a tile has about a hundred flagged dots
    // there, on a CU that holds no second workgroup, and its chains phase measured shorter that way.
    const int nwords = W * ROWS;
    const f32x4 *xb = reinterpret_cast<const f32x4 *>(g.x + row0 * D), *ab = reinterpret_cast<const f32x4 *>(g.a32);
    f32x4 *pieceL = lds;
    unsigned long long nflag = 0ull;
    __syncthreads();
    const int s1 = (int)segn[0], s2 = s1 + (int)segn[1], s3 = s2 + (int)segn[2];   // where the runs of waves 1, 2, 3 begin
    const int nw = s3 + (int)segn[3];
    for (int e = tid; e < nw; e += 256) {
        const int w = (e >= s1 ? 1 : 0) + (e >= s2 ? 1 : 0) + (e >= s3 ? 1 : 0);
        const uint32_t idx = wordL[w * SEG + e - (w == 3 ? s3 : w == 2 ? s2 : w == 1 ? s1 : 0)];
        uint32_t m = flagsL[idx];
        listL[e] = idx * 32u + (uint32_t)__builtin_ctz(m);
        m &= m - 1u;
        if (m != 0u) {
            uint32_t pos = (uint32_t)nw + atomicAdd(&cnt, (uint32_t)__builtin_popcount(m));
            while (m != 0u && pos < (uint32_t)LIST_CAP) {
                listL[pos++] = idx * 32u + (uint32_t)__builtin_ctz(m);
                m &= m - 1u;
            }
            if (m != 0u) more = 1u;
        }
        flagsL[idx] = m;
    }
    __syncthreads();
    int n = (uint32_t)nw + cnt < (uint32_t)LIST_CAP ? nw + (int)cnt : LIST_CAP;
    bool again = more != 0u;
    LSHF_STAMP(3);
    for (;;) {
        if constexpr (JS == 2) {
            for (int e = tid; e < n; e += 256) {
                const uint32_t ent = listL[e];
                const int idx = (int)(ent >> 5), b = (int)(ent & 31u);
                const f32x4 *xr = xb + (idx % ROWS) * (D / 4), *ar = ab + ((idx / ROWS) * 32 + b) * (D / 4);
                float acc = 0.f;
#pragma unroll 16
                for (int k = 0; k < D / 4; ++k) {
                    const f32x4 u = xr[k], v = ar[k];
                    acc = fmaf(u[0], v[0], acc);
                    acc = fmaf(u[1], v[1], acc);
                    acc = fmaf(u[2], v[2], acc);
                    acc = fmaf(u[3], v[3], acc);
                }
                if (acc >= 0.f) atomicOr(&codesL[idx], 1u << b);
            }
        }
        for (int base = 0; JS == 1 && base < n; base += 256) {
            const int m = n - base < 256 ? n - base : 256;
            const int q = tid & 3, sw = (tid >> 4) & 3;
            int xo[4], ao[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int el = 64 * i + (tid >> 2);
                const uint32_t ent = listL[base + (el < m ? el : 0)];
                const int idx = (int)(ent >> 5), b = (int)(ent & 31u);
                xo[i] = (idx % ROWS) * (D / 4) + q;
                ao[i] = ((idx / ROWS) * 32 + b) * (D / 4) + q;
            }
            const uint32_t mine = listL[base + (tid < m ? tid : 0)];
            f32x4 px[PF][4], pa[PF][4];
#pragma unroll
            for (int p = 0; p < PF; ++p) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    px[p][i] = xb[xo[i] + 4 * p];
                    pa[p][i] = ab[ao[i] + 4 * p];
                }
            }
            float acc = 0.f;
#pragma unroll
            for (int p = 0; p < KS; ++p) {
                __syncthreads();                                               // the piece before (the slabs, the last round) is read
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int at = (64 * i + (tid >> 2)) * 4 + (q ^ sw);
                    pieceL[at] = px[p % PF][i];
                    pieceL[1024 + at] = pa[p % PF][i];
                }
                __syncthreads();
                if (p + PF < KS) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        px[p % PF][i] = xb[xo[i] + 4 * (p + PF)];
                        pa[p % PF][i] = ab[ao[i] + 4 * (p + PF)];
                    }
                }
                if (tid < m) {
                    const int so = (tid >> 2) & 3;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const f32x4 u = pieceL[tid * 4 + (j ^ so)], v = pieceL[1024 + tid * 4 + (j ^ so)];
                        acc = fmaf(u[0], v[0], acc);
                        acc = fmaf(u[1], v[1], acc);
                        acc = fmaf(u[2], v[2], acc);
                        acc = fmaf(u[3], v[3], acc);
                    }
                }
            }
            if (tid < m && acc >= 0.f) atomicOr(&codesL[mine >> 5], 1u << (mine & 31u));
        }
        nflag += (unsigned long long)n;
        if (!again) break;
        __syncthreads();                                                       // the list, cnt and more are read
        if (tid == 0) {
            cnt = 0u;
            more = 0u;
        }
        __syncthreads();
        // a thread counts the flags of its words, reserves that many list slots with ONE atomic and fills those below LIST_CAP;
        // flags that found no slot stay set for the next round
        int own = 0;
#pragma unroll 4
        for (int idx = tid; idx < nwords; idx += 256) own += __builtin_popcount(flagsL[idx]);
        if (own > 0) {
            uint32_t pos = atomicAdd(&cnt, (uint32_t)own);
            if (pos + (uint32_t)own > (uint32_t)LIST_CAP) more = 1u;
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
        n = cnt < (uint32_t)LIST_CAP ? (int)cnt : LIST_CAP;
        again = more != 0u;
    }
    __syncthreads();
    LSHF_STAMP(4);

    // ---- codes of the tile's rows, LSB first
    for (int i = tid; i < nwords; i += 256) {
        const int rl = i / W, w = i % W;
        if (row0 + rl < g.N) g.codes[(row0 + rl) * W + w] = codesL[w * ROWS + rl];
    }
    // ---- and their sign planes: piece (tile * W / 2 + s) * 64 + lane = word 2 s + (lane >> 5) of row 32 tile + (lane & 31),
    // zero for rows past N; the last workgroup also zeroes the padding tiles behind the last tile of the grid
    if (g.planes != nullptr) {
        const int KP = W / 2;
        const int64_t first = (int64_t)blockIdx.x * (ROWS / 32) * KP * 64;
        for (int i = tid; i < nwords; i += 256) {
            const int ln = i & 63, ts = i >> 6;
            const int rl = (ts / KP) * 32 + (ln & 31), w = 2 * (ts % KP) + (ln >> 5);
            uint4 o = make_uint4(0u, 0u, 0u, 0u);
            if (row0 + rl < g.N) o = expand_word(codesL[w * ROWS + rl]);
            if (first + i < g.plane_pieces) g.planes[first + i] = o;
        }
        if (blockIdx.x == gridDim.x - 1)
            for (int64_t i = first + nwords + tid; i < g.plane_pieces; i += 256) g.planes[i] = make_uint4(0u, 0u, 0u, 0u);
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
    return (size_t)area_f4(KS, JS) * 16 + (size_t)(nbits / 32) * (128 / JS) * 8 + (size_t)LIST_CAP * 4 + (size_t)LIST_CAP * 2;
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
static int encode_staged(const float *x, int64_t N, int D, const void *staged, int nbits, uint8_t *codes, void *planes,
                         size_t planes_bytes, ps_stream_t stream) {
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
    g.planes = static_cast<uint4 *>(planes);
    g.plane_pieces = (int64_t)(planes_bytes / 16);
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

int psi_lsh_encode_staged(const float *x, int64_t N, int D, const void *staged, int nbits, uint8_t *codes, ps_stream_t stream) {
    return encode_staged(x, N, D, staged, nbits, codes, nullptr, 0, stream);
}

// the staged ps_lsh_encode and ps_lsh_expand of its codes in one launch: a workgroup writes the planes of its rows from the
// sign words it still holds in LDS
extern "C" int ps_lsh_encode_planes(const float *x, int64_t N, int D, const void *staged, int nbits, uint8_t *codes, void *planes,
                                    ps_stream_t stream) {
    if (N < 0 || D <= 0 || nbits <= 0 || !x || !staged || !codes || !planes) return PS_EINVAL;
    const size_t planes_bytes = ps_lsh_planes_bytes(N, nbits / 8);
    if (planes_bytes == 0 || nbits % 64 != 0 || !served(nbits, D)) return PS_EUNSUPPORTED;
    if (reinterpret_cast<size_t>(codes) % 4 != 0 || reinterpret_cast<size_t>(planes) % 16 != 0) return PS_EUNSUPPORTED;
    return encode_staged(x, N, D, staged, nbits, codes, planes, planes_bytes, stream);
}
