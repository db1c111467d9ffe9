// walk_biased.hip -- node2vec-biased random walks on gfx950.
//
// ps_walk_paths_biased is ps_walk_paths (csrc/walk_sample.hip) with the second-order bias of RandomWalkSampler's p / q: on every
// step that has a previous node t, the weights of the row the walk stands on are multiplied by alpha before
// np.random.choice(dest, p = w / w.sum()) sees them -- 1/p for the edge back to t, 1 for a destination t has an out-edge to,
// 1/q for the rest (include/pinsage_hip.h).  The row's CDF then depends on t, so nothing can be precomputed per row: a step costs
// O(deg) and, numpy's cumsum being a sequential chain, O(deg) of it is sequential.  One wave owns one walk and shares that work:
//   1. lanes compute w * alpha 64 edges at a time (the membership test is a binary search in t's sorted row), into LDS for rows
//      of up to WB_CAP edges, and again for every pass over longer rows (no spill to global memory);
//   2. S = numpy's pairwise sum of w * alpha: its tree is walked leaf by leaf (<= 128 consecutive values), the eight running
//      sums of a leaf in eight lanes;
//   3. cumsum(w * alpha / S): the divisions 64 at a time over the lanes, the chain by every lane from LDS; the accumulator at
//      the end of every 64-edge chunk is kept, `last` is the accumulator at the end of the row;
//   4. the pick, searchsorted(cdf / last, u, 'right'): the first chunk whose kept accumulator / last exceeds u is found by
//      ballot (the CDF is non-decreasing), its chain is replayed with lane j keeping entry j, and a second ballot gives the edge.
// This file is compiled without FMA contraction (csrc/Makefile), like csr_build.hip: every product, sum and quotient is
// rounded once, as numpy rounds it.
// The per-step uniform (csrc/walk_rng.h) and the first step's search of the row's own CDF (csrc/walk_search.h) are the copies
// ps_walk_paths uses.  The visits of the paths are counted by ps_paths_topk (csrc/walk_topk.hip).
#include "ps_common.h"
#include "walk_rng.h"
#include "walk_search.h"

namespace {

constexpr int WB_CAP = 1024;        // rows of up to this many edges keep their w * alpha in LDS between the passes
constexpr int CEND_CAP = 128;       // chunk-end accumulators kept (rows of up to 8192 edges; beyond, the chain is replayed from the last one kept)

struct BiasedArgs {
    const int64_t *rowptr;
    const int32_t *col;
    const double *w;
    const double *cdf;
    const int32_t *nbr;
    int64_t V;
    const int64_t *starts;
    int64_t B;
    int L, rng_mode;
    const double *uniforms;
    const int64_t *uoff;
    uint32_t k0, k1, call;
    int walk_mod;
    const double *bias;
    int32_t *paths;
};

// (row start, row end) of node v; an id or an offset outside the graph gives an empty row and nothing of it is read
__device__ __forceinline__ void safe_row(const int64_t *rowptr, int64_t V, int64_t E, int64_t v, int64_t &lo, int64_t &hi) {
    lo = hi = 0;
    if (v < 0 || v >= V) return;
    const int64_t a = rowptr[v], b = rowptr[v + 1];
    if (a < 0 || b > E || b < a) return;
    lo = a;
    hi = b;
}

// numpy's pairwise leaf (n <= 128) over LDS: the eight running sums r0 .. r7 live in lanes l % 8 == 0 .. 7
__device__ __forceinline__ double leaf_sum(const double *a, int n, int lane) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    const int k = lane & 7;
    double r = a[k];
    int i;
    for (i = 8; i < n - (n % 8); i += 8) r += a[i + k];
    const double r0 = __shfl(r, 0, 64), r1 = __shfl(r, 1, 64), r2 = __shfl(r, 2, 64), r3 = __shfl(r, 3, 64);
    const double r4 = __shfl(r, 4, 64), r5 = __shfl(r, 5, 64), r6 = __shfl(r, 6, 64), r7 = __shfl(r, 7, 64);
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += a[i];
    return res;
}

struct PairwiseStack {          // LDS
    double left[10];
    int off[10], len[10], phase[10];
};

// One biased row of one walk: the wave's view of it
struct BiasedRow {
    const BiasedArgs &a;
    int64_t lo;                 // start of the row the walk stands on
    int64_t tlo, tn;            // the previous node's row of sorted destinations
    int32_t t;
    double inv_p, inv_q;
    double *wbuf;               // LDS [WB_CAP]
    bool cached;
    int lane;

    // w * alpha of edges lo + off .. lo + off + cnt - 1 -> dst[0 .. cnt)
    __device__ __forceinline__ void fill(int64_t off, int cnt, double *dst) const {
        for (int k = lane; k < cnt; k += 64) {
            const int64_t e = lo + off + k;
            const int32_t x = a.col[e];
            double al = inv_p;
            if (x != t) {
                int64_t l = 0, h = tn;
                while (l < h) {
                    const int64_t mid = l + ((h - l) >> 1);
                    if (a.nbr[tlo + mid] < x) l = mid + 1; else h = mid;
                }
                al = (l < tn && a.nbr[tlo + l] == x) ? 1.0 : inv_q;
            }
            dst[k] = a.w[e] * al;
        }
    }
    // the values off .. off + cnt - 1 (cnt <= 128) in LDS
    __device__ __forceinline__ const double *stage(int64_t off, int cnt) const {
        if (cached) return wbuf + off;
        ps_wave_lds_sync();                 // earlier readers of wbuf are done
        fill(off, cnt, wbuf);
        ps_wave_lds_sync();
        return wbuf;
    }
    // numpy's pairwise sum of one ufunc buffer (m <= 8192 values from `base` on): the tree of csr_build.hip's pairwise_block.  Its
    // stack (depth <= 7) lives in LDS: every lane writes and reads the same values, so no lane waits for another, and the
    // registers that dynamically indexed arrays would be spread over stay free (the kernel takes 53 VGPRs).
    __device__ double block_sum(int64_t base, int m, PairwiseStack &s) const {
        int sp = 0;
        s.off[0] = 0; s.len[0] = m; s.phase[0] = 0;
        double ret = 0.0;
        while (sp >= 0) {
            const int off = s.off[sp], len = s.len[sp], phase = s.phase[sp];
            if (phase == 0) {
                if (len <= 128) { ret = leaf_sum(stage(base + off, len), len, lane); --sp; continue; }
                int n2 = len / 2; n2 -= n2 % 8;
                s.phase[sp] = 1;
                s.off[sp + 1] = off; s.len[sp + 1] = n2; s.phase[sp + 1] = 0; ++sp;
            } else if (phase == 1) {
                s.left[sp] = ret;
                int n2 = len / 2; n2 -= n2 % 8;
                s.phase[sp] = 2;
                s.off[sp + 1] = off + n2; s.len[sp + 1] = len - n2; s.phase[sp + 1] = 0; ++sp;
            } else {
                ret = s.left[sp] + ret;
                --sp;
            }
        }
        return ret;
    }
};

// One wave per walk, one workgroup per wave.  Every branch below is wave-uniform: s, the uniforms and the picks are the same in
// all lanes.
__global__ __launch_bounds__(64) void walk_paths_biased_kernel(BiasedArgs a) {
    __shared__ double wbuf[WB_CAP];
    __shared__ double pbuf[64];
    __shared__ double cend[CEND_CAP];
    __shared__ PairwiseStack stack;
    const int lane = threadIdx.x;
    const int64_t E = a.rowptr[a.V];
    const double inv_p = a.bias[0], inv_q = a.bias[1];
    const bool bias_ok = isfinite(inv_p) && isfinite(inv_q) && inv_p > 0.0 && inv_q > 0.0;     // else: no walk moves
    for (int64_t i = blockIdx.x; i < a.B; i += gridDim.x) {
        const int64_t s = a.starts[i];
        int64_t cur = s;
        int32_t prev = -1;
        bool alive = bias_ok && s >= 0 && s < a.V;
        const int64_t ubase = (a.rng_mode == PS_RNG_STREAM) ? a.uoff[i] : 0;
        for (int st = 0; st < a.L; ++st) {
            int32_t nxt = -1;
            int64_t lo = 0, hi = 0;
            if (alive) safe_row(a.rowptr, a.V, E, cur, lo, hi);
            if (hi == lo) alive = false;                      // sink: the walk stops, no uniform is consumed
            if (alive) {
                const double u = walk_step_uniform(a.rng_mode, a.uniforms, ubase, a.k0, a.k1, a.call, a.walk_mod, s, i, st);
                const int64_t n = hi - lo;
                int64_t pick = n - 1;
                if (st == 0) {                                // no previous node: the row's own CDF (no guide in this ABI)
                    pick = cdf_search<int64_t>(a.cdf, nullptr, lo, hi, u) - lo;
                } else {
                    int64_t tlo, thi;
                    safe_row(a.rowptr, a.V, E, prev, tlo, thi);
                    const BiasedRow row{a, lo, tlo, thi - tlo, prev, inv_p, inv_q, wbuf, n <= WB_CAP, lane};
                    ps_wave_lds_sync();                       // the previous step's readers of the LDS buffers are done
                    if (row.cached) {
                        row.fill(0, (int)n, wbuf);
                        ps_wave_lds_sync();
                    }
                    double S = 0.0;                           // numpy's sum: ufunc buffers of 8192 values, added in order
                    for (int64_t b0 = 0; b0 < n; b0 += 8192) S += row.block_sum(b0, (int)(n - b0 < 8192 ? n - b0 : 8192), stack);
                    // cumsum(p), p = w * alpha / S; the accumulator after every chunk of 64 is kept
                    const int64_t nchunks = (n + 63) >> 6;
                    double acc = 0.0;
                    for (int64_t c = 0; c < nchunks; ++c) {
                        const int cnt = (int)(n - c * 64 < 64 ? n - c * 64 : 64);
                        const double *src = row.stage(c * 64, cnt);
                        if (lane < cnt) pbuf[lane] = ps_div_rn(src[lane], S);
                        ps_wave_lds_sync();
                        for (int k = 0; k < cnt; ++k) acc = (c == 0 && k == 0) ? pbuf[0] : acc + pbuf[k];
                        if (c < CEND_CAP && lane == 0) cend[c] = acc;
                        ps_wave_lds_sync();
                    }
                    const double last = acc;
                    // the first kept chunk whose last CDF entry exceeds u (the CDF is non-decreasing)
                    const int nst = (int)(nchunks < CEND_CAP ? nchunks : CEND_CAP);
                    int cf = nst;
                    for (int base = 0; base < nst && cf == nst; base += 64) {
                        const int c = base + lane;
                        const uint64_t m = __ballot(c < nst && ps_div_rn(cend[c], last) > u);
                        if (m != 0ull) cf = base + (int)__builtin_ctzll(m);
                    }
                    // replay that chunk's chain (and, beyond the kept accumulators, every further chunk), lane j keeping entry j
                    double carry = cf > 0 ? cend[cf - 1] : 0.0;
                    for (int64_t c = cf; c < nchunks; ++c) {
                        const int cnt = (int)(n - c * 64 < 64 ? n - c * 64 : 64);
                        const double *src = row.stage(c * 64, cnt);
                        ps_wave_lds_sync();
                        if (lane < cnt) pbuf[lane] = ps_div_rn(src[lane], S);
                        ps_wave_lds_sync();
                        double mine = 0.0;
                        for (int k = 0; k < cnt; ++k) {
                            carry = (c == 0 && k == 0) ? pbuf[0] : carry + pbuf[k];
                            if (k == lane) mine = carry;
                        }
                        const uint64_t m = __ballot(lane < cnt && ps_div_rn(mine, last) > u);
                        if (m != 0ull) { pick = c * 64 + (int64_t)__builtin_ctzll(m); break; }
                    }
                }
                nxt = a.col[lo + pick];
                prev = (int32_t)cur;
                cur = nxt;
            }
            if (lane == 0) a.paths[i * a.L + st] = nxt;
        }
    }
}

}  // namespace

extern "C" int ps_walk_paths_biased(const int64_t *rowptr, const int32_t *col, const double *wsorted, const double *cdf,
                                    const int32_t *nbr_sorted, int64_t V, const int64_t *starts, int64_t B, int L, int rng_mode,
                                    const double *uniforms, const int64_t *uoff, uint64_t seed, uint32_t call, int walk_mod,
                                    const double *bias, int32_t *paths, ps_stream_t stream) {
    if (B < 0 || L < 1 || V < 0) return PS_EINVAL;
    if (B == 0) return PS_OK;
    if (!rowptr || !col || !wsorted || !cdf || !nbr_sorted || !starts || !bias || !paths) return PS_EINVAL;
    if (rng_mode != PS_RNG_STREAM && rng_mode != PS_RNG_PHILOX) return PS_EINVAL;
    if (rng_mode == PS_RNG_STREAM && (!uniforms || !uoff)) return PS_EINVAL;
    const BiasedArgs a{rowptr, col, wsorted, cdf, nbr_sorted, V, starts, B, L, rng_mode, uniforms, uoff,
                       (uint32_t)seed, (uint32_t)(seed >> 32), call, walk_mod, bias, paths};
    const int64_t grid = B > 256 * 256 ? 256 * 256 : B;        // 256 CUs x 16 resident one-wave workgroups (LDS), 16 rounds deep
    hipLaunchKernelGGL(walk_paths_biased_kernel, dim3((unsigned)grid), dim3(64), 0, ps_stream(stream), a);
    PS_CHECK_LAUNCH();
    return PS_OK;
}
