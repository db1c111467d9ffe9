// ppr_push.hip -- personalized-PageRank neighbourhoods on gfx950: exact push sweeps + top-k.
//
// Replaces RandomWalkSampler.compute_ppr_matrix / precompute_top_neighbors (reference utils/random_walk.py:144-229).
// The reference runs, per source, `for node, res in enumerate(residual)` over the LIVE residual vector: a Gauss-Seidel
// sweep, a push to a larger id is seen in the same sweep, to a smaller id in the next one.  With
//   c_k(u)       = (1 - alpha) m  if the mass m of u in sweep k is > 0, else 0
//   share(u->v)  = w / sum(row u), the sum taken left to right
// the mass the reference sees at v in sweep k is the left-to-right fp64 sum
//   init(v, k) + sum_{u > v, ascending u} c_{k-1}(u) share(u->v) + sum_{u < v, ascending u} c_k(u) share(u->v)
// (init = 1 for v == source in sweep 0; a self-loop's push is wiped by the reset that follows it; multi-edges in adjacency
// order).  v needs only lower-numbered in-neighbours of the same sweep, so with level(v) = 1 + max level(u) over the
// in-neighbours u < v a sweep is one pull pass per level, and every (v, source) sum is independent of all others.  The
// in-edge rows arrive already in summation order (u > v ascending, then u < v ascending, self-loops dropped:
// pinsage_hip/ppr.py).  Every product and sum is one rounded fp64 operation (this tree is compiled with -ffp-contract=off) in
// exactly that order, so the scores are the reference's bit for bit; a row is never split across waves, because fp64 addition
// is not associative.
#include "ps_common.h"
#include <cstring>

namespace {

constexpr size_t ALIGN = 256;

// share[e] = w[e] / sum(row), python's sum(): left to right from 0 (utils/random_walk.py:184).  One lane per row: once per graph.
__global__ void shares_kernel(const int64_t *rowptr, const double *w, int64_t V, double *share) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
        const int64_t lo = rowptr[v], hi = rowptr[v + 1];
        double total = 0.0;
        for (int64_t e = lo; e < hi; ++e) total = total + w[e];
        for (int64_t e = lo; e < hi; ++e) share[e] = ps_div_rn(w[e], total);
    }
}

// ppr[source] = 1.0 (:165); column s of the node-major state belongs to sources[s]
__global__ void seed_kernel(const int64_t *sources, int64_t S, int64_t Sc, int64_t Vp, double *score) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int64_t src = sources[s];
    if (src >= 0 && src < Vp) score[src * Sc + s] = 1.0;
}

__device__ __forceinline__ double readlane_f64(double x, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}

struct PushArgs {
    const int64_t *in_rowptr;   // [V + 1]
    const int32_t *in_src;      // u of every in-edge, rows in summation order
    const double *in_share;
    const int32_t *nodes;       // the nodes of this level
    const int64_t *sources;     // [S]
    const double *c_prev;       // [Vp, Sc] what every node pushed in the sweep before
    double *c_cur;              // [Vp, Sc] what it pushes in this one
    const uint8_t *act_prev;    // [Vp, nslab] "some lane of this 64-source slab pushed something"
    uint8_t *act_cur;
    double *score;              // [Vp, Sc]
    int64_t V, Vp, S, Sc, n_nodes, n_extra;
    int nslab, first_sweep;
    double alpha, one_minus_alpha;
};

constexpr int AHEAD = 8;        // row loads in flight per wave; the additions stay in edge order

// One wave = one (node v, slab of 64 sources): lanes are sources.  SKIP: rows whose slab pushed nothing are not read (a +0.0
// addend changes no sum here: with positive finite edge weights -- the precondition of include/pinsage_hip.h -- every share and so
// every term is >= +0.0), and a slab that pushes nothing writes only its activity byte.
template <bool SKIP>
__global__ __launch_bounds__(256) void push_level_kernel(const PushArgs a) {
    const int lane = ps_lane();
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (wave >= (a.n_nodes + a.n_extra) * a.nslab) return;
    const int64_t idx = wave / a.nslab;
    const int slab = (int)(wave - idx * a.nslab);
    const int64_t v = idx < a.n_nodes ? (int64_t)a.nodes[idx] : a.V + (idx - a.n_nodes);   // n_extra: the edgeless ids V..Vp-1
    if (v < 0 || v >= a.Vp) return;
    const int64_t col = (int64_t)slab * 64 + lane;
    double m = 0.0;
    if (a.first_sweep && col < a.S && a.sources[col] == v) m = 1.0;                         // residual[source] = 1.0 (:169)
    int64_t lo = 0, hi = 0;
    if (v < a.V) { lo = a.in_rowptr[v]; hi = a.in_rowptr[v + 1]; }
    for (int64_t e0 = lo; e0 < hi; e0 += 64) {
        const int64_t e = e0 + lane;
        int u = 0;
        double sh = 0.0;
        bool on = false;
        if (e < hi) {
            u = a.in_src[e];
            sh = a.in_share[e];
            on = u >= 0 && (int64_t)u < a.Vp;
            if (SKIP && on) on = (u > v ? a.act_prev : a.act_cur)[(int64_t)u * a.nslab + slab] != 0;
        }
        unsigned long long todo = __ballot(on);
        while (todo) {
            double val[AHEAD], s[AHEAD];
            int n = 0;
#pragma unroll
            for (int q = 0; q < AHEAD; ++q) {
                if (todo) {
                    const int j = __builtin_ctzll(todo);
                    todo &= todo - 1;
                    const int uj = __builtin_amdgcn_readlane(u, j);
                    s[q] = readlane_f64(sh, j);
                    val[q] = (uj > v ? a.c_prev : a.c_cur)[(int64_t)uj * a.Sc + col];       // one coalesced 512-byte row read
                    n = q + 1;
                }
            }
#pragma unroll
            for (int q = 0; q < AHEAD; ++q)
                if (q < n) m = m + val[q] * s[q];                                              // residual[neighbor] += push_val * norm_weight (:185)
        }
    }
    const bool pos = m > 0.0;                                                                  // `if res > 0` (:175)
    const bool any = __ballot(pos) != 0ull;
    const int64_t o = v * a.Sc + col;
    if (pos) a.score[o] = a.score[o] + a.alpha * m;                                            // ppr[node] += alpha * res (:177)
    if (!SKIP || any) a.c_cur[o] = pos ? a.one_minus_alpha * m : 0.0;                          // push_val (:182)
    if (lane == 0) a.act_cur[v * a.nslab + slab] = any ? 1 : 0;
}

// One block per source over its contiguous score row: round r finds the best positive target that comes after round r - 1's
// winner in the order (score descending, id ascending) -- python's stable sort(reverse=True) over the ascending-target list
// (:218) -- so nothing is written back to the row and k rounds give the k best in rank order.
__global__ __launch_bounds__(256) void topk_kernel(const double *score, int64_t ld, int64_t limit, int k, int32_t *ids,
                                                   double *scores, double *wts, int32_t *nvalid) {
    __shared__ double sv[4];
    __shared__ int64_t si[4];
    __shared__ double win_v;
    __shared__ int64_t win_i;
    const int64_t s = blockIdx.x;
    const double *row = score + s * ld;
    const int tid = threadIdx.x;
    double pv = INFINITY;
    int64_t pi = -1;
    int r = 0;
    for (; r < k; ++r) {
        double bv = 0.0;
        int64_t bi = -1;
        for (int64_t t = tid; t < limit; t += 256) {
            const double x = row[t];
            const bool after = x < pv || (x == pv && t > pi);
            if (after && x > bv) { bv = x; bi = t; }                                           // ascending t: a tie keeps the smaller id
        }
        for (int off = 32; off >= 1; off >>= 1) {
            const double ov = __shfl_xor(bv, off, 64);
            const int64_t oi = __shfl_xor(bi, off, 64);
            if (ov > bv || (ov == bv && ov > 0.0 && oi < bi)) { bv = ov; bi = oi; }
        }
        if ((tid & 63) == 0) { sv[tid >> 6] = bv; si[tid >> 6] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; ++w)
                if (sv[w] > bv || (sv[w] == bv && sv[w] > 0.0 && si[w] < bi)) { bv = sv[w]; bi = si[w]; }
            win_v = bv;
            win_i = bi;
            if (bi >= 0) { ids[s * k + r] = (int32_t)bi; scores[s * k + r] = bv; }
        }
        __syncthreads();
        pv = win_v;
        pi = win_i;
        if (pi < 0) break;
    }
    if (tid == 0) {
        double total = 0.0;
        for (int j = 0; j < r; ++j) total = total + scores[s * k + j];                         // sum(weights), rank order (:224)
        for (int j = 0; j < r; ++j) wts[s * k + j] = ps_div_rn(scores[s * k + j], total);
        for (int j = r; j < k; ++j) { ids[s * k + j] = -1; scores[s * k + j] = 0.0; wts[s * k + j] = 0.0; }
        nvalid[s] = r;
    }
}

inline int64_t chunk_columns(int64_t S) { return ps_cdiv(S, 64) * 64; }

}  // namespace

extern "C" int ps_ppr_shares(const int64_t *rowptr, const double *wsorted, int64_t V, double *share, ps_stream_t stream) {
    if (V < 0 || !rowptr) return PS_EINVAL;
    if (V == 0) return PS_OK;
    if (!wsorted || !share) return PS_EINVAL;
    int64_t g = ps_cdiv(V, 256);
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(shares_kernel, dim3((unsigned)g), dim3(256), 0, ps_stream(stream), rowptr, wsorted, V, share);
    PS_CHECK_LAUNCH();
    return PS_OK;
}

extern "C" size_t ps_ppr_push_workspace_bytes(int64_t Vp, int64_t S) {
    if (Vp <= 0 || S <= 0) return 0;
    const int64_t Sc = chunk_columns(S);
    return 2 * ps_align256((size_t)Vp * Sc * sizeof(double)) + 2 * ps_align256((size_t)Vp * (Sc / 64)) + ALIGN;
}

extern "C" int ps_ppr_push(const int64_t *in_rowptr, const int32_t *in_src, const double *in_share, int64_t V, int64_t Vp,
                           const int32_t *level_nodes, const int64_t *h_level_ptr, int n_levels, const int64_t *sources, int64_t S,
                           uint64_t alpha_bits, int sweeps, int flags, double *score, void *workspace, size_t workspace_bytes,
                           ps_stream_t stream) {
    double alpha;
    std::memcpy(&alpha, &alpha_bits, sizeof alpha);
    if (V < 0 || Vp < V || S < 0 || sweeps < 0 || n_levels < 0 || !(alpha > 0.0 && alpha < 1.0) || (flags & ~PS_PPR_NO_SKIP))
        return PS_EINVAL;
    if (Vp >= ((int64_t)1 << 31) || (V > 0 && (!in_rowptr || !h_level_ptr || n_levels < 1))) return PS_EINVAL;
    if (S == 0 || Vp == 0) return PS_OK;
    if (!sources || !score || !workspace || workspace_bytes < ps_ppr_push_workspace_bytes(Vp, S)) return PS_EINVAL;
    if (V > 0 && (h_level_ptr[0] != 0 || h_level_ptr[n_levels] != V || !level_nodes)) return PS_EINVAL;
    for (int l = 0; l < (V > 0 ? n_levels : 0); ++l)
        if (h_level_ptr[l + 1] < h_level_ptr[l]) return PS_EINVAL;
    const int64_t Sc = chunk_columns(S);
    const int nslab = (int)(Sc / 64);
    // a launch covers at most all Vp nodes, four (node, slab) waves per workgroup: refused here, before anything is enqueued
    if (ps_cdiv(Vp * nslab, 4) >= ((int64_t)1 << 31)) return PS_EINVAL;
    hipStream_t st = ps_stream(stream);
    const size_t cbytes = ps_align256((size_t)Vp * Sc * sizeof(double)), abytes = ps_align256((size_t)Vp * nslab);
    char *base = ps_ws_base(workspace);
    double *c[2] = {reinterpret_cast<double *>(base), reinterpret_cast<double *>(base + cbytes)};
    uint8_t *act[2] = {reinterpret_cast<uint8_t *>(base + 2 * cbytes), reinterpret_cast<uint8_t *>(base + 2 * cbytes + abytes)};
    if (ps_fill_async(base, 0, 2 * cbytes + 2 * abytes, st) != hipSuccess) return PS_ELAUNCH;
    if (ps_fill_async(score, 0, (size_t)Vp * Sc * sizeof(double), st) != hipSuccess) return PS_ELAUNCH;
    hipLaunchKernelGGL(seed_kernel, dim3((unsigned)ps_cdiv(S, 256)), dim3(256), 0, st, sources, S, Sc, Vp, score);
    PS_CHECK_LAUNCH();
    PushArgs a;
    a.in_rowptr = in_rowptr; a.in_src = in_src; a.in_share = in_share; a.sources = sources; a.score = score;
    a.V = V; a.Vp = Vp; a.S = S; a.Sc = Sc; a.nslab = nslab;
    a.alpha = alpha; a.one_minus_alpha = 1.0 - alpha;
    const int levels = V > 0 ? n_levels : 1;                         // an edgeless graph: the ids 0..Vp-1 as one level
    for (int k = 0; k < sweeps; ++k) {
        const int cur = k & 1;                                       // the buffers swap between sweeps
        a.c_prev = c[cur ^ 1]; a.c_cur = c[cur]; a.act_prev = act[cur ^ 1]; a.act_cur = act[cur];
        a.first_sweep = k == 0;
        for (int l = 0; l < levels; ++l) {
            a.nodes = V > 0 ? level_nodes + h_level_ptr[l] : nullptr;
            a.n_nodes = V > 0 ? h_level_ptr[l + 1] - h_level_ptr[l] : 0;
            a.n_extra = l == 0 ? Vp - V : 0;                          // ids beyond the graph have no in-edges: level 0
            const int64_t blocks = ps_cdiv((a.n_nodes + a.n_extra) * nslab, 4);
            if (blocks == 0) continue;
            if (flags & PS_PPR_NO_SKIP)
                hipLaunchKernelGGL(push_level_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, a);
            else
                hipLaunchKernelGGL(push_level_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, a);
            PS_CHECK_LAUNCH();
        }
    }
    return PS_OK;                                                    // the mass left after the last sweep is dropped, as in the reference
}

extern "C" int ps_ppr_topk(const double *score, int64_t S, int64_t ld, int64_t Vp, int64_t max_target, int k, int32_t *ids,
                           double *scores, double *wts, int32_t *nvalid, ps_stream_t stream) {
    if (S < 0 || Vp < 0 || ld < Vp || k < 1 || S >= ((int64_t)1 << 31) || Vp >= ((int64_t)1 << 31)) return PS_EINVAL;
    if (S == 0) return PS_OK;
    if ((!score && Vp > 0) || !ids || !scores || !wts || !nvalid) return PS_EINVAL;
    const int64_t limit = (max_target >= 0 && max_target < Vp) ? max_target : Vp;
    hipLaunchKernelGGL(topk_kernel, dim3((unsigned)S), dim3(256), 0, ps_stream(stream), score, ld, limit, k, ids, scores, wts, nvalid);
    PS_CHECK_LAUNCH();
    return PS_OK;
}
