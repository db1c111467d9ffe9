// spmm_exact.hip -- the CSR row gather-reduce of csrc/spmm_csr.hip without atomics, and the per-edge row dot that is the
// gradient of its edge values, on gfx950.
//
// ps_spmm_csr_exact is the forward of GraphConv's edge aggregation under autograd and, over the source-grouped CSR, the gradient
// of its features (pinsage_hip/graph.py: SpmmFn).  Work is cut by edges as in spmm_csr.hip: wave w owns the edge slots
// [w * SLICE, (w + 1) * SLICE), finds its first row by bisection of rowptr and walks the rows that intersect its range; every
// source row is one coalesced 16 B-per-lane sweep, UNROLL rows in flight.  A piece that is a whole row is stored to out; a piece
// of a row that a slice boundary cuts is stored to the workspace with plain vector stores, and a second launch adds each cut
// row's pieces in slice order.  A slice holds at most two such pieces: entry 2 w of the workspace is the piece of the row that
// began in an earlier slice, entry 2 w + 1 the piece of the row that begins in slice w and runs on.
// ps_sddmm_csr walks the same slices; the row of g stays in registers while the CSR row lasts.
// include/pinsage_hip.h states the arithmetic; tests/helpers/spmm_cases.py restates it bit for bit.
#include "ps_common.h"
#include "row_sweep.h"

namespace {

constexpr int SLICE = 512;                     // ps_spmm_exact_slice()
constexpr int UNROLL = 8;

// the last row r in [0, V) with rowptr[r] <= e (rowptr[0] = 0 <= e < rowptr[V])
__device__ __forceinline__ int64_t row_of(const int64_t *__restrict__ rowptr, int64_t V, int64_t e) {
    int64_t a = 0, b = V;
    while (b - a > 1) {
        const int64_t m = (a + b) >> 1;
        if (rowptr[m] <= e) a = m; else b = m;
    }
    return a;
}

template <int VEC>
__global__ __launch_bounds__(256) void spmm_exact_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                         const float *__restrict__ val, const float *__restrict__ x, int64_t N, int H,
                                                         int64_t V, int64_t E, float *__restrict__ out, float *__restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int chunk = 64 * VEC;
    int64_t e_begin = wave * SLICE;
    if (e_begin >= E) return;
    const int64_t e_end = (e_begin + SLICE < E) ? (e_begin + SLICE) : E;
    int64_t r = row_of(rowptr, V, e_begin);
    while (e_begin < e_end && r < V) {
        const int64_t lo = rowptr[r], hi = rowptr[r + 1];
        const int64_t s0 = e_begin, s1 = (hi < e_end) ? hi : e_end;
        if (s1 <= s0) { ++r; continue; }
        // a whole row goes to out; a cut row's piece to the slice's entry for a row that began earlier (2 w) or begins here (2 w + 1)
        float *dst = (s0 == lo && s1 == hi) ? out + r * H : part + (2 * wave + (s0 == lo ? 1 : 0)) * H;
        for (int c0 = 0; c0 < H; c0 += chunk) {
            const int cc = c0 + lane * VEC;
            const bool cact = cc < H;
            float acc[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
            for (int64_t e0 = s0; e0 < s1; e0 += 64) {
                const int64_t e = e0 + lane;
                int32_t myid = -1;
                float myw = 0.f;
                if (e < s1) {
                    myid = col[e];
                    if (myid < 0 || (int64_t)myid >= N) myid = -1;    // a source id outside x is skipped, never read
                    myw = val ? val[e] : 1.f;
                }
                const int kk = (s1 - e0) < 64 ? (int)(s1 - e0) : 64;
                for (int t0 = 0; t0 < kk; t0 += UNROLL) {
                    float rr[UNROLL][VEC], wv[UNROLL];
                    int32_t id[UNROLL];
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) {
                        const int t = t0 + u;
                        const int tl = t < 64 ? t : 0;
                        id[u] = (t < kk) ? __builtin_amdgcn_readlane(myid, tl) : -1;
                        wv[u] = lane_f32(myw, tl);
                        load_vec<VEC>(x + (int64_t)id[u] * H + cc, id[u] >= 0 && cact, rr[u]);
                    }
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) {
                        if (id[u] < 0) continue;                       // wave-uniform
#pragma unroll
                        for (int v = 0; v < VEC; ++v) acc[v] = fmaf(wv[u], rr[u][v], acc[v]);
                    }
                }
            }
            if (cact) store_vec<VEC>(dst + cc, acc);
        }
        e_begin = s1;
        ++r;
    }
}

// Wave w: the row that begins in slice w and runs on past it (if there is one) -- its pieces added in slice order.
template <int VEC>
__global__ __launch_bounds__(256) void spmm_exact_combine_kernel(const int64_t *__restrict__ rowptr, int H, int64_t V, int64_t E,
                                                                 float *__restrict__ out, const float *__restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int chunk = 64 * VEC;
    const int64_t edge = (wave + 1) * SLICE;                       // the slice's right boundary
    if (edge >= E) return;
    const int64_t r = row_of(rowptr, V, edge - 1);
    const int64_t lo = rowptr[r];
    int64_t hi = rowptr[r + 1];
    hi = hi > E ? E : hi;
    if (lo < wave * SLICE || hi <= edge) return;                  // began earlier (another wave's row), or ends with the slice
    const int64_t last = (hi - 1) / SLICE;                         // the row's pieces: slices wave .. last
    for (int c0 = 0; c0 < H; c0 += chunk) {
        const int cc = c0 + lane * VEC;
        const bool cact = cc < H;
        float acc[VEC];
        load_vec<VEC>(part + (2 * wave + 1) * H + cc, cact, acc);
        for (int64_t k0 = wave + 1; k0 <= last; k0 += UNROLL) {
            float rr[UNROLL][VEC];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) load_vec<VEC>(part + 2 * (k0 + u) * H + cc, k0 + u <= last && cact, rr[u]);
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                if (k0 + u > last) continue;
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = acc[v] + rr[u][v];
            }
        }
        if (cact) store_vec<VEC>(out + r * H + cc, acc);
    }
}

// d[e] = g[r] . x[col[e]] for the slots of one slice.  GS > 0: the row of g is held in GS sweeps of registers (H <= GS * 64 * VEC);
// GS == 0: any H, g is read again with every group of UNROLL edges.  The same chain either way.
template <int VEC, int GS>
__global__ __launch_bounds__(256) void sddmm_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                    const float *__restrict__ x, int64_t N, const float *__restrict__ g, int64_t V,
                                                    int H, int64_t E, float *__restrict__ d) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int chunk = 64 * VEC;
    constexpr int NG = GS > 0 ? GS : 1;
    int64_t e_begin = wave * SLICE;
    if (e_begin >= E) return;
    const int64_t e_end = (e_begin + SLICE < E) ? (e_begin + SLICE) : E;
    int64_t r = row_of(rowptr, V, e_begin);
    while (e_begin < e_end && r < V) {
        const int64_t hi = rowptr[r + 1];
        const int64_t s0 = e_begin, s1 = (hi < e_end) ? hi : e_end;
        if (s1 <= s0) { ++r; continue; }
        float gg[NG][VEC];
        if (GS > 0) {
#pragma unroll
            for (int k = 0; k < NG; ++k) load_vec<VEC>(g + r * H + k * chunk + lane * VEC, k * chunk + lane * VEC < H, gg[k]);
        }
        for (int64_t e0 = s0; e0 < s1; e0 += 64) {
            const int64_t e = e0 + lane;
            int32_t myid = -1;
            if (e < s1) {
                myid = col[e];
                if (myid < 0 || (int64_t)myid >= N) myid = -1;
            }
            const int kk = (s1 - e0) < 64 ? (int)(s1 - e0) : 64;
            float myd = 0.f;
            for (int t0 = 0; t0 < kk; t0 += UNROLL) {
                int32_t id[UNROLL];
                float pt[UNROLL];
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    const int t = t0 + u;
                    id[u] = (t < kk) ? __builtin_amdgcn_readlane(myid, t < 64 ? t : 0) : -1;
                    pt[u] = 0.f;
                }
                if (GS > 0) {
#pragma unroll
                    for (int k = 0; k < NG; ++k) {
                        if (k * chunk >= H) continue;                   // wave-uniform
                        const int cc = k * chunk + lane * VEC;
                        float rr[UNROLL][VEC];
#pragma unroll
                        for (int u = 0; u < UNROLL; ++u) load_vec<VEC>(x + (int64_t)id[u] * H + cc, id[u] >= 0 && cc < H, rr[u]);
#pragma unroll
                        for (int u = 0; u < UNROLL; ++u)
#pragma unroll
                            for (int v = 0; v < VEC; ++v) pt[u] = fmaf(gg[k][v], rr[u][v], pt[u]);
                    }
                } else {
                    for (int c0 = 0; c0 < H; c0 += chunk) {
                        const int cc = c0 + lane * VEC;
                        float rr[UNROLL][VEC], g1[VEC];
#pragma unroll
                        for (int u = 0; u < UNROLL; ++u) load_vec<VEC>(x + (int64_t)id[u] * H + cc, id[u] >= 0 && cc < H, rr[u]);
                        load_vec<VEC>(g + r * H + cc, cc < H, g1);
#pragma unroll
                        for (int u = 0; u < UNROLL; ++u)
#pragma unroll
                            for (int v = 0; v < VEC; ++v) pt[u] = fmaf(g1[v], rr[u][v], pt[u]);
                    }
                }
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    if (t0 + u < kk) {                                  // wave-uniform
                        const float s = ps_wave_sum_f32(pt[u]);
                        if (lane == t0 + u) myd = (id[u] >= 0) ? s : 0.f;   // a source id outside x: +0.0
                    }
                }
            }
            if (e < s1) d[e] = myd;
        }
        e_begin = s1;
        ++r;
    }
}

inline size_t exact_bytes(int64_t E, int H) { return 256 + ps_align256((size_t)(2 * ps_cdiv(E, SLICE)) * H * sizeof(float)); }

template <int VEC>
void launch_sddmm(unsigned grid, hipStream_t st, const int64_t *rowptr, const int32_t *col, const float *x, int64_t N, const float *g,
                  int64_t V, int H, int64_t E, float *d) {
    const int sweeps = (int)ps_cdiv(H, 64 * VEC);
    if (sweeps <= 1) hipLaunchKernelGGL((sddmm_kernel<VEC, 1>), dim3(grid), dim3(256), 0, st, rowptr, col, x, N, g, V, H, E, d);
    else if (sweeps <= 2) hipLaunchKernelGGL((sddmm_kernel<VEC, 2>), dim3(grid), dim3(256), 0, st, rowptr, col, x, N, g, V, H, E, d);
    else if (sweeps <= 4) hipLaunchKernelGGL((sddmm_kernel<VEC, 4>), dim3(grid), dim3(256), 0, st, rowptr, col, x, N, g, V, H, E, d);
    else hipLaunchKernelGGL((sddmm_kernel<VEC, 0>), dim3(grid), dim3(256), 0, st, rowptr, col, x, N, g, V, H, E, d);
}

}  // namespace

extern "C" int ps_spmm_exact_slice(void) { return SLICE; }

extern "C" size_t ps_spmm_csr_exact_workspace_bytes(int64_t E, int H) {
    if (E <= 0 || H <= 0) return 0;
    return exact_bytes(E, H);
}

extern "C" int ps_spmm_csr_exact(const int64_t *rowptr, const int32_t *col, const float *val, const float *x, int64_t N, int H,
                                 int64_t V, int64_t E, float *out, void *workspace, size_t workspace_bytes, ps_stream_t stream) {
    if (V < 0 || H <= 0 || N < 0 || E < 0) return PS_EINVAL;
    if (V == 0) return PS_OK;
    if (!out) return PS_EINVAL;
    hipStream_t st = ps_stream(stream);
    if (E == 0) {                                             // every row is empty: +0.0 everywhere
        if (ps_fill_async(out, 0, (size_t)V * H * sizeof(float), st) != hipSuccess) return PS_ELAUNCH;
        return PS_OK;
    }
    if (!rowptr || !col || !x || !workspace) return PS_EINVAL;
    if (workspace_bytes < exact_bytes(E, H)) return PS_EINVAL;
    const int64_t waves = ps_cdiv(E, SLICE);
    const int64_t grid = ps_cdiv(waves, 4);
    if (waves > 0x7fffffff) return PS_EUNSUPPORTED;           // a wave's number is an int
    // the empty rows (no wave visits them) are the zeros of this fill; every other row is stored once by one of the launches
    if (ps_fill_async(out, 0, (size_t)V * H * sizeof(float), st) != hipSuccess) return PS_ELAUNCH;
    float *part = reinterpret_cast<float *>(ps_ws_base(workspace));
    const bool vec4 = (H % 4 == 0) && ps_aligned16({x, out});
    PS_LAUNCH_VEC(spmm_exact_kernel<VEC>, vec4, dim3((unsigned)grid), dim3(256), st, rowptr, col, val, x, N, H, V, E, out, part);
    PS_CHECK_LAUNCH();
    if (waves > 1) {
        PS_LAUNCH_VEC(spmm_exact_combine_kernel<VEC>, vec4, dim3((unsigned)grid), dim3(256), st, rowptr, H, V, E, out, part);
        PS_CHECK_LAUNCH();
    }
    return PS_OK;
}

extern "C" int ps_sddmm_csr(const int64_t *rowptr, const int32_t *col, const float *x, int64_t N, const float *g, int64_t V, int H,
                            int64_t E, float *d, ps_stream_t stream) {
    if (V < 0 || H <= 0 || N < 0 || E < 0) return PS_EINVAL;
    if (V == 0 || E == 0) return PS_OK;
    if (!rowptr || !col || !x || !g || !d) return PS_EINVAL;
    const int64_t waves = ps_cdiv(E, SLICE);
    const int64_t grid = ps_cdiv(waves, 4);
    if (waves > 0x7fffffff) return PS_EUNSUPPORTED;
    hipStream_t st = ps_stream(stream);
    if ((H % 4 == 0) && ps_aligned16({x, g})) launch_sddmm<4>((unsigned)grid, st, rowptr, col, x, N, g, V, H, E, d);
    else launch_sddmm<1>((unsigned)grid, st, rowptr, col, x, N, g, V, H, E, d);
    PS_CHECK_LAUNCH();
    return PS_OK;
}
