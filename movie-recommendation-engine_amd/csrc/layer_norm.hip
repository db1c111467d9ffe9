// layer_norm.hip -- nn.LayerNorm of ImportanceAggregator (reference model/aggregators.py:213-287) on gfx950, both directions, with the
// aggregator's "zeros for a node without neighbours" as a row mask (`live`).  No float atomics, every workspace word that is read was
// written by this call, nothing waits for the host: equal inputs give equal bits.  The operation order is stated in
// include/pinsage_hip.h.
//
// ps_layer_norm       one launch, one wave per row (row_sweep.h: ps_ln_row_stats): the mean, then the centred squares, then
//                     y = fmaf(xh, gamma, beta).  Rows of up to PS_LN_KEEP sweeps are read once and stay in registers; longer rows
//                     are read again by the lane that writes the same addresses afterwards (y may be x).  A dead row is never read.
// ps_layer_norm_bwd   ln_bwd_partial_kernel   the column-sum skeleton of col_sums.h, a workgroup per partition of PS_BN_ROWS rows and
//                                             64 * VEC columns: gy and gy * xh in fp64 over the live rows: part[P, 2, N].
//                     ln_bwd_finish_kernel    one lane per column adds the partitions ascending from 0.0: dbeta, dgamma.
//                     ln_bwd_rows_kernel      one wave per row: c1, c2 (ps_ln_bwd_row_sums) and gx = rstd * fmaf(-xh, k2, gg - k1).
//                                             A lane reads gy[c] for the last time before it writes gx[c]: gx may be gy, and the
//                                             column sums are launched first.
// The first two are left out when dgamma / dbeta are not wanted, the last when gx is not.  Every grid covers its rows / partitions
// with blocks of their own (grid.x up to 2^31 - 1): no kernel strides over rows.  No [M, N] intermediate exists.
#include "ps_common.h"
#include "col_sums.h"
#include "row_sweep.h"

namespace {

constexpr int LN_UNROLL = 4;       // rows a wave of the column-sum pass has in flight
constexpr int KEEP = PS_LN_KEEP;

// a dead row of an output: +0.0 throughout
template <int VEC>
__device__ __forceinline__ void zero_row(float *orow, int N) {
    const int lane = threadIdx.x & 63;
    float o[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = 0.f;
    for (int col = lane * VEC; col < N; col += 64 * VEC) store_vec<VEC>(orow + col, o);
}

template <int VEC>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float *x, int64_t M, int N, const float *__restrict__ gamma,
                                                     const float *__restrict__ beta, float eps, const int32_t *__restrict__ live,
                                                     float *y, float *__restrict__ mean, float *__restrict__ rstd) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    if (i >= M) return;                                                   // a whole wave
    const int chunk = 64 * VEC;
    float *yr = y + i * N;
    if (live && live[i] <= 0) {                                           // wave-uniform: the row of x is not read
        zero_row<VEC>(yr, N);
        if (mean && lane == 0) { mean[i] = 0.f; rstd[i] = 0.f; }
        return;
    }
    const float *xr = x + i * N;
    float kept[KEEP][VEC];
    const float2 mr = ps_ln_row_stats<VEC>(xr, N, eps, kept);
    if (mean && lane == 0) { mean[i] = mr.x; rstd[i] = mr.y; }
#pragma unroll
    for (int k = 0; k < KEEP; ++k) {
        const int col = k * chunk + lane * VEC;
        if (col < N) {
            float ga[VEC], be[VEC], o[VEC];
            load_vec<VEC>(gamma + col, true, ga);
            load_vec<VEC>(beta + col, true, be);
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[e] = fmaf(ps_ln_xhat(kept[k][e], mr.x, mr.y), ga[e], be[e]);
            store_vec<VEC>(yr + col, o);
        }
    }
    for (int c0 = KEEP * chunk; c0 < N; c0 += chunk) {
        const int col = c0 + lane * VEC;
        if (col < N) {
            // every lane reads again what it is about to overwrite (y may be x)
            float xx[VEC], ga[VEC], be[VEC], o[VEC];
            load_vec<VEC>(xr + col, true, xx);
            load_vec<VEC>(gamma + col, true, ga);
            load_vec<VEC>(beta + col, true, be);
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[e] = fmaf(ps_ln_xhat(xx[e], mr.x, mr.y), ga[e], be[e]);
            store_vec<VEC>(yr + col, o);
        }
    }
}

// part[p, 0, c] = sum of gy[r, c], part[p, 1, c] = sum of gy[r, c] * xh[r, c] over the live rows r of partition p (double[P, 2, N])
template <int VEC>
__global__ __launch_bounds__(256) void ln_bwd_partial_kernel(const float *__restrict__ x, const float *__restrict__ gy, int64_t M, int N,
                                                             const float *__restrict__ mean, const float *__restrict__ rstd,
                                                             const int32_t *__restrict__ live, double *__restrict__ part) {
    struct Row { float x[VEC], g[VEC], mean, rstd; bool alive; };
    const int col = (int)blockIdx.y * 64 * VEC + (threadIdx.x & 63) * VEC;
    const bool cact = col < N;
    ps_col_sums_partition<VEC, LN_UNROLL, true>(
        M, N, blockIdx.x, col,
        [&](int64_t rr, bool inside) {
            Row row;
            row.alive = inside && (!live || live[rr] > 0);               // a dead row is not read
            load_vec<VEC>(x + rr * N + col, cact && row.alive, row.x);
            load_vec<VEC>(gy + rr * N + col, cact && row.alive, row.g);
            row.mean = row.alive ? mean[rr] : 0.f;
            row.rstd = row.alive ? rstd[rr] : 0.f;
            return row;
        },
        [&](const Row &row, int e, double &a, double &b) {
            a = row.alive ? (double)row.g[e] : 0.0;                      // a dead row adds (+0.0, +0.0): col_sums.h
            b = row.alive ? (double)row.g[e] * (double)ps_ln_xhat(row.x[e], row.mean, row.rstd) : 0.0;
        },
        part);
}

// P == 0 (no rows): zeros
__global__ __launch_bounds__(64) void ln_bwd_finish_kernel(const double *__restrict__ part, int64_t P, int N,
                                                           float *__restrict__ dgamma, float *__restrict__ dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    const double2 S = ps_col_sums_finish(part, P, N, c);
    dbeta[c] = (float)S.x;
    dgamma[c] = (float)S.y;
}

template <int VEC>
__global__ __launch_bounds__(256) void ln_bwd_rows_kernel(const float *__restrict__ x, const float *gy, int64_t M, int N,
                                                          const float *__restrict__ mean, const float *__restrict__ rstd,
                                                          const float *__restrict__ gamma, const int32_t *__restrict__ live,
                                                          float *gx) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    if (i >= M) return;
    const int chunk = 64 * VEC;
    float *or_ = gx + i * N;
    if (live && live[i] <= 0) {                                           // wave-uniform: neither x nor gy is read
        zero_row<VEC>(or_, N);
        return;
    }
    const float *xr = x + i * N;
    const float *gr = gy + i * N;
    const float m = mean[i], rs = rstd[i];
    float gg[KEEP][VEC], xh[KEEP][VEC];
    const float2 c = ps_ln_bwd_row_sums<VEC>(xr, gr, gamma, N, m, rs, gg, xh);
    const float k1 = c.x / (float)N, k2 = c.y / (float)N;
#pragma unroll
    for (int k = 0; k < KEEP; ++k) {
        const int col = k * chunk + lane * VEC;
        if (col < N) {
            float o[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[e] = rs * fmaf(-xh[k][e], k2, gg[k][e] - k1);
            store_vec<VEC>(or_ + col, o);
        }
    }
    for (int c0 = KEEP * chunk; c0 < N; c0 += chunk) {
        const int col = c0 + lane * VEC;
        if (col < N) {
            float g1[VEC], x1[VEC], o[VEC];
            ps_ln_bwd_elems<VEC>(xr, gr, gamma, col, m, rs, g1, x1);     // gy[c] for the last time, before gx[c] is written
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[e] = rs * fmaf(-x1[e], k2, g1[e] - k1);
            store_vec<VEC>(or_ + col, o);
        }
    }
}

inline size_t ws_bytes(int64_t M, int N) { return (size_t)ps_bn_partitions(M) * 2 * (size_t)N * sizeof(double); }

}  // namespace

extern "C" int ps_layer_norm(const float *x, int64_t M, int N, const float *gamma, const float *beta, float eps, const int32_t *live,
                             float *y, float *mean, float *rstd, ps_stream_t stream) {
    if (M < 0 || N < 1 || (mean == nullptr) != (rstd == nullptr)) return PS_EINVAL;
    if (M == 0) return PS_OK;                                 // before the pointers: an empty tensor's base is NULL
    if (!x || !y || !gamma || !beta) return PS_EINVAL;
    const int64_t row_blocks = ps_cdiv(M, 4);
    if (row_blocks > 0x7fffffff) return PS_EUNSUPPORTED;      // every row has a wave of its own
    hipStream_t st = ps_stream(stream);
    const bool vec4 = (N % 4 == 0) && ps_aligned16({x, y, gamma, beta});
    PS_LAUNCH_VEC(ln_fwd_kernel<VEC>, vec4, dim3((unsigned)row_blocks), dim3(256), st, x, M, N, gamma, beta, eps, live, y, mean, rstd);
    PS_CHECK_LAUNCH();
    return PS_OK;
}

extern "C" size_t ps_layer_norm_bwd_workspace_bytes(int64_t M, int N) {
    if (M < 1 || N < 1) return 0;
    return ws_bytes(M, N);
}

extern "C" int ps_layer_norm_bwd(const float *x, const float *gy, int64_t M, int N, const float *mean, const float *rstd,
                                 const float *gamma, const int32_t *live, float *gx, float *dgamma, float *dbeta, void *workspace,
                                 size_t workspace_bytes, ps_stream_t stream) {
    if (M < 0 || N < 1 || (dgamma == nullptr) != (dbeta == nullptr)) return PS_EINVAL;
    hipStream_t st = ps_stream(stream);
    if (M == 0) {                                             // before the pointers: the sums of no rows are zeros
        if (dgamma) {
            hipLaunchKernelGGL(ln_bwd_finish_kernel, dim3((unsigned)ps_cdiv(N, 64)), dim3(64), 0, st, nullptr, 0, N, dgamma, dbeta);
            PS_CHECK_LAUNCH();
        }
        return PS_OK;
    }
    if (!x || !gy || !mean || !rstd || !gamma) return PS_EINVAL;
    if (dgamma) {
        if (!workspace || reinterpret_cast<size_t>(workspace) % 8 != 0) return PS_EINVAL;
        if (workspace_bytes < ws_bytes(M, N)) return PS_EWORKSPACE;
    }
    const int64_t P = ps_bn_partitions(M);
    const int64_t row_blocks = ps_cdiv(M, 4);
    if (row_blocks > 0x7fffffff) return PS_EUNSUPPORTED;      // every row has a wave of its own
    const bool vec4 = (N % 4 == 0) && ps_aligned16({x, gy, gx, gamma});  // gx may be absent
    const int64_t col_blocks = ps_cdiv(N, vec4 ? 256 : 64);
    if (col_blocks > 65535) return PS_EUNSUPPORTED;           // grid.y of the column-sum pass
    if (dgamma) {
        double *part = static_cast<double *>(workspace);
        PS_LAUNCH_VEC(ln_bwd_partial_kernel<VEC>, vec4, dim3((unsigned)P, (unsigned)col_blocks), dim3(256), st, x, gy, M, N, mean, rstd,
                      live, part);
        PS_CHECK_LAUNCH();
        hipLaunchKernelGGL(ln_bwd_finish_kernel, dim3((unsigned)ps_cdiv(N, 64)), dim3(64), 0, st, part, P, N, dgamma, dbeta);
        PS_CHECK_LAUNCH();
    }
    if (gx) {
        PS_LAUNCH_VEC(ln_bwd_rows_kernel<VEC>, vec4, dim3((unsigned)row_blocks), dim3(256), st, x, gy, M, N, mean, rstd, gamma, live, gx);
        PS_CHECK_LAUNCH();
    }
    return PS_OK;
}
