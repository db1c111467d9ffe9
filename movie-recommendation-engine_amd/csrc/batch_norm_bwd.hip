// batch_norm_bwd.hip -- the backward of GraphConvLayer's training-mode batch norm with its ReLU / F.normalize epilogue
// (pinsage_hip/dense.py: BatchNormFn) on gfx950: y = epi(fmaf(z - mean, scale, beta)) with mean / var / scale the outputs of
// ps_bn_batch_stats for this same z, so the statistics' dependence on z is part of the gradient.  Nothing is saved but z and the
// column vectors: every pass recomputes t = the activation before the norm with the forward's own bits (ps_bn_act), and no
// [M, N] intermediate exists.  No float atomics, every workspace word that is read was written by this call, nothing waits for
// the host: equal inputs give equal bits.  The operation order is stated in include/pinsage_hip.h.
//
// Four passes, any N:
//   bn_bwd_rowscal_kernel   PS_L2NORM only.  One wave per row, ps_row_norm_sums (row_sweep.h, the code of epilogue_bwd_kernel) over
//                           the recomputed t: (nrm, s) go to the workspace, 2 floats per row.
//   bn_bwd_partial_kernel   the column-sum skeleton of col_sums.h (the code of bn_partial_kernel), a workgroup per partition of
//                           PS_BN_ROWS rows and 64 * VEC columns: every lane recomputes ga (ps_epilogue_ga) and xh per element and
//                           adds ga and ga * xh in fp64 (the product of two fp32 values is exact there): part[P, 2, N].
//   bn_bwd_finish_kernel    one lane per column adds the partitions ascending from 0.0: dbeta, dgamma, and rstd / k1 / k2 for the
//                           last pass.
//   bn_bwd_apply_kernel     one wave per row recomputes ga and writes gz = scale * fmaf(-xh, k2, ga - k1).  A lane reads gy[c] for
//                           the last time before it writes gz[c]: gz may be gy.
// Every grid covers its rows / partitions with blocks of their own (grid.x up to 2^31 - 1): no kernel strides over rows.
// A form that fused the first two passes for rows of up to four sweeps (a workgroup per partition, a wave keeping whole rows in
// registers, 5 matrix sweeps instead of 7) gave the same bits and was measured slower at 59 047 x 256 -- 0.158 ms against 0.100 ms --
// and is not kept ("Batch-norm layer, training"; why it was slower was not measured).
#include "ps_common.h"
#include "col_sums.h"
#include "row_sweep.h"

namespace {

constexpr int BN_UNROLL = 4;       // rows a wave of the column-sum pass has in flight

template <int VEC>
__device__ __forceinline__ void rstd_of(const float (&var)[VEC], float eps, float (&rstd)[VEC]) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) rstd[e] = 1.0f / sqrtf(var[e] + eps);
}

// rows[i] = (nrm, s) of row i
template <int VEC>
__global__ __launch_bounds__(256) void bn_bwd_rowscal_kernel(const float *__restrict__ z, const float *__restrict__ gy, int64_t M, int N,
                                                             const float *__restrict__ mean, const float *__restrict__ scale,
                                                             const float *__restrict__ beta, int flags, float2 *__restrict__ rows) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    if (i >= M) return;                                                   // a whole wave
    const bool relu = (flags & PS_RELU) != 0;
    const float *zr = z + i * N;
    const float2 ns = ps_row_norm_sums<VEC>(N, gy + i * N, [&](int col, bool ok, float (&t)[VEC]) {
        ps_bn_act_vec<VEC>(zr, mean, scale, beta, col, ok, relu, t);
    });
    if (lane == 0) rows[i] = ns;
}

// part[p, 0, c] = sum of ga[r, c], part[p, 1, c] = sum of ga[r, c] * xh[r, c] over the rows r of partition p (double[P, 2, N])
template <int VEC>
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const float *__restrict__ z, const float *__restrict__ gy, int64_t M, int N,
                                                             const float *__restrict__ mean, const float *__restrict__ var,
                                                             const float *__restrict__ scale, const float *__restrict__ beta, float eps,
                                                             int flags, const float2 *__restrict__ rows, double *__restrict__ part) {
    struct Row { float z[VEC], g[VEC]; float2 rs; };
    const int col = (int)blockIdx.y * 64 * VEC + (threadIdx.x & 63) * VEC;
    const bool cact = col < N;
    const bool relu = (flags & PS_RELU) != 0, l2 = (flags & PS_L2NORM) != 0;
    float mm[VEC], vv[VEC], sc[VEC], bb[VEC], rstd[VEC];
    load_vec<VEC>(mean + col, cact, mm);
    load_vec<VEC>(var + col, cact, vv);
    load_vec<VEC>(scale + col, cact, sc);
    load_vec<VEC>(beta + col, cact, bb);
    rstd_of<VEC>(vv, eps, rstd);
    ps_col_sums_partition<VEC, BN_UNROLL, true>(
        M, N, blockIdx.x, col,
        [&](int64_t rr, bool live) {
            Row row;
            load_vec<VEC>(z + rr * N + col, cact && live, row.z);
            load_vec<VEC>(gy + rr * N + col, cact && live, row.g);
            row.rs = (l2 && live) ? rows[rr] : make_float2(1.f, 0.f);
            return row;
        },
        [&](const Row &row, int e, double &a, double &b) {
            const float d = row.z[e] - mm[e];
            const float tt = ps_bn_act(d, sc[e], bb[e], relu);
            const float xh = d * rstd[e];
            const float ga = ps_epilogue_ga(tt, row.g[e], relu, l2, ps_row_clamp(row.rs.x), row.rs.x < 1e-12f, row.rs.y);
            a = (double)ga;
            b = (double)ga * (double)xh;
        },
        part);
}

// colv = float[3, ldc]: rstd, k1 = dbeta / M, k2 = dgamma / M
__global__ __launch_bounds__(64) void bn_bwd_finish_kernel(const double *__restrict__ part, int64_t P, int64_t M, int N,
                                                           const float *__restrict__ var, float eps, float *__restrict__ dgamma,
                                                           float *__restrict__ dbeta, float *__restrict__ colv, int ldc) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    const double2 S = ps_col_sums_finish(part, P, N, c);
    const float db = (float)S.x, dg = (float)S.y;
    if (dbeta) dbeta[c] = db;
    if (dgamma) dgamma[c] = dg;
    colv[c] = 1.0f / sqrtf(var[c] + eps);
    colv[ldc + c] = db / (float)M;
    colv[2 * ldc + c] = dg / (float)M;
}

template <int VEC>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float *__restrict__ z, const float *gy, int64_t M, int N,
                                                           const float *__restrict__ mean, const float *__restrict__ scale,
                                                           const float *__restrict__ beta, int flags, const float2 *__restrict__ rows,
                                                           const float *__restrict__ colv, int ldc, float *gz) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    if (i >= M) return;
    const int chunk = 64 * VEC;
    const bool relu = (flags & PS_RELU) != 0, l2 = (flags & PS_L2NORM) != 0;
    float c = 1.f, s = 0.f;
    bool below = false;
    if (l2) {
        const float2 rs = rows[i];
        c = ps_row_clamp(rs.x);
        below = rs.x < 1e-12f;
        s = rs.y;
    }
    const float *zr = z + i * N;
    const float *gr = gy + i * N;
    float *or_ = gz + i * N;
    for (int c0 = 0; c0 < N; c0 += chunk) {
        const int col = c0 + lane * VEC;
        if (col >= N) continue;
        float zz[VEC], gg[VEC], mm[VEC], sc[VEC], bb[VEC], rstd[VEC], k1[VEC], k2[VEC], o[VEC];
        load_vec<VEC>(zr + col, true, zz);
        load_vec<VEC>(gr + col, true, gg);
        load_vec<VEC>(mean + col, true, mm);
        load_vec<VEC>(scale + col, true, sc);
        load_vec<VEC>(beta + col, true, bb);
        load_vec<VEC>(colv + col, true, rstd);
        load_vec<VEC>(colv + ldc + col, true, k1);
        load_vec<VEC>(colv + 2 * ldc + col, true, k2);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float d = zz[e] - mm[e];
            const float t = ps_bn_act(d, sc[e], bb[e], relu);
            const float xh = d * rstd[e];
            const float ga = ps_epilogue_ga(t, gg[e], relu, l2, c, below, s);
            o[e] = sc[e] * fmaf(-xh, k2[e], ga - k1[e]);
        }
        store_vec<VEC>(or_ + col, o);
    }
}

inline size_t align16(size_t x) { return (x + 15) / 16 * 16; }
inline int col_ld(int N) { return (N + 3) / 4 * 4; }                     // the three column vectors each start on a 16-byte boundary

// the workspace: double part[P, 2, N] | to a 16-byte boundary | float colv[3, ldc] | float2 rows[M]
struct BnBwdWs {
    double *part;
    float *colv;
    float2 *rows;
};
inline size_t ws_bytes(int64_t M, int N) {
    return (size_t)ps_bn_partitions(M) * 2 * (size_t)N * sizeof(double) + 16 + 3 * (size_t)col_ld(N) * sizeof(float) +
           (size_t)M * sizeof(float2);
}
inline BnBwdWs ws_carve(void *workspace, int64_t M, int N) {
    BnBwdWs w;
    w.part = static_cast<double *>(workspace);
    char *p = reinterpret_cast<char *>(align16(reinterpret_cast<size_t>(w.part + ps_bn_partitions(M) * 2 * (int64_t)N)));
    w.colv = reinterpret_cast<float *>(p);
    w.rows = reinterpret_cast<float2 *>(p + 3 * (size_t)col_ld(N) * sizeof(float));
    return w;
}

int bn_bwd_launch(const float *z, const float *gy, int64_t M, int N, const float *mean, const float *var, const float *scale,
                  const float *beta, float eps, int flags, float *gz, float *dgamma, float *dbeta, void *workspace,
                  size_t workspace_bytes, ps_stream_t stream) {
    if (M < 2 || N < 1 || (flags & ~(PS_RELU | PS_L2NORM))) return PS_EINVAL;
    if (!z || !gy || !mean || !var || !scale || !beta || !workspace) return PS_EINVAL;
    if (reinterpret_cast<size_t>(workspace) % 8 != 0) return PS_EINVAL;
    if (workspace_bytes < ws_bytes(M, N)) return PS_EWORKSPACE;
    const int64_t P = ps_bn_partitions(M);
    const int64_t row_blocks = ps_cdiv(M, 4);
    if (row_blocks > 0x7fffffff) return PS_EUNSUPPORTED;                  // every row has a wave of its own
    const bool vec4 = (N % 4 == 0) && ps_aligned16({z, gy, mean, var, scale, beta, gz});     // gz may be absent
    const bool l2 = (flags & PS_L2NORM) != 0;
    const int64_t col_blocks = ps_cdiv(N, vec4 ? 256 : 64);
    if (col_blocks > 65535) return PS_EUNSUPPORTED;                       // grid.y of the column-sum pass
    if (!gz && !dgamma && !dbeta) return PS_OK;
    hipStream_t st = ps_stream(stream);
    const BnBwdWs w = ws_carve(workspace, M, N);
    const int ldc = col_ld(N);
    const dim3 rows_g((unsigned)row_blocks), cols_g((unsigned)P, (unsigned)col_blocks);
    if (l2) {
        PS_LAUNCH_VEC(bn_bwd_rowscal_kernel<VEC>, vec4, rows_g, dim3(256), st, z, gy, M, N, mean, scale, beta, flags, w.rows);
        PS_CHECK_LAUNCH();
    }
    PS_LAUNCH_VEC(bn_bwd_partial_kernel<VEC>, vec4, cols_g, dim3(256), st, z, gy, M, N, mean, var, scale, beta, eps, flags, w.rows,
                  w.part);
    PS_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3((unsigned)ps_cdiv(N, 64)), dim3(64), 0, st, w.part, P, M, N, var, eps, dgamma, dbeta,
                       w.colv, ldc);
    PS_CHECK_LAUNCH();
    if (gz) {
        PS_LAUNCH_VEC(bn_bwd_apply_kernel<VEC>, vec4, rows_g, dim3(256), st, z, gy, M, N, mean, scale, beta, flags, w.rows, w.colv, ldc,
                      gz);
        PS_CHECK_LAUNCH();
    }
    return PS_OK;
}

}  // namespace

extern "C" size_t ps_bn_bwd_workspace_bytes(int64_t M, int N) {
    if (M < 2 || N < 1) return 0;
    return ws_bytes(M, N);
}

extern "C" int ps_bn_bwd(const float *z, const float *gy, int64_t M, int N, const float *mean, const float *var, const float *scale,
                         const float *beta, float eps, int flags, float *gz, float *dgamma, float *dbeta, void *workspace,
                         size_t workspace_bytes, ps_stream_t stream) {
    return bn_bwd_launch(z, gy, M, N, mean, var, scale, beta, eps, flags, gz, dgamma, dbeta, workspace, workspace_bytes, stream);
}
