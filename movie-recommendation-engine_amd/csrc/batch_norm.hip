// batch_norm.hip -- nn.BatchNorm1d of GraphConvLayer (reference model/layers.py:68-75) on gfx950: column statistics of z[M, N]
// and the per-column affine map with the layer's ReLU and F.normalize behind it (two HBM-bound sweeps over z).
//
// ps_bn_batch_stats  one pass over z, the column-sum skeleton of col_sums.h with z and z * z as the two addends (the square of an
//                    fp32 value is exact in fp64): a workgroup takes a partition of PS_BN_ROWS rows and 64 * VEC columns and
//                    strides over the partitions when there are more than 65 535; a second kernel adds the partitions in
//                    ascending order, one lane per column, and makes mean / var / scale and the running update.
// ps_bn_apply        one wave per row, the sweeps of row_sweep.h: 16 B per lane when N % 4 == 0 and the
//                    pointers allow it, a scalar sweep otherwise, grid-stride over the rows.  Rows of up to KEEP sweeps stay in
//                    registers between the sum of squares and the division; longer rows are read a second time (by the lane
//                    that writes the same addresses afterwards, so y may be z).
#include "ps_common.h"
#include "col_sums.h"
#include "row_sweep.h"

namespace {

constexpr int BN_UNROLL = 8;       // rows a wave has in flight
constexpr int KEEP = 4;            // sweeps of a row that ps_bn_apply keeps in registers

// part[p, 0, c] = sum of z[r, c], part[p, 1, c] = sum of z[r, c]^2 over the rows r of partition p (double[P, 2, N])
template <int VEC>
__global__ __launch_bounds__(256) void bn_partial_kernel(const float *__restrict__ z, int64_t M, int N, int64_t P,
                                                         double *__restrict__ part) {
    struct Row { float z[VEC]; };
    const int col = (int)blockIdx.y * 64 * VEC + (threadIdx.x & 63) * VEC;
    for (int64_t p = blockIdx.x; p < P; p += gridDim.x) {
        ps_col_sums_partition<VEC, BN_UNROLL, false>(
            M, N, p, col,
            [&](int64_t rr, bool live) {
                Row row;
                load_vec<VEC>(z + rr * N + col, col < N && live, row.z);
                return row;
            },
            [](const Row &row, int e, double &a, double &b) {
                a = (double)row.z[e];                                    // a row past the partition: +0.0 and +0.0
                b = a * a;
            },
            part);
        __syncthreads();                                                 // the LDS words are reused by the next partition
    }
}

__global__ __launch_bounds__(64) void bn_finish_kernel(const double *__restrict__ part, int64_t P, int64_t M, int N,
                                                       const float *__restrict__ gamma, double eps, double momentum,
                                                       float *__restrict__ running_mean, float *__restrict__ running_var,
                                                       float *__restrict__ mean, float *__restrict__ var,
                                                       float *__restrict__ scale) {
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < N; c += gridDim.x * blockDim.x) {
        const double2 sq = ps_col_sums_finish(part, P, N, c);
        const double m = sq.x / (double)M;
        double v = sq.y / (double)M - m * m;
        v = v > 0.0 ? v : 0.0;
        mean[c] = (float)m;
        var[c] = (float)v;
        scale[c] = (float)((double)gamma[c] / sqrt(v + eps));
        if (running_mean) {
            const double unbiased = v * ((double)M / (double)(M - 1));
            running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * m);
            running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unbiased);
        }
    }
}

// t = fmaf(z - mean, scale, beta), ReLU when RELU
template <int VEC>
__device__ __forceinline__ void bn_affine(const float (&zz)[VEC], const float (&mm)[VEC], const float (&sc)[VEC],
                                          const float (&bb)[VEC], bool relu, float (&t)[VEC]) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) t[e] = ps_bn_act(zz[e] - mm[e], sc[e], bb[e], relu);
}

template <int VEC>
__global__ __launch_bounds__(256) void bn_apply_kernel(const float *z, int64_t M, int N, const float *__restrict__ mean,
                                                       const float *__restrict__ scale, const float *__restrict__ beta,
                                                       int flags, float *y) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int nwaves = (int)((gridDim.x * blockDim.x) >> 6);
    const int chunk = 64 * VEC;
    const bool relu = (flags & PS_RELU) != 0, l2 = (flags & PS_L2NORM) != 0;
    const bool fits = N <= KEEP * chunk;
    // the first KEEP sweeps' share of the column vectors is the same for every row
    float m0[KEEP][VEC], s0[KEEP][VEC], b0[KEEP][VEC];
#pragma unroll
    for (int k = 0; k < KEEP; ++k) {
        const int col = k * chunk + lane * VEC;
        load_vec<VEC>(mean + col, col < N, m0[k]);
        load_vec<VEC>(scale + col, col < N, s0[k]);
        load_vec<VEC>(beta + col, col < N, b0[k]);
    }
    for (int64_t i = wave; i < M; i += nwaves) {
        const float *zr = z + i * N;
        float *yr = y + i * N;
        float t[KEEP][VEC];
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < KEEP; ++k) {
            const int col = k * chunk + lane * VEC;
            float zz[VEC];
            load_vec<VEC>(zr + col, col < N, zz);
            bn_affine<VEC>(zz, m0[k], s0[k], b0[k], relu, t[k]);         // a column past N: fmaf(0 - 0, 0, 0) = +0.0
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc = fmaf(t[k][e], t[k][e], acc);
        }
        // the rest of a long row, for both passes: use(col, cact, tt) gets the activation of every further sweep
        auto rest = [&](auto use) {
            for (int c0 = KEEP * chunk; c0 < N; c0 += chunk) {
                const int col = c0 + lane * VEC;
                float tt[VEC];
                ps_bn_act_vec<VEC>(zr, mean, scale, beta, col, col < N, relu, tt);
                use(col, col < N, tt);
            }
        };
        if (!fits && l2) {
            rest([&](int, bool, const float (&tt)[VEC]) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc = fmaf(tt[e], tt[e], acc);
            });
        }
        float nrm = 1.f;
        if (l2) {
            nrm = ps_row_clamp(ps_row_norm(acc));                        // a NaN norm stays: the whole row is NaN
        }
#pragma unroll
        for (int k = 0; k < KEEP; ++k) {
            const int col = k * chunk + lane * VEC;
            if (col < N) {
                float o[VEC];
#pragma unroll
                for (int e = 0; e < VEC; ++e) o[e] = l2 ? t[k][e] / nrm : t[k][e];
                store_vec<VEC>(yr + col, o);
            }
        }
        if (!fits) {
            // every lane reads again what it is about to overwrite (y may be z)
            rest([&](int col, bool cact, const float (&tt)[VEC]) {
                if (cact) {
                    float o[VEC];
#pragma unroll
                    for (int e = 0; e < VEC; ++e) o[e] = l2 ? tt[e] / nrm : tt[e];
                    store_vec<VEC>(yr + col, o);
                }
            });
        }
    }
}

}  // namespace

extern "C" size_t ps_bn_stats_workspace_bytes(int64_t M, int N) {
    if (M < 2 || N < 1) return 0;
    return (size_t)ps_bn_partitions(M) * 2 * (size_t)N * sizeof(double);
}

extern "C" int ps_bn_batch_stats(const float *z, int64_t M, int N, const float *gamma, float eps, float momentum,
                                 float *running_mean, float *running_var, float *mean, float *var, float *scale,
                                 void *workspace, size_t workspace_bytes, ps_stream_t stream) {
    if (M < 2 || N < 1 || !z || !gamma || !mean || !var || !scale || !workspace) return PS_EINVAL;
    if ((running_mean == nullptr) != (running_var == nullptr)) return PS_EINVAL;
    if (workspace_bytes < ps_bn_stats_workspace_bytes(M, N) || reinterpret_cast<size_t>(workspace) % 8 != 0) return PS_EINVAL;
    hipStream_t st = ps_stream(stream);
    const int64_t P = ps_bn_partitions(M);
    double *part = static_cast<double *>(workspace);
    const unsigned gx = (unsigned)(P > 65535 ? 65535 : P);
    const bool vec4 = (N % 4 == 0) && ps_aligned16({z});
    PS_LAUNCH_VEC(bn_partial_kernel<VEC>, vec4, dim3(gx, (unsigned)ps_cdiv(N, 64 * VEC)), dim3(256), st, z, M, N, P, part);
    PS_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_finish_kernel, dim3((unsigned)ps_cdiv(N, 64)), dim3(64), 0, st, part, P, M, N, gamma, (double)eps,
                       (double)momentum, running_mean, running_var, mean, var, scale);
    PS_CHECK_LAUNCH();
    return PS_OK;
}

extern "C" int ps_bn_apply(const float *z, int64_t M, int N, const float *mean, const float *scale, const float *beta, int flags,
                           float *y, ps_stream_t stream) {
    if (M < 0 || N < 1 || (flags & ~(PS_RELU | PS_L2NORM))) return PS_EINVAL;
    if (M == 0) return PS_OK;                                 // before the pointers: an empty tensor's base is NULL
    if (!z || !mean || !scale || !beta || !y) return PS_EINVAL;
    hipStream_t st = ps_stream(stream);
    const bool vec4 = (N % 4 == 0) && ps_aligned16({z, y, mean, scale, beta});
    PS_LAUNCH_VEC(bn_apply_kernel<VEC>, vec4, dim3(ps_row_grid(M)), dim3(256), st, z, M, N, mean, scale, beta, flags, y);
    PS_CHECK_LAUNCH();
    return PS_OK;
}
