// linear_bwd.hip -- the backward of the dense layers (pinsage_hip/dense.py: LinearFn) on gfx950: the weight-gradient GEMM
// dW = g^T x with the bias gradient beside it, and the backward of ps_linear's ReLU / row-norm epilogue.  (The input gradient
// dx = g W is ps_linear itself over W^T.)  No float atomics: every output bit is a function of the inputs.
//
// ps_linear_wgrad         The contraction index is the row index of both row-major operands, so the operands of
//                         v_mfma_f32_32x32x2_f32 -- lane l: A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31] -- are
//                         g[m + (l >> 5)][n0 + (l & 31)] and x[m + (l >> 5)][k0 + (l & 31)]: rows of the operands as they lie in
//                         memory, no transposition.  A work item is (128 x 128 tile of dW, row partition); its workgroup of four
//                         waves stages WG_ROWS rows of the tile's 128 columns of g and of x in LDS (16-byte requests on the fast
//                         path, 4-byte requests otherwise: the same floats in the same LDS words, so the same bits), the next
//                         chunk's requests in flight while the MFMAs of this one run, and every wave owns a 64 x 64 quarter as
//                         2 x 2 accumulators.  The MFMA adds rows m, m + 1 to an accumulator in that order (it is the fmaf chain
//                         bit for bit), so a partition's tile is the chain over its rows ascending.  A row past the partition and
//                         a column past N / K enter as zeros (fmaf(0, 0, acc) = acc: a chain from +0.0 holds no -0.0).  The
//                         workgroups of the first tile column add the bias gradient's chain from the staged g.  One partition:
//                         the tile goes to dW.  Several: to the workspace, and a second launch adds every element's partials in
//                         partition order.
// ps_linear_epilogue_bwd  one wave per row, the sweeps and the norm of ps_bn_apply (row_sweep.h).  Three sweeps over the row: the
//                         sum of squares of t and s = sum g y (ps_row_norm_sums), then the output; a lane reads g[c] for the last
//                         time before it writes gz[c], so gz may be g.
#include "ps_common.h"
#include "row_sweep.h"

namespace {

constexpr int64_t WG_PART = 512;       // the smallest row partition
constexpr int64_t WG_MAX_PARTS = 256;  // the partition doubles while there would be more
constexpr int WG_TILE = 128;           // a workgroup's tile of dW, both ways
constexpr int WG_ROWS = 32;            // rows staged per step

typedef float f32x16 __attribute__((ext_vector_type(16)));

inline int64_t wgrad_partition(int64_t M) {
    int64_t P = WG_PART;
    while (ps_cdiv(M, P) > WG_MAX_PARTS) P *= 2;
    return P;
}

// rows [m, m + WG_ROWS) x columns [c0, c0 + 128) of a row-major [M, ld] matrix: this thread's share, zeros past m1 / ld
template <bool VEC4>
__device__ __forceinline__ void wg_fetch(const float *__restrict__ a, int64_t m, int64_t m1, int ld, int c0, float (&r)[WG_ROWS / 2]) {
    const int tid = threadIdx.x;
    if (VEC4) {
#pragma unroll
        for (int i = 0; i < WG_ROWS / 8; ++i) {
            const int idx = tid + 256 * i;
            const int64_t row = m + (idx >> 5);
            const int col = c0 + 4 * (idx & 31);
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < m1 && col < ld) q = *reinterpret_cast<const float4 *>(a + row * ld + col);
            r[4 * i] = q.x; r[4 * i + 1] = q.y; r[4 * i + 2] = q.z; r[4 * i + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < WG_ROWS / 2; ++i) {
            const int idx = tid + 256 * i;
            const int64_t row = m + (idx >> 7);
            const int col = c0 + (idx & 127);
            r[i] = (row < m1 && col < ld) ? a[row * ld + col] : 0.f;
        }
    }
}

template <bool VEC4>
__device__ __forceinline__ void wg_stage(float (*s)[WG_TILE], const float (&r)[WG_ROWS / 2]) {
    const int tid = threadIdx.x;
    if (VEC4) {
#pragma unroll
        for (int i = 0; i < WG_ROWS / 8; ++i) {
            const int idx = tid + 256 * i;
            *reinterpret_cast<float4 *>(&s[idx >> 5][4 * (idx & 31)]) = make_float4(r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < WG_ROWS / 2; ++i) {
            const int idx = tid + 256 * i;
            s[idx >> 7][idx & 127] = r[i];
        }
    }
}

// dst / dbdst: dW / db themselves (stride 0, one partition) or the workspace's float[parts, N K] / float[parts, N]
template <bool VEC4>
__global__ __launch_bounds__(256) void wgrad_kernel(const float *__restrict__ g, const float *__restrict__ x, int64_t M, int N, int K,
                                                    int64_t P, int tiles_k, float *__restrict__ dst, int64_t dst_stride,
                                                    float *__restrict__ dbdst, int64_t db_stride) {
    __shared__ __attribute__((aligned(16))) float sg[WG_ROWS][WG_TILE];
    __shared__ __attribute__((aligned(16))) float sx[WG_ROWS][WG_TILE];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tn = (int)blockIdx.x / tiles_k, tk = (int)blockIdx.x % tiles_k;
    const int n0 = tn * WG_TILE, k0 = tk * WG_TILE;
    const int64_t p = blockIdx.y;
    const int64_t m0 = p * P;
    const int64_t m1 = (m0 + P < M) ? m0 + P : M;
    const int wn = (wave >> 1) * 64, wk = (wave & 1) * 64;
    const int half = lane >> 5, l31 = lane & 31;
    // 32 x 32 sub-tiles wholly past N or K are left out (wave-uniform); their accumulators stay +0.0 and are not stored
    bool on_n[2], on_k[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        on_n[i] = n0 + wn + 32 * i < N;
        on_k[i] = k0 + wk + 32 * i < K;
    }
    const bool bias = dbdst != nullptr && tk == 0 && tid < WG_TILE;
    float dbacc = 0.f;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float rg[WG_ROWS / 2], rx[WG_ROWS / 2];
    wg_fetch<VEC4>(g, m0, m1, N, n0, rg);
    wg_fetch<VEC4>(x, m0, m1, K, k0, rx);
    for (int64_t m = m0; m < m1; m += WG_ROWS) {
        __syncthreads();                                                 // the previous chunk has been read
        wg_stage<VEC4>(sg, rg);
        wg_stage<VEC4>(sx, rx);
        __syncthreads();
        if (m + WG_ROWS < m1) {
            wg_fetch<VEC4>(g, m + WG_ROWS, m1, N, n0, rg);
            wg_fetch<VEC4>(x, m + WG_ROWS, m1, K, k0, rx);
        }
        if (bias) {
#pragma unroll
            for (int r = 0; r < WG_ROWS; ++r) dbacc += sg[r][tid];
        }
#pragma unroll 4
        for (int s = 0; s < WG_ROWS / 2; ++s) {
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = sg[2 * s + half][wn + 32 * i + l31];
                b[i] = sx[2 * s + half][wk + 32 * i + l31];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (on_n[i] && on_k[j]) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
    float *out = dst + p * dst_stride;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int kc = k0 + wk + 32 * j + l31;
            if (!(on_n[i] && on_k[j]) || kc >= K) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + wn + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (n < N) out[(int64_t)n * K + kc] = acc[i][j][r];
            }
        }
    if (bias && n0 + tid < N) dbdst[p * db_stride + n0 + tid] = dbacc;
}

// out[e] = ((part[0, e] + part[1, e]) + part[2, e]) + ... for the N K elements of dW, then (db given) the N of db
__global__ __launch_bounds__(256) void wgrad_sum_kernel(const float *__restrict__ wpart, const float *__restrict__ bpart, int64_t parts,
                                                        int64_t nk, int N, float *__restrict__ dW, float *__restrict__ db) {
    const int64_t total = nk + (db ? N : 0);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const bool w = e < nk;
        const float *src = w ? wpart + e : bpart + (e - nk);
        const int64_t step = w ? nk : N;
        float s = src[0];
#pragma unroll 8
        for (int64_t q = 1; q < parts; ++q) s += src[q * step];
        if (w) dW[e] = s;
        else db[e - nk] = s;
    }
}

template <int VEC>
__global__ __launch_bounds__(256) void epilogue_bwd_kernel(const float *t, const float *g, int64_t M, int N, int flags, float *gz) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int nwaves = (int)((gridDim.x * blockDim.x) >> 6);
    const int chunk = 64 * VEC;
    const bool relu = (flags & PS_RELU) != 0, l2 = (flags & PS_L2NORM) != 0;
    for (int64_t i = wave; i < M; i += nwaves) {
        const float *tr = t + i * N;
        const float *gr = g + i * N;
        float *zr = gz + i * N;
        float c = 1.f, s = 0.f;
        bool below = false;
        if (l2) {
            const float2 ns = ps_row_norm_sums<VEC>(N, gr, [&](int col, bool ok, float (&tt)[VEC]) { load_vec<VEC>(tr + col, ok, tt); });
            c = ps_row_clamp(ns.x);
            below = ns.x < 1e-12f;
            s = ns.y;
        }
        for (int c0 = 0; c0 < N; c0 += chunk) {
            const int col = c0 + lane * VEC;
            if (col >= N) continue;
            float tt[VEC], gg[VEC], o[VEC];
            load_vec<VEC>(tr + col, true, tt);
            load_vec<VEC>(gr + col, true, gg);
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[e] = ps_epilogue_ga(tt[e], gg[e], relu, l2, c, below, s);
            store_vec<VEC>(zr + col, o);
        }
    }
}

}  // namespace

extern "C" int64_t ps_linear_wgrad_partition(int64_t M) { return wgrad_partition(M); }

extern "C" size_t ps_linear_wgrad_workspace_bytes(int64_t M, int N, int K) {
    if (N < 1 || K < 1 || M <= wgrad_partition(M)) return 0;
    const size_t parts = (size_t)ps_cdiv(M, wgrad_partition(M));
    return 256 + parts * ((size_t)N * (size_t)K + (size_t)N) * sizeof(float);
}

// ps_linear_wgrad with the partition size given (P == 0: the rule's)
static int wgrad_launch(const float *g, int64_t M, int N, const float *x, int K, float *dW, float *db, void *workspace,
                        size_t workspace_bytes, ps_stream_t stream, int64_t P_given) {
    if (M < 0 || N < 1 || K < 1 || !dW) return PS_EINVAL;
    hipStream_t st = ps_stream(stream);
    const int64_t nk = (int64_t)N * K;
    if (M == 0) {                                             // before the operands: an empty tensor's base is NULL
        if (ps_fill_async(dW, 0, (size_t)nk * sizeof(float), st) != hipSuccess) return PS_ELAUNCH;
        if (db && ps_fill_async(db, 0, (size_t)N * sizeof(float), st) != hipSuccess) return PS_ELAUNCH;
        return PS_OK;
    }
    if (!g || !x) return PS_EINVAL;
    const int64_t P = P_given > 0 ? P_given : wgrad_partition(M);
    const int64_t parts = ps_cdiv(M, P);
    const int tiles_n = (int)ps_cdiv(N, WG_TILE), tiles_k = (int)ps_cdiv(K, WG_TILE);
    if ((int64_t)tiles_n * tiles_k > 0x7fffffff) return PS_EUNSUPPORTED;
    float *dst = dW, *dbdst = db, *wpart = nullptr, *bpart = nullptr;
    int64_t dst_stride = 0, db_stride = 0;
    if (parts > 1) {
        if (!workspace) return PS_EINVAL;
        if (workspace_bytes < 256 + (size_t)parts * ((size_t)nk + (size_t)N) * sizeof(float)) return PS_EWORKSPACE;
        wpart = reinterpret_cast<float *>(ps_ws_base(workspace));
        bpart = wpart + parts * nk;
        dst = wpart;
        dst_stride = nk;
        if (db) {
            dbdst = bpart;
            db_stride = N;
        }
    }
    const bool vec4 = N % 4 == 0 && K % 4 == 0 && ps_aligned16({g, x});
    const dim3 grid((unsigned)(tiles_n * tiles_k), (unsigned)parts);
    if (vec4)
        hipLaunchKernelGGL(wgrad_kernel<true>, grid, dim3(256), 0, st, g, x, M, N, K, P, tiles_k, dst, dst_stride, dbdst, db_stride);
    else
        hipLaunchKernelGGL(wgrad_kernel<false>, grid, dim3(256), 0, st, g, x, M, N, K, P, tiles_k, dst, dst_stride, dbdst, db_stride);
    PS_CHECK_LAUNCH();
    if (parts > 1) {
        const int64_t total = nk + (db ? N : 0);
        const int64_t blocks = ps_cdiv(total, 256);
        hipLaunchKernelGGL(wgrad_sum_kernel, dim3((unsigned)(blocks > 65535 ? 65535 : blocks)), dim3(256), 0, st, wpart, bpart, parts, nk,
                           N, dW, db);
        PS_CHECK_LAUNCH();
    }
    return PS_OK;
}

extern "C" int ps_linear_wgrad(const float *g, int64_t M, int N, const float *x, int K, float *dW, float *db, void *workspace,
                               size_t workspace_bytes, ps_stream_t stream) {
    return wgrad_launch(g, M, N, x, K, dW, db, workspace, workspace_bytes, stream, 0);
}

// an export outside the header, for tools/linear_bwd_probe.py: the same launches with partitions of P rows (P > 0, at most 65 535
// partitions; workspace 256 + ceil(M / P) (N K + N) floats), to measure the candidates of the partition rule
extern "C" int ps_debug_linear_wgrad(const float *g, int64_t M, int N, const float *x, int K, float *dW, float *db, void *workspace,
                                     size_t workspace_bytes, ps_stream_t stream, int64_t P) {
    if (P < 1 || ps_cdiv(M, P) > 65535) return PS_EINVAL;
    return wgrad_launch(g, M, N, x, K, dW, db, workspace, workspace_bytes, stream, P);
}

extern "C" int ps_linear_epilogue_bwd(const float *t, const float *g, int64_t M, int N, int flags, float *gz, ps_stream_t stream) {
    if (M < 0 || N < 1 || (flags & ~(PS_RELU | PS_L2NORM))) return PS_EINVAL;
    if (M == 0) return PS_OK;                                 // before the pointers: an empty tensor's base is NULL
    if (!g || !gz || (flags && !t)) return PS_EINVAL;
    hipStream_t st = ps_stream(stream);
    if (!flags) {                                             // gz = g
        if (gz != g && ps_copy_async(gz, g, (size_t)M * (size_t)N * sizeof(float), st) != hipSuccess) return PS_ELAUNCH;
        return PS_OK;
    }
    const bool vec4 = (N % 4 == 0) && ps_aligned16({t, g, gz});
    PS_LAUNCH_VEC(epilogue_bwd_kernel<VEC>, vec4, dim3(ps_row_grid(M)), dim3(256), st, t, g, M, N, flags, gz);
    PS_CHECK_LAUNCH();
    return PS_OK;
}
