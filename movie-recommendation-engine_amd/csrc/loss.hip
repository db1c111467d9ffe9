// loss.hip -- the ranking losses of the reference's model/loss.py (MaxMarginRankingLoss, BatchHardTripletLoss, CurriculumLoss)
// from ONE packed word per query row: the largest negative similarity and the smallest index that attains it.
//
//   ps_hardest_negative : best[b] = max_j ps_best_pack(Q_b . X_j, j) (csrc/ps_select.h).  Shared candidates X [N, D]: ps_linear's
//                         fp32-MFMA tiles with a row-arg-max epilogue (csrc/dense_mfma.hip, EPI 3), no [B, N] slab.  Per-query
//                         candidates X [B, N, D]: one thread per candidate row, the fmaf chain of ps_row_dot.  Both are the chain
//                         acc = fmaf(q[k], x[k], acc), k ascending from +0.0, so the two forms agree bit for bit on equal data.
//   ps_margin_loss      : per row relu((margin + neg) - pos), the active mask, the arg-max index, and the mean over the rows by
//                         a reduction of fixed shape (per-thread strided sums, then a tree in LDS): the same bits on every run.
//   ps_margin_loss_bwd  : the closed-form gradient over those indices (include/pinsage_hip.h); every sum over rows runs in
//                         ascending row order inside one wave -- no float atomics anywhere in this file.
#include "ps_select.h"

namespace {

// acc = fmaf(x[k], y[k], acc), k ascending from +0.0: row_dot_kernel's chain (csrc/ps_common.h)
__device__ __forceinline__ float chain_dot(const float *__restrict__ x, const float *__restrict__ y, int D, bool vec) {
    return ps_fma_chain(x, y, D, vec, 0.f);
}

__device__ __forceinline__ bool vec_ok(const float *a, const float *b, int D) {
    return D % 4 == 0 && reinterpret_cast<size_t>(a) % 16 == 0 && reinterpret_cast<size_t>(b) % 16 == 0;
}

// per-query candidates: thread i = (b, n) reads row i of X once
__global__ void hardest_rows_kernel(const float *__restrict__ Q, const float *__restrict__ X, int64_t B, int64_t N, int D,
                                    unsigned long long *__restrict__ best) {
    const bool vec = vec_ok(Q, X, D);
    const int64_t total = B * N;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / N, n = i - b * N;
        const float s = chain_dot(Q + b * D, X + i * D, D, vec);
        atomicMax(best + b, ps_best_pack(s, (uint32_t)n));
    }
}

__global__ void best_unpack_kernel(const unsigned long long *__restrict__ best, int64_t B, float *__restrict__ sim,
                                   int64_t *__restrict__ idx) {
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < B; b += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long w = best[b];
        if (sim) sim[b] = ps_best_sim(w);
        if (idx) idx[b] = ps_best_idx(w);
    }
}

// relu and its mask as torch evaluates them: relu(NaN) = NaN, and the gradient passes wherever !(x <= 0)
__global__ void hinge_rows_kernel(const float *__restrict__ Q, const float *__restrict__ P, int64_t B, int D,
                                  const unsigned long long *__restrict__ best, float margin, float *__restrict__ row_loss,
                                  int64_t *__restrict__ idx, uint8_t *__restrict__ active) {
    const bool vec = vec_ok(Q, P, D);
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < B; b += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long w = best[b];
        const float pos = chain_dot(Q + b * D, P + b * D, D, vec);
        const float l = (margin + ps_best_sim(w)) - pos;
        row_loss[b] = l <= 0.f ? 0.f : l;
        idx[b] = ps_best_idx(w);
        active[b] = l <= 0.f ? 0 : 1;
    }
}

constexpr int MEAN_THREADS = 1024;
__global__ __launch_bounds__(MEAN_THREADS) void mean_kernel(const float *__restrict__ v, int64_t B, float *__restrict__ out) {
    __shared__ float s[MEAN_THREADS];
    const int tid = threadIdx.x;
    float t = 0.f;
    for (int64_t b = tid; b < B; b += MEAN_THREADS) t += v[b];
    s[tid] = t;
    __syncthreads();
    for (int w = MEAN_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) s[tid] += s[tid + w];
        __syncthreads();
    }
    if (tid == 0) out[0] = s[0] / (float)B;
}

// One wave per query row b: dQ[b] = g X[a] + (-g P[b]), dP[b] = -g Q[b]; per-query candidates also dX[b, n] = g Q[b] for
// n = a and +0.0 for every other n.  g = grad_out / B on an active row with an index inside [0, N), else 0.
__global__ __launch_bounds__(256) void loss_bwd_rows_kernel(const float *__restrict__ Q, const float *__restrict__ P,
                                                            const float *__restrict__ X, int64_t B, int64_t N, int D, int mode,
                                                            const int64_t *__restrict__ idx, const uint8_t *__restrict__ active,
                                                            const float *__restrict__ grad_out, float *__restrict__ dQ,
                                                            float *__restrict__ dP, float *__restrict__ dX) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const float go = grad_out[0];
    for (int64_t b = wave; b < B; b += nw) {
        const int64_t a = idx[b];
        const bool hit = a >= 0 && a < N;
        const float g = (active[b] && hit) ? go / (float)B : 0.f;
        const float *q = Q + b * D;
        if (dQ) {
            const float *p = P + b * D;
            const float *xa = hit ? X + (mode == PS_LOSS_PER_QUERY ? b * N + a : a) * D : nullptr;
            for (int k = lane; k < D; k += 64) {
                const float t = hit ? g * xa[k] : 0.f;
                dQ[b * D + k] = t + (-g * p[k]);
            }
        }
        if (dP)
            for (int k = lane; k < D; k += 64) dP[b * D + k] = -g * q[k];
        if (dX)
            for (int64_t n = 0; n < N; ++n)
                for (int k = lane; k < D; k += 64) dX[(b * N + n) * D + k] = n == a ? g * q[k] : 0.f;
    }
}

// One wave per candidate row j: S_j = sum over the active rows b with idx[b] == j of g Q[b], b ASCENDING (the wave scans the B
// indices 64 at a time and walks the set bits of the ballot from the lowest), 256 columns per pass.
// shared candidates: out[j] = S_j (dX);  batch-hard: out[j] = (-g_j Q[j]) + S_j (dP).
constexpr int SCAT_KC = 4;
__global__ __launch_bounds__(256) void loss_bwd_scatter_kernel(const float *__restrict__ Q, int64_t B, int64_t N, int D, int mode,
                                                               const int64_t *__restrict__ idx, const uint8_t *__restrict__ active,
                                                               const float *__restrict__ grad_out, float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const float g = grad_out[0] / (float)B;
    for (int64_t j = wave; j < N; j += nw) {
        for (int k0 = 0; k0 < D; k0 += 64 * SCAT_KC) {
            float acc[SCAT_KC];
#pragma unroll
            for (int c = 0; c < SCAT_KC; ++c) acc[c] = 0.f;
            for (int64_t b0 = 0; b0 < B; b0 += 64) {
                const int64_t b = b0 + lane;
                unsigned long long m = __ballot(b < B && idx[b] == j && active[b] != 0);
                while (m) {
                    const int t = __builtin_ctzll(m);
                    m &= m - 1;
                    const float *q = Q + (b0 + t) * D;
#pragma unroll
                    for (int c = 0; c < SCAT_KC; ++c) {
                        const int k = k0 + lane + 64 * c;
                        if (k < D) acc[c] = acc[c] + g * q[k];
                    }
                }
            }
            float gj = 0.f;
            if (mode == PS_LOSS_BATCH_HARD) {                      // j < B = N: the row's own -g_j Q[j]
                const int64_t a = idx[j];
                gj = (active[j] && a >= 0 && a < N) ? g : 0.f;
            }
#pragma unroll
            for (int c = 0; c < SCAT_KC; ++c) {
                const int k = k0 + lane + 64 * c;
                if (k < D) out[j * D + k] = mode == PS_LOSS_BATCH_HARD ? (-gj * Q[j * D + k]) + acc[c] : acc[c];
            }
        }
    }
}

unsigned grid_for(int64_t items, int per_block) {
    int64_t g = ps_cdiv(items, per_block);
    return (unsigned)(g > 4096 ? 4096 : g < 1 ? 1 : g);
}

}  // namespace

extern "C" int ps_hardest_negative(const float *Q, int64_t B, int D, const float *X, int64_t N, int flags, uint64_t *best,
                                   float *sim, int64_t *idx, ps_stream_t stream) {
    if (B < 0 || N < 0 || D <= 0 || (flags & ~(PS_HN_PER_QUERY | PS_HN_EXCLUDE_DIAG))) return PS_EINVAL;
    if (B > 0x7fffffff || N > 0x7fffffff) return PS_EUNSUPPORTED;
    if (B == 0) return PS_OK;
    if (N == 0) return PS_EINVAL;                                  // a maximum over no candidate
    if (!Q || !X || !best || reinterpret_cast<size_t>(best) % 8 != 0) return PS_EINVAL;
    if ((flags & PS_HN_PER_QUERY) && (flags & PS_HN_EXCLUDE_DIAG)) return PS_EINVAL;
    hipStream_t st = ps_stream(stream);
    unsigned long long *w = reinterpret_cast<unsigned long long *>(best);
    if (ps_fill_async(w, 0, sizeof(unsigned long long) * (size_t)B, st) != hipSuccess) return PS_ELAUNCH;
    if (flags & PS_HN_PER_QUERY) {
        hipLaunchKernelGGL(hardest_rows_kernel, dim3(grid_for(B * N, 256)), dim3(256), 0, st, Q, X, B, N, D, w);
        PS_CHECK_LAUNCH();
    } else {
        const int rc = psi_hardest_shared(Q, B, D, X, N, (flags & PS_HN_EXCLUDE_DIAG) ? 1 : 0, w, stream);
        if (rc != PS_OK) return rc;
    }
    if (sim || idx) {
        hipLaunchKernelGGL(best_unpack_kernel, dim3(grid_for(B, 256)), dim3(256), 0, st, w, B, sim, idx);
        PS_CHECK_LAUNCH();
    }
    return PS_OK;
}

extern "C" int ps_margin_loss(const float *Q, const float *P, int64_t B, int D, const uint64_t *best, float margin,
                              float *row_loss, int64_t *idx, uint8_t *active, float *loss, ps_stream_t stream) {
    if (B < 0 || D <= 0) return PS_EINVAL;
    if (B > 0x7fffffff) return PS_EUNSUPPORTED;
    if (B == 0) return PS_OK;
    if (!Q || !P || !best || !row_loss || !idx || !active || !loss) return PS_EINVAL;
    hipStream_t st = ps_stream(stream);
    hipLaunchKernelGGL(hinge_rows_kernel, dim3(grid_for(B, 64)), dim3(64), 0, st, Q, P, B, D,
                       reinterpret_cast<const unsigned long long *>(best), margin, row_loss, idx, active);
    PS_CHECK_LAUNCH();
    hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(MEAN_THREADS), 0, st, row_loss, B, loss);
    PS_CHECK_LAUNCH();
    return PS_OK;
}

extern "C" int ps_margin_loss_bwd(const float *Q, const float *P, const float *X, int64_t B, int64_t N, int D, int mode,
                                  const int64_t *idx, const uint8_t *active, const float *grad_out, float *dQ, float *dP,
                                  float *dX, ps_stream_t stream) {
    if (B < 0 || N < 0 || D <= 0) return PS_EINVAL;
    if (mode != PS_LOSS_SHARED && mode != PS_LOSS_PER_QUERY && mode != PS_LOSS_BATCH_HARD) return PS_EINVAL;
    if (B > 0x7fffffff || N > 0x7fffffff) return PS_EUNSUPPORTED;
    if (mode == PS_LOSS_BATCH_HARD && (N != B || dX)) return PS_EINVAL;      // the candidates ARE the positives: their gradient is dP
    if (B == 0) return PS_OK;
    if (!Q || !P || !idx || !active || !grad_out) return PS_EINVAL;
    if (mode != PS_LOSS_BATCH_HARD && !X && (dQ || dX)) return PS_EINVAL;
    hipStream_t st = ps_stream(stream);
    const bool hard = mode == PS_LOSS_BATCH_HARD;
    float *row_dP = hard ? nullptr : dP, *row_dX = mode == PS_LOSS_PER_QUERY ? dX : nullptr;
    if (dQ || row_dP || row_dX) {
        hipLaunchKernelGGL(loss_bwd_rows_kernel, dim3(grid_for(B, 4)), dim3(256), 0, st, Q, P, hard ? P : X, B, N, D, mode, idx,
                           active, grad_out, dQ, row_dP, row_dX);
        PS_CHECK_LAUNCH();
    }
    float *scat = hard ? dP : mode == PS_LOSS_SHARED ? dX : nullptr;
    if (scat && N > 0) {
        hipLaunchKernelGGL(loss_bwd_scatter_kernel, dim3(grid_for(N, 4)), dim3(256), 0, st, Q, B, N, D, mode, idx, active, grad_out,
                           scat);
        PS_CHECK_LAUNCH();
    }
    return PS_OK;
}
