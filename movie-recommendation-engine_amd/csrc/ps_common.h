// Shared helpers for the gfx950 kernels of libpinsage_hip.so (CDNA4 only: wave = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <initializer_list>
#include "../../include/pinsage_hip.h"

#define PS_WAVE 64

#define PS_CHECK_LAUNCH()                                   \
    do {                                                    \
        hipError_t e_ = hipGetLastError();                  \
        if (e_ != hipSuccess) return PS_ELAUNCH;            \
    } while (0)

static inline hipStream_t ps_stream(ps_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Per-device results of one-time host queries (function attributes set, resident-workgroup counts).  The work behind them is
// idempotent, so two host threads that make a first call at the same time merely both do it; the slots are atomics so that this
// repeat is the ONLY consequence (no torn or stale read): the library keeps no state a caller could observe
// (include/pinsage_hip.h).  Zero-initialised statics; 0 = not known yet.
struct PsPerDevice {
    std::atomic<int> v[64];
    int get(int dev) const { return v[dev].load(std::memory_order_acquire); }
    void set(int dev, int x) { v[dev].store(x, std::memory_order_release); }
};
// the current device's slot of a PsPerDevice; false: no device, or one beyond the 64 slots
static inline bool ps_device_index(int *dev) { return hipGetDevice(dev) == hipSuccess && *dev >= 0 && *dev < 64; }
// dynamic LDS beyond 64 KiB has to be allowed per kernel and device (idempotent; every caller remembers it in a PsPerDevice of
// its OWN: one process may drive several GPUs)
template <typename K>
bool ps_allow_lds(K kernel, size_t bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) ==
           hipSuccess;
}
// ... for launchers whose slot remembers nothing else: allow `bytes` for every kernel of the list on the current device,
// once per device; false: no device slot, or the runtime refused
template <typename... K>
bool ps_allow_lds_once(PsPerDevice &done, size_t bytes, K... kernels) {
    int dv = 0;
    if (!ps_device_index(&dv)) return false;
    if (done.get(dv)) return true;
    if (!(ps_allow_lds(kernels, bytes) && ...)) return false;
    done.set(dv, 1);
    return true;
}

static inline int64_t ps_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
// workspaces are carved in 256-byte units from the first 256-byte boundary at or after the caller's pointer
static inline size_t ps_align256(size_t x) { return (x + 255) / 256 * 256; }
static inline char *ps_ws_base(void *workspace) { return reinterpret_cast<char *>(ps_align256(reinterpret_cast<size_t>(workspace))); }

// ---- launch glue of the row and column kernels ----
// one wave per row, 4 waves per workgroup; beyond 16 384 waves the kernel strides over the rows (no caller passes rows < 1)
static inline unsigned ps_row_grid(int64_t rows) {
    const int64_t grid = ps_cdiv(rows, 4);
    return (unsigned)(grid > 256 * 16 ? 256 * 16 : (grid < 1 ? 1 : grid));
}
// four rows per wave (a 16-lane group each: csrc/pool_row.h), 16 per workgroup
static inline unsigned ps_row4_grid(int64_t rows) {
    const int64_t grid = ps_cdiv(rows, 16);
    return (unsigned)(grid > 256 * 64 ? 256 * 64 : (grid < 1 ? 1 : grid));
}
// may every pointer be the base of 16-byte requests?  A null (absent) pointer does not object.
static inline bool ps_aligned16(std::initializer_list<const void *> ps) {
    size_t m = 0;
    for (const void *p : ps) m |= reinterpret_cast<size_t>(p);
    return m % 16 == 0;
}
// A kernel template's 16-byte or 4-byte form: KERNEL is written with VEC where the floats per lane go, e.g.
// PS_LAUNCH_VEC(bn_apply_kernel<VEC>, vec4, ...) or PS_LAUNCH_VEC((transposed_kernel<VEC, MODE>), vec4, ...).
#define PS_LAUNCH_VEC(KERNEL, vec4, grid, block, stream, ...)                     \
    do {                                                                          \
        if (vec4) {                                                               \
            constexpr int VEC = 4;                                                \
            hipLaunchKernelGGL(KERNEL, grid, block, 0, stream, __VA_ARGS__);      \
        } else {                                                                  \
            constexpr int VEC = 1;                                                \
            hipLaunchKernelGGL(KERNEL, grid, block, 0, stream, __VA_ARGS__);      \
        }                                                                         \
    } while (0)

// Fills and device-to-device copies inside an entry point are plain kernels (ps_fill_async / ps_copy_async), not
// hipMemsetAsync / hipMemcpyAsync.  Captured into a hipGraph those two become memset / memcpy NODES.  Observed on the MI355X
// (tests/test_hip_abi_contract.py against a build with hipMemsetAsync; capture by torch.cuda.graph, one stream): the first
// replay was right, and from the second replay on the ranges that seven entry points clear held bytes that were neither the
// zeros asked for nor what the range held before -- pointer-like words in ps_graph_stats' flags.  What the node wrote was not
// isolated outside that setting, so this is a record of the symptom, not a statement about the runtime.  A kernel node replays
// like every other launch of the call.  (Only memset nodes were seen to fail; the generator's three copies go the same way so
// that a captured call consists of kernel nodes alone.  rocprim's sort: see csrc/csr_build.hip.)  Any alignment and size; nothing
// outside [dst, dst + nbytes) is written.
static __global__ void ps_fill_kernel(unsigned char *dst, unsigned int byte, size_t nbytes) {
    size_t head = (16 - (reinterpret_cast<size_t>(dst) & 15)) & 15;          // bytes in front of the first 16-byte boundary
    if (head > nbytes) head = nbytes;
    const size_t body = (nbytes - head) / 16;
    const unsigned int w = (byte & 0xffu) * 0x01010101u;
    const uint4 v = make_uint4(w, w, w, w);
    uint4 *b = reinterpret_cast<uint4 *>(dst + head);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < body; i += stride) b[i] = v;
    if (blockIdx.x == 0) {                                                   // fewer than 16 bytes at either end
        for (size_t i = threadIdx.x; i < head; i += blockDim.x) dst[i] = (unsigned char)byte;
        for (size_t i = head + body * 16 + threadIdx.x; i < nbytes; i += blockDim.x) dst[i] = (unsigned char)byte;
    }
}
static __global__ void ps_copy_kernel(unsigned char *dst, const unsigned char *src, size_t nbytes) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (((reinterpret_cast<size_t>(dst) | reinterpret_cast<size_t>(src)) & 15) == 0) {
        const size_t body = nbytes / 16;
        const uint4 *s = reinterpret_cast<const uint4 *>(src);
        uint4 *d = reinterpret_cast<uint4 *>(dst);
        for (size_t i = tid; i < body; i += stride) d[i] = s[i];
        for (size_t i = body * 16 + tid; i < nbytes; i += stride) dst[i] = src[i];
    } else {
        for (size_t i = tid; i < nbytes; i += stride) dst[i] = src[i];
    }
}
static inline unsigned ps_fill_grid(size_t nbytes) {
    const size_t g = (nbytes / 16 + 255) / 256;
    return (unsigned)(g < 1 ? 1 : g > 4096 ? 4096 : g);
}
// hipMemsetAsync(dst, byte, nbytes, st) as a kernel; hipSuccess for nbytes == 0
static inline hipError_t ps_fill_async(void *dst, int byte, size_t nbytes, hipStream_t st) {
    if (nbytes == 0) return hipSuccess;
    hipLaunchKernelGGL(ps_fill_kernel, dim3(ps_fill_grid(nbytes)), dim3(256), 0, st, reinterpret_cast<unsigned char *>(dst),
                       (unsigned int)byte, nbytes);
    return hipGetLastError();
}
// hipMemcpyAsync(dst, src, nbytes, hipMemcpyDeviceToDevice, st) as a kernel (the ranges must not overlap)
static inline hipError_t ps_copy_async(void *dst, const void *src, size_t nbytes, hipStream_t st) {
    if (nbytes == 0) return hipSuccess;
    hipLaunchKernelGGL(ps_copy_kernel, dim3(ps_fill_grid(nbytes)), dim3(256), 0, st, reinterpret_cast<unsigned char *>(dst),
                       reinterpret_cast<const unsigned char *>(src), nbytes);
    return hipGetLastError();
}

// internal (not part of the C ABI): grouped x W^T of csrc/dense_mfma.hip, used by the inverted-file scan
int psi_linear_grouped(const float *x, int64_t M, int K, const float *W, int ldw, float *y, const int64_t *grp, int max_cols,
                       ps_stream_t stream);

// internal: the shared-candidate product of ps_hardest_negative (csrc/loss.hip), ps_linear's tiles with a row-arg-max epilogue
// (csrc/dense_mfma.hip, EPI 3).  best[b] (zeroed by the caller) = max over the candidates of ps_best_pack(Q_b . X_j, j).
int psi_hardest_shared(const float *Q, int64_t B, int D, const float *X, int64_t N, int exclude_diag, unsigned long long *best,
                       ps_stream_t stream);

// internal: ps_lsh_encode over an image of ps_lsh_stage (csrc/lsh_filter.hip: bf16 MFMA sign filter + exact fmaf recheck)
int psi_lsh_encode_staged(const float *x, int64_t N, int D, const void *staged, int nbits, uint8_t *codes, ps_stream_t stream);

__device__ __forceinline__ int ps_lane() { return threadIdx.x & 63; }

// The inner product of ps_linear / ps_dot_topk / ps_row_dot for one pair of rows: acc = fmaf(x[k], y[k], acc), k ascending over
// n columns, continued from s (+0.0 starts a product).  vec: 16-byte reads -- n % 4 == 0 and both rows 16-byte aligned; the
// floats, and so the bits, are the same either way.  The rows may lie in global memory or in LDS.
__device__ __forceinline__ float ps_fma_chain(const float *__restrict__ x, const float *__restrict__ y, int n, bool vec, float s) {
    if (vec) {
        for (int k = 0; k < n; k += 4) {
            const float4 u = *reinterpret_cast<const float4 *>(x + k), v = *reinterpret_cast<const float4 *>(y + k);
            s = fmaf(u.x, v.x, s);
            s = fmaf(u.y, v.y, s);
            s = fmaf(u.z, v.z, s);
            s = fmaf(u.w, v.w, s);
        }
    } else {
        for (int k = 0; k < n; ++k) s = fmaf(x[k], y[k], s);
    }
    return s;
}

// a / b rounded to nearest, as numpy and python divide.  The instruction sequence the compiler emits for an fp64 `/` is faithful
// but not always correctly rounded: a quotient within a hair of a rounding midpoint can come out one ulp off (11 of
// SYN-25M's 50 M CDF entries did).  q is within an ulp of a / b, so the residuals a - q b are exact (fma), and the
// neighbour of q on the residual's side replaces q when its residual is smaller (a quotient is never exactly a midpoint).
__device__ __forceinline__ double ps_div_rn(double a, double b) {
    const double q = a / b;
    const double r = fma(-q, b, a);
    if (r == 0.0 || !isfinite(q)) return q;
    const double q1 = nextafter(q, ((r > 0.0) == (b > 0.0)) ? INFINITY : -INFINITY);
    return fabs(fma(-q1, b, a)) < fabs(r) ? q1 : q;
}

// All LDS traffic of a wave is issued in order; this makes earlier LDS writes/atomics of the
// wave visible to all of its lanes (waits lgkmcnt) and stops the compiler reordering across it.
__device__ __forceinline__ void ps_wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Reductions over the 16 lanes of a DPP row and over the wave.  DPP only (quad_perm, row_half_mirror, row_mirror, then
// row_bcast:15 / :31 and a v_readlane of lane 63): __shfl_xor goes through the LDS crossbar, which all waves of a CU share.
//
// One step: lane l's copy of the v of the lane that CTRL names, taken in the rows of mask ROWS.  A lane that the step does not
// reach reads 0 under BOUND (bound_ctrl) and fill otherwise.  T is int or float.
template <int CTRL, int ROWS, bool BOUND, typename T>
__device__ __forceinline__ T ps_dpp_step(T v, T fill) {
    static_assert(sizeof(T) == 4, "a DPP step moves one 32-bit register");
    return __builtin_bit_cast(
        T, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, fill), __builtin_bit_cast(int, v), CTRL, ROWS, 0xf, BOUND));
}
struct PsSum {                                 // v + the other lane's v; an unreached lane adds 0
    template <int CTRL, int ROWS, typename T>
    static __device__ __forceinline__ T step(T v) { return v + ps_dpp_step<CTRL, ROWS, true>(v, T(0)); }
};
struct PsMax {                                 // fmaxf, which drops a NaN operand; an unreached lane offers -inf
    template <int CTRL, int ROWS>
    static __device__ __forceinline__ float step(float v) {
        return fmaxf(v, ps_dpp_step<CTRL, ROWS, false>(v, __builtin_bit_cast(float, 0xff800000u)));
    }
};
// over the 16 lanes of a row, result in each of them
template <typename OP, typename T>
__device__ __forceinline__ T ps_row16_reduce(T v) {
    v = OP::template step<0xB1, 0xf>(v);       // quad_perm [1, 0, 3, 2]
    v = OP::template step<0x4E, 0xf>(v);       // quad_perm [2, 3, 0, 1]
    v = OP::template step<0x141, 0xf>(v);      // row_half_mirror
    v = OP::template step<0x140, 0xf>(v);      // row_mirror
    return v;
}
// over the wave, result in every lane
template <typename OP, typename T>
__device__ __forceinline__ T ps_wave_reduce(T v) {
    v = ps_row16_reduce<OP>(v);
    v = OP::template step<0x142, 0xa>(v);      // row_bcast:15 into rows 1 and 3
    v = OP::template step<0x143, 0xc>(v);      // row_bcast:31 into rows 2 and 3
    return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ int ps_row16_sum_i32(int v) { return ps_row16_reduce<PsSum>(v); }
__device__ __forceinline__ float ps_row16_sum_f32(float v) { return ps_row16_reduce<PsSum>(v); }
__device__ __forceinline__ int ps_wave_sum_i32(int v) { return ps_wave_reduce<PsSum>(v); }
__device__ __forceinline__ float ps_wave_sum_f32(float v) { return ps_wave_reduce<PsSum>(v); }
// a NaN score surfaces through expf in the softmax (csrc/neigh_agg.hip), not through the maximum
__device__ __forceinline__ float ps_wave_max_f32(float v) { return ps_wave_reduce<PsMax>(v); }
