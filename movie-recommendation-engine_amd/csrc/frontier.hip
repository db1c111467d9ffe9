// frontier.hip -- the set operation behind a minibatch block (PinSage paper, Algorithm 2: the K-hop neighbourhood of a batch is
// expanded from the top layer down) on gfx950: seeds + a [B, T] neighbour table -> the node set "seeds first, then every other
// kept id once, ascending" and the table renumbered into that set.  include/pinsage_hip.h: ps_frontier_build.
//
// Six launches on the caller's stream, integers only; the kernel boundaries are the only ordering the passes need.
//   clear    both bitmaps (limit bits each, padded to whole scan blocks) are zeroed: the workspace arrives with anything in it.
//   mark     one thread per seed and per slot.  A seed is copied to frontier[i], sets its bit in the SEED bitmap and records
//            map[seed] = i.  A kept slot sets its id's bit in the KEPT bitmap with an integer atomicOr: OR is commutative and
//            idempotent, so the bitmap does not depend on the order in which the atomics land (an id repeated in 5 000 slots
//            costs one atomic per wave that still sees the bit clear).
//   count    a scan block = FR_BLOCK_WORDS words = 32 768 ids per workgroup: the popcount of kept & ~seed, summed over the block.
//   scan     one workgroup turns the block sums into exclusive prefixes and writes count[0] = S + their total.
//   emit     every workgroup again: an exclusive scan of its threads' popcounts gives each set bit its rank among the non-seed
//            kept ids -- ascending order falls out of the bit order -- and the id goes to frontier[S + rank], the position to map[id].
//   relabel  one thread per slot: local = map[id] for a kept slot, -1 otherwise.  map is read only at ids whose bit was set in
//            this call, so it is never cleared.
#include "ps_common.h"

namespace {

constexpr int FR_THREADS = 256;
constexpr int FR_BLOCK_WORDS = 4 * FR_THREADS;          // bitmap words per scan block: one uint4 per thread, 32 768 ids

struct FrLayout {
    int64_t nblocks;                                    // scan blocks
    size_t bits_bytes;                                  // ONE bitmap, padded to whole scan blocks
    size_t off_seed, off_bsum, off_map, total;          // from the first 256-byte boundary
};

FrLayout fr_layout(int64_t limit) {
    FrLayout l;
    l.nblocks = ps_cdiv(ps_cdiv(limit, 32), FR_BLOCK_WORDS);
    l.bits_bytes = (size_t)l.nblocks * FR_BLOCK_WORDS * 4;
    l.off_seed = l.bits_bytes;                          // behind the kept bitmap: one clear covers both
    l.off_bsum = 2 * l.bits_bytes;
    l.off_map = l.off_bsum + ps_align256((size_t)l.nblocks * 4);
    l.total = l.off_map + ps_align256((size_t)limit * 4);
    return l;
}

// the keep rule of ps_importance_pool with max_idx = limit - 1; e = i * T + j
__device__ __forceinline__ bool fr_kept(const int32_t *__restrict__ ids, const int32_t *__restrict__ nvalid, uint32_t e, uint32_t T,
                                        int32_t limit, int32_t *id) {
    const uint32_t row = e / T, j = e - row * T;
    const int32_t nv = nvalid[row];                     // j < T always: a count above T means T, a negative one 0
    if (nv <= 0 || j >= (uint32_t)nv) return false;
    *id = ids[e];
    return *id >= 0 && *id < limit;
}

__global__ __launch_bounds__(FR_THREADS) void fr_mark_kernel(const int32_t *__restrict__ seeds, int64_t S, const int32_t *__restrict__ ids,
                                                            const int32_t *__restrict__ nvalid, int64_t slots, int T, int32_t limit,
                                                            int32_t *__restrict__ frontier, uint32_t *kept, uint32_t *seedbits,
                                                            int32_t *__restrict__ map) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < S + slots; i += stride) {
        if (i < S) {
            const int32_t s = seeds[i];
            frontier[i] = s;
            if (s >= 0 && s < limit) {                  // a seed outside the contract is never an index
                atomicOr(&seedbits[s >> 5], 1u << (s & 31));
                map[s] = (int32_t)i;
            }
        } else {
            int32_t id;
            if (fr_kept(ids, nvalid, (uint32_t)(i - S), (uint32_t)T, limit, &id)) {
                const uint32_t bit = 1u << (id & 31);
                // a stale read only costs the atomic it would have saved
                if (!(__hip_atomic_load(&kept[id >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(&kept[id >> 5], bit);
            }
        }
    }
}

// the thread's four words of non-seed kept ids and their popcount
__device__ __forceinline__ int fr_words(const uint32_t *__restrict__ kept, const uint32_t *__restrict__ seedbits, uint4 *w) {
    const size_t at = (size_t)blockIdx.x * FR_THREADS + threadIdx.x;
    const uint4 k = reinterpret_cast<const uint4 *>(kept)[at], s = reinterpret_cast<const uint4 *>(seedbits)[at];
    *w = make_uint4(k.x & ~s.x, k.y & ~s.y, k.z & ~s.z, k.w & ~s.w);
    return __popc(w->x) + __popc(w->y) + __popc(w->z) + __popc(w->w);
}

// inclusive sum over the workgroup's FR_THREADS threads in thread order; *total: the workgroup's sum.  sh: 4 ints of LDS.
__device__ __forceinline__ int fr_block_scan(int v, int *sh, int *total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    __syncthreads();                                    // the previous use of sh is over
    if (lane == 63) sh[wv] = v;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < FR_THREADS / 64; ++w) {
        const int t = sh[w];
        if (w < wv) before += t;
        all += t;
    }
    *total = all;
    return v + before;
}

__global__ __launch_bounds__(FR_THREADS) void fr_count_kernel(const uint32_t *__restrict__ kept, const uint32_t *__restrict__ seedbits,
                                                             int32_t *__restrict__ bsum) {
    __shared__ int sh[FR_THREADS / 64];
    uint4 w;
    int total;
    fr_block_scan(fr_words(kept, seedbits, &w), sh, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: bsum -> its exclusive prefixes, count[0] = S + the total (below 2^31: the entry point checks S + min(B T, limit))
__global__ __launch_bounds__(FR_THREADS) void fr_scan_kernel(int32_t *__restrict__ bsum, int64_t nblocks, int32_t S, int32_t *__restrict__ count) {
    __shared__ int sh[FR_THREADS / 64];
    int carry = 0;
    for (int64_t b0 = 0; b0 < nblocks; b0 += FR_THREADS) {
        const int64_t b = b0 + threadIdx.x;
        const int v = b < nblocks ? bsum[b] : 0;
        int total;
        const int incl = fr_block_scan(v, sh, &total);
        if (b < nblocks) bsum[b] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) count[0] = S + carry;
}

__global__ __launch_bounds__(FR_THREADS) void fr_emit_kernel(const uint32_t *__restrict__ kept, const uint32_t *__restrict__ seedbits,
                                                            const int32_t *__restrict__ bsum, int32_t S, int32_t *__restrict__ frontier,
                                                            int32_t *__restrict__ map) {
    __shared__ int sh[FR_THREADS / 64];
    uint4 w;
    const int c = fr_words(kept, seedbits, &w);
    int total;
    int pos = S + bsum[blockIdx.x] + fr_block_scan(c, sh, &total) - c;
    const int64_t id0 = ((int64_t)blockIdx.x * FR_BLOCK_WORDS + 4 * threadIdx.x) * 32;   // no bit at or beyond `limit` is ever set
    const uint32_t words[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t m = words[q];
        while (m) {
            const int32_t id = (int32_t)(id0 + 32 * q + (__ffs(m) - 1));
            m &= m - 1;
            frontier[pos] = id;
            map[id] = pos;
            ++pos;
        }
    }
}

__global__ __launch_bounds__(FR_THREADS) void fr_relabel_kernel(const int32_t *__restrict__ ids, const int32_t *__restrict__ nvalid, int64_t slots,
                                                               int T, int32_t limit, const int32_t *__restrict__ map,
                                                               int32_t *__restrict__ local) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < slots; e += stride) {
        int32_t id;
        local[e] = fr_kept(ids, nvalid, (uint32_t)e, (uint32_t)T, limit, &id) ? map[id] : -1;
    }
}

unsigned fr_grid(int64_t n) {
    const int64_t g = ps_cdiv(n, FR_THREADS);
    return (unsigned)(g > (1 << 16) ? (1 << 16) : (g < 1 ? 1 : g));
}

// the scalar conditions of both entry points; B * T without overflow
bool fr_shape_ok(int64_t limit, int64_t S, int64_t B, int T) {
    if (T < 1 || limit < 1 || limit > 0x7fffffff || S < 0 || B < 0 || B > 0x7fffffff / T) return false;
    const int64_t slots = B * T;
    return S + (slots < limit ? slots : limit) <= 0x7fffffff;      // positions are int32
}

}  // namespace

extern "C" size_t ps_frontier_workspace_bytes(int64_t limit, int64_t S, int64_t B, int T) {
    if (!fr_shape_ok(limit, S, B, T)) return 0;
    return fr_layout(limit).total + 256;
}

extern "C" int ps_frontier_build(const int32_t *seeds, int64_t S, const int32_t *ids, const int32_t *nvalid, int64_t B, int T,
                                 int64_t limit, int32_t *frontier, int32_t *count, int32_t *local, void *workspace,
                                 size_t workspace_bytes, ps_stream_t stream) {
    if (!fr_shape_ok(limit, S, B, T)) return PS_EINVAL;
    hipStream_t st = ps_stream(stream);
    if (S == 0 && B == 0) {
        if (count && ps_fill_async(count, 0, sizeof(int32_t), st) != hipSuccess) return PS_ELAUNCH;
        return PS_OK;
    }
    if (!frontier || !count || !workspace || (S > 0 && !seeds) || (B > 0 && (!ids || !nvalid || !local))) return PS_EINVAL;
    const FrLayout l = fr_layout(limit);
    if (workspace_bytes < l.total + 256) return PS_EWORKSPACE;          // ps_frontier_workspace_bytes: room for the alignment
    char *base = ps_ws_base(workspace);
    uint32_t *kept = reinterpret_cast<uint32_t *>(base), *seedbits = reinterpret_cast<uint32_t *>(base + l.off_seed);
    int32_t *bsum = reinterpret_cast<int32_t *>(base + l.off_bsum), *map = reinterpret_cast<int32_t *>(base + l.off_map);
    const int64_t slots = B * T;

    if (ps_fill_async(kept, 0, 2 * l.bits_bytes, st) != hipSuccess) return PS_ELAUNCH;
    hipLaunchKernelGGL(fr_mark_kernel, dim3(fr_grid(S + slots)), dim3(FR_THREADS), 0, st, seeds, S, ids, nvalid, slots, T, (int32_t)limit,
                       frontier, kept, seedbits, map);
    PS_CHECK_LAUNCH();
    hipLaunchKernelGGL(fr_count_kernel, dim3((unsigned)l.nblocks), dim3(FR_THREADS), 0, st, kept, seedbits, bsum);
    PS_CHECK_LAUNCH();
    hipLaunchKernelGGL(fr_scan_kernel, dim3(1), dim3(FR_THREADS), 0, st, bsum, l.nblocks, (int32_t)S, count);
    PS_CHECK_LAUNCH();
    hipLaunchKernelGGL(fr_emit_kernel, dim3((unsigned)l.nblocks), dim3(FR_THREADS), 0, st, kept, seedbits, bsum, (int32_t)S, frontier, map);
    PS_CHECK_LAUNCH();
    if (slots > 0) {
        hipLaunchKernelGGL(fr_relabel_kernel, dim3(fr_grid(slots)), dim3(FR_THREADS), 0, st, ids, nvalid, slots, T, (int32_t)limit, map, local);
        PS_CHECK_LAUNCH();
    }
    return PS_OK;
}
