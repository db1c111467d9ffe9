// cooc_sparse.hip -- the item co-occurrence counts of GraphBuilder.build_item_similarity_graph (reference
// data/graph_builder.py:59-116) as a row-wise SPARSE A A^T over the upper triangle: a second producer of the
// {a, b, count, window} records of ps_cooc_pairs (csrc/cooc_mfma.hip) that needs no U x M operand planes, has no
// multiplicity limit and does work proportional to the reference's own pair updates instead of M^2 U / 2.
//
// The distinct (user, item) entries are grouped both ways: by item (iptr / iuser / imult, users ascending) and by user
// (eptr / eitem / emult, items ascending).  One workgroup owns item row a:
//     for every entry (u, m_ua) of a, for every entry (b, m_ub) of u with b > a:  count[b] += m_ua m_ub,  first[b] = min(first[b], u)
//     count[a] = sum_u m_ua (m_ua - 1) / 2,  first[a] = the smallest u with m_ua >= 2
// and appends every b >= a with count >= thr as a record; window = first / PS_COOC_WINDOW, what ps_cooc_keys expects.
// Integer adds and mins only (atomics): the records do not depend on scheduling, only their order in the buffer does, and
// the key sort of the caller removes that.
//
// Rows are handed out from `order` (heaviest first, built by the caller) through one device counter: row work
// sum_{u in users(a)} deg(u) is heavily skewed, and a persistent grid that takes the next row when it is free keeps the
// heavy rows from landing on one workgroup.  A 16-lane group takes one user of the row at a time; its lanes stride the
// user's items from the first one > a (binary search).
//
// The accumulator {partner b -> (count, first user)} lives in LDS, S slots (acc_slots; 0 = DEFAULT_SLOTS):
//   direct  slot = b - (a + 1), when all columns right of a fit the S slots; one sweep of them emits and clears;
//   hash    keys[S] with linear probing (at most PROBES probes) otherwise; the occupied slots are listed, so emitting and
//           clearing a row costs its distinct partners, not S.
// A row with more distinct partners than the hash holds fails an insertion; the pass stops, its partial sums are dropped
// and the row goes to the overflow list.  A second kernel redoes the listed rows with the same walk into a global slab per
// workgroup (count / first / touched list, M entries each, atomics at L2), again in one pass: a column-tiled rerun would
// walk a heavy row's users once per S columns, hundreds of times at 10^6 items.  The number of slabs is bounded
// (slab_count: at most MAX_SLABS, at most SLAB_BUDGET bytes, at least MIN_SLABS), so the workspace is
// O(M) + a bounded number of M-long slabs and nothing grows with U M or M^2.  The self pair is emitted by the first kernel.
#include "ps_common.h"

#include <limits.h>

namespace {

constexpr int WINDOW = PS_COOC_WINDOW;
constexpr int THREADS = 256;
constexpr int GROUP = 16;                        // lanes that share one user of the row
constexpr int NGROUPS = THREADS / GROUP;
constexpr int DEFAULT_SLOTS = 4096;              // 64 KiB + header: two workgroups per CU
constexpr int MAX_SLOTS = 10000;                 // 16 B per slot + header <= 160 KiB
constexpr int PROBES = 32;
constexpr int HEADER_BYTES = 64;
constexpr int64_t MAX_SLABS = 512, MIN_SLABS = 4;
constexpr int64_t SLAB_BUDGET = (int64_t)2 << 30;
constexpr size_t COUNTERS_BYTES = 256;           // workspace head: next row, overflow count, next overflow row

// LDS header words
enum { H_ROW = 0, H_NLIST, H_FAIL, H_SELF_COUNT, H_SELF_FIRST };

struct SparseArgs {
    const int64_t *iptr;
    const int32_t *iuser, *imult;
    const int64_t *eptr;
    const int32_t *eitem, *emult;
    const int32_t *order;
    int64_t n, U, M, thr, cap;
    int S;
    int4 *rec;
    unsigned long long *count, *next, *novf, *next_ovf;
    int32_t *ovf;                                // int32[M]: rows that failed the hash
    int32_t *slabs;                              // per workgroup of the second kernel: count[M], first[M], touched[M]
};

inline size_t lds_bytes(int S) { return (size_t)HEADER_BYTES + (size_t)S * 16; }
inline int64_t slab_count(int64_t M) {
    const int64_t n = SLAB_BUDGET / (12 * M);
    return n > MAX_SLABS ? MAX_SLABS : n < MIN_SLABS ? MIN_SLABS : n;
}

__device__ __forceinline__ int64_t first_not_below(const int32_t *__restrict__ v, int64_t lo, int64_t hi, int32_t x) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (v[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void append(const SparseArgs &g, int a, int b, int c, int first) {
    const unsigned long long at = atomicAdd(g.count, 1ull);
    if ((int64_t)at < g.cap) g.rec[at] = make_int4(a, b, c, first / WINDOW);
}

// every (b, m_ua m_ub, u) of row a with b > a -> update(b, v, u); stops early once *stop (LDS) is set
template <typename F>
__device__ __forceinline__ void walk_row(const SparseArgs &g, int a, int64_t i0, int64_t i1, const int *stop, F update) {
    const int grp = threadIdx.x / GROUP, gl = threadIdx.x % GROUP;
    if ((int64_t)a + 1 >= g.M) return;
    for (int64_t x = i0 + grp; x < i1; x += NGROUPS) {
        if (*reinterpret_cast<const volatile int *>(stop) != INT_MAX) break;
        const int u = g.iuser[x], m = g.imult[x];
        if (u < 0 || u >= g.U || m < 1) continue;
        const int64_t e0 = g.eptr[u], e1 = g.eptr[u + 1];
        if (e0 < 0 || e1 > g.n) continue;
        for (int64_t e = first_not_below(g.eitem, e0, e1, a + 1) + gl; e < e1; e += GROUP) {
            const int b = g.eitem[e];
            if (b <= a || b >= g.M) continue;                     // not reached for lists sorted as documented
            update(b, m * g.emult[e], u);
        }
    }
}

// thread 0 takes the next index below `limit` from *counter and publishes rows[index] (or -1) in hdr[H_ROW]
__device__ __forceinline__ int next_row(int *hdr, unsigned long long *counter, unsigned long long limit, const int32_t *rows) {
    __syncthreads();                                              // the previous row is retired
    if (threadIdx.x == 0) {
        const unsigned long long i = atomicAdd(counter, 1ull);
        hdr[H_ROW] = i < limit ? rows[i] : -1;
    }
    __syncthreads();
    return hdr[H_ROW];
}

__global__ __launch_bounds__(THREADS) void cooc_sparse_kernel(const SparseArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *hdr = reinterpret_cast<int *>(smem);
    const int S = g.S;
    int *keys = reinterpret_cast<int *>(smem + HEADER_BYTES), *cnt = keys + S, *first = cnt + S, *list = first + S;
    const int tid = threadIdx.x;
    const int probes = S < PROBES ? S : PROBES;
    const int64_t M = g.M;

    for (int i = tid; i < S; i += THREADS) { keys[i] = -1; cnt[i] = 0; first[i] = INT_MAX; }
    if (tid == 0) { hdr[H_NLIST] = 0; hdr[H_FAIL] = INT_MAX; hdr[H_SELF_COUNT] = 0; hdr[H_SELF_FIRST] = INT_MAX; }

    for (;;) {
        const int a = next_row(hdr, g.next, (unsigned long long)M, g.order);   // its barriers also publish the cleared accumulator
        if (a == -1) break;
        if (a < 0 || a >= M) continue;                            // not a row: `order` was no permutation of 0..M-1
        const int64_t i0 = g.iptr[a], i1 = g.iptr[a + 1];
        if (i0 < 0 || i1 > g.n || i0 >= i1) continue;
        // the self pair
        int self_c = 0, self_f = INT_MAX;
        for (int64_t x = i0 + tid; x < i1; x += THREADS) {
            const int u = g.iuser[x], m = g.imult[x];
            if (u < 0 || u >= g.U || m < 2) continue;
            self_c += (int)((int64_t)m * (m - 1) / 2);
            self_f = u < self_f ? u : self_f;
        }
        if (self_c > 0) {
            atomicAdd(hdr + H_SELF_COUNT, self_c);
            atomicMin(hdr + H_SELF_FIRST, self_f);
        }
        const int base = a + 1;
        const bool direct = M - base <= S;
        if (direct) {
            walk_row(g, a, i0, i1, hdr + H_FAIL, [&](int b, int v, int u) {
                atomicAdd(cnt + (b - base), v);
                atomicMin(first + (b - base), u);
            });
        } else {
            walk_row(g, a, i0, i1, hdr + H_FAIL, [&](int b, int v, int u) {
                int s = (int)(((uint32_t)b * 2654435761u) % (uint32_t)S);
                for (int p = 0; p < probes; ++p) {
                    int k = *reinterpret_cast<volatile int *>(keys + s);
                    if (k == -1) {
                        k = atomicCAS(keys + s, -1, b);
                        if (k == -1) {                            // this lane claimed the slot: list it once
                            list[atomicAdd(hdr + H_NLIST, 1)] = s;
                            k = b;
                        }
                    }
                    if (k == b) {
                        atomicAdd(cnt + s, v);
                        atomicMin(first + s, u);
                        return;
                    }
                    s = s + 1 == S ? 0 : s + 1;
                }
                atomicMin(hdr + H_FAIL, b);                       // no slot: the row has more partners than the hash holds
            });
        }
        __syncthreads();
        const bool failed = hdr[H_FAIL] != INT_MAX;
        const int nlist = hdr[H_NLIST];
        if (tid == 0) {
            const int c = hdr[H_SELF_COUNT];
            if (c > 0 && (int64_t)c >= g.thr) append(g, a, a, c, hdr[H_SELF_FIRST]);
            if (failed) g.ovf[atomicAdd(g.novf, 1ull)] = a;       // each row is taken once: at most M entries
        }
        if (direct) {
            const int w = (int)(M - base);
            for (int i = tid; i < w; i += THREADS) {
                const int c = cnt[i];
                if (c == 0) continue;
                if ((int64_t)c >= g.thr) append(g, a, base + i, c, first[i]);
                cnt[i] = 0;
                first[i] = INT_MAX;
            }
        } else {
            for (int i = tid; i < nlist; i += THREADS) {
                const int s = list[i], c = cnt[s];
                if (!failed && (int64_t)c >= g.thr) append(g, a, keys[s], c, first[s]);
                keys[s] = -1;
                cnt[s] = 0;
                first[s] = INT_MAX;
            }
        }
        __syncthreads();
        if (tid == 0) { hdr[H_NLIST] = 0; hdr[H_FAIL] = INT_MAX; hdr[H_SELF_COUNT] = 0; hdr[H_SELF_FIRST] = INT_MAX; }
    }
}

// The rows of the overflow list, one pass each into this workgroup's global slab.  Slab words are only touched with
// device-scope atomics (adds, mins, loads, stores): the adds run at L2, a plain load could be served from a stale L1 line.
__global__ __launch_bounds__(THREADS) void cooc_sparse_slab_kernel(const SparseArgs g) {
    __shared__ int hdr[8];
    const unsigned long long novf = *g.novf;
    if (blockIdx.x >= novf) return;
    const int tid = threadIdx.x;
    const int64_t M = g.M;
    int *cnt = g.slabs + (int64_t)blockIdx.x * 3 * M, *first = cnt + M, *list = first + M;
    for (int64_t i = tid; i < M; i += THREADS) {
        __hip_atomic_store(cnt + i, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(first + i, INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid == 0) { hdr[H_NLIST] = 0; hdr[H_FAIL] = INT_MAX; }    // H_FAIL stays unset: nothing stops this walk
    __threadfence();
    for (;;) {
        const int a = next_row(hdr, g.next_ovf, novf, g.ovf);     // its barriers order the slab's clears before the next adds
        if (a == -1) break;
        if (a < 0 || a >= M) continue;
        const int64_t i0 = g.iptr[a], i1 = g.iptr[a + 1];
        if (i0 < 0 || i1 > g.n || i0 >= i1) continue;
        walk_row(g, a, i0, i1, hdr + H_FAIL, [&](int b, int v, int u) {
            if (atomicAdd(cnt + b, v) == 0) list[atomicAdd(hdr + H_NLIST, 1)] = b;    // v >= 1: the first add lists b, once
            atomicMin(first + b, u);
        });
        __threadfence();
        __syncthreads();
        const int nlist = hdr[H_NLIST];
        for (int i = tid; i < nlist; i += THREADS) {
            const int b = list[i];
            const int c = __hip_atomic_load(cnt + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((int64_t)c >= g.thr) append(g, a, b, c, __hip_atomic_load(first + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            __hip_atomic_store(cnt + b, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(first + b, INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __threadfence();
        __syncthreads();
        if (tid == 0) hdr[H_NLIST] = 0;
    }
}

}  // namespace

extern "C" size_t ps_cooc_pairs_sparse_workspace_bytes(int64_t M, int acc_slots) {
    if (M <= 0 || M >= ((int64_t)1 << 31) - 64 || acc_slots < 0 || acc_slots > MAX_SLOTS) return 0;
    return COUNTERS_BYTES + ps_align256((size_t)(4 * M)) + (size_t)(slab_count(M) * 12 * M);
}

extern "C" int ps_cooc_pairs_sparse(const int64_t *iptr, const int32_t *iuser, const int32_t *imult, const int64_t *eptr,
                                    const int32_t *eitem, const int32_t *emult, const int32_t *order, int64_t n, int64_t U, int64_t M,
                                    int64_t max_sq, int64_t thr, int acc_slots, ps_cooc_record *records, int64_t capacity,
                                    int64_t *count, int64_t *h_count, void *workspace, size_t workspace_bytes, ps_stream_t stream) {
    if (n < 0 || U <= 0 || U >= ((int64_t)1 << 31) || thr < 1 || capacity < 0 || max_sq < 0) return PS_EINVAL;
    const size_t need = ps_cooc_pairs_sparse_workspace_bytes(M, acc_slots);
    if (need == 0) return PS_EINVAL;
    if (max_sq >= ((int64_t)1 << 31)) return PS_EUNSUPPORTED;         // a count may not fit the record's int32
    if (!iptr || !eptr || !order || !count || !h_count || !workspace || (capacity > 0 && !records)) return PS_EINVAL;
    if (n > 0 && (!iuser || !imult || !eitem || !emult)) return PS_EINVAL;
    if (reinterpret_cast<size_t>(workspace) % 8 != 0) return PS_EINVAL;
    if (workspace_bytes < need) return PS_EWORKSPACE;
    const int S = acc_slots == 0 ? DEFAULT_SLOTS : acc_slots;
    const size_t lds = lds_bytes(S);
    static PsPerDevice cus;                                           // attribute set, CU count known
    int dv = 0;
    if (!ps_device_index(&dv)) return PS_ELAUNCH;
    int ncu = cus.get(dv);
    if (ncu == 0) {
        if (!ps_allow_lds(cooc_sparse_kernel, 160 * 1024)) return PS_ELAUNCH;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dv) != hipSuccess || ncu <= 0) return PS_ELAUNCH;
        cus.set(dv, ncu);
    }
    hipStream_t s = ps_stream(stream);
    char *ws = reinterpret_cast<char *>(workspace);
    unsigned long long *counters = reinterpret_cast<unsigned long long *>(ws);
    if (ps_fill_async(count, 0, sizeof(int64_t), s) != hipSuccess) return PS_ELAUNCH;
    if (ps_fill_async(counters, 0, COUNTERS_BYTES, s) != hipSuccess) return PS_ELAUNCH;
    int64_t per_cu = (int64_t)(160 * 1024) / (int64_t)lds;           // resident workgroups by LDS; 8 waves of 32 by threads
    per_cu = per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu;
    int64_t grid = (int64_t)ncu * per_cu;
    if (grid > M) grid = M;
    SparseArgs g{iptr, iuser, imult, eptr, eitem, emult, order, n, U, M, thr, capacity, S, reinterpret_cast<int4 *>(records),
                 reinterpret_cast<unsigned long long *>(count), counters, counters + 1, counters + 2,
                 reinterpret_cast<int32_t *>(ws + COUNTERS_BYTES),
                 reinterpret_cast<int32_t *>(ws + COUNTERS_BYTES + ps_align256((size_t)(4 * M)))};
    hipLaunchKernelGGL(cooc_sparse_kernel, dim3((unsigned)grid), dim3(THREADS), lds, s, g);
    PS_CHECK_LAUNCH();
    hipLaunchKernelGGL(cooc_sparse_slab_kernel, dim3((unsigned)slab_count(M)), dim3(THREADS), 0, s, g);
    PS_CHECK_LAUNCH();
    if (hipMemcpyAsync(h_count, count, sizeof(int64_t), hipMemcpyDeviceToHost, s) != hipSuccess) return PS_ELAUNCH;
    if (hipStreamSynchronize(s) != hipSuccess) return PS_ELAUNCH;
    return *h_count > capacity ? PS_EWORKSPACE : PS_OK;
}
