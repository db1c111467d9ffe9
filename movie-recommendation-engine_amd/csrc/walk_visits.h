// Visit counting and the top-T cut of the walk sampler: the one copy behind ps_walk_sample / ps_walk_sample_layers
// (csrc/walk_sample.hip, positions staged in LDS by the walk phase) and ps_paths_topk (csrc/walk_topk.hip, positions read from
// given paths).  One wave owns the n positions of a start node, NP per lane in registers, position p = j * 64 + lane:
//   count  : an LDS open-addressing table keyed by node id gives every position its visit count (ds atomics) and first-visit
//            position (atomic min); a bitmap records which counts occur;
//   select : classes of equal count are swept from the highest count down; inside a class, a wave ballot + prefix popcount over
//            positions gives the first-visit rank, i.e. python's stable sorted(Counter(...).items(), reverse=True)[:T]
//            (reference utils/random_walk.py:107).
// Integers only; no global atomics, no inter-wave communication: results do not depend on scheduling.
#pragma once
#include "ps_common.h"

// ---- host side: what a launch sizes from the number of positions P (at most 4096: 64 per lane) ----
static inline int visit_np(int P) {                          // positions per lane: the power of two with NP * 64 >= P
    int np = 1;
    while (np * 64 < P) np <<= 1;
    return np;
}
static inline int visit_table_log2(int P) {                  // table >= 1.25 P slots (load factor <= 0.8), at least 64
    int hs_log2 = 6;
    while ((1 << hs_log2) * 4 < 5 * P) ++hs_log2;
    return hs_log2;
}
__host__ __device__ __forceinline__ int visit_bitmap_words(int P) { return (P >> 5) + 1; }      // one bit per count 0 .. P

// `LAUNCH(NP)` for the NP of a launch (a statement macro; the enclosing function returns an int)
#define PS_VISIT_NP_SWITCH(np, LAUNCH)          \
    switch (np) {                               \
        case 1: LAUNCH(1); break;               \
        case 2: LAUNCH(2); break;               \
        case 4: LAUNCH(4); break;               \
        case 8: LAUNCH(8); break;               \
        case 16: LAUNCH(16); break;             \
        case 32: LAUNCH(32); break;             \
        case 64: LAUNCH(64); break;             \
        default: return PS_EUNSUPPORTED;        \
    }

// ---- device side ----
// The wave's LDS words; where they live is the caller's business.  hkey / hcnt / hfirst: 1 << hs_log2 words each; bitmap: nbw.
struct VisitTable {
    int32_t *hkey, *hcnt, *hfirst;
    uint32_t *bitmap;
    int hs_log2, nbw;
};

// pos(p): the node visited at position p, < 0 = none -> vid[j] = pos(j * 64 + lane); cr[j]: the node's visit count where the
// position is its first visit, else 0; the bitmap has the bits of the counts that occur.  (A position is fetched when its turn
// to be inserted comes: fetching all NP before the table is cleared cost ps_walk_sample's 64-position kernel two VGPRs.)
template <int NP, class Pos>
__device__ __forceinline__ void visit_count(const VisitTable &t, const Pos &pos, int32_t (&vid)[NP], int32_t (&cr)[NP], int lane) {
    const int HS = 1 << t.hs_log2;
    for (int h = lane; h < HS; h += 64) { t.hkey[h] = -1; t.hcnt[h] = 0; t.hfirst[h] = 0x7fffffff; }
    for (int b = lane; b < t.nbw; b += 64) t.bitmap[b] = 0u;
    ps_wave_lds_sync();
    // (inserting the NP positions of a lane together -- all pending compare-and-swaps of a probing round in flight, then the
    // count / first-visit atomics in one batch -- measured 2-4 x SLOWER for this phase: 22 K / 37 K cycles against 9.9 K)
    int32_t slot[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int p = j * 64 + lane;
        vid[j] = pos(p);
        slot[j] = -1;
        if (vid[j] >= 0) {
            uint32_t h = ((uint32_t)vid[j] * 2654435761u) >> (32 - t.hs_log2);
            while (true) {
                const int old = atomicCAS(&t.hkey[h], -1, vid[j]);
                if (old == -1 || old == vid[j]) break;
                h = (h + 1) & (uint32_t)(HS - 1);
            }
            atomicAdd(&t.hcnt[h], 1);
            atomicMin(&t.hfirst[h], p);
            slot[j] = (int32_t)h;
        }
    }
    ps_wave_lds_sync();
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        cr[j] = 0;
        if (slot[j] >= 0 && t.hfirst[slot[j]] == j * 64 + lane) {
            cr[j] = t.hcnt[slot[j]];
            atomicOr(&t.bitmap[cr[j] >> 5], 1u << (cr[j] & 31));
        }
    }
    ps_wave_lds_sync();
}

// The T most visited nodes and their counts -> oid / ocn [T], -1 / 0 past the nvalid[row] = min(T, distinct nodes) found.
// (nvalid comes as base and row: the address formed by the caller before the count phase cost ps_walk_sample's 32- and
// 64-position kernels two VGPRs.)
template <int NP>
__device__ __forceinline__ void visit_select(const VisitTable &t, const int32_t (&vid)[NP], const int32_t (&cr)[NP], int T,
                                             int32_t *oid, int32_t *ocn, int32_t *nvalid, int64_t row, int lane) {
    const uint64_t lanemask_lt = (1ull << lane) - 1ull;
    int emitted = 0;
    for (int wd = t.nbw - 1; wd >= 0 && emitted < T; --wd) {
        uint32_t bits = __builtin_amdgcn_readfirstlane(t.bitmap[wd]);
        while (bits != 0u && emitted < T) {
            const int b = 31 - __builtin_clz(bits);
            bits &= ~(1u << b);
            const int c = wd * 32 + b;
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const bool flag = cr[j] == c;
                const uint64_t mask = __ballot(flag);
                if (flag) {
                    const int r = emitted + __popcll(mask & lanemask_lt);
                    if (r < T) { oid[r] = vid[j]; ocn[r] = c; }
                }
                emitted += __popcll(mask);
            }
        }
    }
    const int nv = emitted < T ? emitted : T;
    for (int t_ = nv + lane; t_ < T; t_ += 64) { oid[t_] = -1; ocn[t_] = 0; }
    if (lane == 0) nvalid[row] = nv;
    ps_wave_lds_sync();
}
