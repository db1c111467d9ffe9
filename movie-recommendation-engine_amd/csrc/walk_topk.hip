// walk_topk.hip -- ps_paths_topk: the visit counting and top-T cut of ps_walk_sample over given paths (the biased sampler's
// walks come from ps_walk_paths_biased, csrc/walk_biased.hip).  One wave per start node reads its n entries from global memory
// into registers and runs visit_count / visit_select of csrc/walk_visits.h, the functions the sampler's own kernel runs
// (csrc/walk_sample.hip); the table and the bitmap are all that lives in LDS.
#include "ps_common.h"
#include "walk_visits.h"

namespace {

constexpr int PT_MAX_ENTRIES = 4096;       // 64 positions per lane

struct TopkArgs {
    const int32_t *paths;
    int64_t B;
    int n, T;
    int32_t *ids, *counts, *nvalid;
    int hs_log2;
};

template <int NP>
__global__ __launch_bounds__(64) void paths_topk_kernel(TopkArgs a) {
    extern __shared__ int32_t smem[];
    const int lane = threadIdx.x;
    const int HS = 1 << a.hs_log2;
    const VisitTable table{smem, smem + HS, smem + 2 * HS, reinterpret_cast<uint32_t *>(smem + 3 * HS), a.hs_log2,
                           visit_bitmap_words(a.n)};
    for (int64_t i = blockIdx.x; i < a.B; i += gridDim.x) {
        const int32_t *src = a.paths + i * a.n;
        int32_t vid[NP], cr[NP];
        visit_count<NP>(table, [src, n = a.n](int p) { return p < n ? src[p] : -1; }, vid, cr, lane);
        visit_select<NP>(table, vid, cr, a.T, a.ids + i * a.T, a.counts + i * a.T, a.nvalid, i, lane);
    }
}

}  // namespace

extern "C" int ps_paths_topk_max_entries(void) { return PT_MAX_ENTRIES; }

extern "C" int ps_paths_topk(const int32_t *paths, int64_t B, int n, int T, int32_t *ids, int32_t *counts, int32_t *nvalid,
                             ps_stream_t stream) {
    if (B < 0 || n < 1 || T < 1) return PS_EINVAL;
    if (B == 0) return PS_OK;
    if (!paths || !ids || !counts || !nvalid) return PS_EINVAL;
    if (n > PT_MAX_ENTRIES) return PS_EUNSUPPORTED;
    const int hs_log2 = visit_table_log2(n);
    const TopkArgs a{paths, B, n, T, ids, counts, nvalid, hs_log2};
    const size_t lds = (3 * ((size_t)1 << hs_log2) + visit_bitmap_words(n)) * sizeof(int32_t);
    const int64_t grid = B > 256 * 256 ? 256 * 256 : B;
    // (the largest table, 3 x 8192 words for n = 4096, is 96.5 KiB: dynamic LDS beyond 64 KiB has to be allowed)
#define PS_PT_LAUNCH(NP_)                                                                                          \
    do {                                                                                                           \
        static PsPerDevice done;                                                                                   \
        if (lds > 64 * 1024 && !ps_allow_lds_once(done, 160 * 1024, paths_topk_kernel<NP_>)) return PS_ELAUNCH;    \
        hipLaunchKernelGGL(paths_topk_kernel<NP_>, dim3((unsigned)grid), dim3(64), lds, ps_stream(stream), a);     \
    } while (0)
    PS_VISIT_NP_SWITCH(visit_np(n), PS_PT_LAUNCH)
#undef PS_PT_LAUNCH
    PS_CHECK_LAUNCH();
    return PS_OK;
}
