// rank_window.hip -- the members of a rank window [lo, hi) of every row of personalized-PageRank scores, and a Floyd subset of
// them: the cut behind hard negatives "ranked 2000-5000 by PPR" (PinSage paper, section 3.3), which the reference names and does
// not have (its ranking holds at most 200 nodes: data/negative_sampler.py:67-77).
//
// ps_ppr_topk's order -- score descending, ties to the smaller id -- over the ids t < limit with score > 0 and t != skip[s].  A
// positive double orders as its 64-bit pattern (+inf included; NaN, zeros and negatives fail `> 0` and never compete), so the two
// boundary keys Ka (rank lo) and Kb (rank min(hi, N) - 1) come from one MSB-first radix select, eight sweeps of eight bits with
// LDS histograms, both boundaries through the same sweeps (one histogram while their prefixes agree).  With ga / gb the number of
// keys above Ka / Kb, an id is a member iff Kb < key < Ka, or key == Ka (Kb) and ga (gb) + its index among the equal keys in id
// order lies in [lo, hi).  One more sweep in ascending id order counts those indices and compacts the members with ballots, so
// the window comes out in ascending id without a sort.  No float arithmetic decides anything but the one product of a pick;
// integer LDS atomics only: the same inputs give the same bytes.
#include "ps_common.h"

namespace {

constexpr int RW_THREADS = 256;
constexpr int RW_WAVES = RW_THREADS / 64;
constexpr int RW_UNROLL = 4;                    // row loads in flight per lane in a histogram sweep
constexpr int RW_MAX_WINDOW = 1 << 16;
constexpr int RW_MAX_PICKS = 64;

// hist[digit] += 1 for every lane with `on`.  The high bytes of a score row hold a handful of exponents: the digit of the first
// lanes is counted once per wave (two rounds), and only what is left goes to the LDS atomic unit lane by lane.
__device__ __forceinline__ void hist_add(unsigned *hist, unsigned digit, bool on, int lane) {
    unsigned long long todo = __ballot(on);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (!todo) break;
        const int lead = __builtin_ctzll(todo);
        const unsigned d0 = (unsigned)__builtin_amdgcn_readlane((int)digit, lead);
        const unsigned long long m = __ballot(on && digit == d0);
        if (lane == lead) atomicAdd(&hist[d0], (unsigned)__builtin_popcountll(m));
        if (digit == d0) on = false;
        todo &= ~m;
    }
    if (on) atomicAdd(&hist[digit], 1u);
}

// a wave's view of a 256-bin histogram: lane l holds bins 4l .. 4l+3, `above` = the sum of the bins of the lanes above it
struct Bins {
    unsigned h[4], above, total;
};
__device__ __forceinline__ Bins load_bins(const unsigned *hist, int lane) {
    Bins b;
    const uint4 v = *reinterpret_cast<const uint4 *>(hist + 4 * lane);
    b.h[0] = v.x; b.h[1] = v.y; b.h[2] = v.z; b.h[3] = v.w;
    const unsigned own = v.x + v.y + v.z + v.w;
    unsigned inc = own;                                                  // inclusive suffix sum over the lanes
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = __shfl_down(inc, off, 64);
        if (lane + off < 64) inc += o;
    }
    b.above = inc - own;
    b.total = __shfl(inc, 0, 64);
    return b;
}
// the digit that holds descending rank r (r < total): the bins above it sum to `above` <= r
__device__ __forceinline__ void pick_digit(const Bins &b, unsigned r, int lane, unsigned *digit, unsigned *above) {
    unsigned a = b.above, fa = 0;
    int found = -1;
#pragma unroll
    for (int j = 3; j >= 0; --j) {
        if (found < 0 && r >= a && r - a < b.h[j]) { found = j; fa = a; }
        a += b.h[j];
    }
    const unsigned long long m = __ballot(found >= 0);
    const int src = m ? __builtin_ctzll(m) : 0;
    *digit = (unsigned)__builtin_amdgcn_readlane(4 * lane + (found < 0 ? 0 : found), src);
    *above = (unsigned)__builtin_amdgcn_readlane((int)fa, src);
}

__device__ __forceinline__ uint64_t key_of(double x, int64_t t, int64_t sk, bool inside) {
    return (inside && x > 0.0 && t != sk) ? (uint64_t)__double_as_longlong(x) : 0ull;    // 0 = no candidate (+0.0 never competes)
}

// Floyd's subset sampling over the positions 0 .. m-1 of the window (include/pinsage_hip.h has the rule)
__device__ void floyd_picks(const int32_t *win, int m, const double *u, int n, int32_t *picks, int *pos) {
    const int c = n < m ? n : m;
    for (int i = 0; i < c; ++i) {
        const int j = m - c + i;
        const double prod = u[i] * (double)(j + 1);
        int t;
        if (!(prod >= 0.0)) t = 0;
        else if (prod >= (double)(j + 1)) t = j;
        else { t = (int)floor(prod); if (t > j) t = j; }
        bool taken = false;
        for (int q = 0; q < i; ++q) taken = taken || pos[q] == t;
        pos[i] = taken ? j : t;
        picks[i] = win[pos[i]];
    }
    for (int i = c; i < n; ++i) picks[i] = -1;
}

__global__ __launch_bounds__(RW_THREADS) void rank_window_kernel(const double *score, int64_t ld, int64_t limit, const int64_t *skip,
                                                                 unsigned lo, unsigned hi, const double *u, int n, int32_t *window,
                                                                 int32_t *nwin, int32_t *picks) {
    __shared__ __attribute__((aligned(16))) unsigned hist[2][256];
    __shared__ unsigned cnt[3][RW_WAVES];
    __shared__ int pos[RW_MAX_PICKS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t s = blockIdx.x;
    const double *row = score + s * ld;
    const int64_t W = (int64_t)hi - lo;
    int32_t *win = window + s * W;
    int64_t sk = skip ? skip[s] : -1;
    if (sk < 0 || sk >= limit) sk = -1;

    uint64_t prefA = 0, prefB = 0;
    unsigned ra = lo, rb = 0, ga = 0, gb = 0, N = 0;
    bool same = true;
    for (int p = 0; p < 8; ++p) {
        const int shift = 56 - 8 * p;
        const uint64_t mask = p == 0 ? 0ull : ~0ull << (shift + 8);
        hist[0][tid] = 0;
        hist[1][tid] = 0;
        __syncthreads();
        for (int64_t base = 0; base < limit; base += RW_THREADS * RW_UNROLL) {
            double x[RW_UNROLL];
#pragma unroll
            for (int q = 0; q < RW_UNROLL; ++q) {
                const int64_t t = base + q * RW_THREADS + tid;
                x[q] = t < limit ? row[t] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < RW_UNROLL; ++q) {
                const int64_t t = base + q * RW_THREADS + tid;
                const uint64_t key = key_of(x[q], t, sk, t < limit);
                const unsigned digit = (unsigned)(key >> shift) & 255u;
                hist_add(hist[0], digit, key != 0 && (key & mask) == prefA, lane);
                if (!same) hist_add(hist[1], digit, key != 0 && (key & mask) == prefB, lane);
            }
        }
        __syncthreads();
        const Bins a = load_bins(hist[0], lane);
        if (p == 0) {
            N = a.total;
            if (N <= lo) break;
            rb = (N < hi ? N : hi) - 1;
        }
        unsigned dA, dB, upA, upB;
        pick_digit(a, ra, lane, &dA, &upA);
        if (same) {
            pick_digit(a, rb, lane, &dB, &upB);
        } else {
            const Bins b = load_bins(hist[1], lane);
            pick_digit(b, rb, lane, &dB, &upB);
        }
        prefA |= (uint64_t)dA << shift; ga += upA; ra -= upA;
        prefB |= (uint64_t)dB << shift; gb += upB; rb -= upB;
        same = same && dA == dB;
        __syncthreads();                                                 // every wave has read the bins before they are cleared
    }

    // the members in ascending id: one block scan per 256 ids for the indices inside the two tie groups, one for the members.
    // The two barriers of a step keep the next step's stores to cnt[0..1] behind this step's reads of them, and its store to
    // cnt[2] behind this step's reads of that.  The members are the ids of ranks lo .. min(hi, N) - 1, one each: m <= hi - lo.
    unsigned seenA = 0, seenB = 0, m = 0;
    if (N > lo) {
        for (int64_t base = 0; base < limit; base += RW_THREADS) {
            const int64_t t = base + tid;
            const uint64_t key = key_of(t < limit ? row[t] : 0.0, t, sk, t < limit);
            const bool isA = key != 0 && key == prefA, isB = key != 0 && key == prefB && !same;
            const unsigned long long bA = __ballot(isA), bB = __ballot(isB);
            const unsigned long long below = (1ull << lane) - 1ull;
            if (lane == 0) {
                cnt[0][wave] = (unsigned)__builtin_popcountll(bA);
                cnt[1][wave] = (unsigned)__builtin_popcountll(bB);
            }
            __syncthreads();
            unsigned iA = seenA + (unsigned)__builtin_popcountll(bA & below), iB = seenB + (unsigned)__builtin_popcountll(bB & below);
#pragma unroll
            for (int w = 0; w < RW_WAVES; ++w) {
                const unsigned cA = cnt[0][w], cB = cnt[1][w];
                if (w < wave) { iA += cA; iB += cB; }
                seenA += cA; seenB += cB;
            }
            bool member = key != 0 && key < prefA && key > prefB;
            if (isA) member = (uint64_t)ga + iA >= lo && (uint64_t)ga + iA < hi;
            if (isB) member = (uint64_t)gb + iB >= lo && (uint64_t)gb + iB < hi;
            const unsigned long long bM = __ballot(member);
            if (lane == 0) cnt[2][wave] = (unsigned)__builtin_popcountll(bM);
            __syncthreads();
            unsigned at = m + (unsigned)__builtin_popcountll(bM & below);
#pragma unroll
            for (int w = 0; w < RW_WAVES; ++w) {
                const unsigned c = cnt[2][w];
                if (w < wave) at += c;
                m += c;
            }
            if (member) win[at] = (int32_t)t;
        }
    }
    for (int64_t i = (int64_t)m + tid; i < W; i += RW_THREADS) win[i] = -1;
    if (tid == 0) nwin[s] = (int32_t)m;
    if (n > 0) {
        __threadfence_block();
        __syncthreads();                                                 // the window's stores, before one lane reads them back
        if (tid == 0) floyd_picks(win, (int)m, u + s * n, n, picks + s * n, pos);
    }
}

}  // namespace

extern "C" int ps_rank_window_max(void) { return RW_MAX_WINDOW; }

extern "C" int ps_rank_window(const double *score, int64_t S, int64_t ld, int64_t Vp, int64_t max_target, const int64_t *skip,
                              int64_t lo, int64_t hi, const double *u, int n, int32_t *window, int32_t *nwin, int32_t *picks,
                              ps_stream_t stream) {
    const int64_t two31 = (int64_t)1 << 31;
    if (S < 0 || Vp < 0 || n < 0 || ld < Vp || lo < 0 || hi <= lo || S >= two31 || Vp >= two31 || hi >= two31) return PS_EINVAL;
    if (S == 0) return PS_OK;
    if ((!score && Vp > 0) || !window || !nwin || (n > 0 && (!u || !picks))) return PS_EINVAL;
    if (hi - lo > RW_MAX_WINDOW || n > RW_MAX_PICKS) return PS_EUNSUPPORTED;
    const int64_t limit = (max_target >= 0 && max_target < Vp) ? max_target : Vp;
    hipLaunchKernelGGL(rank_window_kernel, dim3((unsigned)S), dim3(RW_THREADS), 0, ps_stream(stream), score, ld, limit, skip,
                       (unsigned)lo, (unsigned)hi, u, n, window, nwin, picks);
    PS_CHECK_LAUNCH();
    return PS_OK;
}
