// Selection by totally ordered integer keys: what the searches, the merges and the arg-max of the loss share.
#pragma once
#include "ps_common.h"

// A float's place in its total order as an unsigned word, monotone increasing: -inf < ... < -0 < +0 < ... < +inf, and a NaN by
// its bits (beyond the infinity of its sign).  ps_float_unorder is the inverse.
__device__ __forceinline__ uint32_t ps_float_order(float v) {
    const int32_t b = __float_as_int(v);
    return (uint32_t)(b ^ ((b >> 31) & 0x7fffffff)) ^ 0x80000000u;
}
__device__ __forceinline__ float ps_float_unorder(uint32_t u) {
    const int32_t k = (int32_t)(u ^ 0x80000000u);
    return __int_as_float(k ^ ((k >> 31) & 0x7fffffff));
}

// The key of a top-k selection (ps_dot_topk, ps_l2_topk, ps_ivf_topk, ps_rerank_topk): value word << 32 | id, smallest key first.
// DESC: largest value first (an inner product), else smallest (a distance); equal values by ascending id.  ~0 is no key of a
// candidate whose id is below 2^32 - 1.
template <bool DESC>
__device__ __forceinline__ uint64_t ps_topk_key(float v, uint32_t id) {
    return ((uint64_t)(DESC ? ~ps_float_order(v) : ps_float_order(v)) << 32) | id;
}

// (similarity, candidate index) as ONE unsigned word whose integer order is "larger similarity first, then smaller index":
// high half = the float's place in its total order with every NaN above +inf (a NaN candidate is its row's maximum, as in
// torch.max), low half = ~index.  Every word of a real candidate is > 0, so 0 = "no candidate", and partial maxima combine
// with a 64-bit integer max -- in registers or with a vector atomic -- in any order.
__device__ __forceinline__ unsigned long long ps_best_pack(float v, uint32_t j) {
    const uint32_t key = v != v ? 0xffffffffu : ps_float_order(v);
    return ((unsigned long long)key << 32) | (uint32_t)~j;
}
__device__ __forceinline__ float ps_best_sim(unsigned long long w) {       // 0 (no candidate) -> -inf
    const uint32_t key = (uint32_t)(w >> 32);
    if (w == 0ull) return __int_as_float((int)0xff800000u);
    if (key == 0xffffffffu) return __int_as_float(0x7fc00000);
    return ps_float_unorder(key);
}
__device__ __forceinline__ int64_t ps_best_idx(unsigned long long w) { return w == 0ull ? -1 : (int64_t)(uint32_t)~(uint32_t)w; }

// Keys of a selection: one 64-bit word, or the (distance, 64-bit id) of the shard merge as three unsigned words.  The largest
// key of either width stands for "none".
struct PsKey96 { uint32_t d, hi, lo; };
constexpr uint32_t PS_EMPTY32 = 0xffffffffu;
constexpr uint64_t PS_EMPTY64 = ~0ull;
constexpr PsKey96 PS_EMPTY96 = {0xffffffffu, 0xffffffffu, 0xffffffffu};
__device__ __forceinline__ bool ps_key_less(uint64_t a, uint64_t b) { return a < b; }
__device__ __forceinline__ bool ps_key_less(const PsKey96 &a, const PsKey96 &b) {
    return a.d < b.d || (a.d == b.d && (a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo)));
}
__device__ __forceinline__ bool ps_key_none(const PsKey96 &a) { return (a.d & a.hi & a.lo) == 0xffffffffu; }

// Minimum across lanes by DPP (no LDS crossbar, see ps_common.h).  Four exchange steps inside a row of 16 lanes reach every
// lane, so every lane ends with its row's minimum.  The two row_bcast steps carry a row's last lane into the following row(s)
// and write only the rows of their mask: a lane they do not reach reads all ones (old = -1, bound_ctrl off) and so keeps its
// own value; lane 63 then holds the minimum of the wave.
enum : int {
    PS_DPP_QUAD_XOR1 = 0xB1,         // quad_perm [1, 0, 3, 2]
    PS_DPP_QUAD_XOR2 = 0x4E,         // quad_perm [2, 3, 0, 1]
    PS_DPP_ROW_HALF_MIRROR = 0x141,
    PS_DPP_ROW_MIRROR = 0x140,
    PS_DPP_ROW_BCAST15 = 0x142,      // with row mask 0xa: lane 15 of rows 0 / 2 -> rows 1 / 3
    PS_DPP_ROW_BCAST31 = 0x143,      // with row mask 0xc: lane 31 -> rows 2 and 3
};
template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t ps_dpp_word(uint32_t w) {
    constexpr bool all = ROWS == 0xf;
    return (uint32_t)__builtin_amdgcn_update_dpp(all ? 0 : -1, (int)w, CTRL, ROWS, 0xf, all);
}
template <int CTRL, int ROWS>
__device__ __forceinline__ uint64_t ps_dpp_key(uint64_t v) {
    const uint32_t lo = ps_dpp_word<CTRL, ROWS>((uint32_t)v), hi = ps_dpp_word<CTRL, ROWS>((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
template <int CTRL, int ROWS>
__device__ __forceinline__ PsKey96 ps_dpp_key(const PsKey96 &v) {
    return PsKey96{ps_dpp_word<CTRL, ROWS>(v.d), ps_dpp_word<CTRL, ROWS>(v.hi), ps_dpp_word<CTRL, ROWS>(v.lo)};
}
__device__ __forceinline__ uint32_t ps_lane63(uint32_t w) { return (uint32_t)__builtin_amdgcn_readlane((int)w, 63); }
__device__ __forceinline__ uint64_t ps_lane63(uint64_t v) { return ((uint64_t)ps_lane63((uint32_t)(v >> 32)) << 32) | ps_lane63((uint32_t)v); }
__device__ __forceinline__ PsKey96 ps_lane63(const PsKey96 &v) { return PsKey96{ps_lane63(v.d), ps_lane63(v.hi), ps_lane63(v.lo)}; }

template <int CTRL, int ROWS, typename K>
__device__ __forceinline__ K ps_dpp_min_step(K v) {
    const K o = ps_dpp_key<CTRL, ROWS>(v);
    return ps_key_less(o, v) ? o : v;
}
// every lane: the minimum of its row of 16 lanes
template <typename K>
__device__ __forceinline__ K ps_row_min(K v) {
    v = ps_dpp_min_step<PS_DPP_QUAD_XOR1, 0xf>(v);
    v = ps_dpp_min_step<PS_DPP_QUAD_XOR2, 0xf>(v);
    v = ps_dpp_min_step<PS_DPP_ROW_HALF_MIRROR, 0xf>(v);
    return ps_dpp_min_step<PS_DPP_ROW_MIRROR, 0xf>(v);
}
// every lane: the minimum of the wave
template <typename K>
__device__ __forceinline__ K ps_wave_min(K v) {
    v = ps_row_min(v);
    v = ps_dpp_min_step<PS_DPP_ROW_BCAST15, 0xa>(v);
    v = ps_dpp_min_step<PS_DPP_ROW_BCAST31, 0xc>(v);
    return ps_lane63(v);
}
__device__ __forceinline__ uint64_t ps_wave_min_u64(uint64_t v) { return ps_wave_min(v); }
// the minimum over the LANES (16: a row, 64: the wave) that serve one query
template <int LANES, typename K>
__device__ __forceinline__ K ps_lanes_min(K v) {
    static_assert(LANES == 16 || LANES == 64, "a row or the wave");
    if constexpr (LANES == 16) return ps_row_min(v);
    else return ps_wave_min(v);
}

// Hamming keys are distance << shift | slice-local id in one 32-bit word: distances of nbits-bit codes (0 .. nbits) need
// log2(nbits) + 1 bits, the ids get the rest
static inline int ps_hamming_key_shift(int nbits) {
    int dbits = 1;
    while ((1 << (dbits - 1)) < nbits) ++dbits;
    return 32 - dbits;
}
