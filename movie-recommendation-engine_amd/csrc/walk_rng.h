// The uniforms of the walk kernels (csrc/walk_sample.hip, csrc/walk_biased.hip): one copy, so that a walk replayed by another
// kernel draws the same numbers.
#pragma once
#include "ps_common.h"

// genrand_res53: two 32-bit words -> a double in [0, 1), as numpy's random_sample combines them
__device__ __forceinline__ double ps_res53(uint32_t a, uint32_t b) {
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

// PS_RNG_STREAM_RAW: the stream as the generator leaves it (untempered MT19937 state words); uniform i = words 2i, 2i+1,
// tempered and combined by ps_res53 -- saves the separate conversion pass over the stream
__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
}

// One Philox4x32-10 block = the uniforms of two consecutive steps of a walk: counter (node, walk, step / 2, call);
// words (0, 1) -> even step, (2, 3) -> odd step.
__device__ __forceinline__ void philox_uniform2(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2,
                                                uint32_t c3, double &u_even, double &u_odd) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    u_even = ps_res53(c0, c1);
    u_odd = ps_res53(c2, c3);
}

// The uniform of step `st` of walk i (start node s) in the kernels that walk one walk at a time (ps_walk_paths,
// ps_walk_paths_biased): stream position ubase + st, or the half of the Philox block (s, walk, st / 2, call) that the step's
// parity names, where walk = i % walk_mod for walk_mod > 0 (the walk's number under its start node in ps_walk_sample) and i otherwise
__device__ __forceinline__ double walk_step_uniform(int rng_mode, const double *uniforms, int64_t ubase, uint32_t k0, uint32_t k1,
                                                    uint32_t call, int walk_mod, int64_t s, int64_t i, int st) {
    if (rng_mode == PS_RNG_STREAM) return uniforms[ubase + st];
    double u, u_odd;
    philox_uniform2(k0, k1, (uint32_t)s, (uint32_t)(walk_mod > 0 ? i % walk_mod : i), (uint32_t)(st >> 1), call, u, u_odd);
    return (st & 1) ? u_odd : u;
}
