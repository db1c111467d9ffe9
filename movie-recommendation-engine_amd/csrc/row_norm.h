// What the one-wave-per-row kernels that divide a row by its norm share (ps_bn_apply, ps_linear_epilogue_bwd): the 16-byte /
// 4-byte sweeps of a row and the clamped norm of F.normalize.  A lane's sum of squares is its own fmaf chain over its columns
// 64 VEC k + VEC lane + e (sweep k and element e ascending); ps_row_norm turns the 64 chains into the norm.
#pragma once
#include "ps_common.h"

template <int VEC>
__device__ __forceinline__ void load_vec(const float *__restrict__ p, bool ok, float (&r)[VEC]) {
    if (VEC == 4) {
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok) q = *reinterpret_cast<const float4 *>(p);
        r[0] = q.x; r[1 % VEC] = q.y; r[2 % VEC] = q.z; r[3 % VEC] = q.w;
    } else {
        r[0] = ok ? p[0] : 0.f;
    }
}

template <int VEC>
__device__ __forceinline__ void store_vec(float *__restrict__ p, const float (&r)[VEC]) {
    if (VEC == 4) *reinterpret_cast<float4 *>(p) = make_float4(r[0], r[1 % VEC], r[2 % VEC], r[3 % VEC]);
    else p[0] = r[0];
}

// sqrtf of the wave sum of the lanes' chains (in every lane); ps_row_clamp is F.normalize's clamp_min(1e-12)
__device__ __forceinline__ float ps_row_norm(float lane_acc) { return sqrtf(ps_wave_sum_f32(lane_acc)); }
__device__ __forceinline__ float ps_row_clamp(float nrm) {
    return nrm < 1e-12f ? 1e-12f : nrm;                                  // a NaN norm stays (fmaxf would drop it): the whole row is NaN
}
