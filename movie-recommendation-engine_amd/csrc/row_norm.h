// What the one-wave-per-row kernels that divide a row by its norm share (ps_bn_apply, ps_linear_epilogue_bwd, ps_bn_bwd): the
// 16-byte / 4-byte sweeps of a row, the clamped norm of F.normalize, the batch-norm pre-activation and the epilogue's backward.
// A lane's sum of squares is its own fmaf chain over its columns 64 VEC k + VEC lane + e (sweep k and element e ascending);
// ps_row_norm turns the 64 chains into the norm.
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

constexpr int PS_BN_ROWS = 128;        // rows per partition of the column sums (ps_bn_batch_stats, ps_bn_bwd): a function of M only

// the batch-norm layer's activation before the row norm from d = z - mean (already rounded): fmaf(d, scale, beta), ReLU when relu
__device__ __forceinline__ float ps_bn_act(float d, float scale, float beta, bool relu) {
    const float a = fmaf(d, scale, beta);
    return (relu && a < 0.f) ? 0.f : a;
}

// one element of ps_linear_epilogue_bwd: the gradient of the pre-activation from the activation t, the output's gradient g and
// the row's c = ps_row_clamp(nrm), below = nrm < 1e-12f, s = sum g (t / c)
__device__ __forceinline__ float ps_epilogue_ga(float t, float g, bool relu, bool l2, float c, bool below, float s) {
    float gt = g;
    if (l2) gt = below ? g / c : fmaf(-(t / c), s, g) / c;
    return (relu && !(t > 0.f)) ? 0.f : gt;
}
