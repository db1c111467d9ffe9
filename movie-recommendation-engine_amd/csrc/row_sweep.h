// What the one-wave-per-row kernels share: the 16-byte / 4-byte sweeps of a row (VEC = 4 / 1 floats per lane), the kept id of a
// neighbour slot and a lane's value for the whole wave (the gathers of neigh_agg*.hip, spmm_exact.hip), and for the kernels that
// divide a row by its norm (ps_bn_apply, ps_linear_epilogue_bwd, ps_bn_bwd) the clamped norm of F.normalize, the batch-norm
// pre-activation and the epilogue's backward.
// A lane's sum of squares is its own fmaf chain over its columns 64 VEC k + VEC lane + e (sweep k and element e ascending);
// ps_row_norm turns the 64 chains into the norm.
#pragma once
#include "ps_common.h"

// the VEC floats at p (zeros when !ok: nothing is requested)
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
__device__ __forceinline__ void load_veci(const int32_t *__restrict__ p, bool ok, int32_t (&r)[VEC]) {      // -1 when !ok
    if (VEC == 4) {
        int4 q = make_int4(-1, -1, -1, -1);
        if (ok) q = *reinterpret_cast<const int4 *>(p);
        r[0] = q.x; r[1 % VEC] = q.y; r[2 % VEC] = q.z; r[3 % VEC] = q.w;
    } else {
        r[0] = ok ? p[0] : -1;
    }
}
template <int VEC>
__device__ __forceinline__ void store_vec(float *__restrict__ p, const float (&r)[VEC]) {
    if (VEC == 4) *reinterpret_cast<float4 *>(p) = make_float4(r[0], r[1 % VEC], r[2 % VEC], r[3 % VEC]);
    else p[0] = r[0];
}
template <int VEC>
__device__ __forceinline__ void store_veci(int32_t *__restrict__ p, const int32_t (&r)[VEC]) {
    if (VEC == 4) *reinterpret_cast<int4 *>(p) = make_int4(r[0], r[1 % VEC], r[2 % VEC], r[3 % VEC]);
    else p[0] = r[0];
}

// lane t's v (t wave-uniform)
__device__ __forceinline__ float lane_f32(float v, int t) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), t));
}

// the kept id of slot jj of row i of ids[., T] (-1: not kept): jj < k = min(nvalid[i], T) and 0 <= id < N
__device__ __forceinline__ int32_t kept_id(const int32_t *__restrict__ ids, int64_t i, int T, int jj, int k, int64_t N) {
    int32_t id = -1;
    if (jj < k) {
        id = ids[i * T + jj];
        if (id < 0 || (int64_t)id >= N) id = -1;
    }
    return id;
}

// sqrtf of the wave sum of the lanes' chains (in every lane); ps_row_clamp is F.normalize's clamp_min(1e-12)
__device__ __forceinline__ float ps_row_norm(float lane_acc) { return sqrtf(ps_wave_sum_f32(lane_acc)); }
__device__ __forceinline__ float ps_row_clamp(float nrm) {
    return nrm < 1e-12f ? 1e-12f : nrm;                                  // a NaN norm stays (fmaxf would drop it): the whole row is NaN
}

// The two row sums of the norm's backward, in every lane: nrm = ps_row_norm of the chains of t^2, and s = the wave sum of the
// chains of g (t / c), c = ps_row_clamp(nrm).  act(col, ok, t) yields the activation's VEC elements at column col (+0.0 for !ok,
// a column past N); g is the row of the output's gradient.  Two sweeps, columns ascending in both.
template <int VEC, typename ACT>
__device__ __forceinline__ float2 ps_row_norm_sums(int N, const float *g, ACT act) {
    const int lane = threadIdx.x & 63;
    const int chunk = 64 * VEC;
    float acc = 0.f;
    for (int c0 = 0; c0 < N; c0 += chunk) {
        const int col = c0 + lane * VEC;
        float tt[VEC];
        act(col, col < N, tt);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc = fmaf(tt[e], tt[e], acc);
    }
    const float nrm = ps_row_norm(acc);
    const float c = ps_row_clamp(nrm);
    acc = 0.f;
    for (int c0 = 0; c0 < N; c0 += chunk) {
        const int col = c0 + lane * VEC;
        float tt[VEC], gg[VEC];
        act(col, col < N, tt);
        load_vec<VEC>(g + col, col < N, gg);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc = fmaf(gg[e], tt[e] / c, acc);
    }
    return make_float2(nrm, ps_wave_sum_f32(acc));
}

// the batch-norm layer's activation before the row norm from d = z - mean (already rounded): fmaf(d, scale, beta), ReLU when relu
__device__ __forceinline__ float ps_bn_act(float d, float scale, float beta, bool relu) {
    const float a = fmaf(d, scale, beta);
    return (relu && a < 0.f) ? 0.f : a;
}
// ps_bn_act over the VEC columns at col of row zr (a column past N: fmaf(0 - 0, 0, 0) = +0.0)
template <int VEC>
__device__ __forceinline__ void ps_bn_act_vec(const float *zr, const float *__restrict__ mean, const float *__restrict__ scale,
                                              const float *__restrict__ beta, int col, bool ok, bool relu, float (&t)[VEC]) {
    float zz[VEC], mm[VEC], sc[VEC], bb[VEC];
    load_vec<VEC>(zr + col, ok, zz);
    load_vec<VEC>(mean + col, ok, mm);
    load_vec<VEC>(scale + col, ok, sc);
    load_vec<VEC>(beta + col, ok, bb);
#pragma unroll
    for (int e = 0; e < VEC; ++e) t[e] = ps_bn_act(zz[e] - mm[e], sc[e], bb[e], relu);
}

// one element of ps_linear_epilogue_bwd: the gradient of the pre-activation from the activation t, the output's gradient g and
// the row's c = ps_row_clamp(nrm), below = nrm < 1e-12f, s = sum g (t / c)
__device__ __forceinline__ float ps_epilogue_ga(float t, float g, bool relu, bool l2, float c, bool below, float s) {
    float gt = g;
    if (l2) gt = below ? g / c : fmaf(-(t / c), s, g) / c;
    return (relu && !(t > 0.f)) ? 0.f : gt;
}
