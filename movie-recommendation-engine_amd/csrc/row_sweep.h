// What the one-wave-per-row kernels share: the 16-byte / 4-byte sweeps of a row (VEC = 4 / 1 floats per lane), the kept id of a
// neighbour slot and a lane's value for the whole wave (the gathers of neigh_agg*.hip, spmm_exact.hip), and for the kernels that
// divide a row by its norm (ps_bn_apply, ps_linear_epilogue_bwd, ps_bn_bwd) the clamped norm of F.normalize, the batch-norm
// pre-activation and the epilogue's backward; for the layer norm (layer_norm.hip) a row's mean and rstd, its xh and the two
// row sums of its backward.
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

// ---- layer norm over a row (csrc/layer_norm.hip) ----
// Rows of up to PS_LN_KEEP sweeps stay in registers between the passes over them; the sweeps beyond are read again, by the lane
// that read them before (and that writes the same addresses afterwards: the output may be the input).  Both forms run the same
// chains in the same order and give the same bits.
constexpr int PS_LN_KEEP = 4;

// xh of one element: the difference rounded, then the product
__device__ __forceinline__ float ps_ln_xhat(float x, float mean, float rstd) { return (x - mean) * rstd; }

// (mean, rstd) of the row xr[0..N), in every lane, two passes: S = the wave sum of the lane chains acc = acc + x from +0.0,
// mean = S / (float)N, Q = the wave sum of the chains acc = fmaf(d, d, acc) of d = x - mean, rstd = 1 / sqrtf(Q / (float)N + eps).
// kept[k] receives the lane's share of sweep k < PS_LN_KEEP (+0.0 past N).  A column past N adds +0.0 to S and nothing to Q.
template <int VEC>
__device__ __forceinline__ float2 ps_ln_row_stats(const float *xr, int N, float eps, float (&kept)[PS_LN_KEEP][VEC]) {
    const int lane = threadIdx.x & 63;
    const int chunk = 64 * VEC;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < PS_LN_KEEP; ++k) {
        const int col = k * chunk + lane * VEC;
        load_vec<VEC>(xr + col, col < N, kept[k]);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc = acc + kept[k][e];
    }
    for (int c0 = PS_LN_KEEP * chunk; c0 < N; c0 += chunk) {
        const int col = c0 + lane * VEC;
        float xx[VEC];
        load_vec<VEC>(xr + col, col < N, xx);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc = acc + xx[e];
    }
    const float mean = ps_wave_sum_f32(acc) / (float)N;
    acc = 0.f;
#pragma unroll
    for (int k = 0; k < PS_LN_KEEP; ++k) {
        if (k * chunk + lane * VEC < N) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float d = kept[k][e] - mean;
                acc = fmaf(d, d, acc);
            }
        }
    }
    for (int c0 = PS_LN_KEEP * chunk; c0 < N; c0 += chunk) {
        const int col = c0 + lane * VEC;
        if (col < N) {
            float xx[VEC];
            load_vec<VEC>(xr + col, true, xx);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float d = xx[e] - mean;
                acc = fmaf(d, d, acc);
            }
        }
    }
    const float var = ps_wave_sum_f32(acc) / (float)N;
    return make_float2(mean, 1.0f / sqrtf(var + eps));
}

// the VEC elements at column col < N of the layer norm's backward: gg = gy * gamma (rounded) and xh
template <int VEC>
__device__ __forceinline__ void ps_ln_bwd_elems(const float *xr, const float *gr, const float *__restrict__ gamma, int col,
                                                float mean, float rstd, float (&gg)[VEC], float (&xh)[VEC]) {
    float xx[VEC], g[VEC], ga[VEC];
    load_vec<VEC>(xr + col, true, xx);
    load_vec<VEC>(gr + col, true, g);
    load_vec<VEC>(gamma + col, true, ga);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        gg[e] = g[e] * ga[e];
        xh[e] = ps_ln_xhat(xx[e], mean, rstd);
    }
}

// (c1, c2) of a row of the layer norm's backward, in every lane: the wave sums of the lane chains acc = acc + gg and
// acc = fmaf(gg, xh, acc) from +0.0.  gg[k] / xh[k] receive the lane's share of sweep k < PS_LN_KEEP (untouched past N).
template <int VEC>
__device__ __forceinline__ float2 ps_ln_bwd_row_sums(const float *xr, const float *gr, const float *__restrict__ gamma, int N,
                                                     float mean, float rstd, float (&gg)[PS_LN_KEEP][VEC],
                                                     float (&xh)[PS_LN_KEEP][VEC]) {
    const int lane = threadIdx.x & 63;
    const int chunk = 64 * VEC;
    float a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int k = 0; k < PS_LN_KEEP; ++k) {
        const int col = k * chunk + lane * VEC;
        if (col < N) {
            ps_ln_bwd_elems<VEC>(xr, gr, gamma, col, mean, rstd, gg[k], xh[k]);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                a1 = a1 + gg[k][e];
                a2 = fmaf(gg[k][e], xh[k][e], a2);
            }
        }
    }
    for (int c0 = PS_LN_KEEP * chunk; c0 < N; c0 += chunk) {
        const int col = c0 + lane * VEC;
        if (col < N) {
            float g1[VEC], x1[VEC];
            ps_ln_bwd_elems<VEC>(xr, gr, gamma, col, mean, rstd, g1, x1);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                a1 = a1 + g1[e];
                a2 = fmaf(g1[e], x1[e], a2);
            }
        }
    }
    return make_float2(ps_wave_sum_f32(a1), ps_wave_sum_f32(a2));
}
