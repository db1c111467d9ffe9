// The pick of a walk step, searchsorted(cdf[lo:hi], u, 'right') on a row's fp64 CDF, where the walk kernels share it
// (csrc/walk_sample.hip, csrc/walk_biased.hip): the bucket index of the guide table and the scalar search.  The lock-step and
// record searches of ps_walk_sample (search_two*) stay in csrc/walk_sample.hip and use the bucket index.
#pragma once
#include "ps_common.h"

constexpr int LIN_PROBES = 12;   // forward-scan probes after the guide lookup before falling back to bisection

// floor(u * deg) clamped to deg - 1: the 1/deg-wide bucket of the row lo .. hi (deg = hi - lo > 0) that u falls into
template <class I>
__device__ __forceinline__ uint32_t cdf_bucket(I lo, I hi, double u) {
    const uint32_t deg = (uint32_t)(hi - lo);
    const uint32_t j = (uint32_t)(u * (double)deg);
    return j >= deg ? deg - 1 : j;
}

// The edge that searchsorted(cdf[lo:hi], u, 'right') picks in a non-empty row (the last one where u >= cdf[hi - 1]).  With a
// guide table (guide[lo + j] = #{cdf <= (j/deg)(1-2^-50)} <= answer) the search starts at the guide entry of u's bucket, scans
// LIN_PROBES entries forward and then bisects; a null guide bisects from lo.
template <class I>
__device__ __forceinline__ I cdf_search(const double *cdf, const int32_t *guide, I lo, I hi, double u) {
    I l = lo, h = hi;
    int n = LIN_PROBES;
    if (guide) {
        l = lo + (I)guide[lo + cdf_bucket(lo, hi, u)];
        n = 0;
    }
    while (l < h) {
        const I mid = (n < LIN_PROBES) ? l : l + ((h - l) >> 1);
        if (cdf[mid] <= u) l = mid + 1; else h = mid;
        ++n;
    }
    return l >= hi ? hi - 1 : l;
}
