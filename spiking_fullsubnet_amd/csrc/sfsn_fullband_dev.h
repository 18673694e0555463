// sfsn_fullband_dev.h -- the cIRM-GSN model's per-element arithmetic, shared by the offline kernels (sfsn_fullband.hip) and the
// one-launch streaming hop (sfsn_fullband_hop.hip): one definition of every expression is what keeps the two bit-identical.
// gfx950 only.
#ifndef SFSN_FULLBAND_DEV_H
#define SFSN_FULLBAND_DEV_H
#include <hip/hip_runtime.h>
#include <math.h>

#include "sfsn.h"
#include "sfsn_feat_dev.h"
#include "sfsn_scan_dev.h"

// One feature row over a wave: lane holds v[u] = |X|^fdrc of bin lane + 64 u (0 for bins >= F) -> y[u] = LayerNorm over the F bins
// (feat_chunk_rows' LayerNorm, expression for expression), or v itself without one.  A slot past ceil(F / 64) holds zeros and adds
// nothing to either sum, so NU may be larger than the row needs.
template <int NU>
__device__ __forceinline__ void fullband_norm_row(const float (&v)[NU], int lane, int F, bool ln, const float (&lw)[NU], const float (&lb)[NU],
                                                  float eps, float (&y)[NU]) {
    if (!ln) {
#pragma unroll
        for (int u = 0; u < NU; ++u) y[u] = v[u];
        return;
    }
    const float inv_I = 1.0f / (float)F;
    float sum = 0.0f;
#pragma unroll
    for (int u = 0; u < NU; ++u) sum += v[u];
    const float mean = wave_sum(sum) * inv_I;
    float ss = 0.0f;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const float d = v[u] - mean;
        if (lane + 64 * u < F) ss += d * d;
    }
    const float rstd = __builtin_amdgcn_rsqf(wave_sum(ss) * inv_I + eps);
#pragma unroll
    for (int u = 0; u < NU; ++u) y[u] = ((v[u] - mean) * rstd) * lw[u] + lb[u];
}

__device__ __forceinline__ float fbd_act(float v, int act) {
    if (act == SFSN_ACT_TANH) return tanhf(v);
    if (act == SFSN_ACT_SIGMOID) return 1.0f / (1.0f + expf(-v));
    if (act == SFSN_ACT_RELU) return v < 0.0f ? 0.0f : v;
    return v;
}

// a projection output from its three exact digit sums: sfsn_spike_proj's epilogue
__device__ __forceinline__ float fbd_coef(int a0, int a1, int a2, float dq, float bias) { return recombine3(a0, a1, a2) * dq + bias; }

// one deep-filter tap, the oracle's deepfilter_group: taps are added d ascending, no contraction (-ffp-contract=off)
__device__ __forceinline__ void fbd_tap(float& yr, float& yi, float2 xv, float cr, float ci) {
    yr += xv.x * cr - xv.y * ci;
    yi += xv.x * ci + xv.y * cr;
}

// |.| as glibc's hypotf rounds it (the oracle's finish_spectrum): the double sum of squares, one correctly rounded sqrt
__device__ __forceinline__ float fbd_mag(float yr, float yi) {
    return (float)__builtin_sqrt((double)yr * (double)yr + (double)yi * (double)yi);
}

#endif
