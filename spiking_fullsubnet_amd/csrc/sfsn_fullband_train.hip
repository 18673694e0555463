// sfsn_fullband_train.hip -- the cIRM-GSN deep filter of the TRAINING path (training.FullbandDeepFilterFn), forward and backward.
// gfx950 only.
//
// The coefficients are the projection's output in its own layout, coef [T][B][P], P = 2 df S F, channel p = ((c df + d) S + s) F + f:
// 395 MB at the recipe's B = 64, T = 1000.  Both kernels stream them exactly once; the only difficulty is layout -- coefficient rows
// run along f, spectrum / output / cotangent rows along t.
//
// Work item = one workgroup of 256 threads: (clip b, 32 frames, 32 bins), every speaker and tap.
//   * the spectrum tile X[b][f0 .. f0+31][t0-(df-1) .. t0+31] goes to LDS once (lanes along t: 256-byte runs), zero left of frame 0;
//   * coefficient side: thread (hi, lo) = (tid / 32, tid % 32) owns bin f0 + lo and frames t0 + hi + 8 k, k < 4, so a wave touches two
//     coefficient rows per instruction in runs of 32 bins (128 bytes);
//   * spectrum side: thread (hi, lo) owns frame t0 + lo and bins f0 + hi + 8 k: runs of 32 frames (256 bytes);
//   * the [32 bins][32 frames] tile of complex values is turned in LDS between the two (float2 elements).
// LDS rows have an odd number of float2 elements (47 = 32 + 15 for the spectrum tile with its df - 1 <= 15 history frames, 33 for the
// turned tile): a row stride of 2 * odd dwords puts the 32 bins of a half wave on 32 different bank pairs for ds_read_b64 (64 banks)
// and the 16 bins of a ds_write_b64 lane group on 16 different pairs of the 32 store banks.
// No atomics, no waits between workgroups, static LDS (20 KB): a launch is the launch and nothing else.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sfsn.h"

#define FDT_TT 32  // frames per workgroup
#define FDT_FB 32  // bins per workgroup
#define FDT_XW 47  // float2 per row of the spectrum tile: FDT_TT + 15 history frames (df <= 16); odd
#define FDT_YW 33  // float2 per row of the turned tile; odd

struct FdtGeom {
    int B, F, T, S, df, NFB, NTT;
};

// the spectrum tile of a work item: xs[fl][j] = X[b][f0 + fl][t0 - (df - 1) + j], zero outside [0, T) and for bins >= F
__device__ __forceinline__ void fdt_stage_spectrum(const float* __restrict__ spec, const FdtGeom& g, int b, int f0, int t0, int hi, int lo,
                                                   float2 (*xs)[FDT_XW]) {
    const int W = FDT_TT + g.df - 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int fl = hi + 8 * k, f = f0 + fl;
        for (int j = lo; j < W; j += 32) {
            const int t = t0 - (g.df - 1) + j;
            float2 v = make_float2(0.0f, 0.0f);
            if (f < g.F && t >= 0 && t < g.T) v = *reinterpret_cast<const float2*>(spec + (((size_t)b * g.F + f) * g.T + t) * 2);
            xs[fl][j] = v;
        }
    }
}

__global__ __launch_bounds__(256) void fullband_df_fwd_kernel(const float* __restrict__ spec, const float* __restrict__ coef,
                                                              float* __restrict__ enh, const FdtGeom g) {
    __shared__ float2 xs[FDT_FB][FDT_XW];
    __shared__ float2 ys[FDT_FB][FDT_YW];
    const unsigned blk = blockIdx.x;
    const int fb = (int)(blk % (unsigned)g.NFB);
    const unsigned rest = blk / (unsigned)g.NFB;
    const int tile = (int)(rest % (unsigned)g.NTT), b = (int)(rest / (unsigned)g.NTT);
    const int f0 = fb * FDT_FB, t0 = tile * FDT_TT;
    const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;
    const int F = g.F, T = g.T, S = g.S, df = g.df;
    fdt_stage_spectrum(spec, g, b, f0, t0, hi, lo, xs);
    __syncthreads();
    const int f = f0 + lo;
    const size_t P = (size_t)2 * df * S * F;
    const float* crow[4];
    bool live[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int t = t0 + hi + 8 * k;
        live[k] = f < F && t < T;
        crow[k] = coef + ((size_t)(live[k] ? t : 0) * g.B + b) * P + (live[k] ? f : 0);
    }
    for (int s = 0; s < S; ++s) {
        float yr[4] = {0.0f, 0.0f, 0.0f, 0.0f}, yi[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int d = 0; d < df; ++d) {  // taps ascending
            const size_t pr = ((size_t)d * S + s) * F, pi = ((size_t)(df + d) * S + s) * F;
            float cr[4], ci[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                cr[k] = live[k] ? crow[k][pr] : 0.0f;
                ci[k] = live[k] ? crow[k][pi] : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float2 x = xs[lo][hi + 8 * k + d];
                yr[k] += x.x * cr[k] - x.y * ci[k];
                yi[k] += x.x * ci[k] + x.y * cr[k];
            }
        }
        if (s > 0) __syncthreads();  // the previous speaker's tile has been read out
#pragma unroll
        for (int k = 0; k < 4; ++k) ys[lo][hi + 8 * k] = make_float2(yr[k], yi[k]);
        __syncthreads();
        const int t = t0 + lo;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int fl = hi + 8 * k, f2 = f0 + fl;
            if (f2 < F && t < T) *reinterpret_cast<float2*>(enh + ((((size_t)b * S + s) * F + f2) * T + t) * 2) = ys[fl][lo];
        }
    }
}

__global__ __launch_bounds__(256) void fullband_df_bwd_kernel(const float* __restrict__ spec, const float* __restrict__ gy,
                                                              float* __restrict__ d_coef, const FdtGeom g) {
    __shared__ float2 xs[FDT_FB][FDT_XW];
    __shared__ float2 gs[FDT_FB][FDT_YW];
    const unsigned blk = blockIdx.x;
    const int fb = (int)(blk % (unsigned)g.NFB);
    const unsigned rest = blk / (unsigned)g.NFB;
    const int tile = (int)(rest % (unsigned)g.NTT), b = (int)(rest / (unsigned)g.NTT);
    const int f0 = fb * FDT_FB, t0 = tile * FDT_TT;
    const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;
    const int F = g.F, T = g.T, S = g.S, df = g.df;
    fdt_stage_spectrum(spec, g, b, f0, t0, hi, lo, xs);
    const int f = f0 + lo;
    const size_t P = (size_t)2 * df * S * F;
    float* crow[4];
    bool live[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int t = t0 + hi + 8 * k;
        live[k] = f < F && t < T;
        crow[k] = d_coef + ((size_t)(live[k] ? t : 0) * g.B + b) * P + (live[k] ? f : 0);
    }
    for (int s = 0; s < S; ++s) {
        if (s > 0) __syncthreads();  // the previous speaker's cotangent tile has been used
        {
            const int t = t0 + lo;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int fl = hi + 8 * k, f2 = f0 + fl;
                float2 v = make_float2(0.0f, 0.0f);
                if (f2 < F && t < T) v = *reinterpret_cast<const float2*>(gy + ((((size_t)b * S + s) * F + f2) * T + t) * 2);
                gs[fl][lo] = v;
            }
        }
        __syncthreads();  // (the first one also covers the spectrum tile)
        float2 gv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) gv[k] = gs[lo][hi + 8 * k];
        for (int d = 0; d < df; ++d) {
            const size_t pr = ((size_t)d * S + s) * F, pi = ((size_t)(df + d) * S + s) * F;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float2 x = xs[lo][hi + 8 * k + d];
                if (live[k]) {
                    crow[k][pr] = x.x * gv[k].x + x.y * gv[k].y;
                    crow[k][pi] = x.x * gv[k].y - x.y * gv[k].x;
                }
            }
        }
    }
}

static int fdt_geometry(const void* spec, const void* other, const void* out, int B, int F, int T, int S, int df, FdtGeom* g,
                        unsigned* grid) {
    if (!spec || !other || !out || B <= 0 || F <= 0 || T <= 0 || S <= 0 || df <= 0) return SFSN_EINVAL;
    if (F > 320 || S > 4 || df > 16) return SFSN_EUNSUPPORTED;
    g->B = B; g->F = F; g->T = T; g->S = S; g->df = df;
    g->NFB = (F + FDT_FB - 1) / FDT_FB;
    const long long ntt = ((long long)T + FDT_TT - 1) / FDT_TT;
    const long long items = (long long)B * ntt * g->NFB;
    if (items > 0xffffffLL) return SFSN_EUNSUPPORTED;  // (HIP refuses a grid of 2^32 threads or more: 2^24 workgroups of 256)
    g->NTT = (int)ntt;
    *grid = (unsigned)items;
    return SFSN_OK;
}

extern "C" int sfsn_fullband_deepfilter_fwd(const float* spec_ri, const float* coef, int B, int F, int T, int S, int df, float* enh_ri,
                                            void* stream) {
    FdtGeom g;
    unsigned grid;
    const int rc = fdt_geometry(spec_ri, coef, enh_ri, B, F, T, S, df, &g, &grid);
    if (rc != SFSN_OK) return rc;
    if ((reinterpret_cast<uintptr_t>(spec_ri) & 7u) || (reinterpret_cast<uintptr_t>(enh_ri) & 7u) || (reinterpret_cast<uintptr_t>(coef) & 3u))
        return SFSN_EINVAL;
    hipLaunchKernelGGL(fullband_df_fwd_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), spec_ri, coef, enh_ri, g);
    return hipGetLastError() == hipSuccess ? SFSN_OK : SFSN_EHIP;
}

extern "C" int sfsn_fullband_deepfilter_bwd(const float* spec_ri, const float* g_ri, int B, int F, int T, int S, int df, float* d_coef,
                                            void* stream) {
    FdtGeom g;
    unsigned grid;
    const int rc = fdt_geometry(spec_ri, g_ri, d_coef, B, F, T, S, df, &g, &grid);
    if (rc != SFSN_OK) return rc;
    if ((reinterpret_cast<uintptr_t>(spec_ri) & 7u) || (reinterpret_cast<uintptr_t>(g_ri) & 7u) || (reinterpret_cast<uintptr_t>(d_coef) & 3u))
        return SFSN_EINVAL;
    hipLaunchKernelGGL(fullband_df_bwd_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), spec_ri, g_ri, d_coef, g);
    return hipGetLastError() == hipSuccess ? SFSN_OK : SFSN_EHIP;
}
