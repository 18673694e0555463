// sfsn_resample_dev.h -- the outer sample rate and format of the waveform sessions, defined once: the 3:1 decimator and the 1:3
// interpolator around the model's own rate (one 96-tap linear-phase low-pass, polyphase on the way up) and the two sample formats
// (float32, 16-bit PCM).  The stand-alone kernels (sfsn_resample.hip) and the one-launch hop (sfsn_hop_wave_dev.h) call THESE
// functions, so they give the same bits -- the rule sfsn_fft_dev.h follows for the transforms.  gfx950 only.
//
// Summation order (part of the contract, include/sfsn.h): one fp32 accumulator that starts at 0.0f, fmaf, ascending tap index.
#ifndef SFSN_RESAMPLE_DEV_H
#define SFSN_RESAMPLE_DEV_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RS_TAPS 96        // h[0 .. 95]
#define RS_PHASE_TAPS 32  // 3 h[3 j + p], j = 0 .. 31, per phase p
#define RS_DEC_KEEP 93    // input samples the decimator carries (RS_TAPS - 3), oldest first, in a row of RS_DEC_ROW floats
#define RS_DEC_ROW 96
#define RS_INT_KEEP 31    // model-rate samples the interpolator carries (RS_PHASE_TAPS - 1), oldest first, in a row of RS_INT_ROW
#define RS_INT_ROW 32
#define RS_F32 0          // = SFSN_SAMPLE_F32
#define RS_S16 1          // = SFSN_SAMPLE_S16

// sample i of a buffer of format FMT as float ("s16": s * 2^-15, exact)
template <int FMT>
__device__ __forceinline__ float rs_load(const void* p, size_t i) {
    if constexpr (FMT == RS_S16) return (float)static_cast<const int16_t*>(p)[i] * (1.0f / 32768.0f);
    return static_cast<const float*>(p)[i];
}
// "s16" out: clamp(rintf(v * 32768), -32768, 32767), ties to even, NaN -> 0
__device__ __forceinline__ int16_t rs_quantise(float v) {
    const float r = rintf(v * 32768.0f);
    if (!(r == r)) return (int16_t)0;
    return (int16_t)(int)fminf(fmaxf(r, -32768.0f), 32767.0f);
}
template <int FMT>
__device__ __forceinline__ void rs_store(void* p, size_t i, float v) {
    if constexpr (FMT == RS_S16) static_cast<int16_t*>(p)[i] = rs_quantise(v);
    else static_cast<float*>(p)[i] = v;
}

// One decimator output: y[m] = sum_k h[k] x[3 m + 2 - k].  w(i), i = 0 .. 95: the 96 input samples x[3 m - 93 + i], oldest first.
template <class W>
__device__ __forceinline__ float rs_down3_sum(const float* __restrict__ taps, W w) {
    float acc = 0.0f;
#pragma unroll 8
    for (int k = 0; k < RS_TAPS; ++k) acc = fmaf(taps[k], w(RS_TAPS - 1 - k), acc);
    return acc;
}
// One interpolator output of phase p: z[3 m + p] = sum_j g_p[j] y[m - j], g_p = phase_taps + 32 p.  w(i), i = 0 .. 31: the 32
// model-rate samples y[m - 31 + i], oldest first.
template <class W>
__device__ __forceinline__ float rs_up3_sum(const float* __restrict__ g, W w) {
    float acc = 0.0f;
#pragma unroll 8
    for (int j = 0; j < RS_PHASE_TAPS; ++j) acc = fmaf(g[j], w(RS_PHASE_TAPS - 1 - j), acc);
    return acc;
}

// N outputs of one lane side by side (the hop: a lane owns two positions): every output keeps its own accumulator chain in the stated
// order -- the bits of rs_down3_sum / rs_up3_sum -- while the loads of all chains are in flight together, and the three phases of one
// position share each window sample.  w(n, i): window sample i of output (position) n.
template <int N, class W>
__device__ __forceinline__ void rs_down3_sums(const float* __restrict__ taps, float (&acc)[N], W w) {
#pragma unroll
    for (int n = 0; n < N; ++n) acc[n] = 0.0f;
#pragma unroll 8
    for (int k = 0; k < RS_TAPS; ++k) {
        const float t = taps[k];
#pragma unroll
        for (int n = 0; n < N; ++n) acc[n] = fmaf(t, w(n, RS_TAPS - 1 - k), acc[n]);
    }
}
template <int N, class W>
__device__ __forceinline__ void rs_up3_sums(const float* __restrict__ g, float (&acc)[N][3], W w) {
#pragma unroll
    for (int n = 0; n < N; ++n) acc[n][0] = acc[n][1] = acc[n][2] = 0.0f;
#pragma unroll 8
    for (int j = 0; j < RS_PHASE_TAPS; ++j) {
#pragma unroll
        for (int n = 0; n < N; ++n) {
            const float x = w(n, RS_PHASE_TAPS - 1 - j);
#pragma unroll
            for (int p = 0; p < 3; ++p) acc[n][p] = fmaf(g[RS_PHASE_TAPS * p + j], x, acc[n][p]);
        }
    }
}

#endif
