// sfsn_resample.hip -- the 3:1 decimator and the 1:3 interpolator of sfsn_resample_dev.h as stand-alone launches with carried state
// (sfsn_resample_down3 / sfsn_resample_up3): what a waveform session with outer samples uses for its first call, and what checks the
// one-launch hop's converted samples bit for bit.  One workgroup per row: the row's old state is parked in LDS before anything is
// written, so the state is updated in place.  gfx950 only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sfsn.h"

#include "sfsn_resample_dev.h"
#include "sfsn_host.h"

namespace {

#define RS_THREADS 256

// in: [B] rows of 3 n_out samples (row stride in_stride samples) -> out [B][n_out]; state [B][96] (NULL: zeros, not written)
template <int FMT>
__global__ __launch_bounds__(RS_THREADS) void resample_down3_kernel(const void* in, int n_out, long long in_stride, const float* taps,
                                                                    float* state, float* out) {
    __shared__ float old[RS_DEC_ROW];
    const int b = blockIdx.x, tid = threadIdx.x;
    float* st = state ? state + (size_t)b * RS_DEC_ROW : nullptr;
    if (tid < RS_DEC_ROW) old[tid] = st && tid < RS_DEC_KEEP ? st[tid] : 0.0f;
    __syncthreads();
    const size_t row = (size_t)b * (size_t)in_stride;
    const long long n_in = 3ll * n_out;
    // sample n of the row's history: n >= 0 the new samples, n < 0 the carried ones (old[93 + n])
    auto x = [&](long long n) { return n >= 0 ? rs_load<FMT>(in, row + (size_t)n) : old[RS_DEC_KEEP + n]; };
    for (int m = tid; m < n_out; m += RS_THREADS) {
        const long long n0 = 3ll * m - RS_DEC_KEEP;
        out[(size_t)b * n_out + m] = rs_down3_sum(taps, [&](int i) { return x(n0 + i); });
    }
    if (st && tid < RS_DEC_ROW) st[tid] = tid < RS_DEC_KEEP ? x(n_in - RS_DEC_KEEP + tid) : 0.0f;
}

// in: [R][n_in] -> out: [R] rows of 3 n_in samples (row stride out_stride samples); state [R][32] (NULL: zeros, not written)
template <int FMT>
__global__ __launch_bounds__(RS_THREADS) void resample_up3_kernel(const float* in, int n_in, const float* phase_taps, float* state, void* out,
                                                                  long long out_stride) {
    __shared__ float old[RS_INT_ROW];
    const int r = blockIdx.x, tid = threadIdx.x;
    float* st = state ? state + (size_t)r * RS_INT_ROW : nullptr;
    if (tid < RS_INT_ROW) old[tid] = st && tid < RS_INT_KEEP ? st[tid] : 0.0f;
    __syncthreads();
    const float* src = in + (size_t)r * n_in;
    auto y = [&](int n) { return n >= 0 ? src[n] : old[RS_INT_KEEP + n]; };
    const size_t row = (size_t)r * (size_t)out_stride;
    for (int m = tid; m < n_in; m += RS_THREADS) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
            rs_store<FMT>(out, row + 3 * (size_t)m + p, rs_up3_sum(phase_taps + RS_PHASE_TAPS * p, [&](int i) { return y(m - RS_INT_KEEP + i); }));
    }
    if (st && tid < RS_INT_ROW) st[tid] = tid < RS_INT_KEEP ? y(n_in - RS_INT_KEEP + tid) : 0.0f;
}

bool known_format(int f) { return f == SFSN_SAMPLE_F32 || f == SFSN_SAMPLE_S16; }

}  // namespace

extern "C" int sfsn_resample_down3(const void* in, int in_format, int B, int n_out, long long in_stride, const float* taps, float* state,
                                   float* out, void* stream) {
    if (!known_format(in_format)) return SFSN_EINVAL;
    if (!in || !taps || !out || B <= 0 || n_out <= 0 || n_out > (1 << 28) || in_stride < 3ll * n_out) return SFSN_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (in_format == SFSN_SAMPLE_S16)
        hipLaunchKernelGGL(resample_down3_kernel<RS_S16>, dim3(B), dim3(RS_THREADS), 0, st, in, n_out, in_stride, taps, state, out);
    else
        hipLaunchKernelGGL(resample_down3_kernel<RS_F32>, dim3(B), dim3(RS_THREADS), 0, st, in, n_out, in_stride, taps, state, out);
    return hip_ok(hipGetLastError());
}

extern "C" int sfsn_resample_up3(const float* in, int R, int n_in, const float* phase_taps, float* state, void* out, int out_format,
                                 long long out_stride, void* stream) {
    if (!known_format(out_format)) return SFSN_EINVAL;
    if (!in || !phase_taps || !out || R <= 0 || n_in <= 0 || n_in > (1 << 28) || out_stride < 3ll * n_in) return SFSN_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (out_format == SFSN_SAMPLE_S16)
        hipLaunchKernelGGL(resample_up3_kernel<RS_S16>, dim3(R), dim3(RS_THREADS), 0, st, in, n_in, phase_taps, state, out, out_stride);
    else
        hipLaunchKernelGGL(resample_up3_kernel<RS_F32>, dim3(R), dim3(RS_THREADS), 0, st, in, n_in, phase_taps, state, out, out_stride);
    return hip_ok(hipGetLastError());
}
