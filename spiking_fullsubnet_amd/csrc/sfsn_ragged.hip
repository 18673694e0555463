// Batches of clips of different lengths (include/sfsn.h, "ragged batches"): the kernels at the edges of the path whose result
// depends on where a clip ends -- STFT, inverse STFT, the utterance statistics of the frozen front-end, per-clip spike counts --
// with per-clip lengths (device int32 arrays, one entry per clip), and the launch that zeroes an output's frames past each end.
//
// Every kernel here is its equal-length sibling (sfsn_fft.hip, sfsn_kernels.hip) with the clip's own length in place of the
// batch's: the same expressions on the same values in the same order, absent terms skipped, never reordered.  Clip b of a ragged
// call therefore has the bits of the sibling called on that clip alone (tests/test_ragged_kernels.py: torch.equal).  The siblings
// stay as they are: the hot equal-length path carries no length argument.
//
// The lengths are read on the device and cannot be checked by the host without a synchronisation: every kernel clamps them to
// the buffer's extent ([0, L], [0, T]) before it forms an address.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sfsn.h"

#include "sfsn_feat_dev.h"
#include "sfsn_fft_dev.h"
#include "sfsn_host.h"

namespace {

__device__ __forceinline__ int clamp_len(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ---------------------------------------------------------------------------------------------------------------------
// STFT (stft_kernel with L -> clip_len[b]): samples at index >= clip_len[b] read as zero whatever the buffer holds
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stft_ragged_kernel(const float* __restrict__ wave, const float* __restrict__ window,
                                                           float* __restrict__ X, const int32_t* __restrict__ clip_len, int B, int L, int T,
                                                           int hop) {
    __shared__ float2 fbuf[4][FFT_N];
    __shared__ float2 stage[FFT_F][FFT_TT + 1];
    const int b = blockIdx.y, t0 = blockIdx.x * FFT_TT;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __shared__ float2 unit[FFT_NFFT];
    fill_unit_table(unit, tid, 256);
    __syncthreads();
    const Twiddles tw = make_twiddles<false>(unit, lane);
    float2 win[4], wk[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = 2 * (lane + 64 * r);
        win[r] = make_float2(window[n], window[n + 1]);
        wk[r] = unit_at<false>(unit, lane + 64 * r);
    }
    const int Lb = clamp_len(clip_len[b], L);
    const float* wrow = wave + (size_t)b * L;
    for (int ft = wv; ft < FFT_TT; ft += 4) {
        const int t = t0 + ft;
        if (t >= T) break;  // wave-uniform
        const int s0 = t * hop - FFT_NFFT / 2;
        float2 v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int s = s0 + 2 * (lane + 64 * r);
            const float x0 = (s >= 0 && s < Lb) ? wrow[s] : 0.0f, x1 = (s + 1 >= 0 && s + 1 < Lb) ? wrow[s + 1] : 0.0f;
            v[r] = make_float2(x0 * win[r].x, x1 * win[r].y);
        }
        float2* buf = fbuf[wv];
        fft256<false>(v, buf, lane, tw);
        float2 Xk[4], nyq = make_float2(0.0f, 0.0f);
        rfft512_split(v, buf, lane, wk, Xk, nyq);
#pragma unroll
        for (int r = 0; r < 4; ++r) stage[lane + 64 * r][ft] = Xk[r];
        if (lane == 0) stage[FFT_N][ft] = nyq;
    }
    __syncthreads();
    const int nt = (T - t0 < FFT_TT) ? T - t0 : FFT_TT;
    for (int idx = tid; idx < FFT_F * FFT_TT; idx += 256) {
        const int f = idx >> 4, ft = idx & (FFT_TT - 1);
        if (ft < nt) *reinterpret_cast<float2*>(X + (((size_t)b * FFT_F + f) * T + t0 + ft) * 2) = stage[f][ft];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// inverse STFT (istft_kernel with T -> clip_frames[b] in every "does frame t exist" test, length -> clip_len[b] for what is kept):
// same tile origin, same ascending-frame accumulation, same env rule.  The strides stay those of the padded batch (T, length).
// A tile that lies wholly past the clip's end transforms nothing and stores zeros.
// ---------------------------------------------------------------------------------------------------------------------
#define IFFT_HALO 3
#define IFFT_WAVES 8
#define IFFT_NFR (FFT_TT + IFFT_HALO)
#define IFFT_XS_BYTES (FFT_F * (IFFT_NFR + 2) * 8)
#define IFFT_LDS (IFFT_WAVES * FFT_N * 8 + FFT_NFFT * 8 + FFT_NFFT * 4 + IFFT_XS_BYTES)
__global__ __launch_bounds__(IFFT_WAVES * 64) void istft_ragged_kernel(const float* __restrict__ X, const float* __restrict__ window,
                                                                       float* __restrict__ wave, const int32_t* __restrict__ clip_frames,
                                                                       const int32_t* __restrict__ clip_len, int B, int T, int hop, int length) {
    extern __shared__ __attribute__((aligned(16))) char ifft_smem[];
    constexpr int NFR = IFFT_NFR, FPW = (NFR + IFFT_WAVES - 1) / IFFT_WAVES;  // frames per wave
    float2(*fbuf)[FFT_N] = reinterpret_cast<float2(*)[FFT_N]>(ifft_smem);
    float2* unit = reinterpret_cast<float2*>(ifft_smem + IFFT_WAVES * FFT_N * 8);
    float* wl = reinterpret_cast<float*>(ifft_smem + IFFT_WAVES * FFT_N * 8 + FFT_NFFT * 8);
    char* region = ifft_smem + IFFT_WAVES * FFT_N * 8 + FFT_NFFT * 8 + FFT_NFFT * 4;
    float2(*xs)[NFR + 2] = reinterpret_cast<float2(*)[NFR + 2]>(region);
    float(*tbuf)[FFT_NFFT] = reinterpret_cast<float(*)[FFT_NFFT]>(region);
    static_assert(IFFT_NFR * FFT_NFFT * 4 <= IFFT_XS_BYTES, "time-domain frames must fit in the spectrum tile");
    const int b = blockIdx.y, t0 = blockIdx.x * FFT_TT;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tfirst = t0 - IFFT_HALO;
    const int Tb = clamp_len(clip_frames[b], T), Lb = clamp_len(clip_len[b], length);
    if (Tb == 0 || t0 * hop - FFT_NFFT / 2 >= Lb) {  // (workgroup-uniform) nothing of the clip in this tile
        for (int i = tid; i < FFT_TT * hop; i += IFFT_WAVES * 64) {
            const int m = t0 * hop + i - FFT_NFFT / 2;
            if (m >= 0 && m < length) wave[(size_t)b * length + m] = 0.0f;
        }
        return;
    }
    {
        const int c = tid & 31, t = tfirst + c;
        const bool live = c < NFR && t >= 0 && t < Tb;
        const int tc = live ? t : (t < 0 ? 0 : Tb - 1);
        const float* src = X + ((size_t)b * FFT_F * T + tc) * 2;
        for (int f0 = tid >> 5; f0 < FFT_F; f0 += 8 * (IFFT_WAVES * 2)) {
            float2 v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                int f = f0 + i * (IFFT_WAVES * 2);
                if (f > FFT_F - 1) f = FFT_F - 1;
                v[i] = *reinterpret_cast<const float2*>(src + (size_t)f * T * 2);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int f = f0 + i * (IFFT_WAVES * 2);
                if (f < FFT_F && c < NFR) xs[f][c] = live ? v[i] : make_float2(0.0f, 0.0f);
            }
        }
    }
    fill_unit_table(unit, tid, IFFT_WAVES * 64);
    for (int i = tid; i < FFT_NFFT; i += IFFT_WAVES * 64) wl[i] = window[i];
    __syncthreads();
    const Twiddles tw = make_twiddles<true>(unit, lane);
    float2 win[4], wk[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = 2 * (lane + 64 * r);
        win[r] = make_float2(wl[n], wl[n + 1]);
        wk[r] = unit_at<true>(unit, lane + 64 * r);
    }
    float2 res[FPW][4];
#pragma unroll
    for (int i = 0; i < FPW; ++i) {
        const int c = wv + i * IFFT_WAVES, t = tfirst + c;
        if (c >= NFR || t < 0 || t >= Tb) continue;  // wave-uniform
        float2 v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = lane + 64 * r;
            v[r] = irfft512_presplit(xs[k][c], xs[FFT_N - k][c], k, wk[r]);
        }
        fft256<true>(v, fbuf[wv], lane, tw);
        const float sc = 1.0f / (float)FFT_N;
#pragma unroll
        for (int r = 0; r < 4; ++r) res[i][r] = make_float2(v[r].x * sc * win[r].x, v[r].y * sc * win[r].y);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < FPW; ++i) {
        const int c = wv + i * IFFT_WAVES, t = tfirst + c;
        if (c >= NFR || t < 0 || t >= Tb) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) *reinterpret_cast<float2*>(&tbuf[c][2 * (lane + 64 * r)]) = res[i][r];
    }
    __syncthreads();
    const int nover = FFT_NFFT / hop;
    for (int i = tid; i < FFT_TT * hop; i += IFFT_WAVES * 64) {
        const int n = t0 * hop + i, m = n - FFT_NFFT / 2;
        if (m < 0 || m >= length) continue;
        if (m >= Lb) {  // past the clip's end: exactly zero
            wave[(size_t)b * length + m] = 0.0f;
            continue;
        }
        const int tq = n / hop;
        float acc = 0.0f, env = 0.0f;
        for (int q = nover - 1; q >= 0; --q) {  // ascending frame index
            const int t = tq - q, off = n - t * hop;
            if (t < 0 || t >= Tb || off >= FFT_NFFT) continue;
            const float w = wl[off];
            acc += tbuf[t - tfirst][off];
            env += w * w;
        }
        wave[(size_t)b * length + m] = env > 1e-11f ? acc / env : 0.0f;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// utterance statistics: rowsum_kernel / laplace_mu_kernel / gaussian_stats_kernel with T -> clip_frames[b].  The t = lane,
// lane + 64, ... partition, the double accumulators and the reduction tree are the siblings': the sums are those of the clip alone.
// ---------------------------------------------------------------------------------------------------------------------
struct RaggedGroup {
    int lo, N, ctr, nbr, ctr_fb, nbr_fb, I1, I;
};
struct RaggedStatParams {
    RaggedGroup g[SFSN_MAX_GROUPS];
    int B, F, T, FB;
};

__global__ __launch_bounds__(256) void rowsum_ragged_kernel(const float* __restrict__ stft, const float* __restrict__ fb,
                                                             float* __restrict__ rs, double* __restrict__ rs2,
                                                             const int32_t* __restrict__ clip_frames, int B, int F, int T, int FB, float fdrc) {
    const int nf = F - 1, per_b = nf + FB;
    const int wid = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wid >= B * per_b) return;
    const int b = wid / per_b, f = wid - b * per_b;
    const int Tb = clamp_len(clip_frames[b], T);
    double acc = 0.0, acc2 = 0.0;
    if (f < nf) {
        const float* src = stft + ((size_t)b * F + f) * T * 2;
        for (int t = lane; t < Tb; t += 64) {
            const float2 c = *reinterpret_cast<const float2*>(src + 2 * (size_t)t);
            const double m = (double)compress_mag(c.x, c.y, fdrc);
            acc += m;
            acc2 += m * m;
        }
    } else if (fb) {
        for (int t = lane; t < Tb; t += 64) {
            const double m = (double)fb[((size_t)t * B + b) * FB + (f - nf)];
            acc += m;
            acc2 += m * m;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { acc += __shfl_xor(acc, o); acc2 += __shfl_xor(acc2, o); }
    if (lane == 0) {
        rs[wid] = (float)acc;
        if (rs2) { rs2[wid] = acc2; reinterpret_cast<double*>(rs2 + (size_t)B * per_b)[wid] = acc; }
    }
}

__global__ __launch_bounds__(64) void gaussian_stats_ragged_kernel(const double* __restrict__ rs2, const RaggedStatParams p,
                                                                    const int32_t* __restrict__ clip_frames, float* __restrict__ mu,
                                                                    float* __restrict__ sd) {
    const int gi = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const RaggedGroup g = p.g[gi];
    const int nf = p.F - 1, per_b = nf + p.FB;
    const int Tb = clamp_len(clip_frames[b], p.T);
    const double* r2 = rs2 + (size_t)b * per_b;
    const double* r1 = rs2 + (size_t)p.B * per_b + (size_t)b * per_b;
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < g.N; ++k)
        for (int j = lane; j < g.I; j += 64) {
            const int idx = j < g.I1 ? reflect_bin(g.lo + k * g.ctr - g.nbr + j, nf)
                                     : nf + (reflect_bin(g.lo + k * g.ctr_fb - g.nbr_fb + (j - g.I1), nf) % p.FB);
            s1 += r1[idx];
            s2 += r2[idx];
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
    if (lane == 0) {
        const double n = (double)Tb * g.N * g.I, m = s1 / n;
        double var = (s2 - n * m * m) / (n - 1.0);
        if (var < 0.0) var = 0.0;
        mu[(size_t)gi * p.B + b] = (float)m;
        sd[(size_t)gi * p.B + b] = (float)sqrt(var);
    }
}

__global__ __launch_bounds__(64) void laplace_mu_ragged_kernel(const float* __restrict__ rs, const RaggedStatParams p,
                                                                const int32_t* __restrict__ clip_frames, float* __restrict__ mu) {
    const int gi = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const RaggedGroup g = p.g[gi];
    const int nf = p.F - 1, per_b = nf + p.FB;
    const int Tb = clamp_len(clip_frames[b], p.T);
    const float* r = rs + (size_t)b * per_b;
    double acc = 0.0;
    for (int k = 0; k < g.N; ++k)
        for (int j = lane; j < g.I; j += 64) {
            if (j < g.I1)
                acc += (double)r[reflect_bin(g.lo + k * g.ctr - g.nbr + j, nf)];
            else
                acc += (double)r[nf + (reflect_bin(g.lo + k * g.ctr_fb - g.nbr_fb + (j - g.I1), nf) % p.FB)];
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) mu[(size_t)gi * p.B + b] = (float)(acc / ((double)Tb * g.N * g.I));
}

// the geometry checks of the equal-length statistics calls (the group's pointers are not read)
int fill_stat_params(RaggedStatParams& p, const sfsn_feature_group* groups, int n_groups, int B, int F, int T, int FB) {
    if (!groups || n_groups <= 0 || n_groups > SFSN_MAX_GROUPS || B <= 0 || F < 2 || T <= 0 || FB < 0) return SFSN_EINVAL;
    const int nf = F - 1;
    p.B = B; p.F = F; p.T = T; p.FB = FB;
    for (int i = 0; i < n_groups; ++i) {
        const sfsn_feature_group& g = groups[i];
        if (g.n_units <= 0 || g.ctr <= 0 || g.nbr < 0 || g.ctr_fb < 0 || g.nbr_fb < 0 || g.lo < 0) return SFSN_EINVAL;
        const int I1 = g.ctr + 2 * g.nbr, I2 = g.ctr_fb > 0 ? g.ctr_fb + 2 * g.nbr_fb : 0;
        if (I1 + I2 > 256) return SFSN_EUNSUPPORTED;
        if (g.lo + g.n_units * g.ctr > nf || g.nbr >= nf || (I2 && (FB <= 0 || g.nbr_fb >= nf))) return SFSN_EINVAL;
        RaggedGroup& d = p.g[i];
        d.lo = g.lo; d.N = g.n_units; d.ctr = g.ctr; d.nbr = g.nbr; d.ctr_fb = g.ctr_fb; d.nbr_fb = g.nbr_fb; d.I1 = I1; d.I = I1 + I2;
    }
    return SFSN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// per-clip spike counts (spike_count_rows_kernel with the window cut at the clip's end).  One workgroup per (tensor, clip), the
// only writer of its counter: a plain load + store.  The (frame, vector) pairs of the window are one flat index space, so all 256
// threads have work however few rows a clip has.
// ---------------------------------------------------------------------------------------------------------------------
struct RaggedCountParams {
    const int8_t* src[SFSN_MAX_COUNT_TENSORS];
    unsigned long long* dst[SFSN_MAX_COUNT_TENSORS];
    int R[SFSN_MAX_COUNT_TENSORS], HP[SFSN_MAX_COUNT_TENSORS], rpc[SFSN_MAX_COUNT_TENSORS];
    int n, B, t0, nt;
};

__global__ __launch_bounds__(256) void spike_count_rows_ragged_kernel(const RaggedCountParams p, const int32_t* __restrict__ clip_frames) {
    const int ti = blockIdx.x / p.B, b = blockIdx.x - ti * p.B;
    const int t1 = min(p.t0 + p.nt, max(clip_frames[b], 0));  // (host: t0 + nt <= T of every tensor)
    const size_t nvec = (size_t)p.rpc[ti] * p.HP[ti] / 16;  // 16-byte vectors of one frame of the clip
    const size_t frame = (size_t)p.R[ti] * p.HP[ti];
    const int8_t* base = p.src[ti] + (size_t)b * p.rpc[ti] * p.HP[ti];
    const size_t total = t1 > p.t0 ? (size_t)(t1 - p.t0) * nvec : 0;
    unsigned cnt = 0;
    for (size_t i = threadIdx.x; i < total; i += 256) {
        const size_t dt = i / nvec, k = i - dt * nvec;
        const int4 v = reinterpret_cast<const int4*>(base + ((size_t)p.t0 + dt) * frame)[k];
        cnt += __builtin_popcount((unsigned)v.x) + __builtin_popcount((unsigned)v.y) + __builtin_popcount((unsigned)v.z) +
               __builtin_popcount((unsigned)v.w);
    }
    __shared__ unsigned part[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long* d = p.dst[ti] + b;
        *d = *d + (unsigned long long)(part[0] + part[1] + part[2] + part[3]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// x [B][rows][T][width] float: frames t >= clip_frames[b] := 0.  grid (ceil(rows / 64), B); the tail of a row is contiguous
// ((T - T_b) * width floats), consecutive threads write consecutive floats of it, every element once.
// ---------------------------------------------------------------------------------------------------------------------
#define ZT_ROWS 64
__global__ __launch_bounds__(256) void zero_tail_frames_kernel(float* __restrict__ x, const int32_t* __restrict__ clip_frames, int rows, int T,
                                                                int width) {
    const int b = blockIdx.y, r0 = blockIdx.x * ZT_ROWS;
    const int Tb = clamp_len(clip_frames[b], T);
    const int tail = (T - Tb) * width;  // floats per row (host: T * width < 2^31)
    if (tail == 0) return;
    const int nr = rows - r0 < ZT_ROWS ? rows - r0 : ZT_ROWS;
    const size_t row_len = (size_t)T * width;
    float* base = x + ((size_t)b * rows + r0) * row_len + (size_t)Tb * width;
    for (int r = 0; r < nr; ++r)
        for (int i = threadIdx.x; i < tail; i += 256) base[(size_t)r * row_len + i] = 0.0f;
}

}  // namespace

extern "C" int sfsn_stft_ragged(const float* wave, int B, int L, int n_fft, int hop, const float* window, float* stft_ri, int T,
                                const int32_t* clip_len, void* stream) {
    if (!wave || !window || !stft_ri || !clip_len || B <= 0 || B > 65535 || L <= 0 || hop <= 0 || T <= 0) return SFSN_EINVAL;
    if (n_fft != FFT_NFFT) return SFSN_EUNSUPPORTED;
    if (T != 1 + L / hop || (reinterpret_cast<uintptr_t>(stft_ri) & 7)) return SFSN_EINVAL;
    hipLaunchKernelGGL(stft_ragged_kernel, dim3((T + FFT_TT - 1) / FFT_TT, B), dim3(256), 0, static_cast<hipStream_t>(stream), wave, window,
                       stft_ri, clip_len, B, L, T, hop);
    return hip_ok(hipGetLastError());
}

extern "C" int sfsn_istft_ragged(const float* stft_ri, int B, int T, int n_fft, int hop, const float* window, float* wave, int length,
                                 const int32_t* clip_frames, const int32_t* clip_len, void* stream) {
    if (!wave || !window || !stft_ri || !clip_frames || !clip_len || B <= 0 || B > 65535 || T <= 0 || hop <= 0 || length <= 0)
        return SFSN_EINVAL;
    if (n_fft != FFT_NFFT || FFT_NFFT % hop != 0 || FFT_NFFT / hop > IFFT_HALO + 1) return SFSN_EUNSUPPORTED;
    if (length > (T - 1) * hop + FFT_NFFT / 2 || (reinterpret_cast<uintptr_t>(stft_ri) & 7)) return SFSN_EINVAL;
    const int nblk = (length + FFT_NFFT / 2 + FFT_TT * hop - 1) / (FFT_TT * hop);
    return launch_lds<istft_ragged_kernel>(dim3(nblk, B), dim3(IFFT_WAVES * 64), IFFT_LDS, static_cast<hipStream_t>(stream), stft_ri, window,
                                           wave, clip_frames, clip_len, B, T, hop, length);
}

extern "C" int sfsn_laplace_means_ragged(const float* stft_ri, const float* fb_tbf, int B, int F, int T, int FB, float fdrc,
                                         const sfsn_feature_group* groups, int n_groups, const int32_t* clip_frames, float* mu_out,
                                         float* scratch, void* stream) {
    if (!stft_ri || !mu_out || !scratch || !clip_frames || B > 65535) return SFSN_EINVAL;
    RaggedStatParams p;
    int rc = fill_stat_params(p, groups, n_groups, B, F, T, FB);
    if (rc != SFSN_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rows = B * (F - 1 + FB);
    hipLaunchKernelGGL(rowsum_ragged_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, stft_ri, fb_tbf, scratch, static_cast<double*>(nullptr),
                       clip_frames, B, F, T, FB, fdrc);
    hipLaunchKernelGGL(laplace_mu_ragged_kernel, dim3(n_groups, B), dim3(64), 0, st, scratch, p, clip_frames, mu_out);
    return hip_ok(hipGetLastError());
}

extern "C" int sfsn_gaussian_stats_ragged(const float* stft_ri, const float* fb_tbf, int B, int F, int T, int FB, float fdrc,
                                          const sfsn_feature_group* groups, int n_groups, const int32_t* clip_frames, float* mu_out,
                                          float* sd_out, float* scratch, void* stream) {
    if (!stft_ri || !mu_out || !sd_out || !scratch || !clip_frames || B > 65535 || (reinterpret_cast<uintptr_t>(scratch) & 7u))
        return SFSN_EINVAL;
    if (T < 2) return SFSN_EINVAL;  // (no clip of the batch can have the two frames the unbiased estimate needs)
    RaggedStatParams p;
    int rc = fill_stat_params(p, groups, n_groups, B, F, T, FB);
    if (rc != SFSN_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rows = B * (F - 1 + FB);
    double* rs2 = reinterpret_cast<double*>(scratch + (size_t)((rows + 1) & ~1));
    hipLaunchKernelGGL(rowsum_ragged_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, stft_ri, fb_tbf, scratch, rs2, clip_frames, B, F, T, FB,
                       fdrc);
    hipLaunchKernelGGL(gaussian_stats_ragged_kernel, dim3(n_groups, B), dim3(64), 0, st, rs2, p, clip_frames, mu_out, sd_out);
    return hip_ok(hipGetLastError());
}

extern "C" int sfsn_spike_count_rows_ragged(const sfsn_row_count* tensors, int n_tensors, int t0, int nt, const int32_t* clip_frames, int B,
                                            void* stream) {
    if (!tensors || !clip_frames || n_tensors <= 0 || n_tensors > SFSN_MAX_COUNT_TENSORS || t0 < 0 || nt <= 0 || B <= 0) return SFSN_EINVAL;
    RaggedCountParams p;
    p.n = n_tensors; p.B = B; p.t0 = t0; p.nt = nt;
    for (int i = 0; i < n_tensors; ++i) {
        const sfsn_row_count& t = tensors[i];
        if (!t.spikes_i8 || !t.counts || t.T <= 0 || t.R <= 0 || t.HP <= 0 || t.rows_per_clip <= 0 || (long long)t0 + nt > t.T ||
            t.R != (long long)B * t.rows_per_clip || t.HP % 16 || (reinterpret_cast<uintptr_t>(t.spikes_i8) & 15))
            return SFSN_EINVAL;
        p.src[i] = t.spikes_i8; p.dst[i] = t.counts; p.R[i] = t.R; p.HP[i] = t.HP; p.rpc[i] = t.rows_per_clip;
    }
    if ((long long)B * n_tensors > 0x7fffffffLL) return SFSN_EUNSUPPORTED;
    hipLaunchKernelGGL(spike_count_rows_ragged_kernel, dim3((unsigned)(B * n_tensors)), dim3(256), 0, static_cast<hipStream_t>(stream), p,
                       clip_frames);
    return hip_ok(hipGetLastError());
}

extern "C" int sfsn_zero_tail_frames(float* x, int B, int rows, int T, int width, const int32_t* clip_frames, void* stream) {
    if (!x || !clip_frames || B <= 0 || B > 65535 || rows <= 0 || T <= 0 || width <= 0) return SFSN_EINVAL;
    if ((long long)T * width > 0x7fffffffLL) return SFSN_EUNSUPPORTED;
    hipLaunchKernelGGL(zero_tail_frames_kernel, dim3((unsigned)((rows + ZT_ROWS - 1) / ZT_ROWS), B), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, clip_frames, rows, T, width);
    return hip_ok(hipGetLastError());
}
