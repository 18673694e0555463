// sfsn_loss.hip -- the intel_ndns recipe's training loss (audiozen/loss.py: freq_MAE + mag_MAE + SISNRLoss) and its gradient with
// respect to the estimate, in two launches.  gfx950 only.
//
//   launch 1 (loss_frames_kernel): frame workgroups take LOSS_FPW consecutive (row, frame) pairs each: load both windowed frames
//     with the reflect padding folded into the index, one 2048-point complex transform of z = e w + i t w, the conjugate-symmetry
//     split into E and T, the three L1 sums of the frame (one fp32 partial per frame in scratch), the cotangent G written over
//     the spectrum, the inverse transform and the windowed frame gradient into the [rows][T'][2048] scratch.  Behind them, row-sum
//     workgroups accumulate the five SI-SNR sums of LOSS_CHUNK samples in fp64 (one partial per chunk in scratch).
//   launch 2 (loss_finish_kernel): gather workgroups sum, for each output sample, the frames that cover it and the two reflected
//     margins that mirror onto it, in a fixed order, and add the pointwise SI-SNR term; one last workgroup reduces the partials in
//     a fixed order (fp64) into the four loss values.
//
// No atomics, no waits between workgroups, no host synchronisation: a call is two plain launches on the caller's stream.
//
// sfsn_recipe_loss_ragged (loss_frames_ragged_kernel, loss_finish_ragged_kernel) is the same pair of launches for rows of different
// lengths in one padded batch, with the REVERB recipe's time-domain L1 as a fourth term.  Both grids are sized on the padded row; a
// workgroup reads its row's length from the device, clamps it into the row and leaves when its frame, chunk or sample does not
// exist.  A row's frames, chunk sums and gathered samples are computed by the device functions the equal-length kernels call, in the
// same order, so a row has the bits of the equal-length call on that row alone.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "sfsn.h"
#include "sfsn_host.h"

#define LOSS_NFFT 2048
#define LOSS_HOP 512
#define LOSS_PAD 1024
#define LOSS_BINS 1025
#define LOSS_THREADS 256
#define LOSS_FPW 4       // (row, frame) pairs per frame workgroup: the unit table is filled once for all of them
#define LOSS_CHUNK 8192  // samples per row-sum workgroup
#define LOSS_SPW 1024    // output samples per gather workgroup

namespace {

__device__ __forceinline__ float2 lcmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

template <bool INV>
__device__ __forceinline__ float2 lunit(const float2* unit, int m) {
    const float2 u = unit[m & (LOSS_NFFT - 1)];
    return INV ? make_float2(u.x, -u.y) : u;
}

template <bool INV>
__device__ __forceinline__ void lfft4(float2 (&v)[4]) {
    const float2 a = make_float2(v[0].x + v[2].x, v[0].y + v[2].y), b = make_float2(v[0].x - v[2].x, v[0].y - v[2].y);
    const float2 c = make_float2(v[1].x + v[3].x, v[1].y + v[3].y), d = make_float2(v[1].x - v[3].x, v[1].y - v[3].y);
    v[0] = make_float2(a.x + c.x, a.y + c.y);
    v[2] = make_float2(a.x - c.x, a.y - c.y);
    const float2 p = make_float2(b.x + d.y, b.y - d.x), m = make_float2(b.x - d.y, b.y + d.x);  // b - i d, b + i d
    v[1] = INV ? m : p;
    v[3] = INV ? p : m;
}

// In-place 2048-point complex transform of buf (natural order in, natural order out, unnormalised) by one workgroup of 256 threads:
// five radix-4 Stockham passes (Ns = 1, 4, 16, 64, 256; 512 butterflies, two per thread, through registers) and one radix-2 pass
// (Ns = 1024; its outputs land on its own inputs).  unit[m] = exp(-2 pi i m / 2048).  Ends with a barrier.
template <bool INV>
__device__ __forceinline__ void fft2048(float2* buf, const float2* unit, int tid) {
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const int ns = 1 << (2 * s);
        float2 v[2][4];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int j = tid + LOSS_THREADS * b, k = j & (ns - 1);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[b][r] = buf[j + 512 * r];
            if (s > 0) {
#pragma unroll
                for (int r = 1; r < 4; ++r) v[b][r] = lcmul(v[b][r], lunit<INV>(unit, k * r * (512 / ns)));  // 2 pi k r / (4 Ns)
            }
            lfft4<INV>(v[b]);
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int j = tid + LOSS_THREADS * b, k = j & (ns - 1), j0 = (j - k) * 4 + k;
#pragma unroll
            for (int r = 0; r < 4; ++r) buf[j0 + r * ns] = v[b][r];
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = tid + LOSS_THREADS * q;
        const float2 a = buf[j], b = lcmul(buf[j + 1024], lunit<INV>(unit, j));
        buf[j] = make_float2(a.x + b.x, a.y + b.y);
        buf[j + 1024] = make_float2(a.x - b.x, a.y - b.y);
    }
    __syncthreads();
}

__device__ __forceinline__ float sgnf(float x) { return (float)((x > 0.0f) - (x < 0.0f)); }

// Sum over the workgroup in a fixed order (lanes by halving shuffles, then the four waves in order); the result is valid in thread 0.
template <class T>
__device__ __forceinline__ T block_sum(T v, T* red /* [4] */, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    const T r = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return r;
}

// One bin of the split: E and T from Z[k] and Z[N-k], the three L1 terms into acc, the cotangent returned.
__device__ __forceinline__ float2 split_bin(float2 zk, float2 zm, float cf, float cm, float (&acc)[3]) {
    const float2 E = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
    const float2 T = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
    const float dre = E.x - T.x, dim = E.y - T.y;
    const float ae = sqrtf(E.x * E.x + E.y * E.y), at = sqrtf(T.x * T.x + T.y * T.y);
    const float dm = ae - at;
    acc[0] += fabsf(dre);
    acc[1] += fabsf(dim);
    acc[2] += fabsf(dm);
    const float sm = cm * sgnf(dm);
    const float ux = ae > 0.0f ? E.x / ae : 0.0f, uy = ae > 0.0f ? E.y / ae : 0.0f;
    return make_float2(cf * sgnf(dre) + sm * ux, cf * sgnf(dim) + sm * uy);
}

// unit[m] = exp(-2 pi i m / 2048), filled by the whole workgroup.  Ends with a barrier.
__device__ __forceinline__ void fill_unit(float2* unit, int tid) {
    for (int m = tid; m < LOSS_NFFT; m += LOSS_THREADS) {
        float sn, cs;
        sincospif((float)m / 1024.0f, &sn, &cs);
        unit[m] = make_float2(cs, -sn);
    }
    __syncthreads();
}

// The sums of samples [lo, min(L, lo + LOSS_CHUNK)) of one row in fp64: the five SI-SNR sums and, with NS == 6, sum |e - t| (the
// difference of two fp32 values is exact in fp64).  out[NS] is written by thread 0.
template <int NS>
__device__ __forceinline__ void chunk_sums(const float* __restrict__ e, const float* __restrict__ t, int lo, int L, double* __restrict__ out,
                                           double* red, int tid) {
    const int hi = min(L, lo + LOSS_CHUNK);
    double s[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) s[i] = 0.0;
    for (int n = lo + tid; n < hi; n += LOSS_THREADS) {
        const double a = e[n], b = t[n];
        s[0] += a; s[1] += b; s[2] += a * a; s[3] += b * b; s[4] += a * b;
        if (NS == 6) s[NS - 1] += fabs(a - b);
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const double r = block_sum<double>(s[i], red, tid);
        if (tid == 0) out[i] = r;
    }
}

// Frame f of one row of L samples (e, t: the row's first samples): the three L1 sums into partial[0..2] and, with want_grad, the
// windowed frame gradient into g[2048].  Every thread of the workgroup takes part.
__device__ __forceinline__ void frame_pass(const float* __restrict__ e, const float* __restrict__ t, int L, int f, float cf, float cm,
                                           int want_grad, float* __restrict__ partial, float* __restrict__ g, float2* buf, const float2* unit,
                                           float* fred, int tid) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int n = tid + LOSS_THREADS * q;
        int p = f * LOSS_HOP - LOSS_PAD + n;  // -1024 <= p <= L + 1023 and L >= 1025: one reflection lands inside
        p = p < 0 ? -p : (p > L - 1 ? 2 * (L - 1) - p : p);
        const float w = 0.5f - 0.5f * unit[n].x;  // periodic Hann
        buf[n] = make_float2(e[p] * w, t[p] * w);
    }
    __syncthreads();
    fft2048<false>(buf, unit, tid);
    // thread tid owns bins k = tid + 256 j and their mirrors 2048 - k (thread 0 also bin 1024): it reads both and writes both
    float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = tid + LOSS_THREADS * j, km = (LOSS_NFFT - k) & (LOSS_NFFT - 1);
        const float2 G = split_bin(buf[k], buf[km], cf, cm, acc);
        if (k) buf[km] = make_float2(0.0f, 0.0f);
        buf[k] = G;
    }
    if (tid == 0) buf[1024] = split_bin(buf[1024], buf[1024], cf, cm, acc);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float r = block_sum<float>(acc[i], fred, tid);
        if (tid == 0) partial[i] = r;
    }
    if (want_grad) {  // (block_sum ended with a barrier: G is complete)
        fft2048<true>(buf, unit, tid);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int n = tid + LOSS_THREADS * q;
            g[n] = buf[n].x * (0.5f - 0.5f * unit[n].x);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(LOSS_THREADS) void loss_frames_kernel(const float* __restrict__ est, const float* __restrict__ tgt, int L, int T,
                                                                   int n_frames, int n_frame_wgs, float cf, float cm, int want_grad,
                                                                   float* __restrict__ partial /* [n_frames][4] */,
                                                                   float* __restrict__ fgrad /* [n_frames][2048] */, int n_chunks,
                                                                   double* __restrict__ rowpart /* [rows][n_chunks][5] */) {
    __shared__ float2 unit[LOSS_NFFT];
    __shared__ float2 buf[LOSS_NFFT];
    __shared__ double red[4];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= n_frame_wgs) {  // the five SI-SNR sums of one chunk of one row, in fp64
        const int idx = blockIdx.x - n_frame_wgs, row = idx / n_chunks, chunk = idx - row * n_chunks;
        chunk_sums<5>(est + (size_t)row * L, tgt + (size_t)row * L, chunk * LOSS_CHUNK, L, rowpart + (size_t)idx * 5, red, tid);
        return;
    }
    fill_unit(unit, tid);
    float* fred = reinterpret_cast<float*>(red);
    for (int fi = 0; fi < LOSS_FPW; ++fi) {
        const int frame = blockIdx.x * LOSS_FPW + fi;
        if (frame >= n_frames) break;  // (the same for every thread)
        const int row = frame / T, f = frame - row * T;
        frame_pass(est + (size_t)row * L, tgt + (size_t)row * L, L, f, cf, cm, want_grad, partial + (size_t)frame * 4,
                   fgrad + (size_t)frame * LOSS_NFFT, buf, unit, fred, tid);
    }
}

struct RowStats {
    double me, mt, alpha, ratio, coef;  // grad_sdr[q] = coef * (alpha b - ratio (a - alpha b)),  a = e - me, b = t - mt
    double value;                       // 10 log10(ratio + eps)
};

// The SI-SNR quantities of one row of L samples from its n_chunks chunk partials (NS doubles each, the row's first at index `first`),
// combined in chunk order (fp64).
template <int NS>
__device__ __forceinline__ RowStats row_stats(const double* __restrict__ rowpart, size_t first, int n_chunks, int L) {
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < n_chunks; ++c)
#pragma unroll
        for (int i = 0; i < 5; ++i) s[i] += rowpart[(first + c) * NS + i];
    const double eps = 1.1920928955078125e-07;  // 2^-23 (torch.finfo(torch.float32).eps)
    RowStats r;
    r.me = s[0] / L;
    r.mt = s[1] / L;
    const double en = s[2] - s[0] * r.me, tn = s[3] - s[1] * r.mt, dot = s[4] - s[0] * r.mt;
    r.alpha = dot / tn;
    const double P = r.alpha * dot, Nn = en - P;
    r.ratio = P / (Nn + eps);
    r.value = 10.0 * log10(r.ratio + eps);
    r.coef = (10.0 / 2.302585092994046) / (r.ratio + eps) * 2.0 / (Nn + eps);
    return r;
}

// The spectral part of d total / d est at sample q of a row of L samples and T frames: the frames that cover q and the two reflected
// margins that mirror onto it, in a fixed order.  fg: the row's frame gradients [T][2048].
__device__ __forceinline__ float gather_spec(const float* __restrict__ fg, int q, int L, int T) {
    float g = 0.0f;
    // padded positions that read sample q: q + 1024 itself, 1024 - q (left margin, 1 <= q <= 1024) and
    // 2 (L - 1) - q + 1024 (right margin, L - 1025 <= q <= L - 2); frames of each in ascending order
    int P[3] = {q + LOSS_PAD, (q >= 1 && q <= LOSS_PAD) ? LOSS_PAD - q : -1,
                (q >= L - 1 - LOSS_PAD && q <= L - 2) ? 2 * (L - 1) - q + LOSS_PAD : -1};
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        if (P[m] < 0) continue;
        const int f1 = min(T - 1, P[m] / LOSS_HOP);
        for (int f = max(0, (P[m] - LOSS_NFFT + LOSS_HOP) / LOSS_HOP); f <= f1; ++f) g += fg[(size_t)f * LOSS_NFFT + (P[m] - f * LOSS_HOP)];
    }
    return g;
}

// The SI-SNR part at a sample with values e, t of a row with statistics rs; cs = c_sdr / rows.
__device__ __forceinline__ float sdr_grad(const RowStats& rs, double cs, float e, float t) {
    const double a = (double)e - rs.me, b = (double)t - rs.mt;
    const double pb = rs.alpha * b;
    return (float)(cs * rs.coef * (pb - rs.ratio * (a - pb)));
}

__global__ __launch_bounds__(LOSS_THREADS) void loss_finish_kernel(const float* __restrict__ est, const float* __restrict__ tgt, int rows, int L,
                                                                   int T, int n_frames, int n_gather_wgs, int wgs_per_row,
                                                                   const float* __restrict__ partial, const float* __restrict__ fgrad,
                                                                   int n_chunks, const double* __restrict__ rowpart, float c_freq, float c_mag,
                                                                   float c_sdr, int flags, float* __restrict__ terms, float* __restrict__ grad) {
    __shared__ double red[4];
    __shared__ RowStats rs;
    const int tid = threadIdx.x;
    const bool spec = (flags & 3) != 0, sdr = (flags & 4) != 0;
    if ((int)blockIdx.x < n_gather_wgs) {
        const int row = blockIdx.x / wgs_per_row, base = (blockIdx.x - row * wgs_per_row) * LOSS_SPW;
        if (sdr) {
            if (tid == 0) rs = row_stats<5>(rowpart, (size_t)row * n_chunks, n_chunks, L);
            __syncthreads();
        }
        const float* fg = fgrad + (size_t)row * T * LOSS_NFFT;
        const double cs = (double)c_sdr / rows;
#pragma unroll
        for (int i = 0; i < LOSS_SPW / LOSS_THREADS; ++i) {
            const int q = base + tid + LOSS_THREADS * i;
            if (q >= L) break;
            float g = 0.0f;
            if (spec) g = gather_spec(fg, q, L, T);
            if (sdr) g += sdr_grad(rs, cs, est[(size_t)row * L + q], tgt[(size_t)row * L + q]);
            grad[(size_t)row * L + q] = g;
        }
        return;
    }
    // the last workgroup: the four loss values
    double s[3] = {0.0, 0.0, 0.0};
    if (spec)
        for (int f = tid; f < n_frames; f += LOSS_THREADS)
#pragma unroll
            for (int i = 0; i < 3; ++i) s[i] += (double)partial[(size_t)f * 4 + i];
    double v = 0.0;
    if (sdr)
        for (int r = tid; r < rows; r += LOSS_THREADS) v += row_stats<5>(rowpart, (size_t)r * n_chunks, n_chunks, L).value;
    const double s_re = block_sum<double>(s[0], red, tid), s_im = block_sum<double>(s[1], red, tid);
    const double s_mag = block_sum<double>(s[2], red, tid), s_val = block_sum<double>(v, red, tid);
    if (tid == 0) {
        const double N = (double)rows * LOSS_BINS * T;
        const float freq = (flags & 1) ? (float)((s_re + s_im) / N) : 0.0f;
        const float mag = (flags & 2) ? (float)(s_mag / N) : 0.0f;
        const float sisnr = sdr ? (float)(s_val / rows) : 0.0f;
        terms[0] = freq;
        terms[1] = mag;
        terms[2] = sisnr;
        terms[3] = (c_freq * freq + c_mag * mag) + c_sdr * sisnr;
    }
}

// Row r of a ragged batch has row_len[r] samples (NULL: all n_samples), clamped into [1025, n_samples] before anything is indexed.
__device__ __forceinline__ int row_length(const int* __restrict__ row_len, int row, int n_samples) {
    return row_len ? min(max(row_len[row], LOSS_PAD + 1), n_samples) : n_samples;
}

// loss_frames_kernel for rows of their own lengths: Ls is the row stride, T the frame count of the padded row (the frame grid and the
// partial / fgrad slots are laid out on it), n_chunks the chunk count of the padded row.  cf, cm of a row: c / (rows 1025 T_r).
__global__ __launch_bounds__(LOSS_THREADS) void loss_frames_ragged_kernel(const float* __restrict__ est, const float* __restrict__ tgt, int rows,
                                                                          int Ls, const int* __restrict__ row_len, int T, int n_frames,
                                                                          int n_frame_wgs, float c_freq, float c_mag, int flags, int want_grad,
                                                                          float* __restrict__ partial /* [rows][T][4] */,
                                                                          float* __restrict__ fgrad /* [rows][T][2048] */, int n_chunks,
                                                                          double* __restrict__ rowpart /* [rows][n_chunks][6] */) {
    __shared__ float2 unit[LOSS_NFFT];
    __shared__ float2 buf[LOSS_NFFT];
    __shared__ double red[4];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= n_frame_wgs) {  // the six sums of one chunk of one row; a chunk past the row's end does nothing
        const int idx = blockIdx.x - n_frame_wgs, row = idx / n_chunks, chunk = idx - row * n_chunks;
        const int L = row_length(row_len, row, Ls);
        if (chunk * LOSS_CHUNK >= L) return;
        chunk_sums<6>(est + (size_t)row * Ls, tgt + (size_t)row * Ls, chunk * LOSS_CHUNK, L, rowpart + (size_t)idx * 6, red, tid);
        return;
    }
    float* fred = reinterpret_cast<float*>(red);
    bool filled = false;
    for (int fi = 0; fi < LOSS_FPW; ++fi) {
        const int frame = blockIdx.x * LOSS_FPW + fi;
        if (frame >= n_frames) break;  // (the same for every thread, like every branch below)
        const int row = frame / T, f = frame - row * T;
        const int L = row_length(row_len, row, Ls), Tr = 1 + L / LOSS_HOP;
        if (f >= Tr) continue;  // the row has no such frame: its slot is never read
        if (!filled) {
            fill_unit(unit, tid);
            filled = true;
        }
        const double N = (double)rows * (double)(LOSS_BINS * Tr);
        const float cf = (flags & SFSN_LOSS_FREQ) ? (float)((double)c_freq / N) : 0.0f;
        const float cm = (flags & SFSN_LOSS_MAG) ? (float)((double)c_mag / N) : 0.0f;
        frame_pass(est + (size_t)row * Ls, tgt + (size_t)row * Ls, L, f, cf, cm, want_grad, partial + (size_t)frame * 4,
                   fgrad + (size_t)frame * LOSS_NFFT, buf, unit, fred, tid);
    }
}

// loss_finish_kernel for rows of their own lengths.  Gather workgroups: as there, on the row's own L_r and T_r, then the time term
// c_time sgn(e - t) / (rows L_r); samples in [L_r, Ls) are written as 0.  The last workgroup: every row's four terms (each as the
// equal-length kernel reduces a one-row call: frames strided by thread, block_sum, fp64), then their means in row order (fp64).
__global__ __launch_bounds__(LOSS_THREADS) void loss_finish_ragged_kernel(const float* __restrict__ est, const float* __restrict__ tgt, int rows,
                                                                          int Ls, const int* __restrict__ row_len, int T, int n_gather_wgs,
                                                                          int wgs_per_row, const float* __restrict__ partial,
                                                                          const float* __restrict__ fgrad, int n_chunks,
                                                                          const double* __restrict__ rowpart, float c_freq, float c_mag,
                                                                          float c_sdr, float c_time, int flags, float* __restrict__ terms,
                                                                          float* __restrict__ row_terms, float* __restrict__ rt /* [rows][4] */,
                                                                          float* __restrict__ grad) {
    __shared__ double red[4];
    __shared__ RowStats rs;
    const int tid = threadIdx.x;
    const bool spec = (flags & 3) != 0, sdr = (flags & SFSN_LOSS_SDR) != 0, tim = (flags & SFSN_LOSS_TIME) != 0;
    if ((int)blockIdx.x < n_gather_wgs) {
        const int row = blockIdx.x / wgs_per_row, base = (blockIdx.x - row * wgs_per_row) * LOSS_SPW;
        const int L = row_length(row_len, row, Ls), Tr = 1 + L / LOSS_HOP;
        if (sdr && base < L) {
            if (tid == 0) rs = row_stats<6>(rowpart, (size_t)row * n_chunks, (L + LOSS_CHUNK - 1) / LOSS_CHUNK, L);
            __syncthreads();
        }
        const float* fg = fgrad + (size_t)row * T * LOSS_NFFT;
        const double cs = (double)c_sdr / rows, ct = (double)c_time / ((double)rows * L);
#pragma unroll
        for (int i = 0; i < LOSS_SPW / LOSS_THREADS; ++i) {
            const int q = base + tid + LOSS_THREADS * i;
            if (q >= Ls) break;
            float g = 0.0f;
            if (q < L) {
                const float e = est[(size_t)row * Ls + q], t = tgt[(size_t)row * Ls + q];
                if (spec) g = gather_spec(fg, q, L, Tr);
                if (sdr) g += sdr_grad(rs, cs, e, t);
                if (tim) g += (float)(ct * (double)((e > t) - (e < t)));
            }
            grad[(size_t)row * Ls + q] = g;
        }
        return;
    }
    // the last workgroup.  Pointwise terms: one thread per row
    for (int r = tid; r < rows; r += LOSS_THREADS) {
        const int L = row_length(row_len, r, Ls), nc = (L + LOSS_CHUNK - 1) / LOSS_CHUNK;
        double sabs = 0.0;
        if (tim)
            for (int c = 0; c < nc; ++c) sabs += rowpart[((size_t)r * n_chunks + c) * 6 + 5];
        rt[(size_t)r * 4 + 2] = sdr ? (float)row_stats<6>(rowpart, (size_t)r * n_chunks, nc, L).value : 0.0f;
        rt[(size_t)r * 4 + 3] = tim ? (float)(sabs / L) : 0.0f;
    }
    // spectral terms: the workgroup per row
    for (int r = 0; r < rows; ++r) {
        const int Tr = 1 + row_length(row_len, r, Ls) / LOSS_HOP;
        double s[3] = {0.0, 0.0, 0.0};
        if (spec)
            for (int f = tid; f < Tr; f += LOSS_THREADS)
#pragma unroll
                for (int i = 0; i < 3; ++i) s[i] += (double)partial[((size_t)r * T + f) * 4 + i];
        double s_re = 0.0, s_im = 0.0, s_mag = 0.0;
        if (spec) {
            s_re = block_sum<double>(s[0], red, tid);
            s_im = block_sum<double>(s[1], red, tid);
            s_mag = block_sum<double>(s[2], red, tid);
        }
        if (tid == 0) {
            const double N = (double)LOSS_BINS * Tr;
            rt[(size_t)r * 4 + 0] = (flags & SFSN_LOSS_FREQ) ? (float)((s_re + s_im) / N) : 0.0f;
            rt[(size_t)r * 4 + 1] = (flags & SFSN_LOSS_MAG) ? (float)(s_mag / N) : 0.0f;
        }
    }
    __syncthreads();  // rt is complete, and visible to the whole workgroup
    if (row_terms)
        for (int i = tid; i < rows * 4; i += LOSS_THREADS) row_terms[i] = rt[i];
    if (tid == 0) {  // every row weighs the same: the mean of the fp32 row terms, in row order
        double m[4] = {0.0, 0.0, 0.0, 0.0};
        for (int r = 0; r < rows; ++r)
#pragma unroll
            for (int i = 0; i < 4; ++i) m[i] += (double)rt[(size_t)r * 4 + i];
        const float freq = (float)(m[0] / rows), mag = (float)(m[1] / rows), sisnr = (float)(m[2] / rows), time = (float)(m[3] / rows);
        terms[0] = freq;
        terms[1] = mag;
        terms[2] = sisnr;
        terms[3] = time;
        terms[4] = ((c_freq * freq + c_mag * mag) + c_sdr * sisnr) + c_time * time;
    }
}

struct LossLayout {
    size_t partial, rowpart, rowterm, fgrad, total;
    int T, n_frames, n_chunks;
};

// SFSN_OK and the scratch layout, or the status the entry points answer with (host only).  sums_per_chunk: 5, or 6 for the ragged
// entry, whose [rows][4] row terms sit in front of its frame gradients.
int loss_layout(int rows, int n_samples, int sums_per_chunk, LossLayout* out) {
    if (rows < 1 || n_samples <= LOSS_PAD) return SFSN_EINVAL;  // reflect padding of 1024 needs more than 1024 samples (torch.stft raises)
    const long long T = 1 + n_samples / LOSS_HOP, n_frames = (long long)rows * T;
    const long long n_chunks = (n_samples + LOSS_CHUNK - 1) / LOSS_CHUNK;
    if ((long long)rows * n_samples > INT_MAX || n_frames * LOSS_NFFT > INT_MAX || (long long)n_samples + 2 * LOSS_NFFT > INT_MAX / 2)
        return SFSN_EUNSUPPORTED;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    out->T = (int)T;
    out->n_frames = (int)n_frames;
    out->n_chunks = (int)n_chunks;
    out->partial = 0;
    out->rowpart = up((size_t)n_frames * 4 * sizeof(float));
    out->rowterm = out->rowpart + up((size_t)rows * n_chunks * sums_per_chunk * sizeof(double));
    out->fgrad = out->rowterm + (sums_per_chunk == 6 ? up((size_t)rows * 4 * sizeof(float)) : 0);
    out->total = out->fgrad + up((size_t)n_frames * LOSS_NFFT * sizeof(float));
    return SFSN_OK;
}

}  // namespace

extern "C" size_t sfsn_recipe_loss_scratch_bytes(int rows, int n_samples) {
    LossLayout lay;
    return loss_layout(rows, n_samples, 5, &lay) == SFSN_OK ? lay.total : 0;
}

extern "C" int sfsn_recipe_loss(const float* est, const float* tgt, int rows, int n_samples, float c_freq, float c_mag, float c_sdr, int flags,
                                float* terms, float* grad_est, void* scratch, void* stream) {
    if (!est || !tgt || !terms || !scratch || !aligned16(est) || !aligned16(tgt) || !aligned16(terms) || !aligned16(grad_est) ||
        !aligned16(scratch))
        return SFSN_EINVAL;
    if (flags < 1 || flags > 7) return SFSN_EINVAL;
    LossLayout lay;
    const int rc = loss_layout(rows, n_samples, 5, &lay);
    if (rc != SFSN_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(scratch);
    float* partial = reinterpret_cast<float*>(base + lay.partial);
    double* rowpart = reinterpret_cast<double*>(base + lay.rowpart);
    float* fgrad = reinterpret_cast<float*>(base + lay.fgrad);
    const bool spec = (flags & 3) != 0, sdr = (flags & 4) != 0;
    const double N = (double)rows * LOSS_BINS * lay.T;
    const float cf = (flags & 1) ? (float)((double)c_freq / N) : 0.0f, cm = (flags & 2) ? (float)((double)c_mag / N) : 0.0f;
    const int n_frame_wgs = spec ? (lay.n_frames + LOSS_FPW - 1) / LOSS_FPW : 0;
    const int n_sum_wgs = sdr ? rows * lay.n_chunks : 0;
    hipLaunchKernelGGL(loss_frames_kernel, dim3(n_frame_wgs + n_sum_wgs), dim3(LOSS_THREADS), 0, st, est, tgt, n_samples, lay.T, lay.n_frames,
                       n_frame_wgs, cf, cm, grad_est ? 1 : 0, partial, fgrad, lay.n_chunks, rowpart);
    if (hipGetLastError() != hipSuccess) return SFSN_EHIP;
    const int wgs_per_row = (n_samples + LOSS_SPW - 1) / LOSS_SPW;
    const int n_gather_wgs = grad_est ? rows * wgs_per_row : 0;
    hipLaunchKernelGGL(loss_finish_kernel, dim3(n_gather_wgs + 1), dim3(LOSS_THREADS), 0, st, est, tgt, rows, n_samples, lay.T, lay.n_frames,
                       n_gather_wgs, wgs_per_row, partial, fgrad, lay.n_chunks, rowpart, (flags & 1) ? c_freq : 0.0f,
                       (flags & 2) ? c_mag : 0.0f, sdr ? c_sdr : 0.0f, flags, terms, grad_est);
    return hip_ok(hipGetLastError());
}

extern "C" size_t sfsn_recipe_loss_ragged_scratch_bytes(int rows, int n_samples) {
    LossLayout lay;
    return loss_layout(rows, n_samples, 6, &lay) == SFSN_OK ? lay.total : 0;
}

extern "C" int sfsn_recipe_loss_ragged(const float* est, const float* tgt, int rows, int n_samples, const int32_t* row_len, float c_freq,
                                       float c_mag, float c_sdr, float c_time, int flags, float* terms, float* row_terms, float* grad_est,
                                       void* scratch, void* stream) {
    if (!est || !tgt || !terms || !scratch || !aligned16(est) || !aligned16(tgt) || !aligned16(row_len) || !aligned16(terms) ||
        !aligned16(row_terms) || !aligned16(grad_est) || !aligned16(scratch))
        return SFSN_EINVAL;
    if (flags < 1 || flags > 15) return SFSN_EINVAL;
    LossLayout lay;
    const int rc = loss_layout(rows, n_samples, 6, &lay);
    if (rc != SFSN_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(scratch);
    float* partial = reinterpret_cast<float*>(base + lay.partial);
    double* rowpart = reinterpret_cast<double*>(base + lay.rowpart);
    float* rowterm = reinterpret_cast<float*>(base + lay.rowterm);
    float* fgrad = reinterpret_cast<float*>(base + lay.fgrad);
    const bool spec = (flags & 3) != 0, point = (flags & (SFSN_LOSS_SDR | SFSN_LOSS_TIME)) != 0;
    const int n_frame_wgs = spec ? (lay.n_frames + LOSS_FPW - 1) / LOSS_FPW : 0;
    const int n_sum_wgs = point ? rows * lay.n_chunks : 0;
    hipLaunchKernelGGL(loss_frames_ragged_kernel, dim3(n_frame_wgs + n_sum_wgs), dim3(LOSS_THREADS), 0, st, est, tgt, rows, n_samples, row_len,
                       lay.T, lay.n_frames, n_frame_wgs, c_freq, c_mag, flags, grad_est ? 1 : 0, partial, fgrad, lay.n_chunks, rowpart);
    if (hipGetLastError() != hipSuccess) return SFSN_EHIP;
    const int wgs_per_row = (n_samples + LOSS_SPW - 1) / LOSS_SPW;
    const int n_gather_wgs = grad_est ? rows * wgs_per_row : 0;
    hipLaunchKernelGGL(loss_finish_ragged_kernel, dim3(n_gather_wgs + 1), dim3(LOSS_THREADS), 0, st, est, tgt, rows, n_samples, row_len, lay.T,
                       n_gather_wgs, wgs_per_row, partial, fgrad, lay.n_chunks, rowpart, (flags & SFSN_LOSS_FREQ) ? c_freq : 0.0f,
                       (flags & SFSN_LOSS_MAG) ? c_mag : 0.0f, (flags & SFSN_LOSS_SDR) ? c_sdr : 0.0f,
                       (flags & SFSN_LOSS_TIME) ? c_time : 0.0f, flags, terms, row_terms, rowterm, grad_est);
    return hip_ok(hipGetLastError());
}
