// sfsn_pit.hip -- the wsj0-mix recipes' training loss (audiozen/pit.py: PITWrapper(PairwiseNegSDR())): the pairwise negative SI-SDR of
// every (estimate, reference) pair of a clip, the best permutation, the mean loss, the reordered estimates and the gradient with
// respect to the estimates, in two launches.  gfx950 only.
//
//   launch 1 (pit_sums_kernel): one workgroup per (clip, chunk of PIT_CHUNK samples) reads the clip's S estimate and S reference
//     chunks once and accumulates the S^2 + 4S raw sums (sum a, sum r, sum a^2, sum r^2, sum a r) in fp64: per thread in sample order,
//     lanes by halving shuffles, the four waves in order; one partial per chunk in scratch.
//   launch 2 (pit_finish_kernel): every (clip, chunk) workgroup adds its clip's partials in chunk order, forms `pair` from the sums
//     (|noise|^2 = |a|^2 - 2 alpha <a, r> + alpha^2 |r|^2, all in fp64), searches the at most 24 permutations, derives per estimate
//     row the fp32 coefficients of  grad = A est + sum_j R_j ref_j + C  and writes its chunk of grad_est and of reordered.  One further
//     workgroup does the same sums and the same search for every clip and writes pair, perm and loss.  Every workgroup runs the same
//     instructions on the same partials, so the redundant searches agree bit for bit.
//
// No atomics, no waits between workgroups, no host synchronisation: a call is two plain launches on the caller's stream.
//
// sfsn_pit_sdr_ragged is the same call on a padded batch whose clips have their own lengths (pit_sums_ragged_kernel,
// pit_finish_ragged_kernel, further down): every clip as if it ran alone, plus the clips' own minima and audiozen.metric.SISDR of the
// matched rows, which is a function of the same sums.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "sfsn.h"
#include "sfsn_host.h"

#define PIT_THREADS 256
#define PIT_CHUNK 2048  // samples per workgroup (a multiple of 4 PIT_THREADS / 2: two vector passes)
#define PIT_MAX_S 4
#define PIT_BATCH 16  // clips the last workgroup solves side by side

namespace {

// Rows start at 4 L-byte offsets, so with L % 4 != 0 every row after the first is not 16-byte aligned.  A thread's four samples start at
// a multiple of four within the row, so a row is either aligned at every thread's position (one dwordx4 access) or at none (four dword
// accesses, which the wave's neighbouring lanes still complete to whole cache lines); the choice is the same for the whole workgroup.
__device__ __forceinline__ bool quad_aligned(const float* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Samples o .. o + 3 of a row's chunk of `len` samples; positions from `len` on read as zero (they add nothing to any sum).
__device__ __forceinline__ void load4(const float* __restrict__ row, int o, int len, float (&v)[4]) {
    if (o + 4 <= len && quad_aligned(row + o)) {
        const float4 q = *reinterpret_cast<const float4*>(row + o);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = o + k < len ? row[o + k] : 0.0f;
    }
}

__device__ __forceinline__ void store4(float* __restrict__ row, int o, int len, const float (&v)[4]) {
    if (o + 4 <= len && quad_aligned(row + o)) {
        *reinterpret_cast<float4*>(row + o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (o + k < len) row[o + k] = v[k];
    }
}

// Layout of the S^2 + 4S sums of a clip: sum a_i | sum r_j | sum a_i^2 | sum r_j^2 | sum a_i r_j ([i][j]).
template <int S>
__global__ __launch_bounds__(PIT_THREADS) void pit_sums_kernel(const float* __restrict__ est, const float* __restrict__ ref, int L, int n_chunks,
                                                               double* __restrict__ partial /* [clips][n_chunks][NS] */) {
    constexpr int NS = S * S + 4 * S;
    __shared__ double red[4][NS];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / n_chunks, chunk = blockIdx.x - b * n_chunks;
    const int lo = chunk * PIT_CHUNK, len = min(PIT_CHUNK, L - lo);  // (offsets within the chunk: lo + PIT_CHUNK may pass 2^31)
    const float* e = est + (size_t)b * S * L + lo;
    const float* r = ref + (size_t)b * S * L + lo;
    double s[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) s[i] = 0.0;
    for (int o = 4 * tid; o < len; o += 4 * PIT_THREADS) {
        float a[S][4], t[S][4];
#pragma unroll
        for (int i = 0; i < S; ++i) {
            load4(e + (size_t)i * L, o, len, a[i]);
            load4(r + (size_t)i * L, o, len, t[i]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int i = 0; i < S; ++i) {
                const double x = a[i][k], y = t[i][k];
                s[i] += x;
                s[S + i] += y;
                s[2 * S + i] += x * x;
                s[3 * S + i] += y * y;
#pragma unroll
                for (int j = 0; j < S; ++j) s[4 * S + i * S + j] += x * (double)t[j][k];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        double v = s[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((tid & 63) == 0) red[tid >> 6][i] = v;
    }
    __syncthreads();
    if (tid < NS) partial[(size_t)blockIdx.x * NS + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// Sum `idx` of clip b over its chunks, in chunk order.
__device__ __forceinline__ double clip_sum(const double* __restrict__ partial, int b, int n_chunks, int ns, int idx) {
    double v = 0.0;
    for (int c = 0; c < n_chunks; ++c) v += partial[((size_t)b * n_chunks + c) * ns + idx];
    return v;
}

struct PairTerms {
    double value;   // pair[i][j], rounded to fp32 and widened again: what the search adds and what the caller reads
    double ca, cr;  // d pair / d a = ca a + cr r  (a, r: the signals after the mean subtraction)
    double ma, mr;  // the means taken off (0 without zero_mean)
};

// pair[i][j] and the coefficients of its gradient from the clip's sums `tot` (LDS).  With tn' = tn + eps, alpha = dot / tn',
// P = alpha^2 tn, N = en - 2 alpha dot + alpha^2 tn, den = N + eps, arg = P / den + eps:
//   pair = -10 log10(arg),  ca = (20 / ln 10) P / (arg den^2),  cr = -(20 / ln 10) alpha / arg (tn / (tn' den) + P (1 + eps / tn') / den^2)
__device__ __forceinline__ PairTerms pair_terms(const double* tot, int S, int i, int j, int L, int zero_mean, double eps) {
    const double sa = tot[i], sr = tot[S + j], saa = tot[2 * S + i], srr = tot[3 * S + j], sar = tot[4 * S + i * S + j];
    PairTerms t;
    t.ma = zero_mean ? sa / L : 0.0;
    t.mr = zero_mean ? sr / L : 0.0;
    const double en = saa - sa * t.ma, tn = srr - sr * t.mr, dot = sar - sa * t.mr;
    const double tne = tn + eps, alpha = dot / tne;
    const double P = (alpha * alpha) * tn, N = (en - 2.0 * (alpha * dot)) + P;
    const double den = N + eps, arg = P / den + eps;
    const double K = 10.0 / 2.302585092994046;
    t.value = (double)(float)(-10.0 * log10(arg));
    t.ca = 2.0 * K * P / (arg * (den * den));
    t.cr = -(2.0 * K) * alpha / arg * (tn / (tne * den) + P * (1.0 + eps / tne) / (den * den));
    return t;
}

// Entry j of the k-th permutation of 0 .. S-1 in the order of itertools.permutations (lexicographic), two bits per entry.
__device__ __forceinline__ int kth_perm(int k, int S) {
    int avail = (1 << S) - 1, packed = 0, f = 1;
    for (int m = 2; m < S; ++m) f *= m;  // (S - 1)!
    for (int j = 0; j < S; ++j) {
        int d = k / f;
        k -= d * f;
        if (S - 1 - j > 0) f /= (S - 1 - j);
        int p = 0;
        for (int q = 0; q < PIT_MAX_S; ++q) {
            if (!((avail >> q) & 1)) continue;
            if (d == 0) {
                p = q;
                break;
            }
            --d;
        }
        avail &= ~(1 << p);
        packed |= p << (2 * j);
    }
    return packed;
}

// The permutation with the smallest mean of pair[p[j]][j] (the first one on a tie) and that mean; `pw` [S][S] in LDS.
__device__ __forceinline__ int best_perm(const double* pw, int S, double* best_loss) {
    int n_perm = 1;
    for (int m = 2; m <= S; ++m) n_perm *= m;
    int best = 0;
    double lbest = 0.0;
    for (int k = 0; k < n_perm; ++k) {
        const int p = kth_perm(k, S);
        double l = 0.0;
        for (int j = 0; j < S; ++j) l += pw[((p >> (2 * j)) & 3) * S + j];
        l /= S;
        if (k == 0 || l < lbest) {
            lbest = l;
            best = p;
        }
    }
    *best_loss = lbest;
    return best;
}

template <int S>
__global__ __launch_bounds__(PIT_THREADS) void pit_finish_kernel(const float* __restrict__ est, const float* __restrict__ ref, int clips, int L,
                                                                 int n_chunks, int n_main, int zero_mean, float eps,
                                                                 const double* __restrict__ partial, const float* __restrict__ pair_cot,
                                                                 float* __restrict__ pair, int32_t* __restrict__ perm, float* __restrict__ loss,
                                                                 float* __restrict__ grad, float* __restrict__ reordered) {
    constexpr int NS = S * S + 4 * S;
    __shared__ double tot[PIT_BATCH][NS];
    __shared__ double pw[PIT_BATCH][S * S], ca[S * S], cr[S * S], cm[S * S];
    __shared__ double lmin[PIT_BATCH];
    __shared__ float cA[S], cR[S][S], cC[S];
    __shared__ int sperm;
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < n_main) {
        const int b = blockIdx.x / n_chunks, chunk = blockIdx.x - b * n_chunks;
        if (tid < NS) tot[0][tid] = clip_sum(partial, b, n_chunks, NS, tid);
        __syncthreads();
        if (tid < S * S) {
            const PairTerms t = pair_terms(tot[0], S, tid / S, tid % S, L, zero_mean, (double)eps);
            pw[0][tid] = t.value;
            ca[tid] = t.ca;
            cr[tid] = t.cr;
            cm[tid] = -(t.ca * t.ma) - t.cr * t.mr;  // the constant the two mean subtractions leave
        }
        __syncthreads();
        if (tid == 0 && !pair_cot) {
            double l;
            sperm = best_perm(pw[0], S, &l);
        }
        __syncthreads();
        if (tid < S) {  // row tid of the estimates: grad = A est + sum_j R_j ref_j + C
            const int i = tid;
            double A = 0.0, C = 0.0;
            for (int j = 0; j < S; ++j) {
                double w;
                if (pair_cot)
                    w = (double)pair_cot[((size_t)b * S + i) * S + j];
                else
                    w = ((sperm >> (2 * j)) & 3) == i ? 1.0 / ((double)clips * S) : 0.0;
                const bool used = pair_cot || w != 0.0;
                A += used ? w * ca[i * S + j] : 0.0;
                C += used ? w * cm[i * S + j] : 0.0;
                cR[i][j] = used ? (float)(w * cr[i * S + j]) : 0.0f;
            }
            cA[i] = (float)A;
            cC[i] = (float)C;
        }
        __syncthreads();
        const int lo = chunk * PIT_CHUNK, len = min(PIT_CHUNK, L - lo);
        const size_t base = (size_t)b * S * L + lo;
        const float* e = est + base;
        const float* r = ref + base;
        const int p = pair_cot ? 0 : sperm;
        for (int o = 4 * tid; o < len; o += 4 * PIT_THREADS) {
            float a[S][4], t[S][4];
#pragma unroll
            for (int i = 0; i < S; ++i) load4(e + (size_t)i * L, o, len, a[i]);
            if (grad) {
#pragma unroll
                for (int j = 0; j < S; ++j) load4(r + (size_t)j * L, o, len, t[j]);
#pragma unroll
                for (int i = 0; i < S; ++i) {
                    float g[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float v = cA[i] * a[i][k];
#pragma unroll
                        for (int j = 0; j < S; ++j)
                            if (pair_cot || ((p >> (2 * j)) & 3) == i) v += cR[i][j] * t[j][k];  // (the same for every thread)
                        g[k] = v + cC[i];
                    }
                    store4(grad + base + (size_t)i * L, o, len, g);
                }
            }
            if (reordered) {
#pragma unroll
                for (int j = 0; j < S; ++j) {
                    const int src = (p >> (2 * j)) & 3;
                    float v[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        v[k] = a[0][k];
#pragma unroll
                        for (int i = 1; i < S; ++i) v[k] = src == i ? a[i][k] : v[k];
                    }
                    store4(reordered + base + (size_t)j * L, o, len, v);
                }
            }
        }
        return;
    }
    // the last workgroup: pair, perm and loss of every clip, PIT_BATCH clips at a time
    double lsum = 0.0;  // (thread 0)
    for (int b0 = 0; b0 < clips; b0 += PIT_BATCH) {
        const int nb = min(PIT_BATCH, clips - b0);
        for (int q = tid; q < nb * NS; q += PIT_THREADS) tot[q / NS][q % NS] = clip_sum(partial, b0 + q / NS, n_chunks, NS, q % NS);
        __syncthreads();
        for (int q = tid; q < nb * S * S; q += PIT_THREADS) {
            const int c = q / (S * S), ij = q % (S * S);
            const PairTerms t = pair_terms(tot[c], S, ij / S, ij % S, L, zero_mean, (double)eps);
            pw[c][ij] = t.value;
            pair[(size_t)(b0 + c) * S * S + ij] = (float)t.value;
        }
        __syncthreads();
        if (perm && tid < nb) {
            double l;
            const int p = best_perm(pw[tid], S, &l);
            lmin[tid] = l;
            for (int j = 0; j < S; ++j) perm[(size_t)(b0 + tid) * S + j] = (p >> (2 * j)) & 3;
        }
        __syncthreads();
        if (perm && tid == 0)
            for (int c = 0; c < nb; ++c) lsum += lmin[c];  // clips in order
    }
    if (loss && tid == 0) *loss = (float)(lsum / clips);
}

// ---- ragged batches (sfsn_pit_sdr_ragged): clip b ends at L_b = clip_len[b], clamped into [0, L]; L is the padded row length.
// The two kernels above are left as they are, instruction for instruction (scripts/device_code_digest.py pins their device code);
// these two restate them with the clip's own length: the same expressions on the same values in the same order, so a clip has the
// bits of sfsn_pit_sdr on that clip alone.  Nothing at or past L_b is read.

__device__ __forceinline__ int clip_length(const int32_t* __restrict__ clip_len, int b, int L) { return min(max(clip_len[b], 0), L); }

template <int S>
__global__ __launch_bounds__(PIT_THREADS) void pit_sums_ragged_kernel(const float* __restrict__ est, const float* __restrict__ ref, int L, int n_chunks,
                                                                      const int32_t* __restrict__ clip_len,
                                                                      double* __restrict__ partial /* [clips][n_chunks][NS] */) {
    constexpr int NS = S * S + 4 * S;
    __shared__ double red[4][NS];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / n_chunks, chunk = blockIdx.x - b * n_chunks;
    const int Lb = clip_length(clip_len, b, L);
    const int lo = chunk * PIT_CHUNK;
    if (lo >= Lb) return;  // past the clip's end: no partial (the whole workgroup leaves; nobody reads this slot)
    const int len = min(PIT_CHUNK, Lb - lo);
    const float* e = est + (size_t)b * S * L + lo;
    const float* r = ref + (size_t)b * S * L + lo;
    double s[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) s[i] = 0.0;
    for (int o = 4 * tid; o < len; o += 4 * PIT_THREADS) {
        float a[S][4], t[S][4];
#pragma unroll
        for (int i = 0; i < S; ++i) {
            load4(e + (size_t)i * L, o, len, a[i]);
            load4(r + (size_t)i * L, o, len, t[i]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int i = 0; i < S; ++i) {
                const double x = a[i][k], y = t[i][k];
                s[i] += x;
                s[S + i] += y;
                s[2 * S + i] += x * x;
                s[3 * S + i] += y * y;
#pragma unroll
                for (int j = 0; j < S; ++j) s[4 * S + i * S + j] += x * (double)t[j][k];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        double v = s[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((tid & 63) == 0) red[tid >> 6][i] = v;
    }
    __syncthreads();
    if (tid < NS) partial[(size_t)blockIdx.x * NS + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// audiozen.metric.SISDR of estimate row i against reference row j from the clip's sums `tot` (LDS), in fp64: both rows minus their own
// mean over Lb whatever zero_mean says, eps = 2^-23 (torch.finfo(float32).eps), proj = (dot s + eps) / (n + eps) per sample.  With the
// centred sums en = |a|^2, n = |s|^2, dot = <a, s> (sum a = sum s = 0):
//   sum proj^2 = (dot^2 n + Lb eps^2) / (n + eps)^2,  sum a proj = dot^2 / (n + eps),  sum noise^2 = en - 2 sum a proj + sum proj^2
__device__ __forceinline__ double si_sdr_value(const double* tot, int S, int i, int j, int Lb) {
    const double sa = tot[i], sr = tot[S + j], saa = tot[2 * S + i], srr = tot[3 * S + j], sar = tot[4 * S + i * S + j];
    const double eps = 1.1920928955078125e-07;
    const double ma = sa / Lb, mr = sr / Lb;
    const double en = saa - sa * ma, n = srr - sr * mr, dot = sar - sa * mr;
    const double ne = n + eps, d2 = dot * dot;
    const double sp = (d2 * n + (double)Lb * (eps * eps)) / (ne * ne);
    const double sap = d2 / ne;
    const double sn = (en - 2.0 * sap) + sp;
    return 10.0 * log10((sp + eps) / (sn + eps) + eps);
}

template <int S>
__global__ __launch_bounds__(PIT_THREADS) void pit_finish_ragged_kernel(const float* __restrict__ est, const float* __restrict__ ref, int clips, int L,
                                                                        int n_chunks, int n_main, const int32_t* __restrict__ clip_len,
                                                                        int zero_mean, float eps, const double* __restrict__ partial,
                                                                        const float* __restrict__ pair_cot, float* __restrict__ pair,
                                                                        int32_t* __restrict__ perm, float* __restrict__ clip_loss,
                                                                        float* __restrict__ loss, float* __restrict__ grad,
                                                                        float* __restrict__ reordered, float* __restrict__ si_sdr) {
    constexpr int NS = S * S + 4 * S;
    __shared__ double tot[PIT_BATCH][NS];
    __shared__ double pw[PIT_BATCH][S * S], ca[S * S], cr[S * S], cm[S * S];
    __shared__ double lmin[PIT_BATCH];
    __shared__ float cA[S], cR[S][S], cC[S];
    __shared__ int sperm;
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < n_main) {
        const int b = blockIdx.x / n_chunks, chunk = blockIdx.x - b * n_chunks;
        const int Lb = clip_length(clip_len, b, L);
        const int lo = chunk * PIT_CHUNK, span = min(PIT_CHUNK, L - lo);  // span: what this workgroup stores, padding included
        const size_t base = (size_t)b * S * L + lo;
        const float zero[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (lo >= Lb) {  // the whole chunk is padding: zeros, nothing read
            for (int o = 4 * tid; o < span; o += 4 * PIT_THREADS) {
#pragma unroll
                for (int i = 0; i < S; ++i) {
                    if (grad) store4(grad + base + (size_t)i * L, o, span, zero);
                    if (reordered) store4(reordered + base + (size_t)i * L, o, span, zero);
                }
            }
            return;
        }
        const int nc = (Lb + PIT_CHUNK - 1) / PIT_CHUNK;  // the clip's own chunks
        const double* mine = partial + (size_t)b * n_chunks * NS;
        if (tid < NS) tot[0][tid] = clip_sum(mine, 0, nc, NS, tid);
        __syncthreads();
        if (tid < S * S) {
            const PairTerms t = pair_terms(tot[0], S, tid / S, tid % S, Lb, zero_mean, (double)eps);
            pw[0][tid] = t.value;
            ca[tid] = t.ca;
            cr[tid] = t.cr;
            cm[tid] = -(t.ca * t.ma) - t.cr * t.mr;
        }
        __syncthreads();
        if (tid == 0 && !pair_cot) {
            double l;
            sperm = best_perm(pw[0], S, &l);
        }
        __syncthreads();
        if (tid < S) {
            const int i = tid;
            double A = 0.0, C = 0.0;
            for (int j = 0; j < S; ++j) {
                double w;
                if (pair_cot)
                    w = (double)pair_cot[((size_t)b * S + i) * S + j];
                else
                    w = ((sperm >> (2 * j)) & 3) == i ? 1.0 / ((double)clips * S) : 0.0;
                const bool used = pair_cot || w != 0.0;
                A += used ? w * ca[i * S + j] : 0.0;
                C += used ? w * cm[i * S + j] : 0.0;
                cR[i][j] = used ? (float)(w * cr[i * S + j]) : 0.0f;
            }
            cA[i] = (float)A;
            cC[i] = (float)C;
        }
        __syncthreads();
        const int len = min(PIT_CHUNK, Lb - lo);  // the clip's samples in this chunk (len <= span)
        const float* e = est + base;
        const float* r = ref + base;
        const int p = pair_cot ? 0 : sperm;
        for (int o = 4 * tid; o < span; o += 4 * PIT_THREADS) {
            if (o >= len) {  // the tail inside the clip's last chunk
#pragma unroll
                for (int i = 0; i < S; ++i) {
                    if (grad) store4(grad + base + (size_t)i * L, o, span, zero);
                    if (reordered) store4(reordered + base + (size_t)i * L, o, span, zero);
                }
                continue;
            }
            float a[S][4], t[S][4];
#pragma unroll
            for (int i = 0; i < S; ++i) load4(e + (size_t)i * L, o, len, a[i]);
            if (grad) {
#pragma unroll
                for (int j = 0; j < S; ++j) load4(r + (size_t)j * L, o, len, t[j]);
#pragma unroll
                for (int i = 0; i < S; ++i) {
                    float g[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float v = cA[i] * a[i][k];
#pragma unroll
                        for (int j = 0; j < S; ++j)
                            if (pair_cot || ((p >> (2 * j)) & 3) == i) v += cR[i][j] * t[j][k];
                        g[k] = o + k < len ? v + cC[i] : 0.0f;  // (a quad that straddles the clip's end)
                    }
                    store4(grad + base + (size_t)i * L, o, span, g);
                }
            }
            if (reordered) {
#pragma unroll
                for (int j = 0; j < S; ++j) {
                    const int src = (p >> (2 * j)) & 3;
                    float v[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        v[k] = a[0][k];  // (load4 reads positions from len on as +0)
#pragma unroll
                        for (int i = 1; i < S; ++i) v[k] = src == i ? a[i][k] : v[k];
                    }
                    store4(reordered + base + (size_t)j * L, o, span, v);
                }
            }
        }
        return;
    }
    // the last workgroup: pair, perm, clip_loss, si_sdr and loss of every clip, PIT_BATCH clips at a time
    double lsum = 0.0;  // (thread 0)
    for (int b0 = 0; b0 < clips; b0 += PIT_BATCH) {
        const int nb = min(PIT_BATCH, clips - b0);
        for (int q = tid; q < nb * NS; q += PIT_THREADS) {
            const int b = b0 + q / NS;
            const int nc = (clip_length(clip_len, b, L) + PIT_CHUNK - 1) / PIT_CHUNK;
            tot[q / NS][q % NS] = clip_sum(partial + (size_t)b * n_chunks * NS, 0, nc, NS, q % NS);
        }
        __syncthreads();
        for (int q = tid; q < nb * S * S; q += PIT_THREADS) {
            const int c = q / (S * S), ij = q % (S * S);
            const PairTerms t = pair_terms(tot[c], S, ij / S, ij % S, clip_length(clip_len, b0 + c, L), zero_mean, (double)eps);
            pw[c][ij] = t.value;
            pair[(size_t)(b0 + c) * S * S + ij] = (float)t.value;
        }
        __syncthreads();
        if (perm && tid < nb) {
            double l;
            const int p = best_perm(pw[tid], S, &l);
            lmin[tid] = l;
            if (clip_loss) clip_loss[b0 + tid] = (float)l;
            for (int j = 0; j < S; ++j) {
                perm[(size_t)(b0 + tid) * S + j] = (p >> (2 * j)) & 3;
                if (si_sdr)
                    si_sdr[(size_t)(b0 + tid) * S + j] = (float)si_sdr_value(tot[tid], S, (p >> (2 * j)) & 3, j, clip_length(clip_len, b0 + tid, L));
            }
        }
        __syncthreads();
        if (perm && tid == 0)
            for (int c = 0; c < nb; ++c) lsum += lmin[c];  // clips in order
    }
    if (loss && tid == 0) *loss = (float)(lsum / clips);
}

struct PitLayout {
    int n_chunks;
    size_t total;
};

// SFSN_OK and the scratch layout, or the status the entry point answers with (host only).
int pit_layout(int clips, int sources, int n_samples, PitLayout* out) {
    if (clips < 1 || sources < 1 || n_samples < 2) return SFSN_EINVAL;
    if (sources > PIT_MAX_S) return SFSN_EUNSUPPORTED;
    if ((long long)clips * sources * n_samples > INT_MAX) return SFSN_EUNSUPPORTED;
    const int n_chunks = (n_samples + PIT_CHUNK - 1) / PIT_CHUNK;
    out->n_chunks = n_chunks;
    out->total = (((size_t)clips * n_chunks * (sources * sources + 4 * sources) * sizeof(double)) + 255) & ~(size_t)255;
    return SFSN_OK;
}

template <int S>
int pit_launch(const float* est, const float* ref, int clips, int L, int n_chunks, int zero_mean, float eps, const float* pair_cot, float* pair,
               int32_t* perm, float* loss, float* grad, float* reordered, double* partial, hipStream_t st) {
    hipLaunchKernelGGL(pit_sums_kernel<S>, dim3(clips * n_chunks), dim3(PIT_THREADS), 0, st, est, ref, L, n_chunks, partial);
    if (hipGetLastError() != hipSuccess) return SFSN_EHIP;
    const int n_main = (grad || reordered) ? clips * n_chunks : 0;
    hipLaunchKernelGGL(pit_finish_kernel<S>, dim3(n_main + 1), dim3(PIT_THREADS), 0, st, est, ref, clips, L, n_chunks, n_main, zero_mean, eps, partial,
                       pair_cot, pair, perm, loss, grad, reordered);
    return hip_ok(hipGetLastError());
}

template <int S>
int pit_launch_ragged(const float* est, const float* ref, int clips, int L, int n_chunks, const int32_t* clip_len, int zero_mean, float eps,
                      const float* pair_cot, float* pair, int32_t* perm, float* clip_loss, float* loss, float* grad, float* reordered, float* si_sdr,
                      double* partial, hipStream_t st) {
    hipLaunchKernelGGL(pit_sums_ragged_kernel<S>, dim3(clips * n_chunks), dim3(PIT_THREADS), 0, st, est, ref, L, n_chunks, clip_len, partial);
    if (hipGetLastError() != hipSuccess) return SFSN_EHIP;
    const int n_main = (grad || reordered) ? clips * n_chunks : 0;
    hipLaunchKernelGGL(pit_finish_ragged_kernel<S>, dim3(n_main + 1), dim3(PIT_THREADS), 0, st, est, ref, clips, L, n_chunks, n_main, clip_len, zero_mean,
                       eps, partial, pair_cot, pair, perm, clip_loss, loss, grad, reordered, si_sdr);
    return hip_ok(hipGetLastError());
}

}  // namespace

extern "C" size_t sfsn_pit_sdr_scratch_bytes(int clips, int sources, int n_samples) {
    PitLayout lay;
    return pit_layout(clips, sources, n_samples, &lay) == SFSN_OK ? lay.total : 0;
}

extern "C" int sfsn_pit_sdr(const float* est, const float* ref, int clips, int sources, int n_samples, int zero_mean, float eps,
                            const float* pair_cot, float* pair, int32_t* perm, float* loss, float* grad_est, float* reordered, void* scratch,
                            void* stream) {
    PitLayout lay;
    const int rc = pit_layout(clips, sources, n_samples, &lay);
    if (rc == SFSN_EINVAL) return rc;
    if (!est || !ref || !pair) return SFSN_EINVAL;
    if (pair_cot ? (perm || loss || reordered) : (!perm || !loss)) return SFSN_EINVAL;
    if (!aligned16(est) || !aligned16(ref) || !aligned16(pair_cot) || !aligned16(pair) || !aligned16(perm) || !aligned16(loss) ||
        !aligned16(grad_est) || !aligned16(reordered) || !aligned16(scratch))
        return SFSN_EINVAL;
    if (!(eps >= 0.0f) || !isfinite(eps)) return SFSN_EINVAL;
    if (rc != SFSN_OK) return rc;  // (a shape beyond the kernel has no scratch size: answered before scratch is asked for)
    if (!scratch) return SFSN_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* partial = static_cast<double*>(scratch);
    const int zm = zero_mean ? 1 : 0;
    switch (sources) {
        case 1: return pit_launch<1>(est, ref, clips, n_samples, lay.n_chunks, zm, eps, pair_cot, pair, perm, loss, grad_est, reordered, partial, st);
        case 2: return pit_launch<2>(est, ref, clips, n_samples, lay.n_chunks, zm, eps, pair_cot, pair, perm, loss, grad_est, reordered, partial, st);
        case 3: return pit_launch<3>(est, ref, clips, n_samples, lay.n_chunks, zm, eps, pair_cot, pair, perm, loss, grad_est, reordered, partial, st);
        default: return pit_launch<4>(est, ref, clips, n_samples, lay.n_chunks, zm, eps, pair_cot, pair, perm, loss, grad_est, reordered, partial, st);
    }
}

extern "C" int sfsn_pit_sdr_ragged(const float* est, const float* ref, int clips, int sources, int n_samples, const int32_t* clip_len, int zero_mean,
                                   float eps, const float* pair_cot, float* pair, int32_t* perm, float* clip_loss, float* loss, float* grad_est,
                                   float* reordered, float* si_sdr, void* scratch, void* stream) {
    PitLayout lay;
    const int rc = pit_layout(clips, sources, n_samples, &lay);
    if (rc == SFSN_EINVAL) return rc;
    if (!est || !ref || !pair || !clip_len) return SFSN_EINVAL;
    if (pair_cot ? (perm || loss || reordered || clip_loss || si_sdr) : (!perm || !loss)) return SFSN_EINVAL;
    if (!aligned16(est) || !aligned16(ref) || !aligned16(clip_len) || !aligned16(pair_cot) || !aligned16(pair) || !aligned16(perm) ||
        !aligned16(clip_loss) || !aligned16(loss) || !aligned16(grad_est) || !aligned16(reordered) || !aligned16(si_sdr) || !aligned16(scratch))
        return SFSN_EINVAL;
    if (!(eps >= 0.0f) || !isfinite(eps)) return SFSN_EINVAL;
    if (rc != SFSN_OK) return rc;
    if (!scratch) return SFSN_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* partial = static_cast<double*>(scratch);
    const int zm = zero_mean ? 1 : 0;
    switch (sources) {
        case 1: return pit_launch_ragged<1>(est, ref, clips, n_samples, lay.n_chunks, clip_len, zm, eps, pair_cot, pair, perm, clip_loss, loss, grad_est, reordered, si_sdr, partial, st);
        case 2: return pit_launch_ragged<2>(est, ref, clips, n_samples, lay.n_chunks, clip_len, zm, eps, pair_cot, pair, perm, clip_loss, loss, grad_est, reordered, si_sdr, partial, st);
        case 3: return pit_launch_ragged<3>(est, ref, clips, n_samples, lay.n_chunks, clip_len, zm, eps, pair_cot, pair, perm, clip_loss, loss, grad_est, reordered, si_sdr, partial, st);
        default: return pit_launch_ragged<4>(est, ref, clips, n_samples, lay.n_chunks, clip_len, zm, eps, pair_cot, pair, perm, clip_loss, loss, grad_est, reordered, si_sdr, partial, st);
    }
}
