// sfsn_fullband.hip -- the two ends of the cIRM-GSN model (audiozen/models/cirm_gsn/modeling_cirm_gsn.py): one full-band GSN stack
// whose input is LayerNorm(|X|^fdrc) over ALL n_fft/2 + 1 bins (Nyquist included) and whose head projects the last layer's spikes onto
// 2 * df * S * F deep-filter coefficients per frame, applied to the whole spectrum.  The GSN layers run on the existing
// sfsn_gsn_stack_scan.  gfx950 only.
//
//   sfsn_fullband_features:       stft_ri [B][F][T][2] -> x [T][B][F] (features_kernel's magnitude and LayerNorm expressions).
//   sfsn_fullband_input_proj:     layer 0's input term x . W_ih^T + bias for K = F > 192 (an fp32 fmaf chain in k order).
//   sfsn_fullband_proj_deepfilter: spikes [T][B][pad64(H)] -> coefficients (int8 matrix cores, spike_proj's exact three-digit sums,
//                                  `rec * dq + bias`) -> activation -> deep filter over all F bins -> enh_ri / enh_mag.  The coefficients
//                                  live in registers only; `proj` receives the pre-activation rows when asked for.
//
// Work item of the epilogue = one wave: (clip b, 16 consecutive frames, 16 consecutive bins).  The wave holds its 16 spike rows as MFMA
// B fragments and walks the (s, d, c) column tiles of its bin block; W_p is too large for LDS (1.5 MB at the recipe's 268 -> 1542), so
// its A fragments are streamed from L2 per tile -- every item of a bin block reads the same 2 df S tiles.  Lane (m, q) of a tile result
// holds frame m and bins 4q .. 4q + 3, so the deep-filter sum of a (frame, bin) is formed in the lane that computed its coefficients,
// d ascending, with the oracle's expressions; the spectrum reads and enhanced-spectrum writes of 16 lanes are 16 consecutive frames.
#include <hip/hip_runtime.h>
#include <math.h>

#include "sfsn_feat_dev.h"
#include "sfsn_scan_dev.h"
#include "sfsn_fullband_dev.h"

static inline bool fbd_aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }

// =====================================================================================================
// features: |X|^fdrc over all F bins, LayerNorm over F (or none)
// =====================================================================================================
#define FBF_TT 32  // frames per workgroup

template <int NU>
__global__ __launch_bounds__(256) void fullband_features_kernel(const float* __restrict__ stft, int B, int F, int T, float fdrc,
                                                                const float* __restrict__ ln_w, const float* __restrict__ ln_b, float eps,
                                                                float* __restrict__ x, int t0, int t1) {
    extern __shared__ __attribute__((aligned(16))) float fbf_smem[];
    float* magT = fbf_smem;  // [F][33]
    const int b = blockIdx.y, tb = t0 + blockIdx.x * FBF_TT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {
        const int tt = tid & 31, t = tb + tt;
        const bool live = t < t1;
        const int tc = live ? t : t1 - 1;
        const float* src = stft + ((size_t)b * F * T + tc) * 2;
        for (int f0 = tid >> 5; f0 < F; f0 += 64) {
            float2 c[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                int fr = f0 + 8 * i;
                if (fr > F - 1) fr = F - 1;
                c[i] = *reinterpret_cast<const float2*>(src + (size_t)fr * T * 2);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int fr = f0 + 8 * i;
                if (fr < F) magT[fr * 33 + tt] = live ? compress_mag(c[i].x, c[i].y, fdrc) : 0.0f;
            }
        }
    }
    __syncthreads();
    float lw[NU], lb[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int j = lane + 64 * u;
        const bool in = j < F && ln_w;
        lw[u] = in ? ln_w[j] : 0.0f;
        lb[u] = in ? ln_b[j] : 0.0f;
    }
    for (int tt = wave; tt < FBF_TT; tt += 4) {
        const int t = tb + tt;
        if (t >= t1) break;  // wave-uniform
        float v[NU], y[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int j = lane + 64 * u;
            v[u] = j < F ? magT[j * 33 + tt] : 0.0f;
        }
        fullband_norm_row<NU>(v, lane, F, ln_w != nullptr, lw, lb, eps, y);
        float* out = x + ((size_t)t * B + b) * F;
#pragma unroll
        for (int u = 0; u < NU; ++u)
            if (lane + 64 * u < F) out[lane + 64 * u] = y[u];
    }
}

extern "C" int sfsn_fullband_features(const float* stft_ri, int B, int F, int T, float fdrc, const float* ln_w, const float* ln_b,
                                      float ln_eps, float* x, int t0, int nt, void* stream) {
    if (!stft_ri || !x || B <= 0 || F <= 0 || T <= 0 || (ln_w == nullptr) != (ln_b == nullptr)) return SFSN_EINVAL;
    if (t0 < 0 || nt <= 0 || t0 + nt > T) return SFSN_EINVAL;
    if ((reinterpret_cast<uintptr_t>(stft_ri) & 7u) || (reinterpret_cast<uintptr_t>(x) & 3u)) return SFSN_EINVAL;
    if (F > 320) return SFSN_EUNSUPPORTED;
    const dim3 grid((unsigned)((nt + FBF_TT - 1) / FBF_TT), (unsigned)B);
    const size_t lds = (size_t)F * 33 * sizeof(float);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int NU = (F + 63) / 64;
#define FBF_CASE(NU_)                                                                                                  \
    if (NU == NU_) {                                                                                                   \
        hipLaunchKernelGGL(fullband_features_kernel<NU_>, grid, dim3(256), lds, st, stft_ri, B, F, T, fdrc, ln_w, ln_b, \
                           ln_eps, x, t0, t0 + nt);                                                                    \
        return hipGetLastError() == hipSuccess ? SFSN_OK : SFSN_EHIP;                                                  \
    }
    FBF_CASE(1) FBF_CASE(2) FBF_CASE(3) FBF_CASE(4) FBF_CASE(5)
#undef FBF_CASE
    return SFSN_EUNSUPPORTED;
}

// =====================================================================================================
// layer 0's input term for any K: z[m][n] = sum_k x[m][k] w[n][k] (+ bias[n]), fp32 fmaf chain in k order
// (sfsn_input_proj_f32 stops at K <= 192; the full-spectrum rows have K = F = 257)
// =====================================================================================================
#define FBI_TM 64
#define FBI_TN 64
#define FBI_TK 16

__global__ __launch_bounds__(256) void fullband_inproj_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, float* __restrict__ z, int M, int K, int N,
                                                              int ldz) {
    __shared__ __attribute__((aligned(16))) float As[FBI_TK][FBI_TM + 4];
    __shared__ __attribute__((aligned(16))) float Bs[FBI_TK][FBI_TN + 4];
    const int tid = threadIdx.x, tm = tid >> 4, tn = tid & 15;
    const int m0 = blockIdx.x * FBI_TM, n0 = blockIdx.y * FBI_TN;
    const int lr = tid >> 2, lk = (tid & 3) * 4;  // loader: row lr of the tile, k lk .. lk + 3 of the chunk
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += FBI_TK) {
        float av[4], bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = k0 + lk + i;
            av[i] = (m0 + lr < M && k < K) ? x[(size_t)(m0 + lr) * K + k] : 0.0f;
            bv[i] = (n0 + lr < N && k < K) ? w[(size_t)(n0 + lr) * K + k] : 0.0f;
        }
        __syncthreads();  // the previous chunk's reads are done
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            As[lk + i][lr] = av[i];
            Bs[lk + i][lr] = bv[i];
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < FBI_TK; ++kk) {
            const float4 a = *reinterpret_cast<const float4*>(&As[kk][tm * 4]);
            const float4 b = *reinterpret_cast<const float4*>(&Bs[kk][tn * 4]);
            const float ar[4] = {a.x, a.y, a.z, a.w}, br[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(ar[i], br[j], acc[i][j]);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + tm * 4 + i;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + tn * 4 + j;
            if (n < N) z[(size_t)m * ldz + n] = bias ? acc[i][j] + bias[n] : acc[i][j];
        }
    }
}

extern "C" int sfsn_fullband_input_proj(const float* x, const float* w, const float* bias, float* z, int M, int K, int N, int ldz,
                                        void* stream) {
    if (!x || !w || !z || M <= 0 || K <= 0 || N <= 0 || ldz < N) return SFSN_EINVAL;
    if ((reinterpret_cast<uintptr_t>(x) & 3u) || (reinterpret_cast<uintptr_t>(w) & 3u) || (reinterpret_cast<uintptr_t>(z) & 3u))
        return SFSN_EINVAL;
    const long long mb = ((long long)M + FBI_TM - 1) / FBI_TM;
    if (mb > 0x7fffffffLL) return SFSN_EUNSUPPORTED;
    const dim3 grid((unsigned)mb, (unsigned)((N + FBI_TN - 1) / FBI_TN));
    hipLaunchKernelGGL(fullband_inproj_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), x, w, bias, z, M, K, N, ldz);
    return hipGetLastError() == hipSuccess ? SFSN_OK : SFSN_EHIP;
}

// =====================================================================================================
// projection + activation + full-spectrum deep filter
// =====================================================================================================
struct FbdfParams {
    const float* stft;   // [B][F][T][2]
    const int8_t* s;     // [T][B][KS*64]
    const int8_t* w;     // packed, bin-major rows (see sfsn.h)
    const float* dq;     // [NTT*16]
    const float* bias;   // [NTT*16] or nullptr
    float* proj;         // [T][B][P] or nullptr
    float* enh;          // [B][S][F][T][2]
    float* mag;          // [B][S][F][T] or nullptr
    int B, F, T, S, df, act, NFB, NCT, NTT, P;
    int t0, t1, ntile, items;
};

template <int KS>
__global__ __launch_bounds__(256) void fullband_projdf_kernel(const FbdfParams p) {
    constexpr int KP = KS * 64;
    const int lane = threadIdx.x & 63;
    const int item = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (item >= p.items) return;  // wave-uniform
    const int fb = item % p.NFB, bt = item / p.NFB;
    const int tile = bt % p.ntile, b = bt / p.ntile;
    const int m = lane & 15, q = lane >> 4;
    const int B = p.B, F = p.F, T = p.T, S = p.S, df = p.df;
    const int t = p.t0 + tile * 16 + m;
    const bool tv = t < p.t1;
    const int tl = tv ? t : p.t1 - 1;  // frames past the window re-read the last one (nothing of theirs is stored)
    const int8_t* srow = p.s + ((size_t)tl * B + b) * KP + q * 16;
    v4i bfr[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) bfr[ks] = *reinterpret_cast<const v4i*>(srow + ks * 64);
    const int fbase = fb * 16 + q * 4;
    // spectrum rows of this lane's four bins (a bin past F re-reads bin F - 1; its results are not stored)
    const float* xrow[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int f = fbase + r < F ? fbase + r : F - 1;
        xrow[r] = p.stft + ((size_t)b * F + f) * T * 2;
    }
    const size_t prow = ((size_t)t * B + b) * p.P;
    for (int s_ = 0; s_ < S; ++s_) {
        float yr[4] = {0.0f, 0.0f, 0.0f, 0.0f}, yi[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int d = 0; d < df; ++d) {
            float cf[2][4];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int j = (c * df + d) * S + s_;  // the reference's (c, d, s) column block
                const int ct = fb * p.NCT + j;        // its packed row tile
                v4i wa[KS][3];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                    for (int dp = 0; dp < 3; ++dp)
                        wa[ks][dp] = *reinterpret_cast<const v4i*>(p.w + ((((size_t)dp * p.NTT + ct) * KS + ks) * 64 + lane) * 16);
                v4i a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0}, a2 = {0, 0, 0, 0};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    a0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa[ks][0], bfr[ks], a0, 0, 0, 0);
                    a1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa[ks][1], bfr[ks], a1, 0, 0, 0);
                    a2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa[ks][2], bfr[ks], a2, 0, 0, 0);
                }
                const v4f dqv = *reinterpret_cast<const v4f*>(p.dq + ct * 16 + q * 4);
                const v4f bv = p.bias ? *reinterpret_cast<const v4f*>(p.bias + ct * 16 + q * 4) : v4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = fbd_coef(a0[r], a1[r], a2[r], dqv[r], bv[r]);  // = sfsn_spike_proj's output
                    if (p.proj && tv && fbase + r < F) p.proj[prow + (size_t)j * F + fbase + r] = v;
                    cf[c][r] = fbd_act(v, p.act);
                }
            }
            const int ts = tl - (df - 1) + d;
            const int tsc = ts < 0 ? 0 : ts;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float2 xv = *reinterpret_cast<const float2*>(xrow[r] + (size_t)tsc * 2);
                if (ts < 0) xv = make_float2(0.0f, 0.0f);
                fbd_tap(yr[r], yi[r], xv, cf[0][r], cf[1][r]);
            }
        }
        if (tv) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = fbase + r;
                if (f >= F) continue;
                const size_t o = (((size_t)b * S + s_) * F + f) * T + t;
                *reinterpret_cast<float2*>(p.enh + 2 * o) = make_float2(yr[r], yi[r]);
                if (p.mag) p.mag[o] = fbd_mag(yr[r], yi[r]);
            }
        }
    }
}

// The length-aware sibling (sfsn_fullband_proj_deepfilter_ragged): fullband_projdf_kernel's item, expression for expression, except that
// clip b ends at T_b = clip_frames[b] clamped into [0, T] and the item's window at t1 = min(p.t1, T_b).  The lanes of frames >= t1 re-read
// frame t1 - 1, as the lanes past the window do above, so nothing at or past T_b is read; those still inside the window store 0.  An item
// whose tile starts at or past t1 stores its zeros and returns before any spike or weight load.  (A kernel of its own, not a flag on the
// one above, whose code object stays what it was: scripts/device_code_digest.py, profiles/cirm_ragged.md.)
template <int KS>
__global__ __launch_bounds__(256) void fullband_projdf_ragged_kernel(const FbdfParams p, const int32_t* __restrict__ clip_frames) {
    constexpr int KP = KS * 64;
    const int lane = threadIdx.x & 63;
    const int item = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (item >= p.items) return;  // wave-uniform
    const int fb = item % p.NFB, bt = item / p.NFB;
    const int tile = bt % p.ntile, b = bt / p.ntile;
    const int m = lane & 15, q = lane >> 4;
    const int B = p.B, F = p.F, T = p.T, S = p.S, df = p.df;
    const int t = p.t0 + tile * 16 + m;
    const int tb = clip_frames[b];  // (b < B: one read per wave, before any other address depends on it)
    const int Tb = tb < 0 ? 0 : (tb > T ? T : tb);
    const int t1 = Tb < p.t1 ? Tb : p.t1;
    if (p.t0 + tile * 16 >= t1) {  // wave-uniform: the whole tile lies past the clip's end
        if (t < p.t1) {
            for (int s_ = 0; s_ < S; ++s_) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = fb * 16 + q * 4 + r;
                    if (f >= F) continue;
                    const size_t o = (((size_t)b * S + s_) * F + f) * T + t;
                    *reinterpret_cast<float2*>(p.enh + 2 * o) = make_float2(0.0f, 0.0f);
                    if (p.mag) p.mag[o] = 0.0f;
                }
            }
        }
        return;
    }
    const bool tv = t < t1;
    const int tl = tv ? t : t1 - 1;  // frames past the window re-read the last one (nothing of theirs is stored)
    const int8_t* srow = p.s + ((size_t)tl * B + b) * KP + q * 16;
    v4i bfr[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) bfr[ks] = *reinterpret_cast<const v4i*>(srow + ks * 64);
    const int fbase = fb * 16 + q * 4;
    // spectrum rows of this lane's four bins (a bin past F re-reads bin F - 1; its results are not stored)
    const float* xrow[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int f = fbase + r < F ? fbase + r : F - 1;
        xrow[r] = p.stft + ((size_t)b * F + f) * T * 2;
    }
    const size_t prow = ((size_t)t * B + b) * p.P;
    for (int s_ = 0; s_ < S; ++s_) {
        float yr[4] = {0.0f, 0.0f, 0.0f, 0.0f}, yi[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int d = 0; d < df; ++d) {
            float cf[2][4];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int j = (c * df + d) * S + s_;  // the reference's (c, d, s) column block
                const int ct = fb * p.NCT + j;        // its packed row tile
                v4i wa[KS][3];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                    for (int dp = 0; dp < 3; ++dp)
                        wa[ks][dp] = *reinterpret_cast<const v4i*>(p.w + ((((size_t)dp * p.NTT + ct) * KS + ks) * 64 + lane) * 16);
                v4i a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0}, a2 = {0, 0, 0, 0};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    a0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa[ks][0], bfr[ks], a0, 0, 0, 0);
                    a1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa[ks][1], bfr[ks], a1, 0, 0, 0);
                    a2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa[ks][2], bfr[ks], a2, 0, 0, 0);
                }
                const v4f dqv = *reinterpret_cast<const v4f*>(p.dq + ct * 16 + q * 4);
                const v4f bv = p.bias ? *reinterpret_cast<const v4f*>(p.bias + ct * 16 + q * 4) : v4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = fbd_coef(a0[r], a1[r], a2[r], dqv[r], bv[r]);  // = sfsn_spike_proj's output
                    if (p.proj && tv && fbase + r < F) p.proj[prow + (size_t)j * F + fbase + r] = v;
                    cf[c][r] = fbd_act(v, p.act);
                }
            }
            const int ts = tl - (df - 1) + d;
            const int tsc = ts < 0 ? 0 : ts;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float2 xv = *reinterpret_cast<const float2*>(xrow[r] + (size_t)tsc * 2);
                if (ts < 0) xv = make_float2(0.0f, 0.0f);
                fbd_tap(yr[r], yi[r], xv, cf[0][r], cf[1][r]);
            }
        }
        if (tv) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = fbase + r;
                if (f >= F) continue;
                const size_t o = (((size_t)b * S + s_) * F + f) * T + t;
                *reinterpret_cast<float2*>(p.enh + 2 * o) = make_float2(yr[r], yi[r]);
                if (p.mag) p.mag[o] = fbd_mag(yr[r], yi[r]);
            }
        } else if (t < p.t1) {  // inside the window, past the clip's end
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = fbase + r;
                if (f >= F) continue;
                const size_t o = (((size_t)b * S + s_) * F + f) * T + t;
                *reinterpret_cast<float2*>(p.enh + 2 * o) = make_float2(0.0f, 0.0f);
                if (p.mag) p.mag[o] = 0.0f;
            }
        }
    }
}

// the two entries' common host side; clip_frames selects the length-aware kernel
static int fbd_launch(const float* stft_ri, const int8_t* spikes_i8, int H, const int8_t* w_packed, const float* w_dq, const float* bias,
                      int act, int B, int F, int T, int S, int df, float* proj, float* enh_ri, float* enh_mag, int t0, int nt,
                      const int32_t* clip_frames, bool ragged, void* stream) {
    if (!stft_ri || !spikes_i8 || !w_packed || !w_dq || !enh_ri || H <= 0 || B <= 0 || F <= 0 || T <= 0 || S <= 0 || df <= 0)
        return SFSN_EINVAL;
    if (ragged && (!clip_frames || (reinterpret_cast<uintptr_t>(clip_frames) & 3u))) return SFSN_EINVAL;
    if (act < SFSN_ACT_NONE || act > SFSN_ACT_RELU) return SFSN_EINVAL;
    if (t0 < 0 || nt <= 0 || t0 + nt > T) return SFSN_EINVAL;
    if (!fbd_aligned16(spikes_i8) || !fbd_aligned16(w_packed) || !fbd_aligned16(w_dq) || !fbd_aligned16(bias) ||
        (reinterpret_cast<uintptr_t>(stft_ri) & 7u) || (reinterpret_cast<uintptr_t>(enh_ri) & 7u) ||
        (reinterpret_cast<uintptr_t>(proj) & 3u) || (reinterpret_cast<uintptr_t>(enh_mag) & 3u))
        return SFSN_EINVAL;
    const int KS = (H + 63) / 64;
    if (KS > 5 || F > 1025 || S > 4 || df > 16) return SFSN_EUNSUPPORTED;
    FbdfParams p;
    p.stft = stft_ri; p.s = spikes_i8; p.w = w_packed; p.dq = w_dq; p.bias = bias; p.proj = proj; p.enh = enh_ri; p.mag = enh_mag;
    p.B = B; p.F = F; p.T = T; p.S = S; p.df = df; p.act = act;
    p.NFB = (F + 15) / 16; p.NCT = 2 * df * S; p.NTT = p.NFB * p.NCT; p.P = 2 * df * S * F;
    p.t0 = t0; p.t1 = t0 + nt; p.ntile = (nt + 15) / 16;
    const long long items = (long long)B * p.ntile * p.NFB;
    if (items > (1LL << 30)) return SFSN_EUNSUPPORTED;
    p.items = (int)items;
    const unsigned grid = (unsigned)((items + 3) / 4);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define FBD_CASE(KS_)                                                                                              \
    if (KS == KS_) {                                                                                               \
        if (ragged)                                                                                                \
            hipLaunchKernelGGL(fullband_projdf_ragged_kernel<KS_>, dim3(grid), dim3(256), 0, st, p, clip_frames);  \
        else                                                                                                       \
            hipLaunchKernelGGL(fullband_projdf_kernel<KS_>, dim3(grid), dim3(256), 0, st, p);                      \
        return hipGetLastError() == hipSuccess ? SFSN_OK : SFSN_EHIP;                                              \
    }
    FBD_CASE(1) FBD_CASE(2) FBD_CASE(3) FBD_CASE(4) FBD_CASE(5)
#undef FBD_CASE
    return SFSN_EUNSUPPORTED;
}

extern "C" int sfsn_fullband_proj_deepfilter(const float* stft_ri, const int8_t* spikes_i8, int H, const int8_t* w_packed, const float* w_dq,
                                             const float* bias, int act, int B, int F, int T, int S, int df, float* proj, float* enh_ri,
                                             float* enh_mag, int t0, int nt, void* stream) {
    return fbd_launch(stft_ri, spikes_i8, H, w_packed, w_dq, bias, act, B, F, T, S, df, proj, enh_ri, enh_mag, t0, nt, nullptr, false, stream);
}

extern "C" int sfsn_fullband_proj_deepfilter_ragged(const float* stft_ri, const int8_t* spikes_i8, int H, const int8_t* w_packed,
                                                    const float* w_dq, const float* bias, int act, int B, int F, int T, int S, int df,
                                                    float* proj, float* enh_ri, float* enh_mag, int t0, int nt,
                                                    const int32_t* clip_frames, void* stream) {
    return fbd_launch(stft_ri, spikes_i8, H, w_packed, w_dq, bias, act, B, F, T, S, df, proj, enh_ri, enh_mag, t0, nt, clip_frames, true, stream);
}
