// sfsn_hop_wave_dev.h -- waveform mode of the one-launch streaming hops (sfsn_hop.hip, sfsn_fullband_hop.hip): complex values as
// tagged granules, the STFT of the new frame and the inverse STFT with its overlap-add state.  One body for both hops, built from
// sfsn_fft_dev.h's transform: the same instructions as spectral.stft / spectral.istft (sfsn_fft.hip), hence the same bits.
// gfx950 only.
#ifndef SFSN_HOP_WAVE_DEV_H
#define SFSN_HOP_WAVE_DEV_H
#include <hip/hip_runtime.h>

#include "sfsn_fft_dev.h"
#include "sfsn_hop_dev.h"
#include "sfsn_resample_dev.h"

// A complex value as two 8-byte {value, tag} granules (waveform mode: the noisy frame comes from the STFT workgroups of this
// launch, the enhanced frame goes to the inverse-STFT workgroups).  Every lane polls its own granules.
__device__ __forceinline__ void hop_put_cplx(float* g, float2 v, unsigned tagw) {
    st64_agent(g, ((unsigned long long)tagw << 32) | __float_as_uint(v.x));
    st64_agent(g + 2, ((unsigned long long)tagw << 32) | __float_as_uint(v.y));
}
__device__ __forceinline__ float2 hop_take_cplx(const float* g, unsigned tagw, bool& ok, unsigned* err) {
    for (unsigned spins = 0;; ++spins) {
        const unsigned long long a = ld64_agent(g), c = ld64_agent(g + 2);
        if (((unsigned)(a >> 32) == tagw && (unsigned)(c >> 32) == tagw) || !ok)
            return make_float2(__uint_as_float((unsigned)a), __uint_as_float((unsigned)c));
        if (spins > HOP_SPIN_LIMIT) {
            st_agent(err, 1u);
            ok = false;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// LDS of the two roles below
#define HOP_WAVE_LDS_STFT (64 + (size_t)FFT_NFFT * 8 + (size_t)HOP_WAVES * FFT_N * 8)
#define HOP_WAVE_LDS_ISTFT (HOP_WAVE_LDS_STFT + (size_t)HOP_WAVES * 264 * 8)

// ---------------------------------------------------------------------------------------------------------------------
// The new frame's spectrum for the clips [b0, b0 + nclip), nclip <= 16, by one workgroup, a wave per clip: the frame is the last
// 384 samples of the state followed by the 128 new ones; sfsn_fft.hip's transform (same code, same bits); the bins leave as
// granules; then the state moves on by one hop.  first_calls(lane, nclip): the wave's mask of clips that make their first call in this
// launch (bit ci: clip b0 + ci; their state reads as zero) -- asked once, before anything leaves this workgroup.  LDS: [64 B][unit table 4 KB][8 x 2 KB exchange].
// HELD (sfsn_stream_hop_held): held_clip(ci) = clip b0 + ci sits this launch out -- its granules leave like everyone's (the stages
// downstream poll them; what they hold is never used), its state does not move and a first call does not take the samples.
// ---------------------------------------------------------------------------------------------------------------------
template <bool HELD, class FirstCalls, class HeldClip>
__device__ __forceinline__ void hop_wave_stft_held(const float* wave_in, float* wave_state, const float* window, float* spec_g, int F, int b0,
                                                   int nclip, unsigned tagw, char* smem, FirstCalls first_calls, HeldClip held_clip) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float2* unit = reinterpret_cast<float2*>(smem + 64);
    float2(*fbuf)[FFT_N] = reinterpret_cast<float2(*)[FFT_N]>(smem + 64 + FFT_NFFT * 8);
    fill_unit_table(unit, tid, HOP_THREADS);
    __syncthreads();
    const Twiddles tw = make_twiddles<false>(unit, lane);
    const unsigned long long first = first_calls(lane, nclip);
    float2 win[4], wk[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = 2 * (lane + 64 * r);
        win[r] = make_float2(window[n], window[n + 1]);
        wk[r] = unit_at<false>(unit, lane + 64 * r);
    }
    for (int ci = wave; ci < nclip; ci += HOP_WAVES) {
        const int b = b0 + ci;
        const float* ws = wave_state + (size_t)b * FFT_NFFT;
        const float* wn = wave_in + (size_t)b * 128;
        const bool zero = (first >> ci) & 1ull;
        float2 v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = 2 * (lane + 64 * r);  // sample j of the frame: state[128 + j] for j < 384, then the new samples
            const float2 x = j < 384 ? (zero ? make_float2(0.0f, 0.0f) : *reinterpret_cast<const float2*>(ws + 128 + j))
                                     : *reinterpret_cast<const float2*>(wn + j - 384);
            v[r] = make_float2(x.x * win[r].x, x.y * win[r].y);
        }
        fft256<false>(v, fbuf[wave], lane, tw);
        float2 X[4], nyq = make_float2(0.0f, 0.0f);
        rfft512_split(v, fbuf[wave], lane, wk, X, nyq);
#pragma unroll
        for (int r = 0; r < 4; ++r) hop_put_cplx(spec_g + ((size_t)b * F + lane + 64 * r) * 4, X[r], tagw);
        if (lane == 0) hop_put_cplx(spec_g + ((size_t)b * F + FFT_N) * 4, nyq, tagw);
    }
    // the state moves on by one hop (every sample is read before any is written; a clip's first call leaves [0 x 384 | samples])
    float keep[16];
#pragma unroll
    for (int ci = 0; ci < 16; ++ci) {
        keep[ci] = 0.0f;
        if (ci < nclip) {
            const int b = b0 + ci;
            if (tid >= 384) keep[ci] = wave_in[(size_t)b * 128 + tid - 384];
            else if (!((first >> ci) & 1ull)) keep[ci] = wave_state[(size_t)b * FFT_NFFT + 128 + tid];
        }
    }
    __syncthreads();
#pragma unroll
    for (int ci = 0; ci < 16; ++ci)
        if (ci < nclip) {
            if constexpr (HELD) {
                if (held_clip(ci)) continue;
            }
            wave_state[(size_t)(b0 + ci) * FFT_NFFT + tid] = keep[ci];
        }
}
template <class FirstCalls>
__device__ __forceinline__ void hop_wave_stft(const float* wave_in, float* wave_state, const float* window, float* spec_g, int F, int b0,
                                              int nclip, unsigned tagw, char* smem, FirstCalls first_calls) {
    hop_wave_stft_held<false>(wave_in, wave_state, window, spec_g, F, b0, nclip, tagw, smem, first_calls, [](int) { return false; });
}

// ---------------------------------------------------------------------------------------------------------------------
// The enhanced frame back to samples.  A wave per (clip, speaker) pair, pair = 8 wg + wave of the role's workgroup wg: polls the
// 257 bins of the enhanced frame (granules written by the deep-filter workgroups), sfsn_fft.hip's inverse transform and window,
// overlap-add in registers against the carried accumulator (ascending frame order, as istft_kernel adds them), the hop that is now
// complete divided by the squared-window envelope of the frames that exist (t - q >= 0), accumulator moved on by one hop.
// frame_of(pair, fi, fresh, mute): the pair's frame index; fresh = its accumulator reads as zero; mute = its output is zero.
// before_done(ok): runs between the samples' store and the completion word.
// LDS: [64 B][unit table 4 KB][8 x 2 KB exchange][8 x 264 float2 spectrum rows].
// HELD (sfsn_stream_hop_held): held_pair(pair) = the pair's clip sits this launch out -- its samples are zero, its completion word is
// written all the same, its accumulator is not touched.
// ---------------------------------------------------------------------------------------------------------------------
template <bool HELD, class FrameOf, class BeforeDone, class HeldPair>
__device__ __forceinline__ void hop_wave_istft_held(float* ola_state, float* wave_out, const float* window, const float* enh_g, unsigned* done,
                                                    unsigned* err, int F, int wg, int npair, unsigned tagw, unsigned done_value, char* smem,
                                                    FrameOf frame_of, BeforeDone before_done, HeldPair held_pair) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pair = wg * HOP_WAVES + wave;  // clip * S + speaker
    float2* unit = reinterpret_cast<float2*>(smem + 64);
    float2(*fbuf)[FFT_N] = reinterpret_cast<float2(*)[FFT_N]>(smem + 64 + FFT_NFFT * 8);
    float2(*xs)[264] = reinterpret_cast<float2(*)[264]>(smem + 64 + FFT_NFFT * 8 + HOP_WAVES * FFT_N * 8);
    fill_unit_table(unit, tid, HOP_THREADS);
    __syncthreads();
    if (pair >= npair) return;
    const Twiddles tw = make_twiddles<true>(unit, lane);
    // the clip's own frame index (per-clip utterances): its accumulator reads as zero in the launch that restarts it, and its
    // output is zero until its frame 2 (calls 0 .. 2 of the utterance)
    int fi;
    bool fresh, mute;
    frame_of(pair, fi, fresh, mute);
    bool held = false;
    if constexpr (HELD) {
        held = held_pair(pair);
        mute = mute || held;
    }
    float2 win[4], wk[4], ola[4];
    float* os = ola_state + (size_t)pair * FFT_NFFT;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = 2 * (lane + 64 * r);
        win[r] = make_float2(window[n], window[n + 1]);
        wk[r] = unit_at<true>(unit, lane + 64 * r);
        ola[r] = make_float2(0.0f, 0.0f);
        if (!fresh) ola[r] = *reinterpret_cast<const float2*>(os + n);
    }
    bool ok = true;
    const float* eg = enh_g + (size_t)pair * F * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) xs[wave][lane + 64 * r] = hop_take_cplx(eg + (size_t)(lane + 64 * r) * 4, tagw, ok, err);
    if (lane == 0) xs[wave][FFT_N] = hop_take_cplx(eg + (size_t)FFT_N * 4, tagw, ok, err);
    __builtin_amdgcn_wave_barrier();
    float2 v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = lane + 64 * r;
        v[r] = irfft512_presplit(xs[wave][k], xs[wave][FFT_N - k], k, wk[r]);
    }
    fft256<true>(v, fbuf[wave], lane, tw);
    const float sc = 1.0f / (float)FFT_N;
    float2 acc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float2 res = make_float2(v[r].x * sc * win[r].x, v[r].y * sc * win[r].y);
        acc[r] = make_float2(ola[r].x + res.x, ola[r].y + res.y);
    }
    // the hop that is complete now: padded positions n = 128 t + 2 lane + e; envelope over the frames t - q that exist, oldest first
    float2 env = make_float2(0.0f, 0.0f);
#pragma unroll
    for (int q = 3; q >= 0; --q)
        if (fi - q >= 0) {
            env.x += win[q].x * win[q].x;
            env.y += win[q].y * win[q].y;
        }
    float2 out = make_float2(env.x > 1e-11f ? acc[0].x / env.x : 0.0f, env.y > 1e-11f ? acc[0].y / env.y : 0.0f);
    if (mute) out = make_float2(0.0f, 0.0f);
    *reinterpret_cast<float2*>(wave_out + (size_t)pair * 128 + 2 * lane) = out;
    before_done(ok);
    if (done) {
        // wave_out (and this word) may be host memory the device can reach: a caller that keeps its samples on the host spins on
        // the word instead of synchronising the stream -- the samples are there when it changes (system-scope release)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(done + pair, done_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if constexpr (HELD) {
        if (held) return;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = 2 * (lane + 64 * r);
        *reinterpret_cast<float2*>(os + n) = r < 3 ? acc[r + 1] : make_float2(0.0f, 0.0f);
    }
}
template <class FrameOf, class BeforeDone>
__device__ __forceinline__ void hop_wave_istft(float* ola_state, float* wave_out, const float* window, const float* enh_g, unsigned* done,
                                               unsigned* err, int F, int wg, int npair, unsigned tagw, unsigned done_value, char* smem,
                                               FrameOf frame_of, BeforeDone before_done) {
    hop_wave_istft_held<false>(ola_state, wave_out, window, enh_g, done, err, F, wg, npair, tagw, done_value, smem, frame_of, before_done,
                               [](int) { return false; });
}

// =====================================================================================================================
// Outer samples that differ from the model's (sfsn_stream_hop_io).  The two roles above are left as they are -- the plain hop's
// kernels compile to the code they were -- and restated below with the conversion in them; what is shared is shared by call:
// the transforms (sfsn_fft_dev.h), the granules, the filters and formats (sfsn_resample_dev.h).
// =====================================================================================================================
// the STFT role with outer samples at three times the model's rate: a decimator window per wave behind the exchange
#define HOP_WAVE_IO_WIN 480  // floats: [93 carried | 384 new] (477), padded
#define HOP_WAVE_LDS_STFT_IO (HOP_WAVE_LDS_STFT + (size_t)HOP_WAVES * HOP_WAVE_IO_WIN * 4)

// RATIO = outer rate / model rate (1 or 3), FMT = RS_F32 / RS_S16, the same format in and out; <1, RS_F32> is the plain hop above.
struct HopWaveIo {
    const void* wave_in;      // [B][128 RATIO] samples of format FMT
    void* wave_out;           // [B][S][128 RATIO]
    float* dec_state;         // [B][96]: the last 93 outer samples (RATIO 3)
    float* int_state;         // [B][S][32]: the last 31 enhanced samples at the model's rate (RATIO 3)
    const float* taps;        // [96]
    const float* phase_taps;  // [3][32]
};

// hop_wave_stft_held with outer samples: the wave that owns a clip reads the clip's outer samples and (RATIO 3) its carried 93
// into its own LDS window [HOP_WAVE_IO_WIN floats behind the exchange], a lane per output forms the 128 samples at the model's rate
// (sfsn_resample_dev.h: one accumulator chain per lane; lane l reads window[3 l + i], stride 3 over the 64 banks: no conflict), the
// frame is built from them as from wave_in, and the same wave moves the clip's state on: the frame as it stands IS the next state,
// and the window's last 93 samples the filter's.  A first call reads the filter state as zero; a held clip writes neither.
template <bool HELD, int RATIO, int FMT, class FirstCalls, class HeldClip>
__device__ __forceinline__ void hop_wave_stft_io(const float* wave_in, float* wave_state, const float* window, float* spec_g, int F, int b0,
                                                 int nclip, unsigned tagw, char* smem, const HopWaveIo& io, FirstCalls first_calls,
                                                 HeldClip held_clip) {
    static_assert(RATIO == 3 || (RATIO == 1 && FMT != RS_F32), "the plain hop is hop_wave_stft_held");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float2* unit = reinterpret_cast<float2*>(smem + 64);
    float2(*fbuf)[FFT_N] = reinterpret_cast<float2(*)[FFT_N]>(smem + 64 + FFT_NFFT * 8);
    fill_unit_table(unit, tid, HOP_THREADS);
    __syncthreads();
    const Twiddles tw = make_twiddles<false>(unit, lane);
    const unsigned long long first = first_calls(lane, nclip);
    float2 win[4], wk[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = 2 * (lane + 64 * r);
        win[r] = make_float2(window[n], window[n + 1]);
        wk[r] = unit_at<false>(unit, lane + 64 * r);
    }
    for (int ci = wave; ci < nclip; ci += HOP_WAVES) {
        const int b = b0 + ci;
        const float* ws = wave_state + (size_t)b * FFT_NFFT;
        const bool zero = (first >> ci) & 1ull;
        float2 v[4];
        float2 fresh_x[4];  // the frame before the window
        float* rw = reinterpret_cast<float*>(smem + HOP_WAVE_LDS_STFT) + wave * HOP_WAVE_IO_WIN;  // (RATIO 3)
        float2 mine = make_float2(0.0f, 0.0f);  // the new samples 2 lane, 2 lane + 1 at the model's rate
        if constexpr (RATIO == 3) {
            const float* dec = io.dec_state + (size_t)b * RS_DEC_ROW;
            for (int i = lane; i < RS_DEC_KEEP; i += 64) rw[i] = zero ? 0.0f : dec[i];
#pragma unroll
            for (int i = 0; i < 6; ++i) rw[RS_DEC_KEEP + lane + 64 * i] = rs_load<FMT>(io.wave_in, (size_t)b * 384 + lane + 64 * i);
            __builtin_amdgcn_wave_barrier();
            float y[2];  // outputs lane and lane + 64: two chains side by side (rs_down3_sum's bits)
            rs_down3_sums<2>(io.taps, y, [&](int n, int i) { return rw[3 * (lane + 64 * n) + i]; });
            __builtin_amdgcn_wave_barrier();
            rw[lane] = y[0];  // (window[0, 128) has been read by every lane; the filter's next state is window[384, 477))
            rw[lane + 64] = y[1];
            __builtin_amdgcn_wave_barrier();
            mine = make_float2(rw[2 * lane], rw[2 * lane + 1]);
        } else {
            mine = make_float2(rs_load<FMT>(io.wave_in, (size_t)b * 128 + 2 * lane), rs_load<FMT>(io.wave_in, (size_t)b * 128 + 2 * lane + 1));
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = 2 * (lane + 64 * r);  // sample j of the frame: state[128 + j] for j < 384, then the new samples
            const float2 x = j < 384 ? (zero ? make_float2(0.0f, 0.0f) : *reinterpret_cast<const float2*>(ws + 128 + j)) : mine;
            fresh_x[r] = x;
            v[r] = make_float2(x.x * win[r].x, x.y * win[r].y);
        }
        fft256<false>(v, fbuf[wave], lane, tw);
        float2 X[4], nyq = make_float2(0.0f, 0.0f);
        rfft512_split(v, fbuf[wave], lane, wk, X, nyq);
#pragma unroll
        for (int r = 0; r < 4; ++r) hop_put_cplx(spec_g + ((size_t)b * F + lane + 64 * r) * 4, X[r], tagw);
        if (lane == 0) hop_put_cplx(spec_g + ((size_t)b * F + FFT_N) * 4, nyq, tagw);
        // the state moves on by one hop, by the wave that owns the clip (every load of it was consumed above; a first call leaves
        // [0 x 384 | samples], as in the plain role)
        bool held = false;
        if constexpr (HELD) held = held_clip(ci);
        if (!held) {
#pragma unroll
            for (int r = 0; r < 4; ++r) *reinterpret_cast<float2*>(wave_state + (size_t)b * FFT_NFFT + 2 * (lane + 64 * r)) = fresh_x[r];
            if constexpr (RATIO == 3) {
                float* dec = io.dec_state + (size_t)b * RS_DEC_ROW;
                for (int i = lane; i < RS_DEC_ROW; i += 64) dec[i] = i < RS_DEC_KEEP ? rw[384 + i] : 0.0f;
            }
        }
        __builtin_amdgcn_wave_barrier();  // (the wave's next clip reuses the window)
    }
}

// hop_wave_istft_held with outer samples: the wave holds the 128 finished samples in `out`; it parks them behind the pair's carried
// 31 in its own spectrum row (free by then: [31 carried | 128 new] floats), runs the interpolator -- lane l takes the model-rate
// positions l and l + 64 with all three phases, one accumulator chain each, reading window[l + i] at stride 1 -- converts and stores
// the 384 (128) outer samples before the completion word, and writes the last 31 back.  The output is zero while the pair's frame index
// is < 2 (with or without clip_start: the interpolator must see the zeros the caller sees) and its carried samples are then zero too;
// a held pair stores zeros and leaves them.  No LDS beyond HOP_WAVE_LDS_ISTFT.
template <bool HELD, int RATIO, int FMT, class FrameOf, class BeforeDone, class HeldPair>
__device__ __forceinline__ void hop_wave_istft_io(float* ola_state, float* wave_out, const float* window, const float* enh_g, unsigned* done,
                                                  unsigned* err, int F, int wg, int npair, unsigned tagw, unsigned done_value, char* smem,
                                                  const HopWaveIo& io, FrameOf frame_of, BeforeDone before_done, HeldPair held_pair) {
    static_assert(RATIO == 3 || (RATIO == 1 && FMT != RS_F32), "the plain hop is hop_wave_istft_held");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pair = wg * HOP_WAVES + wave;  // clip * S + speaker
    float2* unit = reinterpret_cast<float2*>(smem + 64);
    float2(*fbuf)[FFT_N] = reinterpret_cast<float2(*)[FFT_N]>(smem + 64 + FFT_NFFT * 8);
    float2(*xs)[264] = reinterpret_cast<float2(*)[264]>(smem + 64 + FFT_NFFT * 8 + HOP_WAVES * FFT_N * 8);
    fill_unit_table(unit, tid, HOP_THREADS);
    __syncthreads();
    if (pair >= npair) return;
    const Twiddles tw = make_twiddles<true>(unit, lane);
    // the clip's own frame index (per-clip utterances): its accumulator reads as zero in the launch that restarts it, and its
    // output is zero until its frame 2 (calls 0 .. 2 of the utterance)
    int fi;
    bool fresh, mute;
    frame_of(pair, fi, fresh, mute);
    mute = mute || fi < 2;
    bool held = false;
    if constexpr (HELD) {
        held = held_pair(pair);
        mute = mute || held;
    }
    float2 win[4], wk[4], ola[4];
    float* os = ola_state + (size_t)pair * FFT_NFFT;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = 2 * (lane + 64 * r);
        win[r] = make_float2(window[n], window[n + 1]);
        wk[r] = unit_at<true>(unit, lane + 64 * r);
        ola[r] = make_float2(0.0f, 0.0f);
        if (!fresh) ola[r] = *reinterpret_cast<const float2*>(os + n);
    }
    bool ok = true;
    const float* eg = enh_g + (size_t)pair * F * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) xs[wave][lane + 64 * r] = hop_take_cplx(eg + (size_t)(lane + 64 * r) * 4, tagw, ok, err);
    if (lane == 0) xs[wave][FFT_N] = hop_take_cplx(eg + (size_t)FFT_N * 4, tagw, ok, err);
    __builtin_amdgcn_wave_barrier();
    float2 v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = lane + 64 * r;
        v[r] = irfft512_presplit(xs[wave][k], xs[wave][FFT_N - k], k, wk[r]);
    }
    fft256<true>(v, fbuf[wave], lane, tw);
    const float sc = 1.0f / (float)FFT_N;
    float2 acc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float2 res = make_float2(v[r].x * sc * win[r].x, v[r].y * sc * win[r].y);
        acc[r] = make_float2(ola[r].x + res.x, ola[r].y + res.y);
    }
    // the hop that is complete now: padded positions n = 128 t + 2 lane + e; envelope over the frames t - q that exist, oldest first
    float2 env = make_float2(0.0f, 0.0f);
#pragma unroll
    for (int q = 3; q >= 0; --q)
        if (fi - q >= 0) {
            env.x += win[q].x * win[q].x;
            env.y += win[q].y * win[q].y;
        }
    float2 out = make_float2(env.x > 1e-11f ? acc[0].x / env.x : 0.0f, env.y > 1e-11f ? acc[0].y / env.y : 0.0f);
    if (mute) out = make_float2(0.0f, 0.0f);
    float carry = 0.0f;  // (RATIO 3) lane l < 31: the pair's carried sample l after this hop
    if constexpr (RATIO == 3) {
        float* uw = reinterpret_cast<float*>(xs[wave]);
        float* ist = io.int_state + (size_t)pair * RS_INT_ROW;
        __builtin_amdgcn_wave_barrier();  // (every lane has read its bins of the row)
        if (lane < RS_INT_KEEP) uw[lane] = (fresh || mute) ? 0.0f : ist[lane];
        uw[RS_INT_KEEP + 2 * lane] = out.x;
        uw[RS_INT_KEEP + 2 * lane + 1] = out.y;
        __builtin_amdgcn_wave_barrier();
        float z[2][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};  // positions lane and lane + 64, three phases each (rs_up3_sum's bits)
        if (!mute) rs_up3_sums<2>(io.phase_taps, z, [&](int n, int i) { return uw[lane + 64 * n + i]; });
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int p = 0; p < 3; ++p) rs_store<FMT>(io.wave_out, (size_t)pair * 384 + 3 * (lane + 64 * h) + p, z[h][p]);
        if (lane < RS_INT_KEEP) carry = uw[128 + lane];
    } else {
        rs_store<FMT>(io.wave_out, (size_t)pair * 128 + 2 * lane, out.x);
        rs_store<FMT>(io.wave_out, (size_t)pair * 128 + 2 * lane + 1, out.y);
    }
    before_done(ok);
    if (done) {
        // wave_out (and this word) may be host memory the device can reach: a caller that keeps its samples on the host spins on
        // the word instead of synchronising the stream -- the samples are there when it changes (system-scope release)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(done + pair, done_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if constexpr (HELD) {
        if (held) return;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = 2 * (lane + 64 * r);
        *reinterpret_cast<float2*>(os + n) = r < 3 ? acc[r + 1] : make_float2(0.0f, 0.0f);
    }
    if constexpr (RATIO == 3) {
        if (lane < RS_INT_ROW) io.int_state[(size_t)pair * RS_INT_ROW + lane] = carry;  // (word 31: padding, zero)
    }
}

#endif
