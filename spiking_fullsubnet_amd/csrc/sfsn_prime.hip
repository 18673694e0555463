// sfsn_prime.hip -- sfsn_hop_prime: the state of the one-launch streaming hop (sfsn_hop.hip) after a recorded prefix, written in
// ONE launch from what the offline forward of that prefix left behind (gfx950 only).
//
// A session that has streamed N frames of a clip holds: every layer's last spikes (double-buffered by launch parity) and membrane,
// the running sums of the cumulative norm, the last D noisy frames, the spike counts per lane slot and, in waveform mode, the last
// 512 input samples and the overlap-add partial sums of the positions not yet emitted.  All of it is a function of the prefix, and
// the offline forward computes the same bits (include/sfsn.h, sfsn_stream_hop) -- so the launch below copies / re-derives it for
// the listed clips and leaves every other clip's rows alone:
//   * rows role, one section per (sequence, layer): lane (row, j) owns the 4 neurons 4j .. 4j + 3 of a row, as in the hop -- the
//     last frame's spike word into h[launch & 1], the membrane's float4, the slot's count (popcounts of its word over the N frames:
//     the very numbers the hop's lane would have added, one per launch), and for layer 0 the row's running sum into cum[launch & 1]
//     (cumlap_scan_kernel and the hop add the same row sums in the same order: sfsn_kernels.hip / hop_layer_role);
//   * hist role: the last D noisy frames of the bins the groups cover (the hop keeps no history of the pass-through bins);
//   * wave role: the last 512 samples;
//   * ola role: a wave per (clip, speaker) runs hop_wave_istft's recurrence over the last three frames of the enhanced prefix
//     (acc = ola + frame, ola = acc moved on by one hop) with sfsn_fft_dev.h's transform: the same instructions in the same
//     (ascending frame) order, hence the hop's bits.  Earlier frames have left the accumulator by then.
// Plain stores only: the launch boundary publishes them.  The tagged scratch of the hop (spikes, spec_g, enh_g) is not touched and
// launch_index does not move, so its tags stay what the next launch expects.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "sfsn.h"

#include "sfsn_fft_dev.h"
#include "sfsn_host.h"

#define PRIME_THREADS 256
#define PRIME_WAVES 4
#define PRIME_MAX_SEQS (1 + SFSN_HOP_MAX_GROUPS)
#define PRIME_MAX_CLIPS 256  // clip indices travel in the kernel arguments (16 bits each)
// layers of a sequence: sfsn_hop_desc's, or the one sequence of a sfsn_fullband_hop_desc
#define PRIME_MAX_LAYERS (SFSN_HOP_MAX_LAYERS > SFSN_FULLBAND_HOP_MAX_LAYERS ? SFSN_HOP_MAX_LAYERS : SFSN_FULLBAND_HOP_MAX_LAYERS)
#define PRIME_MAX_SECS (PRIME_MAX_SEQS * SFSN_HOP_MAX_LAYERS + 3)
static_assert(PRIME_MAX_SECS >= SFSN_FULLBAND_HOP_MAX_LAYERS + 3, "a cIRM-GSN descriptor's sections fit");

enum { PRIME_ROWS = 0, PRIME_HIST = 1, PRIME_WAVE = 2, PRIME_OLA = 3 };

struct PrimeLayerDev {
    int8_t* h;          // the half of the double buffer the next launch reads
    float* c;
    unsigned* slots;    // this layer's [R][H / 4] slots, or NULL
    const int8_t* s8;   // [N][Bp * units][HP]
    const float* csrc;  // [Bp * units][H]
};
struct PrimeSeqDev {
    PrimeLayerDev layer[PRIME_MAX_LAYERS];
    float* cum;  // the half the next launch reads, or NULL
    const float* cum_src;
    int H, HP, units;
};
struct PrimeSecDev {
    int kind, seq, layer, blk0, items;
};
struct PrimeParams {
    PrimeSeqDev seq[PRIME_MAX_SEQS];
    PrimeSecDev sec[PRIME_MAX_SECS];
    unsigned short clips[PRIME_MAX_CLIPS];
    int nsec, n_clips, b0, Bp, N;
    int F, S, D, fcov;
    const float* stft;  // [Bp][F][N][2]
    const float* enh;   // [Bp][S][F][N][2]
    const float* tail;  // [Bp][512]
    float* hist;
    float* wave_state;
    float* ola_state;
    const float* window;
};
static_assert(sizeof(PrimeParams) <= 4096, "PrimeParams travels as a kernel argument");

__device__ __forceinline__ void prime_rows(const PrimeParams& p, const PrimeSecDev& sd, int item) {
    const PrimeSeqDev& sq = p.seq[sd.seq];
    const PrimeLayerDev& L = sq.layer[sd.layer];
    const int W = sq.H >> 2, N = p.N;
    const int j = item % W, rr = item / W;
    const int k = rr % sq.units, i = rr / sq.units;
    const size_t Rs = (size_t)p.Bp * sq.units;
    const size_t row_s = (size_t)(p.b0 + i) * sq.units + k, row_d = (size_t)p.clips[i] * sq.units + k;
    const int8_t* sp = L.s8 + row_s * sq.HP + 4 * j;  // my word of frame 0; a frame further every Rs * HP bytes
    const size_t fs = Rs * sq.HP;
    unsigned last = 0u, nspk = 0u;
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (N > 0) {
        last = *reinterpret_cast<const unsigned*>(sp + (size_t)(N - 1) * fs) & 0x01010101u;
        c = *reinterpret_cast<const float4*>(L.csrc + row_s * sq.H + 4 * j);
    }
    *reinterpret_cast<unsigned*>(L.h + row_d * sq.HP + 4 * j) = last;
    *reinterpret_cast<float4*>(L.c + row_d * sq.H + 4 * j) = c;
    if (sd.layer == 0 && j == 0 && sq.cum) sq.cum[row_d] = N > 0 ? sq.cum_src[row_s] : 0.0f;
    if (!L.slots) return;
    for (int t0 = 0; t0 < N; t0 += 8) {  // eight independent loads in flight
        unsigned w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) w[u] = *reinterpret_cast<const unsigned*>(sp + (size_t)(t0 + u < N ? t0 + u : N - 1) * fs);
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (t0 + u < N) nspk += __builtin_popcount(w[u] & 0x01010101u);
    }
    L.slots[row_d * W + j] = nspk;  // (replaces the slot: the clip's utterance begins with the prefix)
}

__device__ __forceinline__ void prime_hist(const PrimeParams& p, int item) {
    const int D = p.D, N = p.N;
    const int d = item % D, r = item / D;
    const int f = r % p.fcov, i = r / p.fcov;
    const int t = N - D + d;  // frames before the prefix's first read as zero, as a fresh session's history does
    float2 v = make_float2(0.0f, 0.0f);
    if (t >= 0) v = *reinterpret_cast<const float2*>(p.stft + (((size_t)(p.b0 + i) * p.F + f) * N + t) * 2);
    *reinterpret_cast<float2*>(p.hist + (((size_t)p.clips[i] * p.F + f) * D + d) * 2) = v;
}

__device__ __forceinline__ void prime_wave(const PrimeParams& p, int item) {
    const int n = item & (FFT_NFFT - 1), i = item >> 9;
    p.wave_state[(size_t)p.clips[i] * FFT_NFFT + n] = p.tail[(size_t)(p.b0 + i) * FFT_NFFT + n];
}

// hop_wave_istft's arithmetic (sfsn_hop_wave_dev.h), frame after frame, without its hand-off and its output
__device__ __forceinline__ void prime_ola(const PrimeParams& p, int blk, char* smem) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float2* unit = reinterpret_cast<float2*>(smem);
    float2(*fbuf)[FFT_N] = reinterpret_cast<float2(*)[FFT_N]>(smem + FFT_NFFT * 8);
    float2(*xs)[264] = reinterpret_cast<float2(*)[264]>(smem + FFT_NFFT * 8 + PRIME_WAVES * FFT_N * 8);
    fill_unit_table(unit, tid, PRIME_THREADS);
    __syncthreads();
    const int pair = blk * PRIME_WAVES + wave;
    if (pair >= p.n_clips * p.S) return;
    const int i = pair / p.S, s = pair - i * p.S, N = p.N, F = p.F;
    const Twiddles tw = make_twiddles<true>(unit, lane);
    float2 win[4], wk[4], ola[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = 2 * (lane + 64 * r);
        win[r] = make_float2(p.window[n], p.window[n + 1]);
        wk[r] = unit_at<true>(unit, lane + 64 * r);
        ola[r] = make_float2(0.0f, 0.0f);
    }
    const float* eg = p.enh + ((size_t)(p.b0 + i) * p.S + s) * F * N * 2;
    const float sc = 1.0f / (float)FFT_N;
    for (int t = N > 3 ? N - 3 : 0; t < N; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) xs[wave][lane + 64 * r] = *reinterpret_cast<const float2*>(eg + ((size_t)(lane + 64 * r) * N + t) * 2);
        if (lane == 0) xs[wave][FFT_N] = *reinterpret_cast<const float2*>(eg + ((size_t)FFT_N * N + t) * 2);
        __builtin_amdgcn_wave_barrier();
        float2 v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = lane + 64 * r;
            v[r] = irfft512_presplit(xs[wave][k], xs[wave][FFT_N - k], k, wk[r]);
        }
        fft256<true>(v, fbuf[wave], lane, tw);
        float2 acc[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float2 res = make_float2(v[r].x * sc * win[r].x, v[r].y * sc * win[r].y);
            acc[r] = make_float2(ola[r].x + res.x, ola[r].y + res.y);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) ola[r] = r < 3 ? acc[r + 1] : make_float2(0.0f, 0.0f);
        __builtin_amdgcn_wave_barrier();  // (this frame's reads of xs / fbuf before the next frame's writes)
    }
    float* os = p.ola_state + ((size_t)p.clips[i] * p.S + s) * FFT_NFFT;
#pragma unroll
    for (int r = 0; r < 4; ++r) *reinterpret_cast<float2*>(os + 2 * (lane + 64 * r)) = ola[r];
}

__global__ __launch_bounds__(PRIME_THREADS) void hop_prime_kernel(const PrimeParams p) {
    __shared__ __attribute__((aligned(16))) char smem[FFT_NFFT * 8 + PRIME_WAVES * FFT_N * 8 + PRIME_WAVES * 264 * 8];
    int si = 0;
    for (int i = 1; i < p.nsec; ++i)
        if ((int)blockIdx.x >= p.sec[i].blk0) si = i;  // (block-uniform: sections are in block order)
    const PrimeSecDev& sd = p.sec[si];
    const int blk = (int)blockIdx.x - sd.blk0;
    if (sd.kind == PRIME_OLA) {
        prime_ola(p, blk, smem);
        return;
    }
    const int item = blk * PRIME_THREADS + (int)threadIdx.x;
    if (item >= sd.items) return;
    if (sd.kind == PRIME_ROWS)
        prime_rows(p, sd, item);
    else if (sd.kind == PRIME_HIST)
        prime_hist(p, item);
    else
        prime_wave(p, item);
}

// =====================================================================================================================
// host side
// =====================================================================================================================
static inline bool aligned4(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3u) == 0; }

extern "C" int sfsn_hop_prime(const sfsn_hop_desc* desc, const int* clips, int n_clips, const sfsn_prime_src* src, void* stream) {
    if (!desc || !clips || !src || n_clips <= 0) return SFSN_EINVAL;
    // the descriptor is one sfsn_stream_hop would run (its plan validates the geometry and every state pointer)
    if (desc->n_groups < 1 || desc->n_groups > SFSN_HOP_MAX_GROUPS) return SFSN_EUNSUPPORTED;
    if (sfsn_hop_spike_slots(desc) == 0) return SFSN_EUNSUPPORTED;
    const bool wave = desc->wave_in != nullptr;
    const int N = src->N, B = desc->B, D = desc->D;
    if (N < 0 || (!wave && N < desc->hop) || N % desc->hop != 0) return SFSN_EINVAL;
    if (src->Bp < 1 || src->b0 < 0 || n_clips > src->Bp - src->b0) return SFSN_EINVAL;
    if (B > 65535) return SFSN_EUNSUPPORTED;
    if (n_clips > PRIME_MAX_CLIPS) return SFSN_EUNSUPPORTED;  // (the caller primes them in several calls)
    PrimeParams p;
    memset(&p, 0, sizeof(p));
    for (int i = 0; i < n_clips; ++i) {
        if (clips[i] < 0 || clips[i] >= B) return SFSN_EINVAL;
        for (int j = 0; j < i; ++j)
            if (clips[j] == clips[i]) return SFSN_EINVAL;  // (two lanes would own one row)
        p.clips[i] = (unsigned short)clips[i];
    }
    if (N > 0 && D > 0 && (!src->stft_ri || (reinterpret_cast<uintptr_t>(src->stft_ri) & 7u))) return SFSN_EINVAL;
    if (wave && (!src->wave_tail || !aligned4(src->wave_tail) || (N > 0 && (!src->enh_ri || (reinterpret_cast<uintptr_t>(src->enh_ri) & 7u)))))
        return SFSN_EINVAL;
    const unsigned par = desc->launch_index & 1u;
    p.n_clips = n_clips; p.b0 = src->b0; p.Bp = src->Bp; p.N = N;
    p.F = desc->F; p.S = desc->S; p.D = D;
    p.stft = src->stft_ri; p.enh = src->enh_ri; p.tail = src->wave_tail;
    p.hist = desc->hist_ri; p.wave_state = desc->wave_state; p.ola_state = desc->ola_state; p.window = desc->window;
    int nsec = 0, blk = 0, fcov = 0;
    size_t slot0 = 0;
    auto add = [&](int kind, int seq, int layer, int items, int per_block) {
        PrimeSecDev& s = p.sec[nsec++];
        s.kind = kind; s.seq = seq; s.layer = layer; s.blk0 = blk; s.items = items;
        blk += (items + per_block - 1) / per_block;
    };
    for (int q = 0; q < 1 + desc->n_groups; ++q) {
        const sfsn_hop_seq& hs = q == 0 ? desc->fb : desc->sb[q - 1];
        const sfsn_prime_seq& ps = q == 0 ? src->fb : src->sb[q - 1];
        PrimeSeqDev& d = p.seq[q];
        d.H = hs.H; d.HP = (hs.H + 63) / 64 * 64; d.units = hs.feat.n_units;
        const size_t R = (size_t)B * d.units;
        if (q > 0 && hs.feat.lo + d.units * hs.fc > fcov) fcov = hs.feat.lo + d.units * hs.fc;
        if (hs.feat.norm == SFSN_NORM_CUMLAPLACE) {
            if (N > 0 && (!ps.cum || !aligned4(ps.cum))) return SFSN_EINVAL;
            d.cum = hs.cum[par]; d.cum_src = ps.cum;
        }
        for (int l = 0; l < hs.n_layers; ++l) {
            PrimeLayerDev& o = d.layer[l];
            if (N > 0 && (!ps.layer[l].spikes_i8 || !ps.layer[l].c || !aligned4(ps.layer[l].spikes_i8) || !aligned16(ps.layer[l].c))) return SFSN_EINVAL;
            if (!aligned4(hs.layer[l].h[par]) || !aligned16(hs.layer[l].c)) return SFSN_EINVAL;
            o.h = hs.layer[l].h[par]; o.c = hs.layer[l].c; o.s8 = ps.layer[l].spikes_i8; o.csrc = ps.layer[l].c;
            o.slots = desc->spike_slots ? desc->spike_slots + slot0 : nullptr;
            slot0 += R * (hs.H / 4);
            add(PRIME_ROWS, q, l, n_clips * d.units * (hs.H / 4), PRIME_THREADS);
        }
    }
    p.fcov = fcov;
    if (D > 0 && fcov > 0) add(PRIME_HIST, 0, 0, n_clips * fcov * D, PRIME_THREADS);
    if (wave) {
        add(PRIME_WAVE, 0, 0, n_clips * FFT_NFFT, PRIME_THREADS);
        add(PRIME_OLA, 0, 0, n_clips * desc->S, PRIME_WAVES);
    }
    p.nsec = nsec;
    hipLaunchKernelGGL(hop_prime_kernel, dim3(blk), dim3(PRIME_THREADS), 0, static_cast<hipStream_t>(stream), p);
    return hip_ok(hipGetLastError());
}

// =====================================================================================================================
// A backlog on a clip that is ALREADY RUNNING (sfsn_hop_seed / sfsn_hop_advance, include/sfsn.h): the way out of a session into the
// offline kernels and the way back.  The seed launch writes what the offline kernels start from -- (h, c) as they take them (fp32
// 0/1 spikes, membranes), the running sums, the D frames of history in front of the new frames and, in waveform mode, the 384 samples
// the next frame begins with -- for the listed clips; a clip whose origin is this launch index reads as zero, as it does in the hop.
// The advance launch is sfsn_hop_prime's continuing form: the end state into the session, the slots ADDED to, the history taken from
// the [history | new] buffer, the overlap-add accumulator continued over every new frame with the c output blocks written.
// Plain loads and stores; nothing waits.
// =====================================================================================================================
enum { SEED_ROWS = 0, SEED_HIST = 1, SEED_WAVE = 2 };
#define SEED_CTX 384  // samples of wave_state the next frame begins with

struct SeedLayerDev {
    const int8_t* h;  // the half of the double buffer the next launch reads
    const float* c;
    float* hd;        // [Bp * units][H] fp32 0/1
    float* cd;        // [Bp * units][H]
};
struct SeedSeqDev {
    SeedLayerDev layer[PRIME_MAX_LAYERS];
    const float* cum;  // the half the next launch reads, or NULL
    float* cum_d;
    int H, HP, units;
};
struct SeedParams {
    SeedSeqDev seq[PRIME_MAX_SEQS];
    PrimeSecDev sec[PRIME_MAX_SECS];
    unsigned short clips[PRIME_MAX_CLIPS];
    int nsec, n_clips, b0, T;
    int F, D, fcov, ctx_stride;
    unsigned k, span;  // span: origins k .. k + span read as zero (0; the cIRM-GSN waveform hop: 1, the clip without a call)
    const unsigned* clip_start;
    const float* hist;
    const float* wave_state;
    float* stft;  // [Bp][F][T][2]
    float* ctx;   // [Bp][ctx_stride]
};
static_assert(sizeof(SeedParams) <= 4096, "SeedParams travels as a kernel argument");

__device__ __forceinline__ bool clip_fresh(const unsigned* clip_start, unsigned k, unsigned span, int clip) {
    return clip_start && clip_start[clip] - k <= span;  // (unsigned, wrap-safe)
}

__device__ __forceinline__ void seed_rows(const SeedParams& p, const PrimeSecDev& sd, int item) {
    const SeedSeqDev& sq = p.seq[sd.seq];
    const SeedLayerDev& L = sq.layer[sd.layer];
    const int W = sq.H >> 2;
    const int j = item % W, rr = item / W;
    const int k = rr % sq.units, i = rr / sq.units;
    const size_t row_s = (size_t)p.clips[i] * sq.units + k, row_d = (size_t)(p.b0 + i) * sq.units + k;
    const bool fresh = clip_fresh(p.clip_start, p.k, p.span, p.clips[i]);
    float4 h = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c = h;
    float cum = 0.0f;
    if (!fresh) {
        const unsigned w = *reinterpret_cast<const unsigned*>(L.h + row_s * sq.HP + 4 * j);
        h = make_float4((float)(w & 1u), (float)((w >> 8) & 1u), (float)((w >> 16) & 1u), (float)((w >> 24) & 1u));
        c = *reinterpret_cast<const float4*>(L.c + row_s * sq.H + 4 * j);
        if (sd.layer == 0 && j == 0 && sq.cum) cum = sq.cum[row_s];
    }
    *reinterpret_cast<float4*>(L.hd + row_d * sq.H + 4 * j) = h;
    *reinterpret_cast<float4*>(L.cd + row_d * sq.H + 4 * j) = c;
    if (sd.layer == 0 && j == 0 && sq.cum) sq.cum_d[row_d] = cum;
}

__device__ __forceinline__ void seed_hist(const SeedParams& p, int item) {
    const int D = p.D;
    const int d = item % D, r = item / D;
    const int f = r % p.F, i = r / p.F;
    float2 v = make_float2(0.0f, 0.0f);  // (the hop keeps no history of the bins no group covers: nobody reads theirs)
    if (f < p.fcov && !clip_fresh(p.clip_start, p.k, p.span, p.clips[i]))
        v = *reinterpret_cast<const float2*>(p.hist + (((size_t)p.clips[i] * p.F + f) * D + d) * 2);
    *reinterpret_cast<float2*>(p.stft + (((size_t)(p.b0 + i) * p.F + f) * p.T + d) * 2) = v;
}

__device__ __forceinline__ void seed_wave(const SeedParams& p, int item) {
    const int n = item % SEED_CTX, i = item / SEED_CTX;
    // (span: a clip whose origin is the launch after this one has made no call yet -- its old samples read as zero)
    const bool nocall = p.span && p.clip_start[p.clips[i]] - p.k == 1u;
    p.ctx[(size_t)(p.b0 + i) * p.ctx_stride + n] = nocall ? 0.0f : p.wave_state[(size_t)p.clips[i] * FFT_NFFT + (FFT_NFFT - SEED_CTX) + n];
}

__global__ __launch_bounds__(PRIME_THREADS) void hop_seed_kernel(const SeedParams p) {
    int si = 0;
    for (int i = 1; i < p.nsec; ++i)
        if ((int)blockIdx.x >= p.sec[i].blk0) si = i;  // (block-uniform: sections are in block order)
    const PrimeSecDev& sd = p.sec[si];
    const int item = ((int)blockIdx.x - sd.blk0) * PRIME_THREADS + (int)threadIdx.x;
    if (item >= sd.items) return;
    if (sd.kind == SEED_ROWS)
        seed_rows(p, sd, item);
    else if (sd.kind == SEED_HIST)
        seed_hist(p, item);
    else
        seed_wave(p, item);
}

struct AdvParams {
    PrimeParams base;  // (stft / enh: rows of T frames, the new ones last; s8 / csrc / cum_src: of the N new frames)
    int T, frame_index;
    unsigned k, span;  // span: as in SeedParams
    const unsigned* clip_start;
    float* wave_out;  // [Bp][S][128 * N]
};
static_assert(sizeof(AdvParams) <= 4096, "AdvParams travels as a kernel argument");

__device__ __forceinline__ void adv_rows(const AdvParams& a, const PrimeSecDev& sd, int item) {
    const PrimeParams& p = a.base;
    const PrimeSeqDev& sq = p.seq[sd.seq];
    const PrimeLayerDev& L = sq.layer[sd.layer];
    const int W = sq.H >> 2, N = p.N;
    const int j = item % W, rr = item / W;
    const int k = rr % sq.units, i = rr / sq.units;
    const size_t Rs = (size_t)p.Bp * sq.units;
    const size_t row_s = (size_t)(p.b0 + i) * sq.units + k, row_d = (size_t)p.clips[i] * sq.units + k;
    const int8_t* sp = L.s8 + row_s * sq.HP + 4 * j;  // my word of the first new frame; a frame further every Rs * HP bytes
    const size_t fs = Rs * sq.HP;
    if (N == 0) {  // (the cIRM-GSN waveform clip whose one call has made no frame: zeros, which its frame 0 reads anyway)
        *reinterpret_cast<unsigned*>(L.h + row_d * sq.HP + 4 * j) = 0u;
        *reinterpret_cast<float4*>(L.c + row_d * sq.H + 4 * j) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    *reinterpret_cast<unsigned*>(L.h + row_d * sq.HP + 4 * j) = *reinterpret_cast<const unsigned*>(sp + (size_t)(N - 1) * fs) & 0x01010101u;
    *reinterpret_cast<float4*>(L.c + row_d * sq.H + 4 * j) = *reinterpret_cast<const float4*>(L.csrc + row_s * sq.H + 4 * j);
    if (sd.layer == 0 && j == 0 && sq.cum) sq.cum[row_d] = sq.cum_src[row_s];
    if (!L.slots) return;
    // (the clip's utterance goes on: its slot is added to -- unless it begins here, where the hop reads the slot as zero)
    unsigned nspk = clip_fresh(a.clip_start, a.k, a.span, p.clips[i]) ? 0u : L.slots[row_d * W + j];
    for (int t0 = 0; t0 < N; t0 += 8) {  // eight independent loads in flight
        unsigned w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) w[u] = *reinterpret_cast<const unsigned*>(sp + (size_t)(t0 + u < N ? t0 + u : N - 1) * fs);
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (t0 + u < N) nspk += __builtin_popcount(w[u] & 0x01010101u);
    }
    L.slots[row_d * W + j] = nspk;
}

__device__ __forceinline__ void adv_hist(const AdvParams& a, int item) {
    const PrimeParams& p = a.base;
    const int D = p.D, T = a.T;
    const int d = item % D, r = item / D;
    const int f = r % p.fcov, i = r / p.fcov;
    // the last D frames of [history | new] (T >= D + N: N < D keeps the tail of the old history, which the seed launch wrote there)
    float2 v = make_float2(0.0f, 0.0f);  // (N == 0: see adv_rows)
    if (p.N > 0) v = *reinterpret_cast<const float2*>(p.stft + (((size_t)(p.b0 + i) * p.F + f) * T + (T - D + d)) * 2);
    *reinterpret_cast<float2*>(p.hist + (((size_t)p.clips[i] * p.F + f) * D + d) * 2) = v;
}

// hop_wave_istft's arithmetic (sfsn_hop_wave_dev.h) over the N new frames, from the clip's carried accumulator: old partial sums
// first, then the new frames in ascending order, each completed hop divided by the envelope of the frames that exist
__device__ __forceinline__ void adv_ola(const AdvParams& a, int blk, char* smem) {
    const PrimeParams& p = a.base;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float2* unit = reinterpret_cast<float2*>(smem);
    float2(*fbuf)[FFT_N] = reinterpret_cast<float2(*)[FFT_N]>(smem + FFT_NFFT * 8);
    float2(*xs)[264] = reinterpret_cast<float2(*)[264]>(smem + FFT_NFFT * 8 + PRIME_WAVES * FFT_N * 8);
    fill_unit_table(unit, tid, PRIME_THREADS);
    __syncthreads();
    const int pair = blk * PRIME_WAVES + wave;
    if (pair >= p.n_clips * p.S) return;
    const int i = pair / p.S, s = pair - i * p.S, N = p.N, F = p.F, T = a.T;
    const int clip = p.clips[i];
    // the frame index of the first new frame; a clip that begins here carries no sums (span 1: also the clip whose first call, which
    // has no frame, is launch k -- age -1 -- and whose frame 0 is the first new frame)
    const int age = a.clip_start ? (int)(a.k - a.clip_start[clip]) : a.frame_index;
    const bool fresh = a.clip_start && age <= 0 && age >= -(int)a.span;
    const int fi0 = fresh ? 0 : age;
    const Twiddles tw = make_twiddles<true>(unit, lane);
    float* os = p.ola_state + ((size_t)clip * p.S + s) * FFT_NFFT;
    float2 win[4], wk[4], ola[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = 2 * (lane + 64 * r);
        win[r] = make_float2(p.window[n], p.window[n + 1]);
        wk[r] = unit_at<true>(unit, lane + 64 * r);
        ola[r] = make_float2(0.0f, 0.0f);
        if (!fresh) ola[r] = *reinterpret_cast<const float2*>(os + n);
    }
    const float* eg = p.enh + ((size_t)(p.b0 + i) * p.S + s) * F * T * 2 + (size_t)(T - N) * 2;
    float* wo = a.wave_out + ((size_t)(p.b0 + i) * p.S + s) * 128 * N;
    const float sc = 1.0f / (float)FFT_N;
    for (int t = 0; t < N; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) xs[wave][lane + 64 * r] = *reinterpret_cast<const float2*>(eg + ((size_t)(lane + 64 * r) * T + t) * 2);
        if (lane == 0) xs[wave][FFT_N] = *reinterpret_cast<const float2*>(eg + ((size_t)FFT_N * T + t) * 2);
        __builtin_amdgcn_wave_barrier();
        float2 v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = lane + 64 * r;
            v[r] = irfft512_presplit(xs[wave][k], xs[wave][FFT_N - k], k, wk[r]);
        }
        fft256<true>(v, fbuf[wave], lane, tw);
        float2 acc[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float2 res = make_float2(v[r].x * sc * win[r].x, v[r].y * sc * win[r].y);
            acc[r] = make_float2(ola[r].x + res.x, ola[r].y + res.y);
        }
        const int fi = fi0 + t;
        float2 env = make_float2(0.0f, 0.0f);
#pragma unroll
        for (int q = 3; q >= 0; --q)
            if (fi - q >= 0) {
                env.x += win[q].x * win[q].x;
                env.y += win[q].y * win[q].y;
            }
        float2 out = make_float2(env.x > 1e-11f ? acc[0].x / env.x : 0.0f, env.y > 1e-11f ? acc[0].y / env.y : 0.0f);
        if (fi < 2) out = make_float2(0.0f, 0.0f);  // (the part torch.istft trims)
        *reinterpret_cast<float2*>(wo + (size_t)128 * t + 2 * lane) = out;
#pragma unroll
        for (int r = 0; r < 4; ++r) ola[r] = r < 3 ? acc[r + 1] : make_float2(0.0f, 0.0f);
        __builtin_amdgcn_wave_barrier();  // (this frame's reads of xs / fbuf before the next frame's writes)
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) *reinterpret_cast<float2*>(os + 2 * (lane + 64 * r)) = ola[r];
}

__global__ __launch_bounds__(PRIME_THREADS) void hop_advance_kernel(const AdvParams a) {
    __shared__ __attribute__((aligned(16))) char smem[FFT_NFFT * 8 + PRIME_WAVES * FFT_N * 8 + PRIME_WAVES * 264 * 8];
    const PrimeParams& p = a.base;
    int si = 0;
    for (int i = 1; i < p.nsec; ++i)
        if ((int)blockIdx.x >= p.sec[i].blk0) si = i;  // (block-uniform: sections are in block order)
    const PrimeSecDev& sd = p.sec[si];
    const int blk = (int)blockIdx.x - sd.blk0;
    if (sd.kind == PRIME_OLA) {
        adv_ola(a, blk, smem);
        return;
    }
    const int item = blk * PRIME_THREADS + (int)threadIdx.x;
    if (item >= sd.items) return;
    if (sd.kind == PRIME_ROWS)
        adv_rows(a, sd, item);
    else if (sd.kind == PRIME_HIST)
        adv_hist(a, item);
    else
        prime_wave(p, item);
}

static inline bool aligned8(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7u) == 0; }

// what both entry points ask of the descriptor and the clip list; the clips go into `out`
static int check_clip_list(const sfsn_hop_desc* desc, const int* clips, int n_clips, unsigned short* out) {
    if (!desc || !clips || n_clips <= 0) return SFSN_EINVAL;
    if (desc->n_groups < 1 || desc->n_groups > SFSN_HOP_MAX_GROUPS) return SFSN_EUNSUPPORTED;
    if (sfsn_hop_spike_slots(desc) == 0) return SFSN_EUNSUPPORTED;
    if (desc->B > 65535 || n_clips > PRIME_MAX_CLIPS) return SFSN_EUNSUPPORTED;
    for (int i = 0; i < n_clips; ++i) {
        if (clips[i] < 0 || clips[i] >= desc->B) return SFSN_EINVAL;
        for (int j = 0; j < i; ++j)
            if (clips[j] == clips[i]) return SFSN_EINVAL;  // (two lanes would own one row)
        out[i] = (unsigned short)clips[i];
    }
    return SFSN_OK;
}

extern "C" int sfsn_hop_seed(const sfsn_hop_desc* desc, const int* clips, int n_clips, const sfsn_seed_dst* dst, void* stream) {
    if (!dst) return SFSN_EINVAL;
    SeedParams p;
    memset(&p, 0, sizeof(p));
    const int rc = check_clip_list(desc, clips, n_clips, p.clips);
    if (rc != SFSN_OK) return rc;
    const bool wave = desc->wave_in != nullptr;
    const int D = desc->D;
    if (dst->Bp < 1 || dst->b0 < 0 || n_clips > dst->Bp - dst->b0) return SFSN_EINVAL;
    if (D > 0 && (dst->T < D || !dst->stft_ri || !aligned8(dst->stft_ri) || !desc->hist_ri || !aligned8(desc->hist_ri))) return SFSN_EINVAL;
    if (wave && (!dst->wave_ctx || !aligned4(dst->wave_ctx) || dst->wave_stride < SEED_CTX || !desc->wave_state || !aligned4(desc->wave_state)))
        return SFSN_EINVAL;
    const unsigned par = desc->launch_index & 1u;
    p.n_clips = n_clips; p.b0 = dst->b0; p.T = dst->T; p.F = desc->F; p.D = D; p.ctx_stride = dst->wave_stride;
    p.k = desc->launch_index; p.clip_start = desc->clip_start;
    p.hist = desc->hist_ri; p.wave_state = desc->wave_state; p.stft = dst->stft_ri; p.ctx = dst->wave_ctx;
    int nsec = 0, blk = 0, fcov = 0;
    auto add = [&](int kind, int seq, int layer, int items) {
        PrimeSecDev& s = p.sec[nsec++];
        s.kind = kind; s.seq = seq; s.layer = layer; s.blk0 = blk; s.items = items;
        blk += (items + PRIME_THREADS - 1) / PRIME_THREADS;
    };
    for (int q = 0; q < 1 + desc->n_groups; ++q) {
        const sfsn_hop_seq& hs = q == 0 ? desc->fb : desc->sb[q - 1];
        const sfsn_seed_seq& ds = q == 0 ? dst->fb : dst->sb[q - 1];
        SeedSeqDev& d = p.seq[q];
        d.H = hs.H; d.HP = (hs.H + 63) / 64 * 64; d.units = hs.feat.n_units;
        if (q > 0 && hs.feat.lo + d.units * hs.fc > fcov) fcov = hs.feat.lo + d.units * hs.fc;
        if (hs.feat.norm == SFSN_NORM_CUMLAPLACE) {
            if (!ds.cum || !aligned4(ds.cum) || !hs.cum[par] || !aligned4(hs.cum[par])) return SFSN_EINVAL;
            d.cum = hs.cum[par]; d.cum_d = ds.cum;
        }
        for (int l = 0; l < hs.n_layers; ++l) {
            SeedLayerDev& o = d.layer[l];
            if (!ds.layer[l].h || !ds.layer[l].c || !aligned16(ds.layer[l].h) || !aligned16(ds.layer[l].c)) return SFSN_EINVAL;
            if (!hs.layer[l].h[par] || !hs.layer[l].c || !aligned4(hs.layer[l].h[par]) || !aligned16(hs.layer[l].c)) return SFSN_EINVAL;
            o.h = hs.layer[l].h[par]; o.c = hs.layer[l].c; o.hd = ds.layer[l].h; o.cd = ds.layer[l].c;
            add(SEED_ROWS, q, l, n_clips * d.units * (hs.H / 4));
        }
    }
    p.fcov = fcov;
    if (D > 0) add(SEED_HIST, 0, 0, n_clips * desc->F * D);
    if (wave) add(SEED_WAVE, 0, 0, n_clips * SEED_CTX);
    p.nsec = nsec;
    hipLaunchKernelGGL(hop_seed_kernel, dim3(blk), dim3(PRIME_THREADS), 0, static_cast<hipStream_t>(stream), p);
    return hip_ok(hipGetLastError());
}

extern "C" int sfsn_hop_advance(const sfsn_hop_desc* desc, const int* clips, int n_clips, const sfsn_advance_src* src, void* stream) {
    if (!src) return SFSN_EINVAL;
    AdvParams a;
    memset(&a, 0, sizeof(a));
    PrimeParams& p = a.base;
    const int rc = check_clip_list(desc, clips, n_clips, p.clips);
    if (rc != SFSN_OK) return rc;
    const bool wave = desc->wave_in != nullptr;
    const int N = src->N, T = src->T, B = desc->B, D = desc->D;
    if (N < desc->hop || N % desc->hop != 0 || T < N + D) return SFSN_EINVAL;
    if (src->Bp < 1 || src->b0 < 0 || n_clips > src->Bp - src->b0) return SFSN_EINVAL;
    if (D > 0 && (!src->stft_ri || !aligned8(src->stft_ri) || !desc->hist_ri || !aligned8(desc->hist_ri))) return SFSN_EINVAL;
    if (wave && (!src->wave_tail || !aligned4(src->wave_tail) || !src->enh_ri || !aligned8(src->enh_ri) || !src->wave_out || !aligned8(src->wave_out) ||
                 !desc->wave_state || !aligned4(desc->wave_state) || !desc->ola_state || !aligned8(desc->ola_state) || !desc->window))
        return SFSN_EINVAL;
    const unsigned par = desc->launch_index & 1u;
    p.n_clips = n_clips; p.b0 = src->b0; p.Bp = src->Bp; p.N = N;
    p.F = desc->F; p.S = desc->S; p.D = D;
    p.stft = src->stft_ri; p.enh = src->enh_ri; p.tail = src->wave_tail;
    p.hist = desc->hist_ri; p.wave_state = desc->wave_state; p.ola_state = desc->ola_state; p.window = desc->window;
    a.T = T; a.frame_index = desc->frame_index; a.k = desc->launch_index; a.clip_start = desc->clip_start; a.wave_out = src->wave_out;
    int nsec = 0, blk = 0, fcov = 0;
    size_t slot0 = 0;
    auto add = [&](int kind, int seq, int layer, int items, int per_block) {
        PrimeSecDev& s = p.sec[nsec++];
        s.kind = kind; s.seq = seq; s.layer = layer; s.blk0 = blk; s.items = items;
        blk += (items + per_block - 1) / per_block;
    };
    for (int q = 0; q < 1 + desc->n_groups; ++q) {
        const sfsn_hop_seq& hs = q == 0 ? desc->fb : desc->sb[q - 1];
        const sfsn_prime_seq& ps = q == 0 ? src->fb : src->sb[q - 1];
        PrimeSeqDev& d = p.seq[q];
        d.H = hs.H; d.HP = (hs.H + 63) / 64 * 64; d.units = hs.feat.n_units;
        const size_t R = (size_t)B * d.units;
        if (q > 0 && hs.feat.lo + d.units * hs.fc > fcov) fcov = hs.feat.lo + d.units * hs.fc;
        if (hs.feat.norm == SFSN_NORM_CUMLAPLACE) {
            if (!ps.cum || !aligned4(ps.cum) || !hs.cum[par] || !aligned4(hs.cum[par])) return SFSN_EINVAL;
            d.cum = hs.cum[par]; d.cum_src = ps.cum;
        }
        for (int l = 0; l < hs.n_layers; ++l) {
            PrimeLayerDev& o = d.layer[l];
            if (!ps.layer[l].spikes_i8 || !ps.layer[l].c || !aligned4(ps.layer[l].spikes_i8) || !aligned16(ps.layer[l].c)) return SFSN_EINVAL;
            if (!hs.layer[l].h[par] || !hs.layer[l].c || !aligned4(hs.layer[l].h[par]) || !aligned16(hs.layer[l].c)) return SFSN_EINVAL;
            o.h = hs.layer[l].h[par]; o.c = hs.layer[l].c; o.s8 = ps.layer[l].spikes_i8; o.csrc = ps.layer[l].c;
            o.slots = desc->spike_slots ? desc->spike_slots + slot0 : nullptr;
            slot0 += R * (hs.H / 4);
            add(PRIME_ROWS, q, l, n_clips * d.units * (hs.H / 4), PRIME_THREADS);
        }
    }
    p.fcov = fcov;
    if (D > 0 && fcov > 0) add(PRIME_HIST, 0, 0, n_clips * fcov * D, PRIME_THREADS);
    if (wave) {
        add(PRIME_WAVE, 0, 0, n_clips * FFT_NFFT, PRIME_THREADS);
        add(PRIME_OLA, 0, 0, n_clips * desc->S, PRIME_WAVES);
    }
    p.nsec = nsec;
    hipLaunchKernelGGL(hop_advance_kernel, dim3(blk), dim3(PRIME_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return hip_ok(hipGetLastError());
}

// =====================================================================================================================
// The same two launches for the cIRM-GSN hop (sfsn_fullband_hop_seed / sfsn_fullband_hop_advance, include/sfsn.h): the kernels above
// from host-filled params -- ONE sequence of one row per clip, H = Hp, every bin has history, and hist_ri is double-buffered by
// launch parity like h (the half that launch k reads).  Waveform mode: span = 1, the clip whose first call is still to come (origin
// k + 1) reads as zero like the clip whose frame 0 is launch k.
// =====================================================================================================================
static bool fullband_covered(const sfsn_fullband_hop_desc* d, bool wave) {
    if (wave) return d->hop == 1 && d->D == d->df - 1 && sfsn_fullband_wave_hop_check(d->Hp, d->n_layers, d->F, d->S, d->df, d->B, d->unshared) == SFSN_OK;
    return sfsn_fullband_hop_check(d->Hp, d->n_layers, d->F, d->S, d->df, d->B, d->hop, d->D, d->unshared) == SFSN_OK;
}

static int fullband_clip_list(const sfsn_fullband_hop_desc* desc, const int* clips, int n_clips, unsigned short* out) {
    for (int i = 0; i < n_clips; ++i) {  // (distinct indices below B <= 16: n_clips <= 16)
        if (clips[i] < 0 || clips[i] >= desc->B) return SFSN_EINVAL;
        for (int j = 0; j < i; ++j)
            if (clips[j] == clips[i]) return SFSN_EINVAL;  // (two lanes would own one row)
        out[i] = (unsigned short)clips[i];
    }
    return SFSN_OK;
}

extern "C" int sfsn_fullband_hop_seed(const sfsn_fullband_hop_desc* desc, const unsigned* spike_slots, const float* wave_state, const int* clips,
                                      int n_clips, const sfsn_fullband_seed_dst* dst, void* stream) {
    if (!desc || !clips || !dst || n_clips < 1) return SFSN_EINVAL;
    const bool wave = wave_state != nullptr;
    if (!fullband_covered(desc, wave) || (spike_slots && wave)) return SFSN_EUNSUPPORTED;
    SeedParams p;
    memset(&p, 0, sizeof(p));
    if (fullband_clip_list(desc, clips, n_clips, p.clips) != SFSN_OK) return SFSN_EINVAL;
    const unsigned par = desc->launch_index & 1u;
    const int D = desc->D, Hp = desc->Hp;
    if (dst->Bp < 1 || dst->b0 < 0 || n_clips > dst->Bp - dst->b0) return SFSN_EINVAL;
    if (D > 0 && (dst->T < D || !dst->stft_ri || !aligned8(dst->stft_ri) || !desc->hist_ri[par] || !aligned8(desc->hist_ri[par]))) return SFSN_EINVAL;
    if (wave && (!desc->clip_start || !dst->wave_ctx || !aligned4(dst->wave_ctx) || dst->wave_stride < SEED_CTX || !aligned4(wave_state)))
        return SFSN_EINVAL;
    if (!aligned4(spike_slots) || !aligned4(desc->clip_start)) return SFSN_EINVAL;
    p.n_clips = n_clips; p.b0 = dst->b0; p.T = dst->T; p.F = desc->F; p.D = D; p.fcov = desc->F; p.ctx_stride = dst->wave_stride;
    p.k = desc->launch_index; p.span = wave ? 1u : 0u; p.clip_start = desc->clip_start;
    p.hist = desc->hist_ri[par]; p.wave_state = wave_state; p.stft = dst->stft_ri; p.ctx = dst->wave_ctx;
    int nsec = 0, blk = 0;
    auto add = [&](int kind, int layer, int items) {
        PrimeSecDev& s = p.sec[nsec++];
        s.kind = kind; s.seq = 0; s.layer = layer; s.blk0 = blk; s.items = items;
        blk += (items + PRIME_THREADS - 1) / PRIME_THREADS;
    };
    SeedSeqDev& d = p.seq[0];
    d.H = Hp; d.HP = (Hp + 63) / 64 * 64; d.units = 1;
    for (int l = 0; l < desc->n_layers; ++l) {
        SeedLayerDev& o = d.layer[l];
        const sfsn_fullband_hop_layer& hl = desc->layer[l];
        if (!dst->layer[l].h || !dst->layer[l].c || !aligned16(dst->layer[l].h) || !aligned16(dst->layer[l].c)) return SFSN_EINVAL;
        if (!hl.h[par] || !hl.c || !aligned4(hl.h[par]) || !aligned16(hl.c)) return SFSN_EINVAL;
        o.h = hl.h[par]; o.c = hl.c; o.hd = dst->layer[l].h; o.cd = dst->layer[l].c;
        add(SEED_ROWS, l, n_clips * (Hp / 4));
    }
    if (D > 0) add(SEED_HIST, 0, n_clips * desc->F * D);
    if (wave) add(SEED_WAVE, 0, n_clips * SEED_CTX);
    p.nsec = nsec;
    hipLaunchKernelGGL(hop_seed_kernel, dim3(blk), dim3(PRIME_THREADS), 0, static_cast<hipStream_t>(stream), p);
    return hip_ok(hipGetLastError());
}

extern "C" int sfsn_fullband_hop_advance(const sfsn_fullband_hop_desc* desc, unsigned* spike_slots, float* wave_state, float* ola_state,
                                         const int* clips, int n_clips, const sfsn_fullband_advance_src* src, void* stream) {
    if (!desc || !clips || !src || n_clips < 1) return SFSN_EINVAL;
    if ((wave_state != nullptr) != (ola_state != nullptr)) return SFSN_EINVAL;
    const bool wave = wave_state != nullptr;
    if (!fullband_covered(desc, wave) || (spike_slots && wave)) return SFSN_EUNSUPPORTED;
    AdvParams a;
    memset(&a, 0, sizeof(a));
    PrimeParams& p = a.base;
    if (fullband_clip_list(desc, clips, n_clips, p.clips) != SFSN_OK) return SFSN_EINVAL;
    const unsigned par = desc->launch_index & 1u;
    const int N = src->N, T = src->T, B = desc->B, D = desc->D, Hp = desc->Hp;
    // (N = 0, waveform mode: the clip without a call whose backlog is one call -- its samples enter wave_state and make no frame)
    if (N < 0 || (!wave && N < desc->hop) || N % desc->hop != 0 || T < N + D) return SFSN_EINVAL;
    if (src->Bp < 1 || src->b0 < 0 || n_clips > src->Bp - src->b0) return SFSN_EINVAL;
    if (D > 0 && (!desc->hist_ri[par] || !aligned8(desc->hist_ri[par]) || (N > 0 && (!src->stft_ri || !aligned8(src->stft_ri))))) return SFSN_EINVAL;
    if (wave && (!desc->clip_start || !src->wave_tail || !aligned4(src->wave_tail) || !src->window || !aligned4(src->window) ||
                 !aligned4(wave_state) || !aligned8(ola_state) ||
                 (N > 0 && (!src->enh_ri || !aligned8(src->enh_ri) || !src->wave_out || !aligned8(src->wave_out)))))
        return SFSN_EINVAL;
    if (!aligned4(spike_slots) || !aligned4(desc->clip_start)) return SFSN_EINVAL;
    p.n_clips = n_clips; p.b0 = src->b0; p.Bp = src->Bp; p.N = N;
    p.F = desc->F; p.S = desc->S; p.D = D; p.fcov = desc->F;
    p.stft = src->stft_ri; p.enh = src->enh_ri; p.tail = src->wave_tail;
    p.hist = desc->hist_ri[par]; p.wave_state = wave_state; p.ola_state = ola_state; p.window = src->window;
    a.T = T; a.k = desc->launch_index; a.span = wave ? 1u : 0u; a.clip_start = desc->clip_start; a.wave_out = src->wave_out;
    int nsec = 0, blk = 0;
    auto add = [&](int kind, int layer, int items, int per_block) {
        PrimeSecDev& s = p.sec[nsec++];
        s.kind = kind; s.seq = 0; s.layer = layer; s.blk0 = blk; s.items = items;
        blk += (items + per_block - 1) / per_block;
    };
    PrimeSeqDev& d = p.seq[0];
    d.H = Hp; d.HP = (Hp + 63) / 64 * 64; d.units = 1;
    for (int l = 0; l < desc->n_layers; ++l) {
        PrimeLayerDev& o = d.layer[l];
        const sfsn_fullband_hop_layer& hl = desc->layer[l];
        if (N > 0 && (!src->layer[l].spikes_i8 || !src->layer[l].c || !aligned4(src->layer[l].spikes_i8) || !aligned16(src->layer[l].c))) return SFSN_EINVAL;
        if (!hl.h[par] || !hl.c || !aligned4(hl.h[par]) || !aligned16(hl.c)) return SFSN_EINVAL;
        o.h = hl.h[par]; o.c = hl.c; o.s8 = src->layer[l].spikes_i8; o.csrc = src->layer[l].c;
        o.slots = spike_slots ? spike_slots + (size_t)l * B * (Hp / 4) : nullptr;
        add(PRIME_ROWS, l, n_clips * (Hp / 4), PRIME_THREADS);
    }
    if (D > 0) add(PRIME_HIST, 0, n_clips * desc->F * D, PRIME_THREADS);
    if (wave) {
        add(PRIME_WAVE, 0, n_clips * FFT_NFFT, PRIME_THREADS);
        add(PRIME_OLA, 0, n_clips * desc->S, PRIME_WAVES);
    }
    p.nsec = nsec;
    hipLaunchKernelGGL(hop_advance_kernel, dim3(blk), dim3(PRIME_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return hip_ok(hipGetLastError());
}
