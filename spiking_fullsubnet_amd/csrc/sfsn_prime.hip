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
#define PRIME_MAX_SECS (PRIME_MAX_SEQS * SFSN_HOP_MAX_LAYERS + 3)

enum { PRIME_ROWS = 0, PRIME_HIST = 1, PRIME_WAVE = 2, PRIME_OLA = 3 };

struct PrimeLayerDev {
    int8_t* h;          // the half of the double buffer the next launch reads
    float* c;
    unsigned* slots;    // this layer's [R][H / 4] slots, or NULL
    const int8_t* s8;   // [N][Bp * units][HP]
    const float* csrc;  // [Bp * units][H]
};
struct PrimeSeqDev {
    PrimeLayerDev layer[SFSN_HOP_MAX_LAYERS];
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
