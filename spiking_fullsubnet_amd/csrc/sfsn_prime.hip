// sfsn_prime.hip -- the way between a streaming session (the one-launch hops of sfsn_hop.hip / sfsn_fullband_hop.hip) and the offline
// kernels, one launch each way, for the listed clips of the session only (gfx950 only; include/sfsn.h: sfsn_hop_prime, sfsn_hop_seed,
// sfsn_hop_advance, sfsn_hop_advance_ragged, sfsn_fullband_hop_seed, sfsn_fullband_hop_advance, sfsn_fullband_hop_advance_ragged).
//
// A session that has streamed some frames of a clip holds: every layer's last spikes (double-buffered by launch parity) and membrane,
// the running sums of the cumulative norm, the last D noisy frames, the spike counts per lane slot and, in waveform mode, the last
// 512 input samples and the overlap-add partial sums of the positions not yet emitted.  All of it is a function of the frames, and
// the offline forward computes the same bits (include/sfsn.h, sfsn_stream_hop).
//
// The TAKE launch (hop_take_kernel) writes that state from what the offline kernels left behind for N frames.  It has two forms, two
// instantiations of one text: the clip's utterance BEGINS with the N frames (sfsn_hop_prime; source rows of N frames), or it
// CONTINUES with them (the advance entry points; source rows of T >= D + N frames, [history | new], and a clip whose origin is this
// launch index reads as zero, as it does in the hop).  Its roles:
//   * rows, one section per (sequence, layer): lane (row, j) owns the 4 neurons 4j .. 4j + 3 of a row, as in the hop -- the last
//     frame's spike word into h[launch & 1], the membrane's float4, the slot's count (popcounts of its word over the N frames: the
//     very numbers the hop's lane would have added, one per launch; the beginning form replaces the slot, the continuing form adds to
//     it), and for layer 0 the row's running sum into cum[launch & 1] (cumlap_scan_kernel and the hop add the same row sums in the
//     same order: sfsn_kernels.hip / hop_layer_role);
//   * hist: the last D noisy frames of the bins the groups cover (the hop keeps no history of the pass-through bins);
//   * wave: the last 512 samples;
//   * ola: a wave per (clip, speaker) runs hop_wave_istft's recurrence (acc = ola + frame, ola = acc moved on by one hop) with
//     sfsn_fft_dev.h's transform: the same instructions in the same (ascending frame) order, hence the hop's bits.  Beginning: from
//     zero over the last three frames -- earlier ones have left the accumulator by then -- and no output.  Continuing: from the carried
//     sums over every new frame, each completed block through the envelope into wave_out.
// The SEED launch (hop_seed_kernel) is the way out: what the offline kernels start from -- (h, c) as they take them (fp32 0/1 spikes,
// membranes), the running sums, the D frames of history in front of the new frames and, in waveform mode, the 384 samples the next
// frame begins with.
// Plain loads and stores only, nothing waits: the launch boundary publishes them.  The tagged scratch of the hop (spikes, spec_g,
// enh_g) is not touched and launch_index does not move, so its tags stay what the next launch expects.
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
#define SEED_CTX 384  // samples of wave_state the next frame begins with

enum { SEC_ROWS = 0, SEC_HIST = 1, SEC_WAVE = 2, SEC_OLA = 3 };

struct SecDev {
    int kind, seq, layer, blk0, items;
};

struct TakeLayerDev {
    int8_t* h;          // the half of the double buffer the next launch reads
    float* c;
    unsigned* slots;    // this layer's [R][H / 4] slots, or NULL
    const int8_t* s8;   // [N][Bp * units][HP]
    const float* csrc;  // [Bp * units][H]
};
struct TakeSeqDev {
    TakeLayerDev layer[PRIME_MAX_LAYERS];
    float* cum;  // the half the next launch reads, or NULL
    const float* cum_src;
    int H, HP, units;
};
struct TakeParams {
    TakeSeqDev seq[PRIME_MAX_SEQS];
    SecDev sec[PRIME_MAX_SECS];
    unsigned short clips[PRIME_MAX_CLIPS];
    int nsec, n_clips, b0, Bp, N;
    int F, S, D, fcov;
    const float* stft;  // [Bp][F][T][2], the N frames last
    const float* enh;   // [Bp][S][F][T][2]
    const float* tail;  // [Bp][512]
    float* hist;
    float* wave_state;
    float* ola_state;
    const float* window;
    // the continuing form only (the beginning form leaves them zero and its rows have T = N frames)
    int T, frame_index;
    unsigned k, span;  // span: origins k .. k + span read as zero (0; the cIRM-GSN waveform hop: 1, the clip without a call)
    const unsigned* clip_start;
    float* wave_out;  // [Bp][S][128 * N]
};
static_assert(sizeof(TakeParams) <= 4096, "TakeParams travels as a kernel argument");

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
    SecDev sec[PRIME_MAX_SECS];
    unsigned short clips[PRIME_MAX_CLIPS];
    int nsec, n_clips, b0, T;
    int F, D, fcov, ctx_stride;
    unsigned k, span;  // as in TakeParams
    const unsigned* clip_start;
    const float* hist;
    const float* wave_state;
    float* stft;  // [Bp][F][T][2]
    float* ctx;   // [Bp][ctx_stride]
};
static_assert(sizeof(SeedParams) <= 4096, "SeedParams travels as a kernel argument");

// the section of this workgroup (block-uniform: sections are in block order)
__device__ __forceinline__ int block_section(const SecDev* sec, int nsec) {
    int si = 0;
    for (int i = 1; i < nsec; ++i)
        if ((int)blockIdx.x >= sec[i].blk0) si = i;
    return si;
}

__device__ __forceinline__ bool clip_fresh(const unsigned* clip_start, unsigned k, unsigned span, int clip) {
    return clip_start && clip_start[clip] - k <= span;  // (unsigned, wrap-safe)
}

template <bool CONTINUE>
__device__ __forceinline__ int row_frames(const TakeParams& p) {
    return CONTINUE ? p.T : p.N;
}

// N == 0 (a waveform clip whose one call has made no frame): zeros to h, c and cum, which its frame 0 reads anyway, and the slot
// replaced by 0.  The continuing form gets there from sfsn_fullband_hop_advance in waveform mode only (every other caller refuses
// N < hop), where the session has neither cum nor slots: h and c are all it writes.
template <bool CONTINUE>
__device__ __forceinline__ void take_rows(const TakeParams& p, const SecDev& sd, int item) {
    const TakeSeqDev& sq = p.seq[sd.seq];
    const TakeLayerDev& L = sq.layer[sd.layer];
    const int W = sq.H >> 2, N = p.N;
    const int j = item % W, rr = item / W;
    const int k = rr % sq.units, i = rr / sq.units;
    const size_t Rs = (size_t)p.Bp * sq.units;
    const size_t row_s = (size_t)(p.b0 + i) * sq.units + k, row_d = (size_t)p.clips[i] * sq.units + k;
    const int8_t* sp = L.s8 + row_s * sq.HP + 4 * j;  // my word of the first of the N frames; a frame further every Rs * HP bytes
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
    if constexpr (CONTINUE) {
        // (the clip's utterance goes on: its slot is added to -- unless it begins here, where the hop reads the slot as zero)
        if (N > 0 && !clip_fresh(p.clip_start, p.k, p.span, p.clips[i])) nspk = L.slots[row_d * W + j];
    }
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

// frame T - D + d of a row of T frames.  Beginning (T = N): frames before the first read as zero, as a fresh session's history does.
// Continuing (T >= D + N): the last D frames of [history | new] -- N < D keeps the tail of the old history, which the seed launch
// wrote there.  N == 0: zero (see take_rows)
template <bool CONTINUE>
__device__ __forceinline__ void take_hist(const TakeParams& p, int item) {
    const int D = p.D, T = row_frames<CONTINUE>(p);
    const int d = item % D, r = item / D;
    const int f = r % p.fcov, i = r / p.fcov;
    const int t = T - D + d;
    float2 v = make_float2(0.0f, 0.0f);
    if (t >= 0 && p.N > 0) v = *reinterpret_cast<const float2*>(p.stft + (((size_t)(p.b0 + i) * p.F + f) * T + t) * 2);
    *reinterpret_cast<float2*>(p.hist + (((size_t)p.clips[i] * p.F + f) * D + d) * 2) = v;
}

__device__ __forceinline__ void take_wave(const TakeParams& p, int item) {
    const int n = item & (FFT_NFFT - 1), i = item >> 9;
    p.wave_state[(size_t)p.clips[i] * FFT_NFFT + n] = p.tail[(size_t)(p.b0 + i) * FFT_NFFT + n];
}

// hop_wave_istft's arithmetic (sfsn_hop_wave_dev.h), frame after frame in ascending order, without its hand-off.  Beginning: from
// zero over the last three of the N frames, no output.  Continuing: the clip's carried partial sums first, then frames T - N .. T - 1,
// each completed hop divided by the envelope of the frames that exist and written to wave_out.
template <bool CONTINUE>
__device__ __forceinline__ void take_ola(const TakeParams& p, int blk, char* smem) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float2* unit = reinterpret_cast<float2*>(smem);
    float2(*fbuf)[FFT_N] = reinterpret_cast<float2(*)[FFT_N]>(smem + FFT_NFFT * 8);
    float2(*xs)[264] = reinterpret_cast<float2(*)[264]>(smem + FFT_NFFT * 8 + PRIME_WAVES * FFT_N * 8);
    fill_unit_table(unit, tid, PRIME_THREADS);
    __syncthreads();
    const int pair = blk * PRIME_WAVES + wave;
    if (pair >= p.n_clips * p.S) return;
    const int i = pair / p.S, s = pair - i * p.S, N = p.N, F = p.F, T = row_frames<CONTINUE>(p);
    const int clip = p.clips[i];
    const int first = CONTINUE ? T - N : (N > 3 ? N - 3 : 0);  // the first frame fed
    bool fresh = true;
    int fi0 = 0;  // the frame index of the first new frame
    if constexpr (CONTINUE) {
        // a clip that begins here carries no sums (span 1: also the clip whose first call, which has no frame, is launch k -- age -1 --
        // and whose frame 0 is the first new frame)
        const int age = p.clip_start ? (int)(p.k - p.clip_start[clip]) : p.frame_index;
        fresh = p.clip_start && age <= 0 && age >= -(int)p.span;
        fi0 = fresh ? 0 : age;
    }
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
    const float* eg = p.enh + ((size_t)(p.b0 + i) * p.S + s) * F * T * 2 + (size_t)first * 2;
    float* wo = CONTINUE ? p.wave_out + ((size_t)(p.b0 + i) * p.S + s) * 128 * N : nullptr;
    const float sc = 1.0f / (float)FFT_N;
    for (int t = 0; t < T - first; ++t) {
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
        if constexpr (CONTINUE) {
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
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) ola[r] = r < 3 ? acc[r + 1] : make_float2(0.0f, 0.0f);
        __builtin_amdgcn_wave_barrier();  // (this frame's reads of xs / fbuf before the next frame's writes)
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) *reinterpret_cast<float2*>(os + 2 * (lane + 64 * r)) = ola[r];
}

// two instantiations, not a flag: the beginning form's code carries neither the clip_start loads nor the output path
template <bool CONTINUE>
__global__ __launch_bounds__(PRIME_THREADS) void hop_take_kernel(const TakeParams p) {
    __shared__ __attribute__((aligned(16))) char smem[FFT_NFFT * 8 + PRIME_WAVES * FFT_N * 8 + PRIME_WAVES * 264 * 8];
    const SecDev& sd = p.sec[block_section(p.sec, p.nsec)];
    const int blk = (int)blockIdx.x - sd.blk0;
    if (sd.kind == SEC_OLA) {
        take_ola<CONTINUE>(p, blk, smem);
        return;
    }
    const int item = blk * PRIME_THREADS + (int)threadIdx.x;
    if (item >= sd.items) return;
    if (sd.kind == SEC_ROWS)
        take_rows<CONTINUE>(p, sd, item);
    else if (sd.kind == SEC_HIST)
        take_hist<CONTINUE>(p, item);
    else
        take_wave(p, item);
}

// ---------------------------------------------------------------------------------------------------------------------
// The continuing TAKE launch with a length of its own per clip (sfsn_hop_advance_ragged): the offline kernels ran a padded batch of
// Nmax new frames behind `lead` = T - Nmax frames of history, clip b0 + i has N_b = frames[b0 + i] of them and everything the launch
// takes ends at the clip's own last frame.  The scans leave c_state after the last PADDED frame only, so the membranes come from the
// per-frame membrane tap (sfsn_scan_segment.membrane: the post-BatchNorm value that becomes c_state), row N_b - 1.  The other roles
// are hop_take_kernel<true>'s with N_b in the place of N; the cumulative norm is refused on the host (its running sums after a
// clip's own last frame exist nowhere).  A kernel of its own: hop_take_kernel's two instantiations keep their code.
struct TakeRaggedLayerDev {
    int8_t* h;          // the half of the double buffer the next launch reads
    float* c;
    unsigned* slots;    // this layer's [R][H / 4] slots, or NULL
    const int8_t* s8;   // [Nmax][Bp * units][HP]
    const float* mem;   // [Nmax][Bp * units][H]
};
struct TakeRaggedSeqDev {
    TakeRaggedLayerDev layer[SFSN_HOP_MAX_LAYERS];
    int H, HP, units;
};
struct TakeRaggedParams {
    TakeRaggedSeqDev seq[PRIME_MAX_SEQS];
    SecDev sec[PRIME_MAX_SECS];
    unsigned short clips[PRIME_MAX_CLIPS];
    int nsec, n_clips, b0, Bp, Nmax, T;
    int F, S, D, fcov, frame_index, ctx_stride;
    unsigned k;
    const int* frames;  // [Bp]
    const float* stft;  // [Bp][F][T][2], the Nmax frames last
    const float* enh;   // [Bp][S][F][T][2]
    const float* ctx;   // [Bp][ctx_stride]: 384 samples of context, then the new samples
    float* hist;
    float* wave_state;
    float* ola_state;
    const float* window;
    const unsigned* clip_start;
    float* wave_out;    // [Bp][S][128 * Nmax]
};
static_assert(sizeof(TakeRaggedParams) <= 4096, "TakeRaggedParams travels as a kernel argument");

// The ragged roles are one text for two parameter blocks: TakeRaggedParams (sfsn_hop_advance_ragged; NOCALL = false) and
// FullbandTakeRaggedParams (sfsn_fullband_hop_advance_ragged; NOCALL = true: the cIRM-GSN waveform hop's clip WITHOUT A CALL, origin
// k + 1 -- hop_take_kernel<true>'s `span`: no carried overlap-add sums, frame index 0 at its first new frame, an STFT-state window that
// ends one hop later in its context row, and N_b = 0 where its backlog is its one first call).
template <bool NOCALL, class P>
__device__ __forceinline__ unsigned ragged_span(const P& p) {
    if constexpr (NOCALL) return p.span;
    return 0u;
}

// launch k is the clip's first call, still to come (the caller guarantees clip_start where span is set)
template <bool NOCALL, class P>
__device__ __forceinline__ bool ragged_nocall(const P& p, int i) {
    if constexpr (NOCALL) return p.span && p.clip_start[p.clips[i]] - p.k == 1u;
    return false;
}

// the clip's own frame count, held inside [1, Nmax] ([0, Nmax] for the clip without a call) whatever the array says: no index below
// leaves the caller's tensors
template <bool NOCALL, class P>
__device__ __forceinline__ int ragged_frames(const P& p, int i) {
    const int n = p.frames[p.b0 + i];
    if constexpr (!NOCALL) {
        return n < 1 ? 1 : (n > p.Nmax ? p.Nmax : n);
    } else {
        const int lo = ragged_nocall<NOCALL>(p, i) ? 0 : 1;
        return n < lo ? lo : (n > p.Nmax ? p.Nmax : n);
    }
}

template <bool NOCALL, class P>
__device__ __forceinline__ void take_rows_ragged(const P& p, const SecDev& sd, int item) {
    const auto& sq = p.seq[sd.seq];
    const TakeRaggedLayerDev& L = sq.layer[sd.layer];
    const int W = sq.H >> 2;
    const int j = item % W, rr = item / W;
    const int k = rr % sq.units, i = rr / sq.units;
    const int N = ragged_frames<NOCALL>(p, i);
    const size_t Rs = (size_t)p.Bp * sq.units;
    const size_t row_s = (size_t)(p.b0 + i) * sq.units + k, row_d = (size_t)p.clips[i] * sq.units + k;
    const int8_t* sp = L.s8 + row_s * sq.HP + 4 * j;  // my word of the first new frame; a frame further every Rs * HP bytes
    const size_t fs = Rs * sq.HP;
    const bool none = NOCALL && N == 0;  // (the clip without a call and no frame: zeros, which its frame 0 reads anyway)
    const unsigned last = none ? 0u : *reinterpret_cast<const unsigned*>(sp + (size_t)(N - 1) * fs) & 0x01010101u;
    const float4 c = none ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : *reinterpret_cast<const float4*>(L.mem + ((size_t)(N - 1) * Rs + row_s) * sq.H + 4 * j);
    *reinterpret_cast<unsigned*>(L.h + row_d * sq.HP + 4 * j) = last;
    *reinterpret_cast<float4*>(L.c + row_d * sq.H + 4 * j) = c;
    if (!L.slots) return;
    unsigned nspk = 0u;  // (a clip that begins here: the hop reads its slot as zero)
    if (!clip_fresh(p.clip_start, p.k, NOCALL ? ragged_span<NOCALL>(p) : 0u, p.clips[i])) nspk = L.slots[row_d * W + j];
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

// the D frames that end with the clip's own last one: frames lead + N_b - D .. lead + N_b - 1 of its row (lead >= D: N_b < D keeps the
// tail of the old history)
template <bool NOCALL, class P>
__device__ __forceinline__ void take_hist_ragged(const P& p, int item) {
    const int D = p.D, T = p.T;
    const int d = item % D, r = item / D;
    const int f = r % p.fcov, i = r / p.fcov;
    const int t = T - p.Nmax + ragged_frames<NOCALL>(p, i) - D + d;
    const bool none = NOCALL && ragged_frames<NOCALL>(p, i) == 0;  // (no frame: zero, as take_hist)
    const float2 v = none ? make_float2(0.0f, 0.0f) : *reinterpret_cast<const float2*>(p.stft + (((size_t)(p.b0 + i) * p.F + f) * T + t) * 2);
    *reinterpret_cast<float2*>(p.hist + (((size_t)p.clips[i] * p.F + f) * D + d) * 2) = v;
}

// the 512 samples that end with the clip's own last one: sample 384 + 128 N_b of its context row -- one hop later for the clip
// without a call, whose first 128 samples made no frame (held inside the row: the host cannot know the clip's kind)
template <bool NOCALL, class P>
__device__ __forceinline__ void take_wave_ragged(const P& p, int item) {
    const int n = item & (FFT_NFFT - 1), i = item >> 9;
    int end = SEED_CTX + 128 * ragged_frames<NOCALL>(p, i);
    if constexpr (NOCALL) {
        if (ragged_nocall<NOCALL>(p, i)) end += 128;
        if (end > p.ctx_stride) end = p.ctx_stride;
    }
    p.wave_state[(size_t)p.clips[i] * FFT_NFFT + n] = p.ctx[(size_t)(p.b0 + i) * p.ctx_stride + end - FFT_NFFT + n];
}

// take_ola<true>'s recurrence over the clip's own N_b frames; the blocks behind them are written as zeros
template <bool NOCALL, class P>
__device__ __forceinline__ void take_ola_ragged(const P& p, int blk, char* smem) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float2* unit = reinterpret_cast<float2*>(smem);
    float2(*fbuf)[FFT_N] = reinterpret_cast<float2(*)[FFT_N]>(smem + FFT_NFFT * 8);
    float2(*xs)[264] = reinterpret_cast<float2(*)[264]>(smem + FFT_NFFT * 8 + PRIME_WAVES * FFT_N * 8);
    fill_unit_table(unit, tid, PRIME_THREADS);
    __syncthreads();
    const int pair = blk * PRIME_WAVES + wave;
    if (pair >= p.n_clips * p.S) return;
    const int i = pair / p.S, s = pair - i * p.S, F = p.F, T = p.T, Nmax = p.Nmax;
    const int N = ragged_frames<NOCALL>(p, i);
    const int clip = p.clips[i];
    const int first = T - Nmax;  // the first frame fed
    // a clip that begins here carries no sums (NOCALL: nor does the clip whose first call is launch k -- age -1, as take_ola)
    const int age = p.clip_start ? (int)(p.k - p.clip_start[clip]) : p.frame_index;
    const bool fresh = NOCALL ? p.clip_start && age <= 0 && age >= -(int)ragged_span<NOCALL>(p) : p.clip_start && age == 0;
    const int fi0 = fresh ? 0 : age;  // the frame index of the first new frame
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
    const float* eg = p.enh + ((size_t)(p.b0 + i) * p.S + s) * F * T * 2 + (size_t)first * 2;
    float* wo = p.wave_out + ((size_t)(p.b0 + i) * p.S + s) * 128 * Nmax;
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
    for (int t = N; t < Nmax; ++t) *reinterpret_cast<float2*>(wo + (size_t)128 * t + 2 * lane) = make_float2(0.0f, 0.0f);
#pragma unroll
    for (int r = 0; r < 4; ++r) *reinterpret_cast<float2*>(os + 2 * (lane + 64 * r)) = ola[r];
}

__global__ __launch_bounds__(PRIME_THREADS) void hop_take_ragged_kernel(const TakeRaggedParams p) {
    __shared__ __attribute__((aligned(16))) char smem[FFT_NFFT * 8 + PRIME_WAVES * FFT_N * 8 + PRIME_WAVES * 264 * 8];
    const SecDev& sd = p.sec[block_section(p.sec, p.nsec)];
    const int blk = (int)blockIdx.x - sd.blk0;
    if (sd.kind == SEC_OLA) {
        take_ola_ragged<false>(p, blk, smem);
        return;
    }
    const int item = blk * PRIME_THREADS + (int)threadIdx.x;
    if (item >= sd.items) return;
    if (sd.kind == SEC_ROWS)
        take_rows_ragged<false>(p, sd, item);
    else if (sd.kind == SEC_HIST)
        take_hist_ragged<false>(p, item);
    else
        take_wave_ragged<false>(p, item);
}

// The same launch for a cIRM-GSN session (sfsn_fullband_hop_advance_ragged): one sequence of up to SFSN_FULLBAND_HOP_MAX_LAYERS layers,
// one row per clip, at most 16 clips, and in waveform mode the clip without a call (NOCALL above).  A kernel of its own:
// hop_take_ragged_kernel keeps its code.
struct FullbandTakeRaggedSeqDev {
    TakeRaggedLayerDev layer[SFSN_FULLBAND_HOP_MAX_LAYERS];
    int H, HP, units;
};
struct FullbandTakeRaggedParams {
    FullbandTakeRaggedSeqDev seq[1];
    SecDev sec[SFSN_FULLBAND_HOP_MAX_LAYERS + 3];
    unsigned short clips[16];
    int nsec, n_clips, b0, Bp, Nmax, T;
    int F, S, D, fcov, frame_index, ctx_stride;
    unsigned k, span;   // span 1 (waveform mode): origins k and k + 1 read as zero
    const int* frames;  // [Bp]
    const float* stft;  // [Bp][F][T][2], the Nmax frames last
    const float* enh;   // [Bp][S][F][T][2]
    const float* ctx;   // [Bp][ctx_stride]: 384 samples of context, then the new samples
    float* hist;
    float* wave_state;
    float* ola_state;
    const float* window;
    const unsigned* clip_start;
    float* wave_out;    // [Bp][S][128 * Nmax]
};

__global__ __launch_bounds__(PRIME_THREADS) void fullband_take_ragged_kernel(const FullbandTakeRaggedParams p) {
    __shared__ __attribute__((aligned(16))) char smem[FFT_NFFT * 8 + PRIME_WAVES * FFT_N * 8 + PRIME_WAVES * 264 * 8];
    const SecDev& sd = p.sec[block_section(p.sec, p.nsec)];
    const int blk = (int)blockIdx.x - sd.blk0;
    if (sd.kind == SEC_OLA) {
        take_ola_ragged<true>(p, blk, smem);
        return;
    }
    const int item = blk * PRIME_THREADS + (int)threadIdx.x;
    if (item >= sd.items) return;
    if (sd.kind == SEC_ROWS)
        take_rows_ragged<true>(p, sd, item);
    else if (sd.kind == SEC_HIST)
        take_hist_ragged<true>(p, item);
    else
        take_wave_ragged<true>(p, item);
}

// a clip whose origin is this launch index reads as zero, as it does in the hop
__device__ __forceinline__ void seed_rows(const SeedParams& p, const SecDev& sd, int item) {
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
    const SecDev& sd = p.sec[block_section(p.sec, p.nsec)];
    const int item = ((int)blockIdx.x - sd.blk0) * PRIME_THREADS + (int)threadIdx.x;
    if (item >= sd.items) return;
    if (sd.kind == SEC_ROWS)
        seed_rows(p, sd, item);
    else if (sd.kind == SEC_HIST)
        seed_hist(p, item);
    else
        seed_wave(p, item);
}

// =====================================================================================================================
// host side
// =====================================================================================================================
static inline bool aligned_to(const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) == 0; }
static inline bool bad(const void* q, uintptr_t a) { return !q || !aligned_to(q, a); }  // missing or misaligned

// the clip list of every entry point; the clips go into `out` (PRIME_MAX_CLIPS entries)
static int check_clips(int B, const int* clips, int n_clips, unsigned short* out) {
    if (!clips || n_clips <= 0) return SFSN_EINVAL;
    if (B > 65535 || n_clips > PRIME_MAX_CLIPS) return SFSN_EUNSUPPORTED;  // (the caller splits a longer list)
    for (int i = 0; i < n_clips; ++i) {
        if (clips[i] < 0 || clips[i] >= B) return SFSN_EINVAL;
        for (int j = 0; j < i; ++j)
            if (clips[j] == clips[i]) return SFSN_EINVAL;  // (two lanes would own one row)
        out[i] = (unsigned short)clips[i];
    }
    return SFSN_OK;
}

// sections of a launch in block order
struct Sections {
    SecDev* sec;
    int nsec = 0, blk = 0;
    void add(int kind, int seq, int layer, int items, int per_block = PRIME_THREADS) {
        SecDev& s = sec[nsec++];
        s.kind = kind; s.seq = seq; s.layer = layer; s.blk0 = blk; s.items = items;
        blk += (items + per_block - 1) / per_block;
    }
};

// A sequence of the hop as both launches see it: rows of `units` per clip, the half of h / cum that launch k reads.
struct SeqView {
    int H, units, n_layers;
    int8_t* h[PRIME_MAX_LAYERS];
    float* c[PRIME_MAX_LAYERS];
    bool cumulative;  // SFSN_NORM_CUMLAPLACE: the rows carry running sums
    float* cum;
};
// The session: a sfsn_hop_desc's full-band model and groups, or the one sequence of one row per clip of a sfsn_fullband_hop_desc
// (H = Hp, every bin has history, hist_ri double-buffered like h; what lives outside that descriptor comes with the call).
struct HopView {
    SeqView seq[PRIME_MAX_SEQS];
    int nseq;
    bool wave;
    int B, F, S, D, fcov, frame_index;
    unsigned k, span;  // span 1: the cIRM-GSN waveform hop, where the clip whose first call is still to come (origin k + 1) reads
                       // as zero like the clip whose frame 0 is launch k
    float* hist;
    float* wave_state;
    float* ola_state;
    const float* window;
    const unsigned* clip_start;
    unsigned* spike_slots;  // sequence by sequence, layer by layer, [B * units][H / 4] each; or NULL
};
// the caller's tensors, per sequence of the view
struct TakeSrc {
    int Bp, N, b0, T;
    const float *stft, *enh, *tail;
    float* wave_out;
    const sfsn_prime_layer* layer[PRIME_MAX_SEQS];
    const float* cum[PRIME_MAX_SEQS];
};
struct SeedDst {
    int Bp, T, b0, wave_stride;
    float *stft, *ctx;
    const sfsn_seed_layer* layer[PRIME_MAX_SEQS];
    float* cum[PRIME_MAX_SEQS];
};

// SFSN_EUNSUPPORTED: a descriptor sfsn_stream_hop would not run (its plan validates the geometry and every state pointer)
static int view_of(const sfsn_hop_desc* d, HopView& v) {
    if (d->n_groups < 1 || d->n_groups > SFSN_HOP_MAX_GROUPS) return SFSN_EUNSUPPORTED;
    if (sfsn_hop_spike_slots(d) == 0) return SFSN_EUNSUPPORTED;
    memset(&v, 0, sizeof(v));
    const unsigned par = d->launch_index & 1u;
    v.nseq = 1 + d->n_groups; v.wave = d->wave_in != nullptr;
    v.B = d->B; v.F = d->F; v.S = d->S; v.D = d->D; v.frame_index = d->frame_index; v.k = d->launch_index;
    v.hist = d->hist_ri; v.wave_state = d->wave_state; v.ola_state = d->ola_state; v.window = d->window;
    v.clip_start = d->clip_start; v.spike_slots = d->spike_slots;
    for (int q = 0; q < v.nseq; ++q) {
        const sfsn_hop_seq& hs = q == 0 ? d->fb : d->sb[q - 1];
        SeqView& s = v.seq[q];
        s.H = hs.H; s.units = hs.feat.n_units; s.n_layers = hs.n_layers;
        if (q > 0 && hs.feat.lo + s.units * hs.fc > v.fcov) v.fcov = hs.feat.lo + s.units * hs.fc;
        s.cumulative = hs.feat.norm == SFSN_NORM_CUMLAPLACE;
        if (s.cumulative) s.cum = hs.cum[par];
        for (int l = 0; l < hs.n_layers; ++l) {
            s.h[l] = hs.layer[l].h[par]; s.c[l] = hs.layer[l].c;
        }
    }
    return SFSN_OK;
}

// SFSN_EUNSUPPORTED: a descriptor the coverage check refuses, spike slots together with the waveform state
static int view_of(const sfsn_fullband_hop_desc* d, unsigned* spike_slots, float* wave_state, float* ola_state, const float* window, HopView& v) {
    const bool wave = wave_state != nullptr;
    const int rc = wave ? (d->hop == 1 && d->D == d->df - 1 ? sfsn_fullband_wave_hop_check(d->Hp, d->n_layers, d->F, d->S, d->df, d->B, d->unshared) : SFSN_EUNSUPPORTED)
                        : sfsn_fullband_hop_check(d->Hp, d->n_layers, d->F, d->S, d->df, d->B, d->hop, d->D, d->unshared);
    if (rc != SFSN_OK || (spike_slots && wave)) return SFSN_EUNSUPPORTED;
    memset(&v, 0, sizeof(v));
    const unsigned par = d->launch_index & 1u;
    v.nseq = 1; v.wave = wave;
    v.B = d->B; v.F = d->F; v.S = d->S; v.D = d->D; v.fcov = d->F; v.k = d->launch_index; v.span = wave ? 1u : 0u;
    v.hist = d->hist_ri[par]; v.wave_state = wave_state; v.ola_state = ola_state; v.window = window;
    v.clip_start = d->clip_start; v.spike_slots = spike_slots;
    SeqView& s = v.seq[0];
    s.H = d->Hp; s.units = 1; s.n_layers = d->n_layers;
    for (int l = 0; l < d->n_layers; ++l) {
        s.h[l] = d->layer[l].h[par]; s.c[l] = d->layer[l].c;
    }
    return SFSN_OK;
}

// the state pointers a launch reads or writes (ola: the accumulator and the window too)
static bool state_ok(const HopView& v, bool ola) {
    if (v.D > 0 && bad(v.hist, 8)) return false;
    if (v.wave && (bad(v.wave_state, 4) || (ola && (bad(v.ola_state, 8) || bad(v.window, 4))))) return false;
    if (!aligned_to(v.spike_slots, 4) || !aligned_to(v.clip_start, 4)) return false;
    for (int q = 0; q < v.nseq; ++q) {
        const SeqView& s = v.seq[q];
        if (s.cumulative && bad(s.cum, 4)) return false;
        for (int l = 0; l < s.n_layers; ++l)
            if (bad(s.h[l], 4) || bad(s.c[l], 16)) return false;
    }
    return true;
}

static int seed_launch(const HopView& v, const int* clips, int n_clips, const SeedDst& dst, void* stream) {
    SeedParams p;
    memset(&p, 0, sizeof(p));
    const int rc = check_clips(v.B, clips, n_clips, p.clips);
    if (rc != SFSN_OK) return rc;
    const int D = v.D;
    if (dst.Bp < 1 || dst.b0 < 0 || n_clips > dst.Bp - dst.b0) return SFSN_EINVAL;
    if (D > 0 && (dst.T < D || bad(dst.stft, 8))) return SFSN_EINVAL;
    if (v.wave && (bad(dst.ctx, 4) || dst.wave_stride < SEED_CTX)) return SFSN_EINVAL;
    if (!state_ok(v, false)) return SFSN_EINVAL;
    p.n_clips = n_clips; p.b0 = dst.b0; p.T = dst.T; p.F = v.F; p.D = D; p.fcov = v.fcov; p.ctx_stride = dst.wave_stride;
    p.k = v.k; p.span = v.span; p.clip_start = v.clip_start;
    p.hist = v.hist; p.wave_state = v.wave_state; p.stft = dst.stft; p.ctx = dst.ctx;
    Sections secs{p.sec};
    for (int q = 0; q < v.nseq; ++q) {
        const SeqView& s = v.seq[q];
        SeedSeqDev& d = p.seq[q];
        d.H = s.H; d.HP = (s.H + 63) / 64 * 64; d.units = s.units;
        if (s.cumulative) {
            if (bad(dst.cum[q], 4)) return SFSN_EINVAL;
            d.cum = s.cum; d.cum_d = dst.cum[q];
        }
        for (int l = 0; l < s.n_layers; ++l) {
            const sfsn_seed_layer& o = dst.layer[q][l];
            if (bad(o.h, 16) || bad(o.c, 16)) return SFSN_EINVAL;
            d.layer[l].h = s.h[l]; d.layer[l].c = s.c[l]; d.layer[l].hd = o.h; d.layer[l].cd = o.c;
            secs.add(SEC_ROWS, q, l, n_clips * s.units * (s.H / 4));
        }
    }
    if (D > 0) secs.add(SEC_HIST, 0, 0, n_clips * v.F * D);
    if (v.wave) secs.add(SEC_WAVE, 0, 0, n_clips * SEED_CTX);
    p.nsec = secs.nsec;
    hipLaunchKernelGGL(hop_seed_kernel, dim3(secs.blk), dim3(PRIME_THREADS), 0, static_cast<hipStream_t>(stream), p);
    return hip_ok(hipGetLastError());
}

// cont: the continuing form (the clips are running: src's rows have T frames, blocks go to wave_out); else the clips begin with the
// N frames.  The sources may be NULL where N == 0 leaves nothing to read.
static int take_launch(const HopView& v, const int* clips, int n_clips, const TakeSrc& src, bool cont, void* stream) {
    TakeParams p;
    memset(&p, 0, sizeof(p));
    const int rc = check_clips(v.B, clips, n_clips, p.clips);
    if (rc != SFSN_OK) return rc;
    const int N = src.N, D = v.D;
    if (cont && src.T < N + D) return SFSN_EINVAL;
    if (src.Bp < 1 || src.b0 < 0 || n_clips > src.Bp - src.b0) return SFSN_EINVAL;
    if (D > 0 && N > 0 && bad(src.stft, 8)) return SFSN_EINVAL;
    if (v.wave && (bad(src.tail, 4) || (N > 0 && (bad(src.enh, 8) || (cont && bad(src.wave_out, 8)))))) return SFSN_EINVAL;
    if (!state_ok(v, true)) return SFSN_EINVAL;
    p.n_clips = n_clips; p.b0 = src.b0; p.Bp = src.Bp; p.N = N;
    p.F = v.F; p.S = v.S; p.D = D; p.fcov = v.fcov;
    p.stft = src.stft; p.enh = src.enh; p.tail = src.tail;
    p.hist = v.hist; p.wave_state = v.wave_state; p.ola_state = v.ola_state; p.window = v.window;
    if (cont) {
        p.T = src.T; p.frame_index = v.frame_index; p.k = v.k; p.span = v.span; p.clip_start = v.clip_start; p.wave_out = src.wave_out;
    }
    Sections secs{p.sec};
    size_t slot0 = 0;
    for (int q = 0; q < v.nseq; ++q) {
        const SeqView& s = v.seq[q];
        TakeSeqDev& d = p.seq[q];
        d.H = s.H; d.HP = (s.H + 63) / 64 * 64; d.units = s.units;
        if (s.cumulative) {
            if (N > 0 && bad(src.cum[q], 4)) return SFSN_EINVAL;
            d.cum = s.cum; d.cum_src = src.cum[q];
        }
        for (int l = 0; l < s.n_layers; ++l) {
            const sfsn_prime_layer& o = src.layer[q][l];
            if (N > 0 && (bad(o.spikes_i8, 4) || bad(o.c, 16))) return SFSN_EINVAL;
            d.layer[l].h = s.h[l]; d.layer[l].c = s.c[l]; d.layer[l].s8 = o.spikes_i8; d.layer[l].csrc = o.c;
            d.layer[l].slots = v.spike_slots ? v.spike_slots + slot0 : nullptr;
            slot0 += (size_t)v.B * s.units * (s.H / 4);
            secs.add(SEC_ROWS, q, l, n_clips * s.units * (s.H / 4));
        }
    }
    if (D > 0 && v.fcov > 0) secs.add(SEC_HIST, 0, 0, n_clips * v.fcov * D);
    if (v.wave) {
        secs.add(SEC_WAVE, 0, 0, n_clips * FFT_NFFT);
        secs.add(SEC_OLA, 0, 0, n_clips * v.S, PRIME_WAVES);
    }
    p.nsec = secs.nsec;
    if (cont)
        hipLaunchKernelGGL(hop_take_kernel<true>, dim3(secs.blk), dim3(PRIME_THREADS), 0, static_cast<hipStream_t>(stream), p);
    else
        hipLaunchKernelGGL(hop_take_kernel<false>, dim3(secs.blk), dim3(PRIME_THREADS), 0, static_cast<hipStream_t>(stream), p);
    return hip_ok(hipGetLastError());
}

// the sub-band sources: sfsn_prime_src and sfsn_advance_src name these fields alike
template <class Src>
static TakeSrc take_src(const Src& s, int n_groups) {
    TakeSrc t;
    memset(&t, 0, sizeof(t));
    t.Bp = s.Bp; t.N = s.N; t.b0 = s.b0; t.T = s.N;
    t.stft = s.stft_ri; t.enh = s.enh_ri; t.tail = s.wave_tail;
    for (int q = 0; q < 1 + n_groups; ++q) {
        const sfsn_prime_seq& ps = q == 0 ? s.fb : s.sb[q - 1];
        t.layer[q] = ps.layer; t.cum[q] = ps.cum;
    }
    return t;
}

// sfsn_seed_dst and sfsn_fullband_seed_dst likewise
template <class Dst>
static SeedDst seed_dst(const Dst& d) {
    SeedDst t;
    memset(&t, 0, sizeof(t));
    t.Bp = d.Bp; t.T = d.T; t.b0 = d.b0; t.wave_stride = d.wave_stride; t.stft = d.stft_ri; t.ctx = d.wave_ctx;
    return t;
}

extern "C" int sfsn_hop_prime(const sfsn_hop_desc* desc, const int* clips, int n_clips, const sfsn_prime_src* src, void* stream) {
    if (!desc || !clips || !src || n_clips <= 0) return SFSN_EINVAL;
    HopView v;
    const int rc = view_of(desc, v);
    if (rc != SFSN_OK) return rc;
    // (N = 0, waveform mode: a clip whose one call of samples has made no frame yet)
    if (src->N < 0 || (!v.wave && src->N < desc->hop) || src->N % desc->hop != 0) return SFSN_EINVAL;
    return take_launch(v, clips, n_clips, take_src(*src, desc->n_groups), false, stream);
}

extern "C" int sfsn_hop_seed(const sfsn_hop_desc* desc, const int* clips, int n_clips, const sfsn_seed_dst* dst, void* stream) {
    if (!desc || !clips || !dst || n_clips <= 0) return SFSN_EINVAL;
    HopView v;
    const int rc = view_of(desc, v);
    if (rc != SFSN_OK) return rc;
    SeedDst t = seed_dst(*dst);
    for (int q = 0; q < v.nseq; ++q) {
        const sfsn_seed_seq& ds = q == 0 ? dst->fb : dst->sb[q - 1];
        t.layer[q] = ds.layer; t.cum[q] = ds.cum;
    }
    return seed_launch(v, clips, n_clips, t, stream);
}

extern "C" int sfsn_hop_advance(const sfsn_hop_desc* desc, const int* clips, int n_clips, const sfsn_advance_src* src, void* stream) {
    if (!desc || !clips || !src || n_clips <= 0) return SFSN_EINVAL;
    HopView v;
    const int rc = view_of(desc, v);
    if (rc != SFSN_OK) return rc;
    if (src->N < desc->hop || src->N % desc->hop != 0) return SFSN_EINVAL;
    TakeSrc t = take_src(*src, desc->n_groups);
    t.T = src->T; t.wave_out = src->wave_out;
    return take_launch(v, clips, n_clips, t, true, stream);
}

extern "C" int sfsn_hop_advance_ragged(const sfsn_hop_desc* desc, const int* clips, int n_clips, const sfsn_advance_ragged_src* src, void* stream) {
    if (!desc || !clips || !src || n_clips <= 0) return SFSN_EINVAL;
    HopView v;
    int rc = view_of(desc, v);
    if (rc != SFSN_OK) return rc;
    for (int q = 0; q < v.nseq; ++q)
        if (v.seq[q].cumulative) return SFSN_EUNSUPPORTED;  // (no running sums after a clip's own last frame: one sfsn_hop_advance per length)
    TakeRaggedParams p;
    memset(&p, 0, sizeof(p));
    rc = check_clips(v.B, clips, n_clips, p.clips);
    if (rc != SFSN_OK) return rc;
    const int Nmax = src->Nmax, D = v.D;
    if (Nmax < desc->hop || Nmax % desc->hop != 0 || src->T < Nmax + D) return SFSN_EINVAL;
    if (src->Bp < 1 || src->b0 < 0 || n_clips > src->Bp - src->b0) return SFSN_EINVAL;
    if (bad(src->frames, 4) || (D > 0 && bad(src->stft_ri, 8))) return SFSN_EINVAL;
    if (v.wave && (bad(src->wave_ctx, 4) || src->wave_stride < SEED_CTX + 128 * Nmax || bad(src->enh_ri, 8) || bad(src->wave_out, 8))) return SFSN_EINVAL;
    if (!state_ok(v, true)) return SFSN_EINVAL;
    p.n_clips = n_clips; p.b0 = src->b0; p.Bp = src->Bp; p.Nmax = Nmax; p.T = src->T;
    p.F = v.F; p.S = v.S; p.D = D; p.fcov = v.fcov; p.frame_index = v.frame_index; p.ctx_stride = src->wave_stride; p.k = v.k;
    p.frames = src->frames; p.stft = src->stft_ri; p.enh = src->enh_ri; p.ctx = src->wave_ctx;
    p.hist = v.hist; p.wave_state = v.wave_state; p.ola_state = v.ola_state; p.window = v.window;
    p.clip_start = v.clip_start; p.wave_out = src->wave_out;
    Sections secs{p.sec};
    size_t slot0 = 0;
    for (int q = 0; q < v.nseq; ++q) {
        const SeqView& s = v.seq[q];
        const sfsn_ragged_seq& rs = q == 0 ? src->fb : src->sb[q - 1];
        TakeRaggedSeqDev& d = p.seq[q];
        d.H = s.H; d.HP = (s.H + 63) / 64 * 64; d.units = s.units;
        for (int l = 0; l < s.n_layers; ++l) {
            const sfsn_ragged_layer& o = rs.layer[l];
            if (bad(o.spikes_i8, 4) || bad(o.membrane, 16)) return SFSN_EINVAL;
            d.layer[l].h = s.h[l]; d.layer[l].c = s.c[l]; d.layer[l].s8 = o.spikes_i8; d.layer[l].mem = o.membrane;
            d.layer[l].slots = v.spike_slots ? v.spike_slots + slot0 : nullptr;
            slot0 += (size_t)v.B * s.units * (s.H / 4);
            secs.add(SEC_ROWS, q, l, n_clips * s.units * (s.H / 4));
        }
    }
    if (D > 0 && v.fcov > 0) secs.add(SEC_HIST, 0, 0, n_clips * v.fcov * D);
    if (v.wave) {
        secs.add(SEC_WAVE, 0, 0, n_clips * FFT_NFFT);
        secs.add(SEC_OLA, 0, 0, n_clips * v.S, PRIME_WAVES);
    }
    p.nsec = secs.nsec;
    hipLaunchKernelGGL(hop_take_ragged_kernel, dim3(secs.blk), dim3(PRIME_THREADS), 0, static_cast<hipStream_t>(stream), p);
    return hip_ok(hipGetLastError());
}

// The same two launches for the cIRM-GSN hop.  Waveform mode (wave_state != NULL) takes every frame index from desc->clip_start.
extern "C" int sfsn_fullband_hop_seed(const sfsn_fullband_hop_desc* desc, const unsigned* spike_slots, const float* wave_state, const int* clips,
                                      int n_clips, const sfsn_fullband_seed_dst* dst, void* stream) {
    if (!desc || !clips || !dst || n_clips < 1) return SFSN_EINVAL;
    HopView v;
    const int rc = view_of(desc, const_cast<unsigned*>(spike_slots), const_cast<float*>(wave_state), nullptr, nullptr, v);  // (the seed launch reads them)
    if (rc != SFSN_OK) return rc;
    if (v.wave && !desc->clip_start) return SFSN_EINVAL;
    SeedDst t = seed_dst(*dst);
    t.layer[0] = dst->layer;
    return seed_launch(v, clips, n_clips, t, stream);
}

extern "C" int sfsn_fullband_hop_advance(const sfsn_fullband_hop_desc* desc, unsigned* spike_slots, float* wave_state, float* ola_state,
                                         const int* clips, int n_clips, const sfsn_fullband_advance_src* src, void* stream) {
    if (!desc || !clips || !src || n_clips < 1) return SFSN_EINVAL;
    if ((wave_state != nullptr) != (ola_state != nullptr)) return SFSN_EINVAL;
    HopView v;
    const int rc = view_of(desc, spike_slots, wave_state, ola_state, src->window, v);
    if (rc != SFSN_OK) return rc;
    if (v.wave && !desc->clip_start) return SFSN_EINVAL;
    // (N = 0, waveform mode: the clip without a call whose backlog is one call -- its samples enter wave_state and make no frame)
    if (src->N < 0 || (!v.wave && src->N < desc->hop) || src->N % desc->hop != 0) return SFSN_EINVAL;
    TakeSrc t;
    memset(&t, 0, sizeof(t));
    t.Bp = src->Bp; t.N = src->N; t.b0 = src->b0; t.T = src->T;
    t.stft = src->stft_ri; t.enh = src->enh_ri; t.tail = src->wave_tail; t.wave_out = src->wave_out;
    t.layer[0] = src->layer;
    return take_launch(v, clips, n_clips, t, true, stream);
}

extern "C" int sfsn_fullband_hop_advance_ragged(const sfsn_fullband_hop_desc* desc, unsigned* spike_slots, float* wave_state, float* ola_state,
                                                const int* clips, int n_clips, const sfsn_fullband_advance_ragged_src* src, void* stream) {
    if (!desc || !clips || !src || n_clips < 1) return SFSN_EINVAL;
    if ((wave_state != nullptr) != (ola_state != nullptr)) return SFSN_EINVAL;
    HopView v;
    int rc = view_of(desc, spike_slots, wave_state, ola_state, src->window, v);
    if (rc != SFSN_OK) return rc;
    if (v.wave && !desc->clip_start) return SFSN_EINVAL;
    if (n_clips > v.B) return SFSN_EINVAL;  // (distinct indices below B <= 16: FullbandTakeRaggedParams::clips holds them)
    FullbandTakeRaggedParams p;
    memset(&p, 0, sizeof(p));
    unsigned short listed[PRIME_MAX_CLIPS];
    rc = check_clips(v.B, clips, n_clips, listed);
    if (rc != SFSN_OK) return rc;
    for (int i = 0; i < n_clips; ++i) p.clips[i] = listed[i];
    const int Nmax = src->Nmax, D = v.D;
    if (Nmax < desc->hop || Nmax % desc->hop != 0 || src->T < Nmax + D) return SFSN_EINVAL;
    if (src->Bp < 1 || src->b0 < 0 || n_clips > src->Bp - src->b0) return SFSN_EINVAL;
    if (bad(src->frames, 4) || (D > 0 && bad(src->stft_ri, 8))) return SFSN_EINVAL;
    if (v.wave && (bad(src->wave_ctx, 4) || src->wave_stride < SEED_CTX + 128 * Nmax || bad(src->enh_ri, 8) || bad(src->wave_out, 8))) return SFSN_EINVAL;
    if (!state_ok(v, true)) return SFSN_EINVAL;
    p.n_clips = n_clips; p.b0 = src->b0; p.Bp = src->Bp; p.Nmax = Nmax; p.T = src->T;
    p.F = v.F; p.S = v.S; p.D = D; p.fcov = v.fcov; p.frame_index = v.frame_index; p.ctx_stride = src->wave_stride; p.k = v.k; p.span = v.span;
    p.frames = src->frames; p.stft = src->stft_ri; p.enh = src->enh_ri; p.ctx = src->wave_ctx;
    p.hist = v.hist; p.wave_state = v.wave_state; p.ola_state = v.ola_state; p.window = v.window;
    p.clip_start = v.clip_start; p.wave_out = src->wave_out;
    Sections secs{p.sec};
    const SeqView& s = v.seq[0];
    FullbandTakeRaggedSeqDev& d = p.seq[0];
    d.H = s.H; d.HP = (s.H + 63) / 64 * 64; d.units = 1;
    for (int l = 0; l < s.n_layers; ++l) {
        const sfsn_ragged_layer& o = src->layer[l];
        if (bad(o.spikes_i8, 4) || bad(o.membrane, 16)) return SFSN_EINVAL;
        d.layer[l].h = s.h[l]; d.layer[l].c = s.c[l]; d.layer[l].s8 = o.spikes_i8; d.layer[l].mem = o.membrane;
        d.layer[l].slots = v.spike_slots ? v.spike_slots + (size_t)l * v.B * (s.H / 4) : nullptr;
        secs.add(SEC_ROWS, 0, l, n_clips * (s.H / 4));
    }
    if (D > 0) secs.add(SEC_HIST, 0, 0, n_clips * v.F * D);
    if (v.wave) {
        secs.add(SEC_WAVE, 0, 0, n_clips * FFT_NFFT);
        secs.add(SEC_OLA, 0, 0, n_clips * v.S, PRIME_WAVES);
    }
    p.nsec = secs.nsec;
    hipLaunchKernelGGL(fullband_take_ragged_kernel, dim3(secs.blk), dim3(PRIME_THREADS), 0, static_cast<hipStream_t>(stream), p);
    return hip_ok(hipGetLastError());
}
