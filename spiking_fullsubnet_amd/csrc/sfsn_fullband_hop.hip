// sfsn_fullband_hop.hip -- the streaming hop of the cIRM-GSN model: `hop` new frames of B <= 16 clips through the features, the whole
// GSN stack and the full-spectrum deep filter in ONE launch (gfx950 only).  The plan is sfsn_hop.hip's:
//
//   * an agent is one wave: it owns one 16-neuron tile of one layer for the one 16-row tile (row = clip), keeps that tile's W_hh and
//     W_ih digits in registers and its slice of the membrane in registers for the launch; eight agents share a workgroup;
//   * the stages  input (features + layer 0's input term) -> layer 0 -> ... -> layer nl-1 -> projection + activation + deep filter
//     hand each frame over through L2 as data-tagged sc1 granules the consumer polls directly: spike words as in sfsn_hop.hip,
//     layer 0's input term as 8-byte {value, tag} granules, each polled by the one lane that needs it;
//   * the recurrent product h(t-1).W_hh of a layer is issued before the layer's input arrives;
//   * every weight a wave needs is requested at launch; the last spikes and the deep-filter history are double-buffered by launch
//     parity; the launch index comes from the caller (tag and parity); every spin is bounded (error word, scratch word 0); the launch
//     is refused unless all workgroups can be resident.  Producers have lower block indices than their consumers.
//
// Stage map (recipe: Hp = 272, 4 layers, F = 257, S = 1, df = 3 -> 9 + 12 + 17 = 38 workgroups of 512 threads):
//   input       ceil(Hp / 32) workgroups: 32 neurons' rows of the fp32 W_ih of layer 0 in LDS (the whole matrix, 280 KB at the
//               recipe, is more than one CU's LDS); every one of them forms the B feature rows of a frame itself (a wave per row),
//               then thread (clip, neuron) runs sfsn_fullband_input_proj's single fmaf chain in k order, + bias.
//   layer l     ceil(Hp / 128) workgroups each: the scans' cell, (x.W_ih + b) + h.W_hh with exact int32 digit sums.
//   projection  ceil(F / 16) * S workgroups: (bin block, speaker); wave w owns the coefficient tiles (c, d) = w, w + 8 of its 2 df;
//               activated coefficients to LDS, then thread (clip, bin) adds the taps in ascending d and shifts the bin's history.
//
// Waveform mode (sfsn_fullband_stream_hop_wave; hop == 1, F = 257: 512-point frames, 128 new samples per clip): a second instantiation
// of the kernel with two more roles, sfsn_hop.hip's waveform stages (sfsn_hop_wave_dev.h, one body for both hops):
//   STFT        one workgroup in front of the input role, a wave per clip (two clips per wave when B > 8): the frame's 257 bins leave
//               as {re, tag, im, tag} granules (spec_g); the input role forms its feature rows from them, thread (clip, bin) of the
//               projection role takes its bin once (new-frame tap and the history it writes).
//   inverse     ceil(B S / 8) workgroups behind the projection role, a wave per (clip, speaker): the enhanced bins arrive as granules
//   STFT        (enh_g, written by the projection role), overlap-add against the carried accumulator, 128 samples out, done words.
// Every granule is written in every launch for every clip, whatever the clip's frame index: the consumers wait on all of them.  The
// spectrum kernel is compiled without any of this (template parameter WAVE): its code is what it was (profiles/cirm_streaming.md).
//
// Spike counts (sfsn_fullband_stream_hop_counted): a third kernel, the spectrum hop with the layer role's COUNT form -- every lane that
// stores spikes adds the set bytes of its words over the launch's frames into a slot of its own (include/sfsn.h).  The other two
// kernels are compiled without it.
//
// Held clips (sfsn_fullband_stream_hop_held / _wave_held; include/sfsn.h has the per-row contract): three more kernels -- held, held +
// counted, held waveform -- whose roles carry the mask (one word by value in the kernel arguments, bit b = clip b sits this launch out)
// under `if constexpr (HELD)`.  Every stage, hand-off, granule and tag runs for every row as always; a held row's carried state is not
// written, its h and history cross the launch parity unchanged, its outputs are zero, and the last workgroup to finish moves its origin
// on by one launch (scratch word 3 counts the finished workgroups; nobody waits on it).  The input role keeps no state and has no held
// form.  The three kernels above are compiled without any of this (profiles/device_code_digest.txt).
//
// Arithmetic: sfsn_fullband_dev.h's expressions (shared with the offline kernels) and scan_body's cell: bit-identical to
// FullbandEngine.forward_stft on the concatenated input (tests/test_cirm_streaming.py).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "sfsn.h"

#include "sfsn_scan_dev.h"
#include "sfsn_feat_dev.h"
#include "sfsn_fullband_dev.h"
#include "sfsn_hop_dev.h"
#include "sfsn_hop_wave_dev.h"
#include "sfsn_host.h"

#define FBH_NPW 32      // layer-0 input-term neurons per input workgroup
#define FBH_LDW (FBH_NPW + 1)
#define FBH_NU 5        // feature slots per lane: F <= 320
#define FBH_TPW 2       // coefficient tiles per projection wave: 2 df <= 16
#define FBH_DF_MAX 5
#define FBH_HELD_CNT 3  // scratch word: workgroups of a held launch that have finished (cleared by the last one), as sfsn_hop.hip's

struct FbhLayerDev {
    const int8_t* w_ih;
    const float* w_ih_dq;
    const int8_t* w_hh;
    const float* w_hh_dq;
    const float* bias;
    const float* alpha;
    const float* beta;
    int8_t* h[2];
    float* c;
    int8_t* spikes;
};
struct FbhParams {
    FbhLayerDev layer[SFSN_FULLBAND_HOP_MAX_LAYERS];
    const float* w_ih0;
    const float* ln_w;
    const float* ln_b;
    const int8_t* w_p;
    const float* w_p_dq;
    const float* b_p;
    const float* inp;
    float* hist[2];
    float* enh;
    float* mag;
    float* z0;
    unsigned* cnt;  // [0] error word; [3] held launches: workgroups that have finished (FBH_HELD_CNT)
    const unsigned* clip_start;
    int nl, Hp, KS, NT, B, F, S, df, hop, D, act, NCT, NTT;
    int nwg_in, wpl, nwg_proj, nblocks;
    float fdrc, eps;
    unsigned launch;
    // waveform mode (appended: the spectrum kernel's argument offsets stay what they were)
    const float* wave_in;
    float* wave_state;
    float* ola_state;
    float* wave_out;
    const float* window;
    float* spec_g;
    float* enh_g;
    unsigned* done;
    int nwg_istft;
};

// clip b restarts in this launch: its carried state and history read as zero (sfsn_hop.hip's hop_clip_k == 0)
__device__ __forceinline__ bool fbh_fresh(const FbhParams& p, int b) {
    return p.clip_start && p.launch == __hip_atomic_load(p.clip_start + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// waveform mode: clip b's frame index in this launch, k = launch - clip_start[b] (unsigned difference: wrap-safe).  k == -1: the clip's
// first call, no frame yet; k == 0: its frame 0 (fbh_fresh); its samples come out from k == 2 on.
__device__ __forceinline__ int fbh_clip_k(const FbhParams& p, int b) {
    return (int)(p.launch - __hip_atomic_load(p.clip_start + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
}

// ---------------------------------------------------------------------------------------------------------------------
// input role.  LDS: [ws: F x 33 floats (my neurons' rows of W_ih, k-major)][xs: F x 16 floats (the frame's feature rows, k-major)]
// ---------------------------------------------------------------------------------------------------------------------
template <bool WAVE>
__device__ __forceinline__ void fbh_input_role(const FbhParams& p, char* smem) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int F = p.F, B = p.B, Hp = p.Hp, hop = WAVE ? 1 : p.hop;
    const int n0 = ((int)blockIdx.x - (WAVE ? 1 : 0)) * FBH_NPW;  // (waveform mode: block 0 is the STFT)
    const int nn = Hp - n0 < FBH_NPW ? Hp - n0 : FBH_NPW;
    float* ws = reinterpret_cast<float*>(smem);
    float* xs = ws + F * FBH_LDW;
    const unsigned tagw = hop_tag(p.launch) * 0x02020202u;
    {  // my rows of W_ih, four requests in flight per thread
        const float* src = p.w_ih0 + (size_t)n0 * F;
        const int cnt = nn * F;
        for (int i0 = tid; i0 < cnt; i0 += HOP_THREADS * 4) {
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int idx = i0 + HOP_THREADS * i;
                if (idx > cnt - 1) idx = cnt - 1;
                v[i] = src[idx];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int idx = i0 + HOP_THREADS * i;
                if (idx < cnt) {
                    const int n = idx / F;
                    ws[(idx - n * F) * FBH_LDW + n] = v[i];
                }
            }
        }
    }
    float lw[FBH_NU], lb[FBH_NU];
#pragma unroll
    for (int u = 0; u < FBH_NU; ++u) {
        const int j = lane + 64 * u;
        const bool in = j < F && p.ln_w;
        lw[u] = in ? p.ln_w[j] : 0.0f;
        lb[u] = in ? p.ln_b[j] : 0.0f;
    }
    const int b = tid & 15, nme = tid >> 4;
    const bool mine = nme < nn && b < B;
    const float bias = mine ? p.layer[0].bias[n0 + nme] : 0.0f;
    [[maybe_unused]] bool ok = true;
    for (int t = 0; t < hop; ++t) {
        if (t > 0) __syncthreads();  // the previous frame's chains have read xs
        for (int b_ = wave; b_ < B; b_ += HOP_WAVES) {
            float v[FBH_NU], y[FBH_NU];
#pragma unroll
            for (int u = 0; u < FBH_NU; ++u) {
                const int j = lane + 64 * u;
                v[u] = 0.0f;
                if (j < F) {
                    float2 xc;
                    if constexpr (WAVE)  // (hop == 1) the STFT workgroup's granules
                        xc = hop_take_cplx(p.spec_g + ((size_t)b_ * F + j) * 4, tagw, ok, p.cnt);
                    else
                        xc = *reinterpret_cast<const float2*>(p.inp + (((size_t)b_ * F + j) * hop + t) * 2);
                    v[u] = compress_mag(xc.x, xc.y, p.fdrc);
                }
            }
            fullband_norm_row<FBH_NU>(v, lane, F, p.ln_w != nullptr, lw, lb, p.eps, y);
#pragma unroll
            for (int u = 0; u < FBH_NU; ++u)
                if (lane + 64 * u < F) xs[(lane + 64 * u) * 16 + b_] = y[u];
        }
        __syncthreads();
        if (mine) {  // sfsn_fullband_input_proj: one fmaf chain in k order, then + bias
            float acc = 0.0f;
            for (int k = 0; k < F; ++k) acc = __builtin_fmaf(xs[k * 16 + b], ws[k * FBH_LDW + nme], acc);
            const float z = acc + bias;
            st64_agent(p.z0 + (((size_t)t * B + b) * Hp + n0 + nme) * 2, ((unsigned long long)tagw << 32) | __float_as_uint(z));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// layer role: 8 agents per workgroup (tiles 8 part .. 8 part + 7).  LDS: [64 B][hbA: 5 KB (own layer, frame t-1)][hbB: 5 KB (input)]
// Reuse of the two gather buffers: a wave may write a buffer again only behind a barrier that every wave reaches after its reads of
// the buffer's previous content.  Layers >= 1 gather into hbA and hbB alternately, so each gather's barrier stands between the other
// buffer's reads and its next writes.  Layer 0 has one gather per frame (its input arrives as granules, polled per lane without a
// barrier), so it alternates hbA / hbB by frame parity instead: frame t + 2's writes come behind frame t + 1's barrier, which every
// wave passes after it has read frame t's fragments.
// ---------------------------------------------------------------------------------------------------------------------
// COUNT (sfsn_fullband_stream_hop_counted): the lane also keeps the running spike count of its four neurons of its clip row in the slot
// it alone owns, slots[(l B + row) Hp / 4 + cc / 4] -- requested with the carried state, read as zero where the clip restarts, written
// back once per launch (plain load + store).  Without COUNT nothing of this is compiled: the role is the uncounted launches' code.
// HELD: bit b of `held` = clip b sits this launch out -- its row runs like every row (its spikes are published: every tile gathers all
// rows), but at the end the bytes of h[k & 1] go to h[(k + 1) & 1] instead of the last frame's spikes, and c and the slot stay.
template <bool L0, bool COUNT = false, bool HELD = false>
__device__ __forceinline__ void fbh_layer_role(const FbhParams& p, int l, int part, char* smem, [[maybe_unused]] unsigned* slots = nullptr,
                                               [[maybe_unused]] unsigned held = 0u) {
    const FbhLayerDev& L = p.layer[l];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, q = lane >> 4;
    const int tile_raw = part * HOP_WAVES + wave;
    const bool active = tile_raw < p.NT;
    const int tile = active ? tile_raw : 0;
    const int H = p.Hp, KS = p.KS, NT = p.NT, R = p.B, HP = KS * 64, hop = p.hop;
    const int row = n, rowc = row < R ? row : R - 1;
    const int cc = 16 * tile + 4 * q;
    const unsigned tagw = hop_tag(p.launch) * 0x02020202u;
    char* hbA = smem + 64;
    char* hbB = hbA + HOP_KS_MAX * 1024;

    // ---- everything this wave will need is requested now; the recurrent half's operands first
    const int8_t* hprev = L.h[p.launch & 1u];
    int8_t* hnext = L.h[(p.launch + 1u) & 1u];
    const bool fresh = fbh_fresh(p, rowc);
    v4i h0[HOP_KS_MAX], Whh[3][HOP_KS_MAX], Wih[3][HOP_KS_MAX];
#pragma unroll
    for (int ks = 0; ks < HOP_KS_MAX; ++ks) {
        h0[ks] = v4i{0, 0, 0, 0};
        if (ks < KS && !fresh) h0[ks] = *reinterpret_cast<const v4i*>(hprev + (size_t)rowc * HP + ks * 64 + q * 16);
    }
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int ks = 0; ks < HOP_KS_MAX; ++ks) {
            Whh[d][ks] = v4i{0, 0, 0, 0};
            if (ks < KS) Whh[d][ks] = *reinterpret_cast<const v4i*>(L.w_hh + ((((size_t)d * NT + tile) * KS + ks) * 64 + lane) * 16);
        }
    v4f c = {0.0f, 0.0f, 0.0f, 0.0f};
    if (!fresh) c = *reinterpret_cast<const v4f*>(L.c + (size_t)rowc * H + cc);
    [[maybe_unused]] unsigned nspk = 0;  // COUNT: my slot's value so far, then + the spikes of this launch's frames
    if constexpr (COUNT) {
        if (active && row < R && !fresh) nspk = slots[((size_t)l * R + row) * (H >> 2) + (cc >> 2)];
    }
    const v4f dq = *reinterpret_cast<const v4f*>(L.w_hh_dq + cc);
    const v4f bf = *reinterpret_cast<const v4f*>(L.bias + cc);
    const v4f bg = *reinterpret_cast<const v4f*>(L.bias + H + cc);
    const v4f alpha = *reinterpret_cast<const v4f*>(L.alpha + cc);
    const v4f beta = *reinterpret_cast<const v4f*>(L.beta + cc);
    v4f dqi = {0.0f, 0.0f, 0.0f, 0.0f};
    if (!L0) dqi = *reinterpret_cast<const v4f*>(L.w_ih_dq + cc);
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int ks = 0; ks < HOP_KS_MAX; ++ks) {
            Wih[d][ks] = v4i{0, 0, 0, 0};
            if (!L0 && ks < KS) Wih[d][ks] = *reinterpret_cast<const v4i*>(L.w_ih + ((((size_t)d * NT + tile) * KS + ks) * 64 + lane) * 16);
        }
    v4f db;
#pragma unroll
    for (int r = 0; r < 4; ++r) db[r] = bg[r] - bf[r];

    bool ok = true;
    unsigned pk = 0;
    for (int t = 0; t < hop; ++t) {
        // ---- recurrent half: needs frame t-1 of my own layer only
        v4i a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0}, a2 = {0, 0, 0, 0};
        {
            v4i b[HOP_KS_MAX];
            if (t == 0) {
#pragma unroll
                for (int ks = 0; ks < HOP_KS_MAX; ++ks) b[ks] = h0[ks];
            } else {
                char* hb = (L0 && (t & 1)) ? hbB : hbA;  // (layer 0: by frame parity, see above)
                ok = hop_gather(L.spikes + (size_t)(t - 1) * R * HP, 0, R, KS, H, tagw, hb, b, ok, p.cnt, wave, lane);
            }
#pragma unroll
            for (int ks = 0; ks < HOP_KS_MAX; ++ks)
                if (ks < KS) {
                    a0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(Whh[0][ks], b[ks], a0, 0, 0, 0);
                    a1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(Whh[1][ks], b[ks], a1, 0, 0, 0);
                    a2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(Whh[2][ks], b[ks], a2, 0, 0, 0);
                }
        }
        // ---- input half
        v4f z;
        if constexpr (L0) {  // my four input terms of this frame: {value, tag} granules of the input workgroups
            const float* g = p.z0 + (((size_t)t * R + rowc) * H + cc) * 2;
            for (unsigned spins = 0;; ++spins) {
                bool bad = false;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const unsigned long long w = ld64_agent(g + 2 * r);
                    bad |= (unsigned)(w >> 32) != tagw;
                    z[r] = __uint_as_float((unsigned)w);
                }
                if (!ok || __ballot(bad) == 0) break;
                if (spins > HOP_SPIN_LIMIT) {
                    st_agent(p.cnt, 1u);
                    ok = false;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
        } else {
            v4i b[HOP_KS_MAX];
            ok = hop_gather(p.layer[l - 1].spikes + (size_t)t * R * HP, 0, R, KS, H, tagw, hbB, b, ok, p.cnt, wave, lane);
            v4i i0 = {0, 0, 0, 0}, i1 = {0, 0, 0, 0}, i2 = {0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < HOP_KS_MAX; ++ks)
                if (ks < KS) {
                    i0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(Wih[0][ks], b[ks], i0, 0, 0, 0);
                    i1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(Wih[1][ks], b[ks], i1, 0, 0, 0);
                    i2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(Wih[2][ks], b[ks], i2, 0, 0, 0);
                }
#pragma unroll
            for (int r = 0; r < 4; ++r) z[r] = recombine3(i0[r], i1[r], i2[r]) * dqi[r] + bf[r];  // sfsn_spike_proj's epilogue
        }
        // ---- cell (scan_body's epilogue, shared gate weights)
        pk = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float pre_f = __builtin_fmaf(recombine3(a0[r], a1[r], a2[r]), dq[r], z[r]);
            const float pre_g = pre_f + db[r];
            const float f = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(pre_f * -1.44269504088896341f));
            const float m = __builtin_fmaf(f, c[r] - pre_g, pre_g);
            const float y = __builtin_fmaf(m, alpha[r], beta[r]);
            c[r] = y;
            pk |= (y >= 0.0f) ? (1u << (8 * r)) : 0u;
        }
        if (active && row < R) st_agent(L.spikes + ((size_t)t * R + row) * HP + cc, pk | tagw);  // data + tag: published
        if constexpr (COUNT) nspk += (unsigned)__builtin_popcount(pk);  // (bytes 0/1: a popcount)
    }
    // (the mask is asked here, and the lane's 4 bytes of h[k & 1] are loaded again: nothing more stays live across the frames)
    bool live = true;
    if constexpr (HELD) {
        live = !((held >> rowc) & 1u);
        if (active && row < R && !live) st_agent(hnext + (size_t)row * HP + cc, *reinterpret_cast<const unsigned*>(hprev + (size_t)row * HP + cc));
    }
    if (HELD ? (live && active && row < R) : (active && row < R)) {
        *reinterpret_cast<v4f*>(L.c + (size_t)row * H + cc) = c;
        st_agent(hnext + (size_t)row * HP + cc, pk);
        if constexpr (COUNT) slots[((size_t)l * R + row) * (H >> 2) + (cc >> 2)] = nspk;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// projection + activation + deep filter of one (bin block, speaker).  LDS: [64 B][hb: 5 KB][cbuf: 16 rows x 2 df tiles x 16 floats]
// ---------------------------------------------------------------------------------------------------------------------
// HELD: a held clip's bins leave as zeros (the enhanced granules too, with their tag: the inverse-STFT waves poll them) and its history
// rows cross the launch parity as they are: hist[(k + 1) & 1] <- hist[k & 1], no shift, none of the new frames.
template <bool WAVE, bool HELD = false>
__device__ __forceinline__ void fbh_proj_role(const FbhParams& p, int idx, char* smem, [[maybe_unused]] unsigned held = 0u) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, q = lane >> 4;
    const int S = p.S, df = p.df, F = p.F, B = p.B, D = p.D, hop = WAVE ? 1 : p.hop, KS = p.KS, HP = KS * 64;
    const int fb = idx / S, s_ = idx - fb * S;
    const int ntl = 2 * df;
    const unsigned tagw = hop_tag(p.launch) * 0x02020202u;
    char* hb = smem + 64;
    float* cbuf = reinterpret_cast<float*>(hb + HOP_KS_MAX * 1024);

    v4i Wp[FBH_TPW][3][HOP_KS_MAX];
    v4f dqv[FBH_TPW], bv[FBH_TPW];
#pragma unroll
    for (int i = 0; i < FBH_TPW; ++i) {
        const int jt = wave + HOP_WAVES * i;  // = c * df + d
        const bool have = jt < ntl;
        const int ct = fb * p.NCT + (have ? jt : 0) * S + s_;  // the packed row tile of (c, d, s) in bin block fb
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int ks = 0; ks < HOP_KS_MAX; ++ks) {
                Wp[i][d][ks] = v4i{0, 0, 0, 0};
                if (have && ks < KS) Wp[i][d][ks] = *reinterpret_cast<const v4i*>(p.w_p + ((((size_t)d * p.NTT + ct) * KS + ks) * 64 + lane) * 16);
            }
        dqv[i] = *reinterpret_cast<const v4f*>(p.w_p_dq + ct * 16 + q * 4);
        bv[i] = p.b_p ? *reinterpret_cast<const v4f*>(p.b_p + ct * 16 + q * 4) : v4f{0.0f, 0.0f, 0.0f, 0.0f};
    }
    // thread (clip, bin) of the deep filter: what does not depend on the network is requested before the wait
    const int rl = tid >> 4, bi = tid & 15;
    const int f = fb * 16 + bi;
    const bool mine = tid < 256 && rl < B && f < F;
    const int b_ = mine ? rl : 0, fc = mine ? f : 0;
    const bool fresh = fbh_fresh(p, b_);
    [[maybe_unused]] bool sits = false;  // HELD: my clip sits this launch out
    if constexpr (HELD) sits = (held >> b_) & 1u;
    const float* hrow = p.hist[p.launch & 1u] + ((size_t)b_ * F + fc) * D * 2;
    const float* irow = p.inp + ((size_t)b_ * F + fc) * hop * 2;
    bool ok = true;
    // tap i of [history (D) | new frames (hop)]; a restarted clip's history reads as zero
    auto tap = [&](int i) -> float2 {
        if (i >= D) return *reinterpret_cast<const float2*>(irow + 2 * (i - D));
        return fresh ? make_float2(0.0f, 0.0f) : *reinterpret_cast<const float2*>(hrow + 2 * i);
    };
    float2 tap0[FBH_DF_MAX];
#pragma unroll
    for (int d = 0; d < FBH_DF_MAX; ++d) tap0[d] = (mine && d < df && !(WAVE && d == D)) ? tap(d) : make_float2(0.0f, 0.0f);
    if constexpr (WAVE) {  // (hop == 1) my bin of the new frame, taken once from the STFT workgroup's granules: tap D = df - 1
        const float2 newv = mine ? hop_take_cplx(p.spec_g + ((size_t)b_ * F + fc) * 4, tagw, ok, p.cnt) : make_float2(0.0f, 0.0f);
#pragma unroll
        for (int d = 0; d < FBH_DF_MAX; ++d)
            if (d == D) tap0[d] = newv;
    }

    const int8_t* last = p.layer[p.nl - 1].spikes;
    for (int t = 0; t < hop; ++t) {
        v4i b[HOP_KS_MAX];
        // (for t > 0 the barrier inside also orders the previous frame's reads of cbuf before the writes below)
        ok = hop_gather(last + (size_t)t * B * HP, 0, B, KS, p.Hp, tagw, hb, b, ok, p.cnt, wave, lane);
#pragma unroll
        for (int i = 0; i < FBH_TPW; ++i) {
            const int jt = wave + HOP_WAVES * i;
            if (jt >= ntl) break;
            v4i a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0}, a2 = {0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < HOP_KS_MAX; ++ks)
                if (ks < KS) {
                    a0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(Wp[i][0][ks], b[ks], a0, 0, 0, 0);
                    a1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(Wp[i][1][ks], b[ks], a1, 0, 0, 0);
                    a2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(Wp[i][2][ks], b[ks], a2, 0, 0, 0);
                }
#pragma unroll
            for (int r = 0; r < 4; ++r)
                cbuf[(n * ntl + jt) * 16 + q * 4 + r] = fbd_act(fbd_coef(a0[r], a1[r], a2[r], dqv[i][r], bv[i][r]), p.act);
        }
        __syncthreads();
        if (mine) {
            float yr = 0.0f, yi = 0.0f;
            for (int d = 0; d < df; ++d) {  // filter tap d of frame t is tap t + d of [history | new frames]
                float2 xv = tap0[0];
                if (t == 0) {
#pragma unroll
                    for (int e = 1; e < FBH_DF_MAX; ++e)
                        if (e == d) xv = tap0[e];
                } else {
                    xv = tap(t + d);
                }
                fbd_tap(yr, yi, xv, cbuf[(rl * ntl + d) * 16 + bi], cbuf[(rl * ntl + df + d) * 16 + bi]);
            }
            if constexpr (HELD) {
                if (sits) yr = yi = 0.0f;  // (whatever the taps gave, NaN included)
            }
            const size_t o = (((size_t)rl * S + s_) * F + f) * hop + t;
            if constexpr (WAVE) {  // the enhanced bin to the inverse-STFT wave of (clip, speaker); the spectrum only on request
                hop_put_cplx(p.enh_g + 4 * o, make_float2(yr, yi), tagw);
                if (p.enh) *reinterpret_cast<float2*>(p.enh + 2 * o) = make_float2(yr, yi);
            } else {
                *reinterpret_cast<float2*>(p.enh + 2 * o) = make_float2(yr, yi);
            }
            if (p.mag) p.mag[o] = fbd_mag(yr, yi);
        }
    }
    // the history the next launch reads (the other half of the double buffer): the last D of [history | new frames]
    if (mine && s_ == 0) {
        float* hnext = p.hist[(p.launch + 1u) & 1u] + ((size_t)rl * F + f) * D * 2;
        if constexpr (HELD) {
            if (sits) {  // (the rows as memory holds them, whether or not a restart is due: it is due in the next launch then)
                for (int i = 0; i < D; ++i) *reinterpret_cast<float2*>(hnext + 2 * i) = *reinterpret_cast<const float2*>(hrow + 2 * i);
                return;
            }
        }
        if constexpr (WAVE) {  // (the taps are in registers: history 1 .. D - 1, then the granule taken above)
#pragma unroll
            for (int i = 0; i < FBH_DF_MAX - 1; ++i)
                if (i < D) *reinterpret_cast<float2*>(hnext + 2 * i) = tap0[i + 1];
        } else {
            for (int i = 0; i < D; ++i) *reinterpret_cast<float2*>(hnext + 2 * i) = tap(i + hop);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// waveform mode: the new frame's spectrum (block 0) and the enhanced frame back to samples (the last blocks); sfsn_hop_wave_dev.h
// ---------------------------------------------------------------------------------------------------------------------
// HELD (sfsn_hop_wave_dev.h's held forms): a held clip's wave_state does not move and a first call does not take the samples; its
// samples out are zero, its done word is written all the same, its accumulator is not touched
template <bool HELD = false>
__device__ __forceinline__ void fbh_stft_role(const FbhParams& p, char* smem, [[maybe_unused]] unsigned held = 0u) {
    hop_wave_stft_held<HELD>(p.wave_in, p.wave_state, p.window, p.spec_g, p.F, 0, p.B, hop_tag(p.launch) * 0x02020202u, smem,
                             [&](int ln, int n) { return __ballot(ln < n && fbh_clip_k(p, ln) == -1); },
                             [&](int ci) { return (bool)((held >> ci) & 1u); });
}
template <bool HELD = false>
__device__ __forceinline__ void fbh_istft_role(const FbhParams& p, int wg, char* smem, [[maybe_unused]] unsigned held = 0u) {
    hop_wave_istft_held<HELD>(
        p.ola_state, p.wave_out, p.window, p.enh_g, p.done, p.cnt, p.F, wg, p.B * p.S, hop_tag(p.launch) * 0x02020202u, p.launch + 1u, smem,
        [&](int pair, int& fi, bool& fresh, bool& mute) {
            fi = fbh_clip_k(p, pair / p.S);
            fresh = fi == 0;
            mute = fi < 2;
        },
        [](bool&) {}, [&](int pair) { return (bool)((held >> (pair / p.S)) & 1u); });
}

#ifndef SFSN_FBH_IO_UNIT  // (sfsn_fullband_hop_io.hip includes this file for the roles, the plan and the checks: the kernels and the exports stay here)
__global__ __launch_bounds__(HOP_THREADS) void fullband_stream_hop_kernel(const FbhParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int bi = (int)blockIdx.x;
    if (bi < p.nwg_in) {
        fbh_input_role<false>(p, smem);
        return;
    }
    const int li = bi - p.nwg_in;
    if (li < p.nl * p.wpl) {
        const int l = li / p.wpl, part = li - l * p.wpl;
        if (l == 0)
            fbh_layer_role<true>(p, 0, part, smem);
        else
            fbh_layer_role<false>(p, l, part, smem);
        return;
    }
    fbh_proj_role<false>(p, li - p.nl * p.wpl, smem);
}
// The counting launch, a kernel of its own (sessions that do not count keep the kernel above): the same roles, the layer role with COUNT
__global__ __launch_bounds__(HOP_THREADS) void fullband_stream_hop_counted_kernel(const FbhParams p, unsigned* slots) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int bi = (int)blockIdx.x;
    if (bi < p.nwg_in) {
        fbh_input_role<false>(p, smem);
        return;
    }
    const int li = bi - p.nwg_in;
    if (li < p.nl * p.wpl) {
        const int l = li / p.wpl, part = li - l * p.wpl;
        if (l == 0)
            fbh_layer_role<true, true>(p, 0, part, smem, slots);
        else
            fbh_layer_role<false, true>(p, l, part, smem, slots);
        return;
    }
    fbh_proj_role<false>(p, li - p.nl * p.wpl, smem);
}
// Waveform mode, a kernel of its own (the spectrum kernel keeps its code and its register allocation): the STFT in front, the inverse
// STFT behind -- producers keep lower block indices than their consumers
__global__ __launch_bounds__(HOP_THREADS) void fullband_stream_hop_wave_kernel(const FbhParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int bi = (int)blockIdx.x - 1;
    if (bi < 0) {
        fbh_stft_role(p, smem);
        return;
    }
    if (bi < p.nwg_in) {
        fbh_input_role<true>(p, smem);
        return;
    }
    const int li = bi - p.nwg_in;
    if (li < p.nl * p.wpl) {
        const int l = li / p.wpl, part = li - l * p.wpl;
        if (l == 0)
            fbh_layer_role<true>(p, 0, part, smem);
        else
            fbh_layer_role<false>(p, l, part, smem);
        return;
    }
    const int pi = li - p.nl * p.wpl;
    if (pi < p.nwg_proj) {
        fbh_proj_role<true>(p, pi, smem);
        return;
    }
    fbh_istft_role(p, pi - p.nwg_proj, smem);
}
#endif  // SFSN_FBH_IO_UNIT

// one held launch of one workgroup: the role its block index selects, in the order of the three kernels above.  (They keep their own
// dispatch: routed through this one with HELD = false, the spectrum kernel came out with a 624-byte private segment.)
template <bool WAVE, bool COUNT>
__device__ __forceinline__ void fbh_held_dispatch(const FbhParams& p, [[maybe_unused]] unsigned* slots, unsigned held, char* smem) {
    const int bi = (int)blockIdx.x - (WAVE ? 1 : 0);
    if constexpr (WAVE) {
        if (bi < 0) {
            fbh_stft_role<true>(p, smem, held);
            return;
        }
    }
    if (bi < p.nwg_in) {
        fbh_input_role<WAVE>(p, smem);
        return;
    }
    const int li = bi - p.nwg_in;
    if (li < p.nl * p.wpl) {
        const int l = li / p.wpl, part = li - l * p.wpl;
        if (l == 0)
            fbh_layer_role<true, COUNT, true>(p, 0, part, smem, slots, held);
        else
            fbh_layer_role<false, COUNT, true>(p, l, part, smem, slots, held);
        return;
    }
    const int pi = li - p.nl * p.wpl;
    if constexpr (WAVE) {
        if (pi >= p.nwg_proj) {
            fbh_istft_role<true>(p, pi - p.nwg_proj, smem, held);
            return;
        }
    }
    fbh_proj_role<WAVE, true>(p, pi, smem, held);
}

// The launches with held clips (sfsn_fullband_stream_hop_held / _wave_held): the same roles with the mask compiled in, then the origins.
// clip_start[b] += 1 must come after every read of clip_start in this launch: each workgroup, its role done and nothing of it in flight
// (every origin it asked for has arrived), counts itself in scratch word FBH_HELD_CNT as its last act; the workgroup that finds itself
// last applies the + 1s and clears the word for the next held launch.  Nobody waits on that word.  Every workgroup gets here: a role
// whose bounded wait expired runs on to its end, and the inverse-STFT waves without a pair only leave their role.  The launch boundary
// orders the new origins before the next launch on the stream.  (stream_hop_held_kernel's protocol, sfsn_hop.hip.)
__device__ __forceinline__ void fbh_held_finish(const FbhParams& p, unsigned held, char* smem) {
    __builtin_amdgcn_s_waitcnt(0);  // vmcnt(0) expcnt(0) lgkmcnt(0): nothing of this wave's role is still in flight
    __syncthreads();
    unsigned* fin = p.cnt + FBH_HELD_CNT;
    if (threadIdx.x == 0)
        *reinterpret_cast<unsigned*>(smem) = __hip_atomic_fetch_add(fin, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (*reinterpret_cast<const unsigned*>(smem) != gridDim.x - 1u) return;
    const int b = threadIdx.x;
    if (b < p.B && ((held >> b) & 1u))
        __hip_atomic_fetch_add(const_cast<unsigned*>(p.clip_start) + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (threadIdx.x == 0) st_agent(fin, 0u);
}
#ifndef SFSN_FBH_IO_UNIT
__global__ __launch_bounds__(HOP_THREADS) void fullband_stream_hop_held_kernel(const FbhParams p, unsigned held) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fbh_held_dispatch<false, false>(p, nullptr, held, smem);
    fbh_held_finish(p, held, smem);
}
__global__ __launch_bounds__(HOP_THREADS) void fullband_stream_hop_held_counted_kernel(const FbhParams p, unsigned* slots, unsigned held) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fbh_held_dispatch<false, true>(p, slots, held, smem);
    fbh_held_finish(p, held, smem);
}
__global__ __launch_bounds__(HOP_THREADS) void fullband_stream_hop_wave_held_kernel(const FbhParams p, unsigned held) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fbh_held_dispatch<true, false>(p, nullptr, held, smem);
    fbh_held_finish(p, held, smem);
}
#endif  // SFSN_FBH_IO_UNIT

#ifdef SFSN_FBH_ROLE_KERNELS
// Each role as a kernel of its own, for the compile report only (never launched): the registers of one role, which the combined
// kernel's figure (the maximum over the roles) hides.  `make -B sfsn_fullband_hop.o EXTRA="-DSFSN_FBH_ROLE_KERNELS
// -Rpass-analysis=kernel-resource-usage"` prints them.
__global__ __launch_bounds__(HOP_THREADS) void fbh_role_input_kernel(const FbhParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fbh_input_role<false>(p, smem);
}
__global__ __launch_bounds__(HOP_THREADS) void fbh_role_layer0_kernel(const FbhParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fbh_layer_role<true>(p, 0, (int)blockIdx.x, smem);
}
__global__ __launch_bounds__(HOP_THREADS) void fbh_role_layer_kernel(const FbhParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fbh_layer_role<false>(p, 1, (int)blockIdx.x, smem);
}
__global__ __launch_bounds__(HOP_THREADS) void fbh_role_layer0_counted_kernel(const FbhParams p, unsigned* slots) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fbh_layer_role<true, true>(p, 0, (int)blockIdx.x, smem, slots);
}
__global__ __launch_bounds__(HOP_THREADS) void fbh_role_layer_counted_kernel(const FbhParams p, unsigned* slots) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fbh_layer_role<false, true>(p, 1, (int)blockIdx.x, smem, slots);
}
__global__ __launch_bounds__(HOP_THREADS) void fbh_role_proj_kernel(const FbhParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fbh_proj_role<false>(p, (int)blockIdx.x, smem);
}
// waveform mode's roles
__global__ __launch_bounds__(HOP_THREADS) void fbh_role_wave_input_kernel(const FbhParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fbh_input_role<true>(p, smem);
}
__global__ __launch_bounds__(HOP_THREADS) void fbh_role_wave_proj_kernel(const FbhParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fbh_proj_role<true>(p, (int)blockIdx.x, smem);
}
__global__ __launch_bounds__(HOP_THREADS) void fbh_role_stft_kernel(const FbhParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fbh_stft_role(p, smem);
}
__global__ __launch_bounds__(HOP_THREADS) void fbh_role_istft_kernel(const FbhParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fbh_istft_role(p, (int)blockIdx.x, smem);
}
#endif

// =====================================================================================================================
// host side
// =====================================================================================================================
#ifndef SFSN_FBH_IO_UNIT
extern "C" int sfsn_fullband_hop_check(int Hp, int n_layers, int F, int S, int df, int B, int hop, int D, int unshared) {
    if (Hp <= 0 || n_layers <= 0 || F <= 0 || S <= 0 || df <= 0 || B <= 0 || hop <= 0 || D != df - 1) return SFSN_EINVAL;
    if (unshared) return SFSN_EUNSUPPORTED;  // separate gate weights: twice the digits per agent
    if (Hp % 16 != 0 || Hp > 64 * HOP_KS_MAX || n_layers > SFSN_FULLBAND_HOP_MAX_LAYERS) return SFSN_EUNSUPPORTED;
    if (F <= 192 || F > 64 * FBH_NU) return SFSN_EUNSUPPORTED;  // F <= 192: the offline layer-0 product is the fp32-MFMA form
    if (S > 2 || df > FBH_DF_MAX || 2 * df > FBH_TPW * HOP_WAVES || D + hop > 32 || B > 16) return SFSN_EUNSUPPORTED;
    return SFSN_OK;
}

extern "C" int sfsn_fullband_wave_hop_check(int Hp, int n_layers, int F, int S, int df, int B, int unshared) {
    const int rc = sfsn_fullband_hop_check(Hp, n_layers, F, S, df, B, 1, df - 1, unshared);
    if (rc != SFSN_OK) return rc;
    return F == FFT_F ? SFSN_OK : SFSN_EUNSUPPORTED;  // sfsn_fft_dev.h: 512-point frames, hop 128
}
#endif  // SFSN_FBH_IO_UNIT

static int fbh_plan(FbhParams& p, size_t& lds, const sfsn_fullband_hop_desc* d, bool wave = false) {
    if (!d) return SFSN_EINVAL;
    if (wave && (d->hop != 1 || d->D != d->df - 1)) return SFSN_EINVAL;
    const int rc = wave ? sfsn_fullband_wave_hop_check(d->Hp, d->n_layers, d->F, d->S, d->df, d->B, d->unshared)
                        : sfsn_fullband_hop_check(d->Hp, d->n_layers, d->F, d->S, d->df, d->B, d->hop, d->D, d->unshared);
    if (rc != SFSN_OK) return rc;
    if (d->act < SFSN_ACT_NONE || d->act > SFSN_ACT_RELU || (d->ln_w == nullptr) != (d->ln_b == nullptr)) return SFSN_EINVAL;
    memset(&p, 0, sizeof(p));
    p.nl = d->n_layers; p.Hp = d->Hp; p.KS = (d->Hp + 63) / 64; p.NT = d->Hp / 16;
    p.B = d->B; p.F = d->F; p.S = d->S; p.df = d->df; p.hop = d->hop; p.D = d->D; p.act = d->act;
    p.NCT = 2 * d->df * d->S; p.NTT = (d->F + 15) / 16 * p.NCT;
    p.fdrc = d->fdrc; p.eps = d->ln_eps;
    p.nwg_in = (d->Hp + FBH_NPW - 1) / FBH_NPW;
    p.wpl = (p.NT + HOP_WAVES - 1) / HOP_WAVES;
    p.nwg_proj = (d->F + 15) / 16 * d->S;
    p.nwg_istft = wave ? (d->B * d->S + HOP_WAVES - 1) / HOP_WAVES : 0;
    p.nblocks = p.nwg_in + p.nl * p.wpl + p.nwg_proj + (wave ? 1 + p.nwg_istft : 0);
    const size_t lds_in = (size_t)d->F * (FBH_LDW + 16) * sizeof(float);
    const size_t lds_layer = 64 + (size_t)2 * HOP_KS_MAX * 1024;
    const size_t lds_proj = 64 + (size_t)HOP_KS_MAX * 1024 + (size_t)16 * 2 * d->df * 16 * sizeof(float);
    lds = lds_in > lds_layer ? lds_in : lds_layer;
    if (lds_proj > lds) lds = lds_proj;
    if (wave && HOP_WAVE_LDS_ISTFT > lds) lds = HOP_WAVE_LDS_ISTFT;  // (37 KB: below the input role's 50 KB at F = 257)
    return SFSN_OK;
}

#ifndef SFSN_FBH_IO_UNIT
extern "C" size_t sfsn_fullband_hop_scratch_bytes(const sfsn_fullband_hop_desc* desc) {
    FbhParams p;
    size_t lds;
    return fbh_plan(p, lds, desc) == SFSN_OK ? 64 : 0;  // word 0: the error word; word 3: the held launches' finishing count
}
#endif  // SFSN_FBH_IO_UNIT

static bool aligned8(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7u) == 0; }

#ifndef SFSN_FBH_IO_UNIT
extern "C" size_t sfsn_fullband_hop_spike_slots(const sfsn_fullband_hop_desc* d) {
    if (!d || sfsn_fullband_hop_check(d->Hp, d->n_layers, d->F, d->S, d->df, d->B, d->hop, d->D, d->unshared) != SFSN_OK) return 0;
    return (size_t)d->n_layers * d->B * (d->Hp / 4);
}

// the launch of every mode; w != nullptr: waveform mode (d = &w->hop); slots != nullptr: the counting spectrum launch; held != 0: the
// held kernels (the mask has passed fbh_held_mask)
static int fbh_launch(const sfsn_fullband_hop_desc* d, const sfsn_fullband_wave_desc* w, void* stream, unsigned* slots = nullptr,
                      unsigned held = 0u) {
    FbhParams p;
    size_t lds;
    const int rc = fbh_plan(p, lds, d, w != nullptr);
    if (rc != SFSN_OK) return rc;
    if (!d->w_ih0 || !d->w_p || !d->w_p_dq || !d->z0 || !d->scratch || d->scratch_bytes < 64) return SFSN_EINVAL;
    if (!w && (!d->inp_ri || !d->enh_ri)) return SFSN_EINVAL;
    if (d->D > 0 && (!d->hist_ri[0] || !d->hist_ri[1])) return SFSN_EINVAL;
    bool al = aligned16(d->w_p) && aligned16(d->w_p_dq) && aligned16(d->b_p) && (w || aligned8(d->inp_ri)) && aligned8(d->enh_ri) &&
              aligned8(d->z0) && aligned8(d->hist_ri[0]) && aligned8(d->hist_ri[1]);
    if (w) {
        if (!d->clip_start || !w->wave_in || !w->wave_state || !w->ola_state || !w->wave_out || !w->window || !w->spec_g || !w->enh_g)
            return SFSN_EINVAL;
        al = al && aligned8(w->wave_in) && aligned8(w->wave_state) && aligned8(w->ola_state) && aligned8(w->wave_out) &&
             aligned8(w->window) && aligned8(w->spec_g) && aligned8(w->enh_g) && (reinterpret_cast<uintptr_t>(w->done) & 3u) == 0;
    }
    for (int l = 0; l < d->n_layers; ++l) {
        const sfsn_fullband_hop_layer& L = d->layer[l];
        if (!L.w_hh || !L.w_hh_dq || !L.bias || !L.bn_alpha || !L.bn_beta || !L.h[0] || !L.h[1] || !L.c || !L.spikes) return SFSN_EINVAL;
        if (l > 0 && (!L.w_ih || !L.w_ih_dq)) return SFSN_EINVAL;
        al = al && aligned16(L.w_ih) && aligned16(L.w_ih_dq) && aligned16(L.w_hh) && aligned16(L.w_hh_dq) && aligned16(L.bias) &&
             aligned16(L.bn_alpha) && aligned16(L.bn_beta) && aligned16(L.h[0]) && aligned16(L.h[1]) && aligned16(L.c) && aligned16(L.spikes);
        FbhLayerDev& o = p.layer[l];
        o.w_ih = L.w_ih; o.w_ih_dq = L.w_ih_dq; o.w_hh = L.w_hh; o.w_hh_dq = L.w_hh_dq; o.bias = L.bias; o.alpha = L.bn_alpha;
        o.beta = L.bn_beta; o.h[0] = L.h[0]; o.h[1] = L.h[1]; o.c = L.c; o.spikes = L.spikes;
    }
    if (!al) return SFSN_EINVAL;
    p.w_ih0 = d->w_ih0; p.ln_w = d->ln_w; p.ln_b = d->ln_b; p.w_p = d->w_p; p.w_p_dq = d->w_p_dq; p.b_p = d->b_p;
    p.inp = w ? nullptr : d->inp_ri;
    p.hist[0] = d->hist_ri[0]; p.hist[1] = d->hist_ri[1]; p.enh = d->enh_ri; p.mag = d->enh_mag; p.z0 = d->z0;
    p.cnt = static_cast<unsigned*>(d->scratch);
    p.clip_start = d->clip_start;
    p.launch = d->launch_index;
    if (w) {
        p.wave_in = w->wave_in; p.wave_state = w->wave_state; p.ola_state = w->ola_state; p.wave_out = w->wave_out;
        p.window = w->window; p.spec_g = w->spec_g; p.enh_g = w->enh_g; p.done = w->done;
    }
    // every workgroup must be resident at once (consumers wait for producers): one per compute unit at most
    if (p.nblocks > cu_count()) return SFSN_EUNSUPPORTED;
    if (lds > 160 * 1024) return SFSN_EUNSUPPORTED;
    if (held) {
        const dim3 grid(p.nblocks), block(HOP_THREADS);
        hipStream_t st = static_cast<hipStream_t>(stream);
        if (w) return launch_lds<fullband_stream_hop_wave_held_kernel>(grid, block, lds, st, p, held);
        if (slots) return launch_lds<fullband_stream_hop_held_counted_kernel>(grid, block, lds, st, p, slots, held);
        return launch_lds<fullband_stream_hop_held_kernel>(grid, block, lds, st, p, held);
    }
    if (w) return launch_lds<fullband_stream_hop_wave_kernel>(dim3(p.nblocks), dim3(HOP_THREADS), lds, static_cast<hipStream_t>(stream), p);
    if (slots) return launch_lds<fullband_stream_hop_counted_kernel>(dim3(p.nblocks), dim3(HOP_THREADS), lds, static_cast<hipStream_t>(stream), p, slots);
    return launch_lds<fullband_stream_hop_kernel>(dim3(p.nblocks), dim3(HOP_THREADS), lds, static_cast<hipStream_t>(stream), p);
}

extern "C" int sfsn_fullband_stream_hop(const sfsn_fullband_hop_desc* d, void* stream) { return fbh_launch(d, nullptr, stream); }

extern "C" int sfsn_fullband_stream_hop_counted(const sfsn_fullband_hop_desc* d, unsigned* spike_slots, void* stream) {
    if (!spike_slots || (reinterpret_cast<uintptr_t>(spike_slots) & 3u) != 0) return SFSN_EINVAL;
    return fbh_launch(d, nullptr, stream, spike_slots);
}

extern "C" int sfsn_fullband_stream_hop_wave(const sfsn_fullband_wave_desc* w, void* stream) {
    if (!w) return SFSN_EINVAL;
    return fbh_launch(&w->hop, w, stream);
}
#endif  // SFSN_FBH_IO_UNIT

// ---- held clips: the mask's own checks come first and need no device
static int fbh_held_mask(const sfsn_fullband_hop_desc* d, unsigned held) {
    if (!d) return SFSN_EINVAL;
    if (d->B < 32 && (held >> (d->B > 0 ? d->B : 0)) != 0) return SFSN_EINVAL;  // a bit at or beyond B
    if (!d->clip_start) return SFSN_EINVAL;                                      // a held clip needs an origin of its own
    return SFSN_OK;
}

#ifndef SFSN_FBH_IO_UNIT
extern "C" int sfsn_fullband_stream_hop_held(const sfsn_fullband_hop_desc* d, unsigned* spike_slots, unsigned held_mask, void* stream) {
    if (held_mask == 0) return spike_slots ? sfsn_fullband_stream_hop_counted(d, spike_slots, stream) : sfsn_fullband_stream_hop(d, stream);
    int rc = fbh_held_mask(d, held_mask);
    if (rc != SFSN_OK) return rc;
    FbhParams p;
    size_t lds;
    if ((rc = fbh_plan(p, lds, d)) != SFSN_OK) return rc;  // (a descriptor the plain launch refuses: its code, before the slots are looked at)
    if ((reinterpret_cast<uintptr_t>(spike_slots) & 3u) != 0) return SFSN_EINVAL;
    return fbh_launch(d, nullptr, stream, spike_slots, held_mask);
}

extern "C" int sfsn_fullband_stream_hop_wave_held(const sfsn_fullband_wave_desc* w, unsigned held_mask, void* stream) {
    if (held_mask == 0) return sfsn_fullband_stream_hop_wave(w, stream);
    if (!w) return SFSN_EINVAL;
    const int rc = fbh_held_mask(&w->hop, held_mask);
    if (rc != SFSN_OK) return rc;
    return fbh_launch(&w->hop, w, stream, nullptr, held_mask);
}
#endif  // SFSN_FBH_IO_UNIT
