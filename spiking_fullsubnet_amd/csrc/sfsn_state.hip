// sfsn_state.hip -- the carried state of listed clips of a one-launch streaming hop (sfsn_hop.hip, sfsn_fullband_hop.hip) out into a
// self-contained per-clip blob and back, each way in ONE launch (gfx950 only).
//
// A clip that has streamed N frames holds exactly what sfsn_hop_prime (sfsn_prime.hip) writes: every layer's last spikes (the half of
// the double buffer the next launch reads), the membranes, the running sums of the cumulative norm, the spike slots, the last D noisy
// frames and, in waveform mode, the last 512 samples and the overlap-add partial sums.  Priming re-derives that from a recorded
// prefix; here it is COPIED, so a clip moved to another slot or another session continues bit for bit, layer 0 included.
//
// The blob is free of launch parity (include/sfsn.h states it byte for byte): a list of sections, each a clip's rows of one array.
// One kernel serves both directions and both hops: the host turns a descriptor into sections {array, clip stride, row stride, row
// bytes, rows per clip, offset in the blob}; sections lie in block order, as in hop_take_kernel; a lane copies one vector of a row --
// 16 bytes where the array's address and strides allow (one lane per 4 neurons of a membrane row), else 8 or 4 (a lane per 4 neurons
// of a spike row whose pitch is not a multiple of 16).  Plain stores only: the launch boundary publishes them.  Nothing waits inside
// the launch; the tagged scratch of the hop (spikes, spec_g, enh_g, z0) is not touched and launch_index does not move.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "sfsn.h"

#include "sfsn_host.h"

#define STATE_THREADS 256
#define STATE_MAX_CLIPS 256  // clip indices travel in the kernel arguments (16 bits each)
// sfsn_hop_desc: (h, c, slots) per sequence and layer, cum per sequence, hist, wave, ola
#define STATE_MAX_SECS ((1 + SFSN_HOP_MAX_GROUPS) * (3 * SFSN_HOP_MAX_LAYERS + 1) + 3)

struct StateSecDev {
    char* state;           // the session's array: for a double-buffered one the half the next launch reads
    unsigned clip_stride;  // bytes from a clip's first row to the next clip's
    unsigned row_stride;   // bytes from row to row inside a clip
    unsigned row_bytes;    // bytes of a row that are state (the blob holds the rows back to back)
    unsigned rows;         // rows per clip
    unsigned blob_off;     // of the section inside a clip's blob (a multiple of 16)
    unsigned vec;          // bytes a lane copies: 16, 8 or 4 (divides row_bytes, both strides and the array's address)
    unsigned items;        // n_clips * rows * row_bytes / vec
    int blk0;
};
struct StateParams {
    StateSecDev sec[STATE_MAX_SECS];
    unsigned short clips[STATE_MAX_CLIPS];
    char* blob;    // [..][bytes]
    size_t bytes;  // of one clip's blob (a multiple of 16)
    int nsec, n_clips, b0, to_state;
};
static_assert(sizeof(StateParams) <= 4096, "StateParams travels as a kernel argument");

__global__ __launch_bounds__(STATE_THREADS) void hop_state_kernel(const StateParams p) {
    int si = 0;
    for (int i = 1; i < p.nsec; ++i)
        if ((int)blockIdx.x >= p.sec[i].blk0) si = i;  // (block-uniform: sections are in block order)
    const StateSecDev& s = p.sec[si];
    const unsigned item = (unsigned)((int)blockIdx.x - s.blk0) * STATE_THREADS + threadIdx.x;
    if (item >= s.items) return;
    const unsigned per_row = s.row_bytes / s.vec, per_clip = per_row * s.rows;
    const unsigned i = item / per_clip, r = item - i * per_clip;
    const unsigned k = r / per_row, x = (r - k * per_row) * s.vec;
    char* st = s.state + (size_t)p.clips[i] * s.clip_stride + (size_t)k * s.row_stride + x;
    char* bl = p.blob + (size_t)(p.b0 + (int)i) * p.bytes + s.blob_off + (size_t)k * s.row_bytes + x;
    const char* src = p.to_state ? bl : st;
    char* dst = p.to_state ? st : bl;
    if (s.vec == 16)
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
    else if (s.vec == 8)
        *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(src);
    else
        *reinterpret_cast<unsigned*>(dst) = *reinterpret_cast<const unsigned*>(src);
}

// =====================================================================================================================
// host side
// =====================================================================================================================
// The sections of a descriptor in blob order.  The sizing calls run it without looking at a pointer; the launches check them.
struct StateLayout {
    StateParams p;
    size_t off = 0;
    int blk = 0, n_clips = 0, rc = SFSN_OK;
    bool sizing = true;

    void add(const void* state, size_t clip_stride, size_t row_stride, size_t row_bytes, size_t rows) {
        off = (off + 15) & ~(size_t)15;
        const size_t at = off;
        off += rows * row_bytes;
        if (sizing || rc != SFSN_OK) return;
        const uintptr_t a = reinterpret_cast<uintptr_t>(state);
        if (!state || ((a | clip_stride | row_stride | row_bytes) & 3u)) {
            rc = SFSN_EINVAL;
            return;
        }
        const uintptr_t m = a | clip_stride | row_stride | row_bytes;
        StateSecDev& s = p.sec[p.nsec++];
        s.state = static_cast<char*>(const_cast<void*>(state));
        s.clip_stride = (unsigned)clip_stride; s.row_stride = (unsigned)row_stride; s.row_bytes = (unsigned)row_bytes;
        s.rows = (unsigned)rows; s.blob_off = (unsigned)at;
        s.vec = (m & 15u) == 0 ? 16u : ((m & 7u) == 0 ? 8u : 4u);
        s.items = (unsigned)((size_t)n_clips * rows * (row_bytes / s.vec));
        s.blk0 = blk;
        blk += (int)((s.items + STATE_THREADS - 1) / STATE_THREADS);
    }
    size_t bytes() const { return (off + 15) & ~(size_t)15; }
};

// sfsn_hop_desc: include/sfsn.h, "Blob of sfsn_hop_state_export"
static void hop_state_layout(StateLayout& y, const sfsn_hop_desc* d) {
    const unsigned par = d->launch_index & 1u;
    const int nseq = 1 + d->n_groups;
    int fcov = 0;
    for (int q = 0; q < nseq; ++q) {
        const sfsn_hop_seq& hs = q == 0 ? d->fb : d->sb[q - 1];
        const size_t H = hs.H, HP = (H + 63) / 64 * 64, units = hs.feat.n_units;
        if (q > 0 && hs.feat.lo + hs.feat.n_units * hs.fc > fcov) fcov = hs.feat.lo + hs.feat.n_units * hs.fc;
        for (int l = 0; l < hs.n_layers; ++l) {
            y.add(hs.layer[l].h[par], units * HP, HP, H, units);
            y.add(hs.layer[l].c, units * H * 4, units * H * 4, units * H * 4, 1);
        }
    }
    for (int q = 0; q < nseq; ++q) {
        const sfsn_hop_seq& hs = q == 0 ? d->fb : d->sb[q - 1];
        const size_t units = hs.feat.n_units;
        if (hs.feat.norm == SFSN_NORM_CUMLAPLACE) y.add(hs.cum[par], units * 4, units * 4, units * 4, 1);
    }
    if (d->spike_slots) {
        size_t slot0 = 0;
        for (int q = 0; q < nseq; ++q) {
            const sfsn_hop_seq& hs = q == 0 ? d->fb : d->sb[q - 1];
            const size_t n = (size_t)hs.feat.n_units * (hs.H / 4);  // a clip's slots of one layer
            for (int l = 0; l < hs.n_layers; ++l) {
                y.add(d->spike_slots + slot0, n * 4, n * 4, n * 4, 1);
                slot0 += (size_t)d->B * n;
            }
        }
    }
    if (d->D > 0 && fcov > 0) y.add(d->hist_ri, (size_t)d->F * d->D * 8, (size_t)d->F * d->D * 8, (size_t)fcov * d->D * 8, 1);
    if (d->wave_in) {
        y.add(d->wave_state, 2048, 2048, 2048, 1);
        y.add(d->ola_state, (size_t)d->S * 2048, (size_t)d->S * 2048, (size_t)d->S * 2048, 1);
    }
}

// sfsn_fullband_hop_desc: include/sfsn.h, "Blob of sfsn_fullband_hop_state_export"
static void fullband_state_layout(StateLayout& y, const sfsn_fullband_hop_desc* d, const unsigned* slots, bool counted, const float* wave_state,
                                  const float* ola_state, bool wave) {
    const unsigned par = d->launch_index & 1u;
    const size_t Hp = d->Hp, HP8 = (Hp + 63) / 64 * 64;
    for (int l = 0; l < d->n_layers; ++l) {
        y.add(d->layer[l].h[par], HP8, HP8, Hp, 1);
        y.add(d->layer[l].c, Hp * 4, Hp * 4, Hp * 4, 1);
    }
    if (counted)
        for (int l = 0; l < d->n_layers; ++l) y.add(slots ? slots + (size_t)l * d->B * (Hp / 4) : nullptr, Hp, Hp, Hp, 1);
    if (d->D > 0) y.add(d->hist_ri[par], (size_t)d->F * d->D * 8, (size_t)d->F * d->D * 8, (size_t)d->F * d->D * 8, 1);
    if (wave) {
        y.add(wave_state, 2048, 2048, 2048, 1);
        y.add(ola_state, (size_t)d->S * 2048, (size_t)d->S * 2048, (size_t)d->S * 2048, 1);
    }
}

// the argument checks both hops share, in the order the header lists them; fills p.clips
static int state_args(StateParams& p, int B, const int* clips, int n_clips, const void* blob, int b0) {
    if (n_clips < 1 || b0 < 0 || !aligned16(blob)) return SFSN_EINVAL;
    if (B > 65535 || n_clips > STATE_MAX_CLIPS) return SFSN_EUNSUPPORTED;  // (the caller splits a longer list)
    for (int i = 0; i < n_clips; ++i) {
        if (clips[i] < 0 || clips[i] >= B) return SFSN_EINVAL;
        for (int j = 0; j < i; ++j)
            if (clips[j] == clips[i]) return SFSN_EINVAL;  // (import: two lanes would own one row)
        p.clips[i] = (unsigned short)clips[i];
    }
    return SFSN_OK;
}

static int state_launch(StateLayout& y, void* blob, int b0, int to_state, void* stream) {
    if (y.rc != SFSN_OK) return y.rc;
    StateParams& p = y.p;
    p.blob = static_cast<char*>(blob); p.bytes = y.bytes(); p.n_clips = y.n_clips; p.b0 = b0; p.to_state = to_state;
    if (p.nsec == 0 || y.blk == 0) return SFSN_EUNSUPPORTED;
    hipLaunchKernelGGL(hop_state_kernel, dim3(y.blk), dim3(STATE_THREADS), 0, static_cast<hipStream_t>(stream), p);
    return hip_ok(hipGetLastError());
}

extern "C" size_t sfsn_hop_state_bytes(const sfsn_hop_desc* desc) {
    if (!desc || sfsn_hop_spike_slots(desc) == 0) return 0;  // (its plan validates the geometry: host only)
    StateLayout y;
    hop_state_layout(y, desc);
    return y.bytes();
}

static int hop_state_move(const sfsn_hop_desc* desc, const int* clips, int n_clips, void* blob, int b0, int to_state, void* stream) {
    if (!desc || !clips || !blob) return SFSN_EINVAL;
    if (desc->n_groups < 1 || desc->n_groups > SFSN_HOP_MAX_GROUPS) return SFSN_EUNSUPPORTED;
    if (sfsn_hop_spike_slots(desc) == 0) return SFSN_EUNSUPPORTED;  // a descriptor sfsn_stream_hop would not run
    StateLayout y;
    memset(&y.p, 0, sizeof(y.p));
    const int rc = state_args(y.p, desc->B, clips, n_clips, blob, b0);
    if (rc != SFSN_OK) return rc;
    y.sizing = false; y.n_clips = n_clips;
    hop_state_layout(y, desc);
    return state_launch(y, blob, b0, to_state, stream);
}

extern "C" int sfsn_hop_state_export(const sfsn_hop_desc* desc, const int* clips, int n_clips, void* blob, void* stream) {
    return hop_state_move(desc, clips, n_clips, blob, 0, 0, stream);
}

extern "C" int sfsn_hop_state_import(const sfsn_hop_desc* desc, const int* clips, int n_clips, const void* blob, int b0, void* stream) {
    return hop_state_move(desc, clips, n_clips, const_cast<void*>(blob), b0, 1, stream);
}

static bool fullband_state_covered(const sfsn_fullband_hop_desc* d, int wave) {
    if (wave) return d->hop == 1 && d->D == d->df - 1 && sfsn_fullband_wave_hop_check(d->Hp, d->n_layers, d->F, d->S, d->df, d->B, d->unshared) == SFSN_OK;
    return sfsn_fullband_hop_check(d->Hp, d->n_layers, d->F, d->S, d->df, d->B, d->hop, d->D, d->unshared) == SFSN_OK;
}

extern "C" size_t sfsn_fullband_hop_state_bytes(const sfsn_fullband_hop_desc* desc, int counted, int wave) {
    if (!desc || !fullband_state_covered(desc, wave)) return 0;
    if (counted && wave) return 0;  // the waveform launch has no counted form
    StateLayout y;
    fullband_state_layout(y, desc, nullptr, counted != 0, nullptr, nullptr, wave != 0);
    return y.bytes();
}

static int fullband_state_move(const sfsn_fullband_hop_desc* desc, unsigned* slots, float* wave_state, float* ola_state, const int* clips,
                               int n_clips, void* blob, int b0, int to_state, void* stream) {
    if (!desc || !clips || !blob) return SFSN_EINVAL;
    if ((wave_state != nullptr) != (ola_state != nullptr)) return SFSN_EINVAL;
    const bool wave = wave_state != nullptr;
    if (!fullband_state_covered(desc, wave) || (slots && wave)) return SFSN_EUNSUPPORTED;
    StateLayout y;
    memset(&y.p, 0, sizeof(y.p));
    const int rc = state_args(y.p, desc->B, clips, n_clips, blob, b0);
    if (rc != SFSN_OK) return rc;
    y.sizing = false; y.n_clips = n_clips;
    fullband_state_layout(y, desc, slots, slots != nullptr, wave_state, ola_state, wave);
    return state_launch(y, blob, b0, to_state, stream);
}

extern "C" int sfsn_fullband_hop_state_export(const sfsn_fullband_hop_desc* desc, const unsigned* spike_slots, const float* wave_state,
                                              const float* ola_state, const int* clips, int n_clips, void* blob, void* stream) {
    return fullband_state_move(desc, const_cast<unsigned*>(spike_slots), const_cast<float*>(wave_state), const_cast<float*>(ola_state), clips,
                               n_clips, blob, 0, 0, stream);
}

extern "C" int sfsn_fullband_hop_state_import(const sfsn_fullband_hop_desc* desc, unsigned* spike_slots, float* wave_state, float* ola_state,
                                              const int* clips, int n_clips, const void* blob, int b0, void* stream) {
    return fullband_state_move(desc, spike_slots, wave_state, ola_state, clips, n_clips, const_cast<void*>(blob), b0, 1, stream);
}
