// sfsn_fullband_hop_io.hip -- the one-launch waveform hop of sfsn_fullband_hop.hip (the cIRM-GSN model) for sessions whose OUTER samples
// differ from the model's: three times the model's rate and / or 16-bit PCM, converted inside the launch
// (sfsn_fullband_stream_hop_wave_io; gfx950 only).
//
// Block 0 and the last blocks are sfsn_hop_wave_dev.h's roles with the conversion in them (hop_wave_stft_io / hop_wave_istft_io, the
// bodies sfsn_hop_io.hip calls for the sibling model: the decimator in front of the frame, the interpolator and the quantiser behind the
// inverse STFT; filters, formats and summation order from sfsn_resample_dev.h, which the stand-alone kernels of sfsn_resample.hip call
// too -- same bits).  Every other role IS the plain hop's: this unit includes sfsn_fullband_hop.hip for its roles, its plan and its
// checks.  That file's kernels and exports are compiled out (SFSN_FBH_IO_UNIT), so the plain hop's unit -- and with it every kernel a
// plain session launches -- is what it was before this unit existed; a translation unit of their own also keeps the optimiser's
// module-wide decisions about the plain kernels away from these.  Dispatch, kernel and launch are restated below for the same reason.
#define SFSN_FBH_IO_UNIT
#undef SFSN_FBH_ROLE_KERNELS  // (the compile report's role kernels belong to the plain unit)
#include "sfsn_fullband_hop.hip"

// RATIO / FMT: the outer samples' rate and format, `io` their buffers; the lambdas are fbh_stft_role's / fbh_istft_role's.
template <bool HELD, int RATIO, int FMT>
__device__ __forceinline__ void fbh_stft_role_io(const FbhParams& p, const HopWaveIo& io, char* smem, [[maybe_unused]] unsigned held) {
    hop_wave_stft_io<HELD, RATIO, FMT>(p.wave_in, p.wave_state, p.window, p.spec_g, p.F, 0, p.B, hop_tag(p.launch) * 0x02020202u, smem, io,
                                       [&](int ln, int n) { return __ballot(ln < n && fbh_clip_k(p, ln) == -1); },
                                       [&](int ci) { return (bool)((held >> ci) & 1u); });
}
template <bool HELD, int RATIO, int FMT>
__device__ __forceinline__ void fbh_istft_role_io(const FbhParams& p, const HopWaveIo& io, int wg, char* smem, [[maybe_unused]] unsigned held) {
    hop_wave_istft_io<HELD, RATIO, FMT>(
        p.ola_state, p.wave_out, p.window, p.enh_g, p.done, p.cnt, p.F, wg, p.B * p.S, hop_tag(p.launch) * 0x02020202u, p.launch + 1u, smem, io,
        [&](int pair, int& fi, bool& fresh, bool& mute) {
            fi = fbh_clip_k(p, pair / p.S);
            fresh = fi == 0;
            mute = fi < 2;
        },
        [](bool&) {}, [&](int pair) { return (bool)((held >> (pair / p.S)) & 1u); });
}

// fullband_stream_hop_wave_kernel (HELD: fbh_held_dispatch<true, false> and fbh_held_finish) with the two roles above; `held` is zero and
// unused without HELD
template <bool HELD, int RATIO, int FMT>
__global__ __launch_bounds__(HOP_THREADS) void fullband_stream_hop_wave_io_kernel(const FbhParams p, unsigned held, const HopWaveIo io) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int bi = (int)blockIdx.x - 1;
    const int li = bi - p.nwg_in;
    const int pi = li - p.nl * p.wpl;
    if (bi < 0) {
        fbh_stft_role_io<HELD, RATIO, FMT>(p, io, smem, held);
    } else if (bi < p.nwg_in) {
        fbh_input_role<true>(p, smem);
    } else if (li < p.nl * p.wpl) {
        const int l = li / p.wpl, part = li - l * p.wpl;
        if (l == 0)
            fbh_layer_role<true, false, HELD>(p, 0, part, smem, nullptr, held);
        else
            fbh_layer_role<false, false, HELD>(p, l, part, smem, nullptr, held);
    } else if (pi < p.nwg_proj) {
        fbh_proj_role<true, HELD>(p, pi, smem, held);
    } else {
        fbh_istft_role_io<HELD, RATIO, FMT>(p, io, pi - p.nwg_proj, smem, held);
    }
    if constexpr (HELD) fbh_held_finish(p, held, smem);
}

// the kernel of an io launch: one instantiation per (held, ratio, format)
template <int RATIO, int FMT>
static int fbh_launch_io_kernel(bool held_form, dim3 grid, dim3 block, size_t lds, hipStream_t st, const FbhParams& p, unsigned held,
                                const HopWaveIo& io) {
    if (held_form) return launch_lds<fullband_stream_hop_wave_io_kernel<true, RATIO, FMT>>(grid, block, lds, st, p, held, io);
    return launch_lds<fullband_stream_hop_wave_io_kernel<false, RATIO, FMT>>(grid, block, lds, st, p, 0u, io);
}

// fbh_launch's waveform branch, restated (w: the descriptor with io's sample buffers in place of its own; the plan dereferences neither)
static int fbh_launch_io(const sfsn_fullband_wave_desc* w, const sfsn_hop_io* io, void* stream, unsigned held) {
    const sfsn_fullband_hop_desc* d = &w->hop;
    FbhParams p;
    size_t lds;
    const int rc = fbh_plan(p, lds, d, true);
    if (rc != SFSN_OK) return rc;
    if (io->ratio == 3 && HOP_WAVE_LDS_STFT_IO > lds) lds = HOP_WAVE_LDS_STFT_IO;  // (40 KB: below the input role's 50 KB at F = 257)
    if (!d->w_ih0 || !d->w_p || !d->w_p_dq || !d->z0 || !d->scratch || d->scratch_bytes < 64) return SFSN_EINVAL;
    if (d->D > 0 && (!d->hist_ri[0] || !d->hist_ri[1])) return SFSN_EINVAL;
    bool al = aligned16(d->w_p) && aligned16(d->w_p_dq) && aligned16(d->b_p) && aligned8(d->enh_ri) && aligned8(d->z0) &&
              aligned8(d->hist_ri[0]) && aligned8(d->hist_ri[1]);
    if (!d->clip_start || !w->wave_in || !w->wave_state || !w->ola_state || !w->wave_out || !w->window || !w->spec_g || !w->enh_g)
        return SFSN_EINVAL;
    al = al && aligned8(w->wave_in) && aligned8(w->wave_state) && aligned8(w->ola_state) && aligned8(w->wave_out) && aligned8(w->window) &&
         aligned8(w->spec_g) && aligned8(w->enh_g) && (reinterpret_cast<uintptr_t>(w->done) & 3u) == 0;
    if (io->ratio == 3)
        al = al && (reinterpret_cast<uintptr_t>(io->dec_state) & 3u) == 0 && (reinterpret_cast<uintptr_t>(io->int_state) & 3u) == 0 &&
             (reinterpret_cast<uintptr_t>(io->taps) & 3u) == 0 && (reinterpret_cast<uintptr_t>(io->phase_taps) & 3u) == 0;
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
    p.inp = nullptr;
    p.hist[0] = d->hist_ri[0]; p.hist[1] = d->hist_ri[1]; p.enh = d->enh_ri; p.mag = d->enh_mag; p.z0 = d->z0;
    p.cnt = static_cast<unsigned*>(d->scratch);
    p.clip_start = d->clip_start;
    p.launch = d->launch_index;
    p.wave_in = w->wave_in; p.wave_state = w->wave_state; p.ola_state = w->ola_state; p.wave_out = w->wave_out;
    p.window = w->window; p.spec_g = w->spec_g; p.enh_g = w->enh_g; p.done = w->done;
    // every workgroup must be resident at once (consumers wait for producers): one per compute unit at most
    if (p.nblocks > cu_count()) return SFSN_EUNSUPPORTED;
    if (lds > 160 * 1024) return SFSN_EUNSUPPORTED;
    const dim3 grid(p.nblocks), block(HOP_THREADS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const HopWaveIo wio = {io->wave_in, io->wave_out, io->dec_state, io->int_state, io->taps, io->phase_taps};
    if (io->ratio == 3)
        return io->format == SFSN_SAMPLE_S16 ? fbh_launch_io_kernel<3, RS_S16>(held != 0, grid, block, lds, st, p, held, wio)
                                             : fbh_launch_io_kernel<3, RS_F32>(held != 0, grid, block, lds, st, p, held, wio);
    return fbh_launch_io_kernel<1, RS_S16>(held != 0, grid, block, lds, st, p, held, wio);
}

extern "C" int sfsn_fullband_stream_hop_wave_io(const sfsn_fullband_wave_desc* desc, const sfsn_hop_io* io, unsigned held_mask, void* stream) {
    if (!io) return sfsn_fullband_stream_hop_wave_held(desc, held_mask, stream);
    if (io->ratio != 1 && io->ratio != 3) return SFSN_EINVAL;
    if (io->format != SFSN_SAMPLE_F32 && io->format != SFSN_SAMPLE_S16) return SFSN_EINVAL;
    if (!desc || !desc->wave_state) return SFSN_EINVAL;  // not a waveform descriptor
    if (!io->wave_in || !io->wave_out) return SFSN_EINVAL;
    if (io->ratio == 3 && (!io->dec_state || !io->int_state || !io->taps || !io->phase_taps)) return SFSN_EINVAL;
    // the descriptor's own sample pointers are ignored: the launch sees the outer buffers in their place
    sfsn_fullband_wave_desc w = *desc;
    w.wave_in = static_cast<const float*>(io->wave_in);
    w.wave_out = static_cast<float*>(io->wave_out);
    if (io->ratio == 1 && io->format == SFSN_SAMPLE_F32) return sfsn_fullband_stream_hop_wave_held(&w, held_mask, stream);  // the plain samples: the plain kernels
    if (held_mask) {
        const int rc = fbh_held_mask(&w.hop, held_mask);
        if (rc != SFSN_OK) return rc;
    }
    return fbh_launch_io(&w, io, stream, held_mask);
}
