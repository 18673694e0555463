// sfsn_hop_io.hip -- the one-launch streaming hop of sfsn_hop.hip for waveform sessions whose OUTER samples differ from the model's:
// three times the model's rate and / or 16-bit PCM, converted inside the launch (sfsn_stream_hop_io; gfx950 only).
//
// The first and the last stage are sfsn_hop_wave_dev.h's roles with the conversion in them (hop_wave_stft_io / hop_wave_istft_io: the
// decimator in front of the frame, the interpolator and the quantiser behind the inverse STFT; filters and formats from
// sfsn_resample_dev.h, which the stand-alone kernels of sfsn_resample.hip call too -- same bits).  Every other stage IS the plain hop's:
// this unit includes sfsn_hop.hip for its roles, its plan and its checks.  That file's kernels are templates, none of which is
// instantiated here, and its exports are compiled out (SFSN_HOP_IO_UNIT), so the plain hop's unit -- and with it every kernel a plain
// session launches -- is what it was before this unit existed; a translation unit of their own also keeps the optimiser's
// module-wide decisions about the plain kernels away from these.  Dispatch and kernel are restated below for the same reason.
#define SFSN_HOP_IO_UNIT
#include "sfsn_hop.hip"

// RATIO / FMT: the outer samples' rate and format, `io` their buffers.
template <bool HELD, int RATIO, int FMT>
__device__ __forceinline__ void hop_stft_role_io(const HopParams& p, const HopStep& hs, const HopStageDev& sd, const HopHeld& hm, const HopWaveIo& io,
                                                 char* smem) {
    const int rt = (int)blockIdx.x - sd.wg0;
    const int nclip = (p.B - 16 * rt) < 16 ? (p.B - 16 * rt) : 16;
    hop_wave_stft_io<HELD, RATIO, FMT>(p.wave_in, p.wave_state, p.window, p.spec_g, p.F, 16 * rt, nclip, hop_tag(hs.launch) * 0x02020202u, smem, io,
                                       [&](int ln, int n) { return p.clip_start ? __ballot(ln < n && hop_clip_k(p, hs, 16 * rt + ln) == -1) : 0ull; },
                                       [&](int ci) { return hop_held<HELD>(hm, 16 * rt + ci); });
}
template <bool HELD, int RATIO, int FMT>
__device__ __forceinline__ void hop_istft_role_io(const HopParams& p, const HopStep& hs, const HopStageDev& sd, const HopHeld& hm, const HopWaveIo& io,
                                                  char* smem) {
    hop_wave_istft_io<HELD, RATIO, FMT>(
        p.ola_state, p.wave_out, p.window, p.enh_g, p.done, p.cnt, p.F, (int)blockIdx.x - sd.wg0, p.B * p.S, hop_tag(hs.launch) * 0x02020202u,
        hs.launch + 1u, smem, io,
        [&](int pair, int& fi, bool& fresh, bool& mute) {
            fi = p.clip_start ? hop_clip_k(p, hs, pair / p.S) : hs.frame_index;
            fresh = p.clip_start && fi == 0;
            mute = p.clip_start && fi < 2;
        },
        [&](bool&) {}, [&](int pair) { return hop_held<HELD>(hm, pair / p.S); });
}
template <int G, bool GIVEN, bool HELD, int RATIO, int FMT>
__device__ __forceinline__ void hop_dispatch_io(const HopParams& p, const HopStep& hs, const HopHeld& hm, const HopWaveIo& io, char* smem) {
    if ((int)blockIdx.x < p.st[0].nwg) {
        hop_layer_role<true, true, G, GIVEN, HELD>(p, hs, p.st[0], p.seq[0], hm, smem);
        return;
    }
    const int si = (int)((p.stage_of_block[blockIdx.x >> 2] >> (8 * (blockIdx.x & 3))) & 0xffu);
    const HopStageDev& sd = p.st[si];
    const HopSeqDev& sq = p.seq[sd.seq];
    if (sd.layer >= 0) {
        if (sd.layer == 0)
            hop_layer_role<true, true, G, GIVEN, HELD>(p, hs, sd, sq, hm, smem);
        else
            hop_layer_role<false, true, G, false, HELD>(p, hs, sd, sq, hm, smem);
    } else if (sd.layer == -1) {
        hop_proj_role<true, HELD>(p, hs, sd, sq, hm, smem);
    } else if (sd.layer == -2) {
        hop_stft_role_io<HELD, RATIO, FMT>(p, hs, sd, hm, io, smem);
    } else {
        hop_istft_role_io<HELD, RATIO, FMT>(p, hs, sd, hm, io, smem);
    }
}
template <int G, bool GIVEN, bool HELD, int RATIO, int FMT>
__global__ __launch_bounds__(HOP_THREADS) void stream_hop_io_kernel(const HopParams p, const HopHeld hm, const HopWaveIo io) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    HOP_STAMP(0);
    HopStep hs;
    hs.launch = p.launch; hs.frame_index = p.frame_index; hs.frames_before = p.frames_before;
    hs.wait_fin = 0;
    hop_dispatch_io<G, GIVEN, HELD, RATIO, FMT>(p, hs, hm, io, smem);
    HOP_STAMP(7);
    if constexpr (HELD) {
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        unsigned* fin = p.cnt + HOP_HELD_CNT;
        if (threadIdx.x == 0)
            *reinterpret_cast<unsigned*>(smem) = __hip_atomic_fetch_add(fin, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (*reinterpret_cast<const unsigned*>(smem) != gridDim.x - 1u) return;
        for (int b = threadIdx.x; b < p.B; b += HOP_THREADS)
            if (hop_held<true>(hm, b)) __hip_atomic_fetch_add(const_cast<unsigned*>(p.clip_start) + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (threadIdx.x == 0) st_agent(fin, 0u);
    }
}

// the kernel of an io launch: one instantiation per (gate weights, given statistics, held, ratio, format)
template <int RATIO, int FMT>
static int hop_launch_io_kernel(bool g2, bool given, bool held, dim3 grid, dim3 block, size_t lds, hipStream_t st, const HopParams& p,
                                const HopHeld& hm, const HopWaveIo& io) {
    if (held) {
        if (given) return g2 ? launch_lds<stream_hop_io_kernel<2, true, true, RATIO, FMT>>(grid, block, lds, st, p, hm, io) : launch_lds<stream_hop_io_kernel<1, true, true, RATIO, FMT>>(grid, block, lds, st, p, hm, io);
        return g2 ? launch_lds<stream_hop_io_kernel<2, false, true, RATIO, FMT>>(grid, block, lds, st, p, hm, io) : launch_lds<stream_hop_io_kernel<1, false, true, RATIO, FMT>>(grid, block, lds, st, p, hm, io);
    }
    if (given) return g2 ? launch_lds<stream_hop_io_kernel<2, true, false, RATIO, FMT>>(grid, block, lds, st, p, hm, io) : launch_lds<stream_hop_io_kernel<1, true, false, RATIO, FMT>>(grid, block, lds, st, p, hm, io);
    return g2 ? launch_lds<stream_hop_io_kernel<2, false, false, RATIO, FMT>>(grid, block, lds, st, p, hm, io) : launch_lds<stream_hop_io_kernel<1, false, false, RATIO, FMT>>(grid, block, lds, st, p, hm, io);
}

static int hop_launch_io(const sfsn_hop_desc* desc, const sfsn_hop_io* io, const uint64_t* held_bits, void* stream) {
    HopParams local;
    size_t lds;
    const int rc = hop_plan(local, lds, desc);
    if (rc != SFSN_OK) return rc;
    if (io->ratio == 3 && HOP_WAVE_LDS_STFT_IO > lds) lds = HOP_WAVE_LDS_STFT_IO;
    if (!desc->scratch || desc->scratch_bytes < hop_counter_bytes(local) + (size_t)local.nblocks * HOP_WAVES * 64) return SFSN_EINVAL;
    local.cnt = static_cast<unsigned*>(desc->scratch);
    local.launch = desc->launch_index;
    local.frames_before = desc->frames_before;
    local.dbg = reinterpret_cast<unsigned long long*>(static_cast<char*>(desc->scratch) + hop_counter_bytes(local));
    HopHeld hm;
    bool any_held = false;
    const int hrc = hop_held_mask(hm, any_held, desc, held_bits);
    if (hrc != SFSN_OK) return hrc;
    const int fit = hop_fits_device(local.nblocks);
    if (fit != SFSN_OK) return fit;
    if (lds > 160 * 1024) return SFSN_EUNSUPPORTED;
    const bool g2 = local.G == 2, given = local.given != 0;
    const dim3 grid(local.nblocks), block(HOP_THREADS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const HopWaveIo w = {io->wave_in, io->wave_out, io->dec_state, io->int_state, io->taps, io->phase_taps};
    if (io->ratio == 3)
        return io->format == SFSN_SAMPLE_S16 ? hop_launch_io_kernel<3, RS_S16>(g2, given, any_held, grid, block, lds, st, local, hm, w)
                                             : hop_launch_io_kernel<3, RS_F32>(g2, given, any_held, grid, block, lds, st, local, hm, w);
    return hop_launch_io_kernel<1, RS_S16>(g2, given, any_held, grid, block, lds, st, local, hm, w);
}

extern "C" int sfsn_stream_hop_io(const sfsn_hop_desc* desc, const sfsn_hop_io* io, const uint64_t* held_bits, void* stream) {
    if (!io) return sfsn_stream_hop_held(desc, held_bits, stream);
    if (io->ratio != 1 && io->ratio != 3) return SFSN_EINVAL;
    if (io->format != SFSN_SAMPLE_F32 && io->format != SFSN_SAMPLE_S16) return SFSN_EINVAL;
    if (!desc || !desc->wave_state) return SFSN_EINVAL;  // not a waveform descriptor
    if (desc->hop != 1) return SFSN_EUNSUPPORTED;
    if (!io->wave_in || !io->wave_out) return SFSN_EINVAL;
    if (io->ratio == 3 && (!io->dec_state || !io->int_state || !io->taps || !io->phase_taps)) return SFSN_EINVAL;
    // the descriptor's own sample pointers are ignored: the plan sees the outer buffers in their place (it dereferences neither)
    sfsn_hop_desc d = *desc;
    d.wave_in = static_cast<const float*>(io->wave_in);
    d.wave_out = static_cast<float*>(io->wave_out);
    if (io->ratio == 1 && io->format == SFSN_SAMPLE_F32) return sfsn_stream_hop_held(&d, held_bits, stream);  // the plain samples: the plain kernels
    return hop_launch_io(&d, io, held_bits, stream);
}
