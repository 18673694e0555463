// sfsn_projdf.hip -- the sub-band epilogue in ONE launch (round 6): projection S2 . W_p^T + b (MODEL:118 / FROZEN:125), output
// re-index + deep filter + Nyquist pass-through + |.| (MODEL:160-167,315-346,450-474; FROZEN:15-39,259-265,588-607).  gfx950 only.
//
// Why: sfsn_spike_proj_multi wrote the coefficient rows (295 MB per forward at B = 64, T = 1000, baseline_m) and sfsn_deepfilter read
// them straight back (674 MB per dispatch, the fattest time-parallel kernel); inside bench.py's timed region the time-parallel half of
// a forward is HBM-bound (profiles/r05_region_marginal_ledger.json), so bytes are time there.  Here the coefficient tile of a
// (clip, frame block, unit range) is formed on the int8 matrix cores, stays in LDS, is written out ONCE (it is `all_layer_outputs[-1]`
// of the module API; skipped when nobody reads it) and is applied to the noisy spectrum from LDS.
//
// Round 3 built this fusion with serial phases behind __syncthreads() in small non-persistent workgroups and measured it slower than the
// two launches (profiles/EXPERIMENTS.md).  What is different: persistent workgroups (the W_p tiles of a job stay in registers for the
// launch, as in spike_proj_fast_body), two LOADER waves per workgroup that keep the tile after next in flight for a whole tile's time
// (see projdf_body), raw barriers that do not drain stores, and a tile order that puts the two 16-frame halves of a 256-byte output
// run back to back in the same workgroup (the L2 merges them).
//
// Arithmetic: the projection is spike_proj_fast_body's instruction for instruction (three exact int8 digit products, recombine3,
// `* dq + bias`), the filter deepfilter_pass_kernel's expression for expression on the same fp32 coefficients: bit-identical to the
// two launches (tests/test_hip_parity.py::test_projection_and_deep_filter_in_one_launch_*).
//
// The tile itself (LDS layout, ring schedule, compute waves, pass-through, the host's split into jobs) is sfsn_projdf_dev.h's, shared
// with the epilogue role of sfsn_pair16e.hip; this unit states the launch of its own: 512 threads, a contiguous range of tiles per
// workgroup, two loader waves with plain loads, pass-through bins as a job of their own.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "sfsn_feat_dev.h"
#include "sfsn_scan_dev.h"
#include "sfsn_host.h"
#include "sfsn_projdf_dev.h"

#define PDF_MAX_JOBS 16
#define PDF_THREADS 512
#define PDF_CW 6     // compute waves (matrix phase, coefficient write-out, filter); waves 6 and 7 are the two loader waves
#define PDF_LW 2
#define PDF_NV 16    // 16-byte spike vectors per LOADER lane and tile (two loaders: <= 2048 per tile)
#define PDF_NX 16    // spectrum elements per loader lane and tile (<= 2048 per tile)

struct PdfJobDev : PdfJob {
    int NWN, tpw;      // compute waves side by side over the column tiles, column tiles per wave
    int FT;            // frames per tile (16)
    int kind;          // 0: projection + filter, 1: pass-through bins [fcov, F)
};
struct PdfParams {
    PdfJobDev job[PDF_MAX_JOBS];
    int n, B, F, T, S, t0, t1, fcov;
    const float* stft;
    float* enh;
    float* mag;
};

// Workgroup = six compute waves + two LOADER waves.  What the first form of this kernel measured (round 6, B = 64, T = 1000: 324 us per
// forward, the same as the two launches it replaces although it moves 0.3 GB less): every wave requested the next tile's operands at
// the top of a tile and parked them behind its matrix phase -- ~1 us later, against 2-3 us of HBM latency under load: 15 k clk per tile
// for ~5 k clk of work.  A wave that does nothing but load has a vmcnt queue of loads only (whatever the compiler's waits look like,
// they never wait for a store) and 200 registers to hold half a tile in flight for a whole tile's time: loader k requests its half of
// tile j + 2 at the top of tile j, crosses the tile's first barrier with the loads in flight, and writes them into ring slot (j + 2) % 3
// (free since tile j - 1's last barrier) before the tile's second barrier (pdf_loader_ring).
template <int TPW, int KS>
__device__ __forceinline__ void projdf_body(const PdfParams& p, const PdfJobDev& jb, int blk, char* smem) {
    constexpr int KP = KS * 64;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int FT = jb.FT, U = jb.U, t1 = p.t1;
    const PdfTile L(KS, FT, U, jb.P, jb.fc, jb.df);
    const int ntile = (t1 - p.t0 + FT - 1) / FT;     // frame tiles per clip
    const int tiles = p.B * ntile;
    // a contiguous range of tiles per workgroup: consecutive frame tiles of one clip follow each other in the same workgroup (the two
    // 16-frame halves of a 256-byte run of the enhanced spectrum are written within microseconds of each other: the L2 merges them)
    const int tl0 = (int)((long long)tiles * blk / jb.nblocks), tl1 = (int)((long long)tiles * (blk + 1) / jb.nblocks);
    auto tile_of = [&](int tl, int& b, int& tb) __attribute__((always_inline)) {
        b = tl / ntile;
        tb = p.t0 + (tl - b * ntile) * FT;
    };
    pdf_fill_rowoff(reinterpret_cast<int*>(smem + L.rowoff_off), L, U, jb.P, tid, PDF_THREADS);

    if (wave >= PDF_CW) {
        // ================================================= loader wave k =================================================
        const int k = wave - PDF_CW;
        constexpr int SROW = KP + 16, C16 = KP / 16;
        // my vectors of a tile: piece index 2 i + k (a piece = 64 consecutive 16-byte vectors / spectrum elements)
        int s_fl[PDF_NV], s_in[PDF_NV], s_lds[PDF_NV];
#pragma unroll
        for (int i = 0; i < PDF_NV; ++i) {
            int v = (PDF_LW * i + k) * 64 + lane;
            const bool have = v < L.NVT;
            if (v > L.NVT - 1) v = L.NVT - 1;
            const int r = v / C16, c16 = v - r * C16;
            const int fl = r / U, u = r - fl * U;
            s_fl[i] = fl;
            s_in[i] = u * KP + c16 * 16;
            s_lds[i] = have ? r * SROW + c16 * 16 : -1;
        }
        int x_jc[PDF_NX];                            // (bin row << 8) | column, or -1: no element
#pragma unroll
        for (int i = 0; i < PDF_NX; ++i) {
            const int e = (PDF_LW * i + k) * 64 + lane;
            const int ec = e < L.NXT ? e : L.NXT - 1;
            const int j = ec / L.XW, c = ec - j * L.XW;
            x_jc[i] = e < L.NXT ? (j << 8) | c : -1;
        }
        const size_t frame_s = (size_t)jb.R * KP;
        const int fbin0 = jb.lo + jb.k0 * jb.fc;
        const int F = p.F, T = p.T;
        v4i pre[PDF_NV];
        float2 xpre[PDF_NX];
        bool x_ok[PDF_NX];
        auto fetch = [&](int tl) __attribute__((always_inline)) {
            int b, tb;
            tile_of(tl, b, tb);
            const int flmax = t1 - 1 - tb;           // frames past the chunk re-read its last frame (their rows are never stored)
            const int8_t* sb = jb.s + (size_t)tb * frame_s + ((size_t)b * jb.N + jb.k0) * KP;
#pragma unroll
            for (int i = 0; i < PDF_NV; ++i) {
                // (no branch around a load: hipcc drains vmcnt(0) at every control-flow merge, which would leave ONE load in flight at a
                //  time -- slots beyond the tile re-read its last vector: same line for all 64 lanes, an issue slot and nothing else)
                const int fl = s_fl[i] < flmax ? s_fl[i] : flmax;
                pre[i] = *reinterpret_cast<const v4i*>(sb + (size_t)fl * frame_s + s_in[i]);
            }
            const float* xb = p.stft + ((size_t)b * F + fbin0) * T * 2;
            const int ts0 = tb - (jb.df - 1);
#pragma unroll
            for (int i = 0; i < PDF_NX; ++i) {
                const int jc = x_jc[i] < 0 ? 0 : x_jc[i];
                const int ts = ts0 + (jc & 255);
                const int tsc = ts < 0 ? 0 : (ts > T - 1 ? T - 1 : ts);
                xpre[i] = *reinterpret_cast<const float2*>(xb + ((size_t)(jc >> 8) * T + tsc) * 2);
                x_ok[i] = ts >= 0 && ts < T;
            }
        };
        auto park = [&](int slot) __attribute__((always_inline)) {
            char* sl = smem + slot * L.SLOTB;
#pragma unroll
            for (int i = 0; i < PDF_NV; ++i)
                if (s_lds[i] >= 0) *reinterpret_cast<v4i*>(sl + s_lds[i]) = pre[i];
            float2* xt = reinterpret_cast<float2*>(sl + L.SBUF);
#pragma unroll
            for (int i = 0; i < PDF_NX; ++i)
                if (x_jc[i] >= 0) xt[(PDF_LW * i + k) * 64 + lane] = x_ok[i] ? xpre[i] : make_float2(0.0f, 0.0f);
        };
        pdf_loader_ring(tl0, tl1, fetch, park);
        return;
    }
    pdf_compute_waves<TPW, KS, PDF_CW>(p, jb, L, FT, jb.NWN, smem, tl0, tl1, tile_of);
}

template <int KS>
__global__ __launch_bounds__(PDF_THREADS) void projdf_kernel(const PdfParams p) {
    extern __shared__ __attribute__((aligned(16))) char pdf_smem[];
    int j = 0;
    for (int i = 1; i < p.n; ++i)
        if ((int)blockIdx.x >= p.job[i].block0) j = i;
    const PdfJobDev& jb = p.job[j];
    const int blk = (int)blockIdx.x - jb.block0;
    if (jb.kind == 1) pdf_passthrough(p, blk, jb.nblocks, PDF_THREADS / 64);
    else if (jb.tpw == 1) projdf_body<1, KS>(p, jb, blk, pdf_smem);
    else if (jb.tpw == 2) projdf_body<2, KS>(p, jb, blk, pdf_smem);
    else projdf_body<3, KS>(p, jb, blk, pdf_smem);
}

extern "C" int sfsn_proj_deepfilter(const float* stft_ri, int B, int F, int T, int S, int H, const sfsn_projdf_group* groups, int n_groups,
                                    float* enh_ri, float* enh_mag, int t0, int nt, void* stream) {
    if (!stft_ri || !enh_ri || !groups || n_groups <= 0 || n_groups > SFSN_MAX_GROUPS || B <= 0 || F < 2 || T <= 0 || S <= 0 || H <= 0)
        return SFSN_EINVAL;
    if (t0 < 0 || nt <= 0 || t0 + nt > T) return SFSN_EINVAL;
    const int KS = (H + 63) / 64;
    if (KS > 4) return SFSN_EUNSUPPORTED;
    const int wgs_env = sfsn_knob("SFSN_PDF_WGS", 0);  // A/B runs: workgroups of the launch
    const size_t lds_cap_env = (size_t)sfsn_knob("SFSN_PDF_LDS_KB", 150) * 1024;
    PdfParams p;
    p.B = B; p.F = F; p.T = T; p.S = S; p.t0 = t0; p.t1 = t0 + nt; p.stft = stft_ri; p.enh = enh_ri; p.mag = enh_mag;
    double wt[PDF_MAX_JOBS];
    int tiles_of[PDF_MAX_JOBS], grp[PDF_MAX_JOBS];
    size_t lds = 0;
    int lo = 0;
    const PdfCaps caps = {PDF_LW * PDF_NV * 64, PDF_LW * PDF_NX * 64, PDF_CW, 3 /* P <= 288 */, PDF_MAX_JOBS - 1};
    const int rc = pdf_split_groups(groups, n_groups, B, S, KS, caps, lds_cap_env, p.job, p.n, grp, wt, lds, lo);
    if (rc != SFSN_OK) return rc;
    if (lo > F) return SFSN_EINVAL;
    p.fcov = lo;
    for (int i = 0; i < p.n; ++i) {
        PdfJobDev& d = p.job[i];
        d.tpw = (d.NT + PDF_CW - 1) / PDF_CW; d.NWN = (d.NT + d.tpw - 1) / d.tpw; d.FT = PDF_FT; d.kind = 0;
        tiles_of[i] = B * ((nt + PDF_FT - 1) / PDF_FT);
        wt[i] = (double)tiles_of[i] * wt[i];
    }
    const int n_cu = cu_count();
    // one persistent workgroup per compute unit (the ring and the coefficient tile take most of a unit's LDS).  Measured with the loader
    // waves, B = 64, T = 1000: 256 / 512 / 1024 workgroups 238 / 246 / 296 us per forward (every workgroup reloads its W_p tiles)
    int total = wgs_env > 0 ? wgs_env : n_cu;
    int n_pass = 0;
    if (lo < F) {  // the pass-through bins: a few workgroups of their own
        PdfJobDev& d = p.job[p.n];
        d = PdfJobDev{};
        d.kind = 1;
        const int tiles = B * ((nt + 63) / 64);
        n_pass = tiles < 8 ? tiles : 8;
        tiles_of[p.n] = tiles;
        wt[p.n] = 0;
        ++p.n;
    }
    // block ranges in proportion to the jobs' bytes, at least one and at most `tiles` each
    {
        double sum = 0;
        for (int i = 0; i < p.n; ++i) sum += wt[i];
        int blocks = 0;
        for (int i = 0; i < p.n; ++i) {
            int nbk = p.job[i].kind == 1 ? n_pass : (int)((total - n_pass) * wt[i] / sum + 0.5);
            if (nbk < 1) nbk = 1;
            if (nbk > tiles_of[i]) nbk = tiles_of[i];
            p.job[i].block0 = blocks; p.job[i].nblocks = nbk;
            blocks += nbk;
        }
        total = blocks;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
#define PDF_CASE(KS_) \
    if (KS == KS_) return launch_lds<projdf_kernel<KS_>>(dim3(total), dim3(PDF_THREADS), lds, st, p);
    PDF_CASE(1) PDF_CASE(2) PDF_CASE(3) PDF_CASE(4)
#undef PDF_CASE
    return SFSN_EUNSUPPORTED;
}
