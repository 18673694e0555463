// sfsn_pair16e.hip -- layers 0 and 1 of a two-layer sub-band stack at 16 rows per workgroup AND the sub-band epilogue (projection + deep
// filter + pass-through + |.|) in ONE launch (gfx950 only): sfsn_gsn_layer_scan_l01_projdf.
//
// sfsn_pair16.hip took layer 1 off the forward's chain of launches; the longest link left that is no recurrence is projdf_kernel
// (sfsn_projdf.hip), which needs layer 1 to have FINISHED only because it is a launch of its own: a tile of it (one clip, 16 frames, the
// clip's units of one group) reads the last layer's int8 spikes of those 16 frames and nothing else the forward computes.  This kernel
// carries three tiers of workgroups:
//   1. layer 0      blocks [0, n0): layer0_role16<.., PUB> (sfsn_pair_dev.h), as in gsn_scan_l01_kernel;
//      padding      blocks [n0, n0pad), n0pad a multiple of eight: they only count themselves out;
//   2. layer 1      blocks [n0pad, n1end): layer1_role16<.., GATED, PUB>: gated on layer-0 block i (n_in = 1) AND publishing;
//   3. the epilogue blocks [n1end, nblocks): projdf16_role below -- projdf_body's work dealt over the 16 waves of a scan workgroup, its
//      loader waves gated on the layer-1 blocks that hold its clips' rows (a contiguous range of counters).
// Same instructions on the same operands: bit-identical to sfsn_gsn_layer_scan_l01 followed by sfsn_proj_deepfilter.
// This unit states what the third tier adds to sfsn_pair16.hip: layer 1's publishing link, the epilogue role's tile order, gate and
// loads, and the deal of epilogue workgroups over the jobs.  The scan roles are sfsn_pair_dev.h's, the checks of the lists and the
// launch sfsn_scan_host.h's, the tile of projection + deep filter and the split of the groups into jobs sfsn_projdf_dev.h's.
//
// Deadlock freedom, for three tiers (the argument of sfsn_pair16.hip / StackLink, sfsn_scan_dev.h): workgroups are dispatched in index
// order and EVERY consumer has a higher block index than each of its producers (layer 1 above layer 0, the epilogue above all of layer 1).
// So when a consumer is resident, each of its producers is resident or has finished; tier 1 never waits for anybody, so it always
// advances; tier 2 waits only for tier 1, so it advances; tier 3 waits only for tier 2.  No case arises in which a resident workgroup
// waits for one that has not been dispatched; where more forwards are in flight than the chip holds workgroups, the consumers start late
// and find everything published.  Every spin is bounded all the same (error word, garbage output, reported by the host).
// Every workgroup (padding blocks too) ends in stack_exit_counters: the last one zeroes all 2 + nblocks words but the error word.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "sfsn.h"

#include "sfsn_feat_dev.h"
#include "sfsn_scan_dev.h"
#include "sfsn_scan3_dev.h"
#include "sfsn_scan3j_dev.h"
#include "sfsn_pair_dev.h"
#include "sfsn_projdf_dev.h"
#include "sfsn_host.h"
#include "sfsn_scan_host.h"

#define EPI_MAX_JOBS 12
#define EPI_CW 12    // compute waves (matrix phase, coefficient write-out, filter); waves 12 .. 15 are the four loader waves
#define EPI_LW 4
#define EPI_NV 8     // 16-byte spike vectors per LOADER lane and tile (four loaders: <= 2048 per tile, as projdf_body's 2 x 16)
#define EPI_NX 8     // spectrum elements per loader lane and tile (<= 2048 per tile)
#ifndef SFSN_L01E_WGS_DEFAULT
#define SFSN_L01E_WGS_DEFAULT 32  // epilogue workgroups of a launch (profiles/l01_epilogue_one_launch.md)
#endif

struct PairEParams {
    unsigned* prog;  // [0] error word, [1] workgroups that have exited, [2 + block] frames published by that workgroup
    int nblocks;     // grid size (padding blocks included)
    int n0;          // layer-0 workgroups: blocks [0, n0)
    int n0pad;       // first layer-1 block (n0 rounded up to a multiple of eight)
    int n1end;       // first epilogue block
    int lag;         // frames a consumer lets its producer run ahead between polls
    int exit_off;    // byte offset of the exit word in the dynamic LDS allocation (behind every role's layout)
};

// (s: frame 0 of the SEQUENCE, the chunk starts at frame t0; block0: counted from the first epilogue block; cnt0 is this launch's)
using EpiJobDev = PdfJob;
struct EpiParams {
    EpiJobDev job[EPI_MAX_JOBS];
    int n, B, F, T, S, t0, t1, fcov, E;
    const float* stft;
    float* enh;
    float* mag;
};
static_assert(2 * sizeof(ScanParams) + sizeof(PairEParams) + sizeof(EpiParams) <= 4096, "kernel arguments");

// Eight agent-scope (sc1) 16-byte loads to registers in one statement the compiler cannot look into (it would otherwise wait for each
// behind the next control-flow merge): spike rows another workgroup of THIS launch has published with write-through stores.  The values
// arrive asynchronously; epi_landed() is the only thing that may follow before they are used.
__device__ __forceinline__ void epi_load8_sc1(v4i (&d)[EPI_NV], unsigned long long base_uniform, const unsigned (&off)[EPI_NV]) {
    asm volatile(
        "global_load_dwordx4 %0, %8, %16 sc1\n\t"
        "global_load_dwordx4 %1, %9, %16 sc1\n\t"
        "global_load_dwordx4 %2, %10, %16 sc1\n\t"
        "global_load_dwordx4 %3, %11, %16 sc1\n\t"
        "global_load_dwordx4 %4, %12, %16 sc1\n\t"
        "global_load_dwordx4 %5, %13, %16 sc1\n\t"
        "global_load_dwordx4 %6, %14, %16 sc1\n\t"
        "global_load_dwordx4 %7, %15, %16 sc1"
        : "=&v"(d[0]), "=&v"(d[1]), "=&v"(d[2]), "=&v"(d[3]), "=&v"(d[4]), "=&v"(d[5]), "=&v"(d[6]), "=&v"(d[7])
        : "v"(off[0]), "v"(off[1]), "v"(off[2]), "v"(off[3]), "v"(off[4]), "v"(off[5]), "v"(off[6]), "v"(off[7]), "s"(base_uniform)
        : "memory");
}
// (the registers pass THROUGH the wait: whatever reads them depends on it)
__device__ __forceinline__ void epi_landed(v4i (&d)[EPI_NV]) {
    asm volatile("s_waitcnt vmcnt(0)"
                 : "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3]), "+v"(d[4]), "+v"(d[5]), "+v"(d[6]), "+v"(d[7])
                 :
                 : "memory");
}

// projdf_body (sfsn_projdf.hip) as a role of a 1,024-thread scan workgroup: twelve compute waves (one column tile each: NT <= 12; NWN = NT
// of them work in the matrix phase when NT does not divide 12) and FOUR loader waves with 8 + 8 prefetch slots per lane (two loaders with
// 16 + 16 do not fit the 128 registers of a 16-wave workgroup).  Arithmetic, LDS layout, ring and barrier scheme are projdf_body's: the
// same functions of sfsn_projdf_dev.h (PdfTile, pdf_loader_ring, pdf_compute_waves<1, KS, 12>).
//
// Ownership and order: workgroup `blk` of the job's `nblocks` owns the clips [c0, c1) and walks their tiles frames outer, clips inner --
// its producers (the layer-1 blocks with rows [c0 N + k0, (c1 - 1) N + k0 + U), counters lk_in[0 .. n_in)) advance together and it follows
// the scan a tile or two behind.  Gating: before a loader wave requests tile j + 2 it makes sure that every producer has published
// min(tb + FT, t1) - t0 frames (lanes poll the counters side by side, bounded; expiry sets the error word and ends the gating).  The
// slots past a tile re-read its last vector / the chunk's last frame, never a frame beyond the tile.  The spectrum is an input of the
// launch (its taps reach back before tb and before t0): plain loads, no gate.  The pass-through bins depend on nothing: every epilogue
// workgroup copies its share of them first, while its producers run up their first frames.
//
// Barriers: all sixteen waves take part (the prologue's __syncthreads and two raw barriers per tile, loaders and compute waves alike),
// and all sixteen return to the kernel's stack_exit_counters: no wave leaves early, so the counts match by construction.
template <int KS>
__device__ __forceinline__ void projdf16_role(const EpiParams& p, const EpiJobDev& jb, int blk, int eblk, char* smem, unsigned* prog, int lag) {
    constexpr int KP = KS * 64, SROW = KP + 16, C16 = KP / 16, FT = PDF_FT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int U = jb.U, B = p.B, F = p.F, T = p.T, t1 = p.t1;
    const PdfTile L(KS, FT, U, jb.P, jb.fc, jb.df);

    // ---- pass-through bins: (clip, 64-frame tile) units over ALL epilogue workgroups
    if (p.fcov < F) pdf_passthrough(p, eblk, p.E, 16);

    const int ntile = (t1 - p.t0 + FT - 1) / FT;     // frame tiles per clip
    const int c0 = (int)((long long)B * blk / jb.nblocks), c1 = (int)((long long)B * (blk + 1) / jb.nblocks);
    const int nc = c1 - c0, ntl = nc * ntile;        // my tiles: j -> (frame tile j / nc, clip c0 + j % nc)
    auto tile_of = [&](int j, int& b, int& tb) __attribute__((always_inline)) {
        const int fi = j / nc;
        b = c0 + (j - fi * nc);
        tb = p.t0 + fi * FT;
    };
    pdf_fill_rowoff(reinterpret_cast<int*>(smem + L.rowoff_off), L, U, jb.P, tid, 1024);

    if (wave >= EPI_CW) {
        // ================================================= loader wave k =================================================
        const int k = wave - EPI_CW;
        const size_t frame_s = (size_t)jb.R * KP;
        const int fbin0 = jb.lo + jb.k0 * jb.fc;
        // my vectors of a tile: piece index 4 i + k (a piece = 64 consecutive 16-byte vectors / spectrum elements)
        int s_fl[EPI_NV], s_in[EPI_NV], s_lds[EPI_NV];
#pragma unroll
        for (int i = 0; i < EPI_NV; ++i) {
            int v = (EPI_LW * i + k) * 64 + lane;
            const bool have = v < L.NVT;
            if (v > L.NVT - 1) v = L.NVT - 1;
            const int r = v / C16, c16 = v - r * C16;
            const int fl = r / U, u = r - fl * U;
            s_fl[i] = fl;
            s_in[i] = u * KP + c16 * 16;
            s_lds[i] = have ? r * SROW + c16 * 16 : -1;
        }
        int x_jc[EPI_NX];                            // (bin row << 8) | column, or -1: no element
#pragma unroll
        for (int i = 0; i < EPI_NX; ++i) {
            const int e = (EPI_LW * i + k) * 64 + lane;
            const int ec = e < L.NXT ? e : L.NXT - 1;
            const int j = ec / L.XW, c = ec - j * L.XW;
            x_jc[i] = e < L.NXT ? (j << 8) | c : -1;
        }
        // my producers: the layer-1 blocks that hold the rows of my clips
        const unsigned* lk_in = prog;
        int n_in = 0;
        if (nc > 0) {
            const int r_lo = c0 * jb.N + jb.k0, r_hi = (c1 - 1) * jb.N + jb.k0 + U - 1;
            lk_in = prog + jb.cnt0 + (r_lo >> 4);
            n_in = (r_hi >> 4) - (r_lo >> 4) + 1;
        }
        const int nt = t1 - p.t0;
        int avail = 0, failed = 0;                   // frames of the chunk known to be published by ALL my producers
        auto ensure = [&](int need) __attribute__((always_inline)) {
            if (need > avail && !failed) {
                const int want = (need + lag < nt) ? need + lag : nt;
                int vv = 0;
                for (unsigned spins = 0;; ++spins) {
                    vv = 0x7fffffff;
                    for (int i = lane; i < n_in; i += 64) {
                        const int pi = (int)__hip_atomic_load(lk_in + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        vv = pi < vv ? pi : vv;
                    }
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        const int ov = __shfl_xor(vv, o, 64);
                        vv = ov < vv ? ov : vv;
                    }
                    vv = __builtin_amdgcn_readfirstlane(vv);
                    if (vv >= want) break;
                    if (spins > SFSN_STACK_SPIN_LIMIT) {
                        if (lane == 0) __hip_atomic_store(prog, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        vv = -1;
                        break;
                    }
                    // (~1.7 us between polls against 27 us per row of tiles.  With s_sleep 8, as in s3_ensure, the workgroups that are
                    //  ahead of the scan polled so densely that the launch got LONGER with more of them: 32 / 48 / 64 workgroups
                    //  1.57 / 1.86 / 2.36 ms alone on the chip against 1.56 / 1.56 / 1.77 with this value)
                    __builtin_amdgcn_s_sleep(64);
                }
                if (vv < 0) failed = 1;
                else avail = vv;
            }
        };
        v4i pre[EPI_NV];
        float2 xpre[EPI_NX];
        unsigned x_ok = 0;
        auto fetch = [&](int j) __attribute__((always_inline)) {
            int b, tb;
            tile_of(j, b, tb);
            ensure((tb + FT < t1 ? tb + FT : t1) - p.t0);
            const int flmax = t1 - 1 - tb;           // frames past the chunk re-read its last frame (their rows are never stored)
            const int8_t* sb = jb.s + (size_t)tb * frame_s + ((size_t)b * jb.N + jb.k0) * KP;
            const unsigned long long a = reinterpret_cast<unsigned long long>(sb);
            // (readfirstlane returns a SIGNED int: through unsigned halves, or bit 31 of the low word spills over the high one)
            const unsigned a_lo = __builtin_amdgcn_readfirstlane((unsigned)a), a_hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
            const unsigned long long sbu = ((unsigned long long)a_hi << 32) | a_lo;
            unsigned off[EPI_NV];
#pragma unroll
            for (int i = 0; i < EPI_NV; ++i) {
                // (no branch around a load; slots beyond the tile re-read its last vector: projdf_body)
                const int fl = s_fl[i] < flmax ? s_fl[i] : flmax;
                off[i] = (unsigned)((size_t)fl * frame_s + s_in[i]);
            }
            epi_load8_sc1(pre, sbu, off);
            const float* xb = p.stft + ((size_t)b * F + fbin0) * T * 2;
            const int ts0 = tb - (jb.df - 1);
            x_ok = 0;
#pragma unroll
            for (int i = 0; i < EPI_NX; ++i) {
                const int jc = x_jc[i] < 0 ? 0 : x_jc[i];
                const int ts = ts0 + (jc & 255);
                const int tsc = ts < 0 ? 0 : (ts > T - 1 ? T - 1 : ts);
                xpre[i] = *reinterpret_cast<const float2*>(xb + ((size_t)(jc >> 8) * T + tsc) * 2);
                x_ok |= (ts >= 0 && ts < T) ? 1u << i : 0u;
            }
        };
        auto park = [&](int slot) __attribute__((always_inline)) {
            epi_landed(pre);
            char* sl = smem + slot * L.SLOTB;
#pragma unroll
            for (int i = 0; i < EPI_NV; ++i)
                if (s_lds[i] >= 0) *reinterpret_cast<v4i*>(sl + s_lds[i]) = pre[i];
            float2* xt = reinterpret_cast<float2*>(sl + L.SBUF);
#pragma unroll
            for (int i = 0; i < EPI_NX; ++i)
                if (x_jc[i] >= 0) xt[(EPI_LW * i + k) * 64 + lane] = ((x_ok >> i) & 1u) ? xpre[i] : make_float2(0.0f, 0.0f);
        };
        pdf_loader_ring(0, ntl, fetch, park);
        return;
    }
    // twelve compute waves, one column tile each (NWN = NT: the host refuses NT > 12)
    pdf_compute_waves<1, KS, EPI_CW>(p, jb, L, FT, jb.NT, smem, 0, ntl, tile_of);
}

// p0 / p1: as gsn_scan_l01_kernel; pe: the epilogue's jobs (block ranges counted from pp.n1end).
template <int KS, int TL, int OUT, int OFF = 0>
__global__ __launch_bounds__(1024) void gsn_scan_l01e_kernel(const ScanParams p0, const ScanParams p1, const PairEParams pp, const EpiParams pe) {
    extern __shared__ __attribute__((aligned(16))) char scan_smem[];
    int* exit_word = reinterpret_cast<int*>(scan_smem + pp.exit_off);
    const int b = (int)blockIdx.x;
    StackLink lk;
    lk.in = nullptr; lk.n_in = 0; lk.out = nullptr; lk.err = pp.prog; lk.lag = pp.lag; lk.dbg = nullptr;
    if (b < pp.n0) {
        // ---- layer 0: publishes the frames whose int8 rows are complete in its own counter
        lk.out = pp.prog + 2 + b;
        layer0_role16<KS, TL, OUT, true>(p0, b, scan_smem, &lk);
    } else if (b >= pp.n0pad && b < pp.n1end) {
        // ---- layer 1: gated on the layer-0 workgroup of the same 16 rows, publishing for the epilogue workgroups
        const int b1 = b - pp.n0pad;
        lk.in = pp.prog + 2 + b1; lk.n_in = 1;
        lk.out = pp.prog + 2 + b;
        layer1_role16<KS, TL, OUT, OFF, true, true>(p1, b1, scan_smem, &lk);
    } else if (b >= pp.n1end) {
        // ---- the epilogue: above every block it waits for
        const int eb = b - pp.n1end;
        int j = 0;
        for (int i = 1; i < pe.n; ++i)
            if (eb >= pe.job[i].block0) j = i;
        projdf16_role<KS>(pe, pe.job[j], eb - pe.job[j].block0, eb, scan_smem, pp.prog, pp.lag);
    }
    stack_exit_counters(pp, exit_word);
}

// The answers and their order: the lists each alone (pair_lists_each: sfsn_gsn_layer_scan_l01's, its T this chunk's nt), the groups
// (pdf_split_groups: sfsn_proj_deepfilter's, with this role's capacities), then what ties them together.  See include/sfsn.h.
extern "C" int sfsn_gsn_layer_scan_l01_projdf(const sfsn_scan_segment* segs_x, const sfsn_fused_x* fin_x, int n_x, const sfsn_scan_segment* segs_z,
                                              int n_z, const sfsn_scan_segment* segs1, const sfsn_fused_input* fin1, int H, int shared, int lag,
                                              void* scratch, size_t scratch_bytes, const float* stft_ri, int B, int F, int T, int S,
                                              const sfsn_projdf_group* groups, int n_groups, float* enh_ri, float* enh_mag, int t0, int nt,
                                              void* stream) {
    // ---- sfsn_proj_deepfilter's scalar arguments (SFSN_EINVAL, as those of the lists: no other answer comes between them)
    if (!stft_ri || !enh_ri || !groups || n_groups <= 0 || n_groups > SFSN_MAX_GROUPS || B <= 0 || F < 2 || T <= 0 || S <= 0) return SFSN_EINVAL;
    if (t0 < 0 || (nt >= 0 && t0 + nt > T)) return SFSN_EINVAL;
    PairLists pl;
    int rc = pair_lists_each(segs_x, fin_x, n_x, segs_z, n_z, segs1, fin1, nt, H, shared, lag, scratch, pl);
    if (rc != SFSN_OK) return rc;
    // ---- the groups
    const int KS = (H + 63) / 64, KP = KS * 64;
    EpiParams pe;
    pe.B = B; pe.F = F; pe.T = T; pe.S = S; pe.t0 = t0; pe.t1 = t0 + nt; pe.stft = stft_ri; pe.enh = enh_ri; pe.mag = enh_mag;
    double wt[EPI_MAX_JOBS];
    int grp[EPI_MAX_JOBS];
    size_t lds_e = 0;
    const PdfCaps caps = {EPI_LW * EPI_NV * 64, EPI_LW * EPI_NX * 64, EPI_CW, 1 /* P <= 192 */, EPI_MAX_JOBS};
    rc = pdf_split_groups(groups, n_groups, B, S, KS, caps, (size_t)sfsn_knob("SFSN_PDF_LDS_KB", 150) * 1024, pe.job, pe.n, grp, wt, lds_e,
                          pe.fcov);
    if (rc != SFSN_OK) return rc;
    if (pe.fcov > F) return SFSN_EINVAL;
    // ---- together: the lists; every group reads one layer-1 segment's rows
    rc = pair_lists_together(pl, nt, H, scratch, scratch_bytes);
    if (rc != SFSN_OK) return rc;
    if (n_groups != pl.n0) return SFSN_EINVAL;
    int seg_of[SFSN_MAX_GROUPS];
    unsigned used = 0;
    for (int i = 0; i < n_groups; ++i) {
        const int R = B * groups[i].n_units;
        const int8_t* want = groups[i].spikes_i8 + (size_t)t0 * R * KP;  // (the segments' tensors start at the chunk's first frame)
        int s = -1;
        for (int k = 0; k < pl.n0; ++k)
            if (!((used >> k) & 1u) && pl.p1.seg[k].spikes_i8 == want && pl.p1.seg[k].R == R) { s = k; break; }
        if (s < 0) return SFSN_EINVAL;
        used |= 1u << s;
        seg_of[i] = s;
    }
    if (nt == 0) return SFSN_OK;
    PairEParams pp;
    pp.prog = static_cast<unsigned*>(scratch);
    pp.n0 = pl.tiles0; pp.n0pad = (pl.tiles0 + 7) & ~7; pp.n1end = pp.n0pad + pl.tiles1; pp.lag = lag;
    // ---- the epilogue workgroups: SFSN_L01E_WGS of them (default: see profiles/l01_epilogue_one_launch.md), dealt over the jobs by the
    //      bytes they move, at least one and at most one per clip each, and no more than the scratch has counters for
    {
        const char* e = getenv("SFSN_L01E_WGS");
        int total = e ? atoi(e) : SFSN_L01E_WGS_DEFAULT;
        if (total < 1) total = 1;
        const long long room = (long long)(scratch_bytes / sizeof(unsigned)) - 2 - pp.n1end;
        if (room < pe.n) return SFSN_EINVAL;
        double sum = 0;
        for (int i = 0; i < pe.n; ++i) sum += wt[i];
        int blocks = 0;
        for (int i = 0; i < pe.n; ++i) {
            int nbk = (int)(total * wt[i] / sum + 0.5);
            if (nbk < 1) nbk = 1;
            if (nbk > B) nbk = B;
            const long long left = room - blocks - (pe.n - 1 - i);  // (every later job keeps one)
            if (nbk > left) nbk = (int)left;
            pe.job[i].block0 = blocks; pe.job[i].nblocks = nbk;
            pe.job[i].cnt0 = 2 + pp.n0pad + pl.p1.seg[seg_of[grp[i]]].tile0;
            blocks += nbk;
        }
        pe.E = blocks;
    }
    pp.nblocks = pp.n1end + pe.E;
    hipStream_t st = static_cast<hipStream_t>(stream);
    SFSN_PAIR_LAUNCH(gsn_scan_l01e_kernel, pl, pp, (int)lds_e, st, pl.p0, pl.p1, pp, pe)
}
