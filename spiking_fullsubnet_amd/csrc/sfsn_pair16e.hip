// sfsn_pair16e.hip -- layers 0 and 1 of a two-layer sub-band stack at 16 rows per workgroup AND the sub-band epilogue (projection + deep
// filter + pass-through + |.|) in ONE launch (gfx950 only): sfsn_gsn_layer_scan_l01_projdf.
//
// sfsn_pair16.hip took layer 1 off the forward's chain of launches; the longest link left that is no recurrence is projdf_kernel
// (sfsn_projdf.hip), which needs layer 1 to have FINISHED only because it is a launch of its own: a tile of it (one clip, 16 frames, the
// clip's units of one group) reads the last layer's int8 spikes of those 16 frames and nothing else the forward computes.  This kernel
// carries three tiers of workgroups:
//   1. layer 0      blocks [0, n0): the roles of gsn_scan_l01_kernel, publishing (scan3y_role<PUB> / scan_body's publishing form);
//      padding      blocks [n0, n0pad), n0pad a multiple of eight: they only count themselves out;
//   2. layer 1      blocks [n0pad, n1end): scan3j_role, gated on layer-0 block i (n_in = 1) AND publishing (scan3j_role<.., GATED, PUB>);
//   3. the epilogue blocks [n1end, nblocks): projdf16_role below -- projdf_body's work dealt over the 16 waves of a scan workgroup, its
//      loader waves gated on the layer-1 blocks that hold its clips' rows (a contiguous range of counters).
// Same instructions on the same operands: bit-identical to sfsn_gsn_layer_scan_l01 followed by sfsn_proj_deepfilter.
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
#include "sfsn_host.h"
#include "sfsn_scan_host.h"

#define EPI_MAX_JOBS 12
#define EPI_CW 12    // compute waves (matrix phase, coefficient write-out, filter); waves 12 .. 15 are the four loader waves
#define EPI_LW 4
#define EPI_NV 8     // 16-byte spike vectors per LOADER lane and tile (four loaders: <= 2048 per tile, as projdf_body's 2 x 16)
#define EPI_NX 8     // spectrum elements per loader lane and tile (<= 2048 per tile)
#define EPI_RING 3   // LDS slots of (spike tile, spectrum tile), as projdf_body
#define EPI_FT 16    // frames per tile
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

struct EpiJobDev {
    const int8_t* s;   // [T][R][KP] int8 spikes of the group's last layer (frame 0 of the SEQUENCE: the chunk starts at frame t0)
    const int8_t* w;   // packed W_p
    const float* dq;
    const float* bias;
    float* y;          // [T][R][P] coefficient rows (API tensor) or nullptr
    int R, N;          // rows per frame of the group (B * N), units per clip
    int k0, U;         // this job's units [k0, k0 + U) of every clip
    int fc, df, lo;    // bins per unit, filter order, first bin of the GROUP
    int P, NT;
    int block0, nblocks;  // this job's epilogue workgroups (counted from the first epilogue block)
    int cnt0;          // index in prog[] of the counter of the layer-1 block that holds the group's row 0
};
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
// 16 + 16 do not fit the 128 registers of a 16-wave workgroup).  Arithmetic, LDS layout, ring and barrier scheme are projdf_body's; every
// output element is computed by ONE thread from the same expressions, so how the elements are dealt does not reach the results.
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
    constexpr int KP = KS * 64, SROW = KP + 16, C16 = KP / 16, FT = EPI_FT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, q = lane >> 4;
    const int U = jb.U, P = jb.P, N = P, NT = jb.NT;
    const int B = p.B, F = p.F, T = p.T, S = p.S, t1 = p.t1;
    const int MR = FT * U, MRT = (MR + 15) >> 4;
    const int LDF = U * P + 1;                       // odd: the 16 frames of a filter wave hit distinct banks
    const int nb = U * jb.fc, XW = FT + jb.df - 1, NXT = nb * XW, NVT = MR * C16;
    const int SBUF = MRT * 16 * SROW, XB = (NXT * 8 + 15) & ~15, SLOTB = SBUF + XB;
    float* obuf = reinterpret_cast<float*>(smem + EPI_RING * SLOTB);                   // [FT][LDF]
    int* rowoff = reinterpret_cast<int*>(obuf + ((FT * LDF + 3) & ~3));                // [MRT*16]: obuf offset of tile row m (or -1)

    // ---- pass-through bins (passthrough_body): (clip, 64-frame tile) units over ALL epilogue workgroups
    if (p.fcov < F) {
        const int tt = tid & 63, fs = tid >> 6;
        const int ntile = (t1 - p.t0 + 63) / 64, tiles = B * ntile;
        for (int tl = eblk; tl < tiles; tl += p.E) {
            const int b = tl / ntile, t = p.t0 + (tl - b * ntile) * 64 + tt;
            if (t >= t1) continue;
            for (int f = p.fcov + fs; f < F; f += 16) {
                const float2 xv = *reinterpret_cast<const float2*>(p.stft + (((size_t)b * F + f) * T + t) * 2);
                for (int s_ = 0; s_ < S; ++s_) {
                    const size_t o = (((size_t)b * S + s_) * F + f) * T + t;
                    *reinterpret_cast<float2*>(p.enh + 2 * o) = xv;
                    if (p.mag) p.mag[o] = fast_abs2(xv.x, xv.y);
                }
            }
        }
    }

    const int ntile = (t1 - p.t0 + FT - 1) / FT;     // frame tiles per clip
    const int c0 = (int)((long long)B * blk / jb.nblocks), c1 = (int)((long long)B * (blk + 1) / jb.nblocks);
    const int nc = c1 - c0, ntl = nc * ntile;        // my tiles: j -> (frame tile j / nc, clip c0 + j % nc)
    const size_t frame_s = (size_t)jb.R * KP;
    const int fbin0 = jb.lo + jb.k0 * jb.fc;

    for (int m = tid; m < MRT * 16; m += 1024) {
        const int fl = m / U, u = m - fl * U;
        rowoff[m] = m < MR ? fl * LDF + u * P : -1;
    }

    if (wave >= EPI_CW) {
        // ================================================= loader wave k =================================================
        const int k = wave - EPI_CW;
        // my vectors of a tile: piece index 4 i + k (a piece = 64 consecutive 16-byte vectors / spectrum elements)
        int s_fl[EPI_NV], s_in[EPI_NV], s_lds[EPI_NV];
#pragma unroll
        for (int i = 0; i < EPI_NV; ++i) {
            int v = (EPI_LW * i + k) * 64 + lane;
            const bool have = v < NVT;
            if (v > NVT - 1) v = NVT - 1;
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
            const int ec = e < NXT ? e : NXT - 1;
            const int j = ec / XW, c = ec - j * XW;
            x_jc[i] = e < NXT ? (j << 8) | c : -1;
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
            const int fi = j / nc, b = c0 + (j - fi * nc), tb = p.t0 + fi * FT;
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
            char* sl = smem + slot * SLOTB;
#pragma unroll
            for (int i = 0; i < EPI_NV; ++i)
                if (s_lds[i] >= 0) *reinterpret_cast<v4i*>(sl + s_lds[i]) = pre[i];
            float2* xt = reinterpret_cast<float2*>(sl + SBUF);
#pragma unroll
            for (int i = 0; i < EPI_NX; ++i)
                if (x_jc[i] >= 0) xt[(EPI_LW * i + k) * 64 + lane] = ((x_ok >> i) & 1u) ? xpre[i] : make_float2(0.0f, 0.0f);
        };
        // prologue: the first two tiles
        for (int d = 0; d < 2; ++d)
            if (d < ntl) {
                fetch(d);
                park(d);
            }
        __syncthreads();
        int slot = 0;
        for (int j = 0; j < ntl; ++j) {
            const bool more = j + 2 < ntl;
            if (more) fetch(j + 2);
            __builtin_amdgcn_s_barrier();            // (the tile's first barrier: my loads stay in flight across it)
            if (more) park(slot == 0 ? 2 : slot - 1);  // = (slot + 2) % 3: free since the last barrier of tile j - 1
            slot = slot == 2 ? 0 : slot + 1;
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_s_barrier();
        }
        return;
    }

    // ================================================= compute waves =================================================
    const int NWN = NT;                              // (one column tile per wave: the host refuses NT > 12)
    const int MW = EPI_CW / NWN;
    const int cg = wave % NWN, mw = wave / NWN;
    const bool worker = mw < MW;
    // ---- W_p tile of this wave -> registers, once
    v4i W[KS][3];
    const int ct = cg;
    const int col = worker ? ct * 16 + q * 4 : -1;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const size_t tile = (size_t)d * NT + (worker ? ct : 0);
            W[ks][d] = *reinterpret_cast<const v4i*>(jb.w + ((tile * KS + ks) * 64 + lane) * 16);
        }
    const v4f dqv = *reinterpret_cast<const v4f*>(jb.dq + (worker ? col : 0));
    v4f bv;
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[r] = (jb.bias && worker && col + r < N) ? jb.bias[col + r] : 0.0f;
    __syncthreads();
    constexpr int CT = EPI_CW * 64;                  // compute threads
    const int tt = tid & (FT - 1), slot0 = tid / FT, nslot = CT / FT;
    const int Q = (U * P) >> 2;                      // 16-byte units of a frame's coefficient rows
    int slot = 0;
    for (int j = 0; j < ntl; ++j) {
        const int fi = j / nc, b = c0 + (j - fi * nc), tb = p.t0 + fi * FT;
        const char* sl = smem + slot * SLOTB;
        const int8_t* sbuf = reinterpret_cast<const int8_t*>(sl);
        const float2* xc = reinterpret_cast<const float2*>(sl + SBUF);
        // ---- matrix phase: coefficient tile -> obuf (three exact digit products, recombine3, * dq + bias)
        if (worker) {
            for (int mi = mw; mi < MRT; mi += MW) {
                const int8_t* sr = sbuf + (mi * 16 + n) * SROW + q * 16;
                v4i bfr[KS];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) bfr[ks] = *reinterpret_cast<const v4i*>(sr + ks * 64);
                const int ro = rowoff[mi * 16 + n];
                v4i a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0}, a2 = {0, 0, 0, 0};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    a0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(W[ks][0], bfr[ks], a0, 0, 0, 0);
                    a1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(W[ks][1], bfr[ks], a1, 0, 0, 0);
                    a2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(W[ks][2], bfr[ks], a2, 0, 0, 0);
                }
                if (ro >= 0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (col + r < N) obuf[ro + col + r] = recombine3(a0[r], a1[r], a2[r]) * dqv[r] + bv[r];
                }
            }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_s_barrier();
        // ---- the coefficient rows leave once: a wave per frame, whole rows
        if (jb.y) {
            for (int fl = wave; fl < FT; fl += EPI_CW) {
                const int t = tb + fl;
                if (t >= t1) continue;
                float* yp = jb.y + (((size_t)t * jb.R) + (size_t)b * jb.N + jb.k0) * P;
                const float* op = obuf + fl * LDF;
                for (int c4 = lane; c4 < Q; c4 += 64) {
                    const v4f o = {op[4 * c4], op[4 * c4 + 1], op[4 * c4 + 2], op[4 * c4 + 3]};
#if SFSN_NT_OUT
                    __builtin_nontemporal_store(o, reinterpret_cast<v4f*>(yp + 4 * c4));
#else
                    *reinterpret_cast<v4f*>(yp + 4 * c4) = o;
#endif
                }
            }
        }
        // ---- deep filter from LDS (deepfilter_pass_kernel's expressions, as projdf_body)
        {
            const int t = tb + tt;
            if (t < t1) {
                const float* pr = obuf + tt * LDF;
                int u = 0, fci = slot0;
                while (fci >= jb.fc) { fci -= jb.fc; ++u; }
                for (int jj = slot0; jj < nb; jj += nslot) {
                    const int f = fbin0 + u * jb.fc + fci;
                    const float* pu = pr + u * P;
                    for (int s_ = 0; s_ < S; ++s_) {
                        float yr = 0.0f, yi = 0.0f;
                        const float2* xr_ = xc + jj * XW + tt;
                        for (int d = 0; d < jb.df; ++d) {
                            const float2 xv = xr_[d];
                            const float cr = pu[((0 * jb.fc + fci) * jb.df + d) * S + s_];
                            const float ci = pu[((1 * jb.fc + fci) * jb.df + d) * S + s_];
                            yr += xv.x * cr - xv.y * ci;
                            yi += xv.x * ci + xv.y * cr;
                        }
                        const size_t o = (((size_t)b * S + s_) * F + f) * T + t;
                        *reinterpret_cast<float2*>(p.enh + 2 * o) = make_float2(yr, yi);
                        if (p.mag) p.mag[o] = fast_abs2(yr, yi);
                    }
                    fci += nslot;
                    while (fci >= jb.fc) { fci -= jb.fc; ++u; }
                }
            }
        }
        slot = slot == 2 ? 0 : slot + 1;
        // obuf and this tile's ring slot are rewritten next: LDS reads done, stores stay in flight (raw barrier)
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_s_barrier();
    }
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
        // ---- layer 0: publishes the frames whose int8 rows are complete in its own counter (gsn_scan_l01_kernel's roles)
        int s = 0;
        for (int i = 1; i < p0.nseg; ++i)
            if (b >= p0.seg[i].tile0) s = i;
        const ScanSegDev& sg = p0.seg[s];
        const int row0 = (b - sg.tile0) * 16;
        lk.out = pp.prog + 2 + b;
        if (sg.x_in != nullptr) {
            Scan3yRole rl;
            rl.x = sg.x_in; rl.w_ih = sg.w_ih_f32; rl.I = sg.I; rl.w_hh = sg.w_hh; rl.w_dq = sg.w_dq; rl.bias = sg.bias;
            rl.bn_alpha = sg.bn_alpha; rl.bn_beta = sg.bn_beta; rl.h_state = sg.h_state; rl.c_state = sg.c_state;
            rl.spikes_f32 = sg.spikes_f32; rl.spikes_i8 = sg.spikes_i8; rl.R = sg.R; rl.row0 = row0;
            rl.count = sg.count; rl.lsplit = p0.lsplit;
            if (sg.I > 32) scan3y_role<KS, TL, OUT, 2, true>(rl, scan_smem, p0.T, p0.H, p0.NT, &lk);
            else scan3y_role<KS, TL, OUT, 1, true>(rl, scan_smem, p0.T, p0.H, p0.NT, &lk);
        } else {
            constexpr int NW = 16;
            const int tid = threadIdx.x, lane = tid & 63;
            const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
            const int n = lane & 15, q = lane >> 4;
            const int R = sg.R;
            const int rowc = (row0 + n < R) ? row0 + n : R - 1;
            scan_prologue<1, KS, NW, 1, OUT, 0>(sg, scan_smem, tid, p0.H, p0.NT, R, row0, 16);
            if (wave < p0.NT)
                scan_body<1, KS, NW, 1, OUT, 0, 1, 2>(sg.zin, sg.w_hh, sg.spikes_f32, sg.spikes_i8, nullptr, sg.h_state, sg.c_state, scan_smem,
                                                      p0.T, p0.H, p0.NT, R, row0, rowc, n, q, tid, wave, 16, &lk, nullptr, sg.count);
            else
                scan_body<1, KS, NW, 1, OUT, 0, 0, 2>(sg.zin, sg.w_hh, sg.spikes_f32, sg.spikes_i8, nullptr, sg.h_state, sg.c_state, scan_smem,
                                                      p0.T, p0.H, p0.NT, R, row0, rowc, n, q, tid, wave, 16, &lk, nullptr, sg.count);
        }
    } else if (b >= pp.n0pad && b < pp.n1end) {
        // ---- layer 1: gated on the layer-0 workgroup of the same 16 rows, publishing for the epilogue workgroups
        const int b1 = b - pp.n0pad;
        int s = 0;
        for (int i = 1; i < p1.nseg; ++i)
            if (b1 >= p1.seg[i].tile0) s = i;
        const ScanSegDev& sg = p1.seg[s];
        lk.in = pp.prog + 2 + b1; lk.n_in = 1;
        lk.out = pp.prog + 2 + b;
        Scan3jRole rl;
        rl.spikes_in = sg.spikes_in; rl.w_ih = sg.w_ih; rl.w_ih_dq = sg.w_ih_dq; rl.w_hh = sg.w_hh; rl.w_dq = sg.w_dq; rl.bias = sg.bias;
        rl.bn_alpha = sg.bn_alpha; rl.bn_beta = sg.bn_beta; rl.h_state = sg.h_state; rl.c_state = sg.c_state;
        rl.spikes_f32 = sg.spikes_f32; rl.spikes_i8 = sg.spikes_i8; rl.R = sg.R; rl.row0 = (b1 - sg.tile0) * 16;
        rl.count = sg.count; rl.lsplit = p1.lsplit;
        scan3j_role<KS, TL, OUT, OFF, true, true>(rl, scan_smem, p1.T, p1.H, p1.NT, &lk);
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

// the LDS layout of projdf16_role (= projdf_body's)
static size_t epi_lds_bytes(int KS, int U, int P, int fc, int df) {
    const int KP = KS * 64, SROW = KP + 16, MRT = (EPI_FT * U + 15) / 16;
    const size_t slot = (size_t)MRT * 16 * SROW + (((size_t)U * fc * (EPI_FT + df - 1) * 8 + 15) & ~(size_t)15);
    const size_t obuf = (size_t)((EPI_FT * (U * P + 1) + 3) & ~3) * 4;
    const size_t rows = (size_t)MRT * 16 * 4;
    return EPI_RING * slot + obuf + rows;
}

// Each list gets the answers of its own entry point, for the list at fault and in the order x, z, layer 1 (sfsn_gsn_layer_scan_l01's),
// groups (sfsn_proj_deepfilter's); then what ties the lists together.  See include/sfsn.h.
extern "C" int sfsn_gsn_layer_scan_l01_projdf(const sfsn_scan_segment* segs_x, const sfsn_fused_x* fin_x, int n_x, const sfsn_scan_segment* segs_z,
                                              int n_z, const sfsn_scan_segment* segs1, const sfsn_fused_input* fin1, int H, int shared, int lag,
                                              void* scratch, size_t scratch_bytes, const float* stft_ri, int B, int F, int T, int S,
                                              const sfsn_projdf_group* groups, int n_groups, float* enh_ri, float* enh_mag, int t0, int nt,
                                              void* stream) {
    // ---- the scalar arguments: sfsn_gsn_layer_scan_l01's (its T is this chunk's nt), then sfsn_proj_deepfilter's
    if (n_x < 0 || n_z < 0 || n_x > SFSN_MAX_SEGMENTS || n_z > SFSN_MAX_SEGMENTS || n_x + n_z == 0 || nt < 0 || H <= 0 || lag < 0) return SFSN_EINVAL;
    if ((n_x > 0 && (!segs_x || !fin_x)) || (n_z > 0 && !segs_z) || !segs1 || !fin1 || !scratch) return SFSN_EINVAL;
    if (!stft_ri || !enh_ri || !groups || n_groups <= 0 || n_groups > SFSN_MAX_GROUPS || B <= 0 || F < 2 || T <= 0 || S <= 0) return SFSN_EINVAL;
    if (t0 < 0 || t0 + nt > T) return SFSN_EINVAL;
    if (H % 16 != 0 || H <= 128 || H > 256) return SFSN_EUNSUPPORTED;
    ScanParams p0, p1;
    p0.wg_times = nullptr; p0.rpw = 16; p0.w16 = 0;
    p1.wg_times = nullptr; p1.rpw = 16; p1.w16 = 0;
    const int n0 = n_x + n_z;
    // ---- layer 0, the fused-x list
    int tiles = 0, imax = 0;
    const int out = 2 | ((n_x > 0 ? segs_x[0].spikes_f32 : segs_z[0].spikes_f32) ? 1 : 0);
    const int rc = fused_x_segments(segs_x, fin_x, n_x, out, p0.seg, tiles, imax);
    if (rc != SFSN_OK) return rc;
    const int NT = H / 16;
    if (NT > 14 || getenv("SFSN_FUSED_V2") || getenv("SFSN_SCAN_V2")) return SFSN_EUNSUPPORTED;
    // ---- layer 0, the input-term list
    ScanSegDev zdev[SFSN_MAX_SEGMENTS];
    int tiles_z = tiles;
    if (n_z > 0) {
        const int out_z = 2 | (segs_z[0].spikes_f32 ? 1 : 0) | (segs_z[0].membrane ? 4 : 0);
        if (out_z == 6) return SFSN_EUNSUPPORTED;
        if (zin_segments(segs_z, n_z, out_z, 16, zdev, tiles_z) != SFSN_OK) return SFSN_EINVAL;
        if ((out_z & 4) || out_z != out) return SFSN_EUNSUPPORTED;
    }
    if (!shared || n0 > SFSN_MAX_SEGMENTS) return SFSN_EUNSUPPORTED;
    for (int i = 0; i < n_z; ++i) p0.seg[n_x + i] = zdev[i];
    // ---- layer 1
    const int out1 = 2 | (segs1[0].spikes_f32 ? 1 : 0);
    int tiles1 = 0;
    if (fused_segments(segs1, fin1, n0, out1, p1.seg, tiles1) != SFSN_OK) return SFSN_EINVAL;
    if (out1 != out) return SFSN_EUNSUPPORTED;
    // ---- the groups (sfsn_proj_deepfilter's checks and its deal of units over jobs, with this role's prefetch slots)
    const int KS = (H + 63) / 64, KP = KS * 64;
    const size_t lds_cap_env = (size_t)sfsn_knob("SFSN_PDF_LDS_KB", 150) * 1024;
    EpiParams pe;
    pe.n = 0; pe.B = B; pe.F = F; pe.T = T; pe.S = S; pe.t0 = t0; pe.t1 = t0 + nt; pe.stft = stft_ri; pe.enh = enh_ri; pe.mag = enh_mag;
    double wt[EPI_MAX_JOBS];
    int grp[EPI_MAX_JOBS];
    size_t lds_e = 0;
    int lo = 0;
    for (int i = 0; i < n_groups; ++i) {
        const sfsn_projdf_group& g = groups[i];
        if (!g.spikes_i8 || !g.w_packed || !g.w_dq || g.n_units <= 0 || g.fc <= 0 || g.df <= 0) return SFSN_EINVAL;
        if (!aligned16(g.spikes_i8) || !aligned16(g.w_packed) || !aligned16(g.w_dq) || !aligned16(g.proj)) return SFSN_EINVAL;
        const int P = 2 * g.fc * g.df * S, NTP = (P + 15) / 16;
        if (P % 4) return SFSN_EUNSUPPORTED;
        if (NTP > EPI_CW) return SFSN_EUNSUPPORTED;  // (one column tile per compute wave: P <= 192)
        int U = g.n_units;
        auto fits = [&](int u) {
            return EPI_FT * u * (KS * 4) <= EPI_LW * EPI_NV * 64 && u * g.fc * (EPI_FT + g.df - 1) <= EPI_LW * EPI_NX * 64 && g.df <= 200 &&
                   epi_lds_bytes(KS, u, P, g.fc, g.df) <= lds_cap_env;
        };
        while (U > 1 && !fits(U)) {
            const int np = (g.n_units + U - 1) / U + 1;  // one more pass
            U = (g.n_units + np - 1) / np;
        }
        if (!fits(U)) return SFSN_EUNSUPPORTED;
        for (int k0 = 0; k0 < g.n_units; k0 += U) {
            if (pe.n >= EPI_MAX_JOBS) return SFSN_EUNSUPPORTED;
            EpiJobDev& d = pe.job[pe.n];
            d.s = g.spikes_i8; d.w = g.w_packed; d.dq = g.w_dq; d.bias = g.bias; d.y = g.proj;
            d.R = B * g.n_units; d.N = g.n_units; d.k0 = k0; d.U = (g.n_units - k0 < U) ? g.n_units - k0 : U;
            d.fc = g.fc; d.df = g.df; d.lo = lo; d.P = P; d.NT = NTP;
            const size_t l = epi_lds_bytes(KS, d.U, P, g.fc, g.df);
            if (l > lds_e) lds_e = l;
            grp[pe.n] = i;
            // bytes a tile moves, as sfsn_proj_deepfilter weighs its jobs (the tile count is the same for every job)
            wt[pe.n] = (double)EPI_FT * d.U * (KP + (d.y ? P * 4.0 : 0.0)) + (double)d.U * g.fc * EPI_FT * (8.0 + S * 12.0);
            ++pe.n;
        }
        lo += g.n_units * g.fc;
    }
    if (lo > F) return SFSN_EINVAL;
    pe.fcov = lo;
    // ---- the lists together: layer 1 reads what layer 0 writes, block for block; every group reads one layer-1 segment's rows
    int rows = 0;
    for (int i = 0; i < n0; ++i) {
        if (p1.seg[i].spikes_in != p0.seg[i].spikes_i8 || p1.seg[i].R != p0.seg[i].R) return SFSN_EINVAL;
        rows += p0.seg[i].R;
    }
    if (tiles1 != tiles_z) return SFSN_EINVAL;  // (cannot happen with equal row counts)
    if (n_groups != n0) return SFSN_EINVAL;
    int seg_of[SFSN_MAX_GROUPS];
    unsigned used = 0;
    for (int i = 0; i < n_groups; ++i) {
        const int R = B * groups[i].n_units;
        const int8_t* want = groups[i].spikes_i8 + (size_t)t0 * R * KP;  // (the segments' tensors start at the chunk's first frame)
        int s = -1;
        for (int k = 0; k < n0; ++k)
            if (!((used >> k) & 1u) && p1.seg[k].spikes_i8 == want && p1.seg[k].R == R) { s = k; break; }
        if (s < 0) return SFSN_EINVAL;
        used |= 1u << s;
        seg_of[i] = s;
    }
    if ((reinterpret_cast<uintptr_t>(scratch) & 3u) || scratch_bytes < sfsn_stack_scratch_bytes(2, n0, rows)) return SFSN_EINVAL;
    if (nt == 0) return SFSN_OK;
    p0.nseg = n0; p0.T = nt; p0.H = H; p0.NT = NT;
    p1.nseg = n0; p1.T = nt; p1.H = H; p1.NT = NT;
    p0.lsplit = sfsn_knob("SFSN_S3Y_LSPLIT", SFSN_S3Y_LSPLIT, 0, 14);
    p1.lsplit = sfsn_knob("SFSN_S3J_LSPLIT", SFSN_S3J_LSPLIT, 0, 14);
    PairEParams pp;
    pp.prog = static_cast<unsigned*>(scratch);
    pp.n0 = tiles_z; pp.n0pad = (tiles_z + 7) & ~7; pp.n1end = pp.n0pad + tiles1; pp.lag = lag;
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
            pe.job[i].cnt0 = 2 + pp.n0pad + p1.seg[seg_of[grp[i]]].tile0;
            blocks += nbk;
        }
        pe.E = blocks;
    }
    pp.nblocks = pp.n1end + pe.E;
    const bool tl = (H & 63) != 0 && (H & 63) <= 32;
    // layer 1 as sfsn_gsn_layer_scan_fused launches it: 14 tiles without an fp32 spike tensor take the OFF form (SFSN_S3J_OFF as there)
    const int offm = getenv("SFSN_S3J_OFF") ? atoi(getenv("SFSN_S3J_OFF")) : 1;
    const bool off = NT == 14 && KS == 4 && tl && (offm == 2 || (offm == 1 && out == 2));
    const int lds_x = KS == 3 ? Scan3yCfg<3, 2>::lds_bytes(NT) : Scan3yCfg<4, 2>::lds_bytes(NT);
    const int lds_j = KS == 3 ? Scan3jCfg<3>::lds_bytes(NT) : (off ? Scan3jCfg<4>::lds_bytes_off(NT) : Scan3jCfg<4>::lds_bytes(NT));
    hipStream_t st = static_cast<hipStream_t>(stream);
#define L01E_CASE(KS_, TL_, OUT_, OFF_)                                                                                         \
    if (KS == KS_ && (int)tl == TL_ && out == OUT_ && (int)off == OFF_) {                                                       \
        const int lds_z = ScanCfg<1, KS_, 16, 1, OUT_, 0>::LDS_BYTES;                                                           \
        int lds = lds_x > lds_z ? lds_x : lds_z;                                                                                \
        lds = lds > lds_j ? lds : lds_j;                                                                                        \
        lds = ((lds > (int)lds_e ? lds : (int)lds_e) + 15) & ~15;                                                               \
        pp.exit_off = lds;                                                                                                      \
        if (lds + 16 > 160 * 1024 - 64) return SFSN_EUNSUPPORTED;                                                               \
        return launch_lds<gsn_scan_l01e_kernel<KS_, TL_, OUT_, OFF_>>(dim3(pp.nblocks), dim3(1024), lds + 16, st, p0, p1, pp, pe); \
    }
    L01E_CASE(3, 0, 2, 0) L01E_CASE(3, 0, 3, 0) L01E_CASE(3, 1, 2, 0) L01E_CASE(3, 1, 3, 0) L01E_CASE(4, 1, 2, 0) L01E_CASE(4, 1, 3, 0)
    L01E_CASE(4, 1, 2, 1) L01E_CASE(4, 1, 3, 1)
#undef L01E_CASE
    return SFSN_EUNSUPPORTED;
}
