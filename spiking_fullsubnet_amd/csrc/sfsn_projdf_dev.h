// sfsn_projdf_dev.h -- one tile of projection + deep filter, for the two launches that run it (gfx950 only):
//   projdf_kernel (sfsn_projdf.hip): 512 threads, six compute waves with up to three column tiles each, two loader waves with 16 + 16
//       prefetch slots per lane, a contiguous range of tiles per workgroup, plain loads;
//   projdf16_role (sfsn_pair16e.hip): a role of a 1,024-thread scan workgroup, twelve compute waves with one column tile each, four loader
//       waves with 8 + 8 slots per lane, frames outer and clips inner, loads gated on the layer-1 workgroups of the same launch.
// Written once here: the job, the tile's LDS layout (host and device), the ring schedule of the loader waves, the compute waves (W_p
// tiles to registers once; per tile the matrix phase, the coefficient write-out and the filter from LDS), the pass-through bins, and
// the host's split of the groups into jobs.  Which tile comes next, a loader lane's share of a tile and how it is requested are the
// callers' (shared lane maps moved projdf_kernel's register count: profiles/pair_launch_refactor.md).  Arithmetic: sfsn_projdf.hip's
// file head.
#ifndef SFSN_PROJDF_DEV_H
#define SFSN_PROJDF_DEV_H
#include "sfsn_feat_dev.h"
#include "sfsn_scan_dev.h"
#include "sfsn_host.h"

#define PDF_RING 3   // LDS slots of (spike tile, spectrum tile): tile j + 2 is written while tile j is multiplied and filtered
#define PDF_FT 16    // frames per tile

// A job: the units [k0, k0 + U) of every clip of one group, on `nblocks` workgroups.
struct PdfJob {
    const int8_t* s;   // [T][R][KP] int8 spikes of the group's last layer (frame 0 of the sequence)
    const int8_t* w;   // packed W_p
    const float* dq;
    const float* bias;
    float* y;          // [T][R][P] coefficient rows (API tensor) or nullptr
    int R, N;          // rows per frame of the group (B * N), units per clip
    int k0, U;         // this job's units [k0, k0 + U) of every clip
    int fc, df, lo;    // bins per unit, filter order, first bin of the GROUP
    int P, NT;
    int block0, nblocks;  // this job's workgroups (counted from the first workgroup that runs jobs)
    int cnt0;          // gated launches: index in prog[] of the counter of the layer-1 block that holds the group's row 0
};

// The dynamic LDS of a tile of FT frames x U units: PDF_RING slots of (spike rows [MRT * 16][SROW], spectrum [nb][XW] float2), the
// coefficient tile obuf [FT][LDF] and the obuf offset of every tile row.  Host and device compute it from the same lines.
struct PdfTile {
    int MR, MRT;       // tile rows (frame-major, U per frame), 16-row blocks of them
    int LDF;           // odd: the 16 frames of a filter wave hit distinct banks
    int nb, XW, NXT;   // bins, spectrum columns per bin (the filter's taps reach back df - 1 frames), spectrum elements
    int NVT;           // 16-byte spike vectors
    int SBUF, SLOTB;   // bytes of a slot's spike rows, of a slot
    int obuf_off, rowoff_off;
    size_t bytes;
    __host__ __device__ __forceinline__ PdfTile(int KS, int FT, int U, int P, int fc, int df) {
        const int KP = KS * 64, SROW = KP + 16;
        MR = FT * U; MRT = (MR + 15) >> 4;
        LDF = U * P + 1;
        nb = U * fc; XW = FT + df - 1; NXT = nb * XW; NVT = MR * (KP / 16);
        SBUF = MRT * 16 * SROW; SLOTB = SBUF + ((NXT * 8 + 15) & ~15);
        obuf_off = PDF_RING * SLOTB;
        rowoff_off = obuf_off + ((FT * LDF + 3) & ~3) * 4;
        bytes = (size_t)rowoff_off + (size_t)MRT * 16 * 4;
    }
};

// rowoff[m]: obuf offset of tile row m (or -1), by all `threads` threads of the workgroup
__device__ __forceinline__ void pdf_fill_rowoff(int* rowoff, const PdfTile& L, int U, int P, int tid, int threads) {
    for (int m = tid; m < L.MRT * 16; m += threads) {
        const int fl = m / U, u = m - fl * U;
        rowoff[m] = m < L.MR ? fl * L.LDF + u * P : -1;
    }
}

// A loader wave's schedule over its workgroup's tiles [j0, j1): fetch(j) requests tile j into registers, park(slot) writes them to a ring
// slot.  The first two tiles before the workgroup's __syncthreads; then tile j + 2 is requested at the top of tile j, crosses the tile's
// first barrier in flight, and lands in slot (j + 2) % 3 (free since tile j - 1's last barrier) before the tile's second barrier.
template <class Fetch, class Park>
__device__ __forceinline__ void pdf_loader_ring(int j0, int j1, Fetch fetch, Park park) {
    for (int d = 0; d < 2; ++d)
        if (j0 + d < j1) {
            fetch(j0 + d);
            park(d);
        }
    __syncthreads();
    int slot = 0;
    for (int j = j0; j < j1; ++j) {
        const bool more = j + 2 < j1;
        if (more) fetch(j + 2);
        __builtin_amdgcn_s_barrier();            // (the tile's first barrier: my loads stay in flight across it)
        if (more) park(slot == 0 ? 2 : slot - 1);  // = (slot + 2) % 3
        slot = slot == 2 ? 0 : slot + 1;
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_s_barrier();
    }
}

// The CW compute waves (waves 0 .. CW - 1) over the workgroup's tiles [j0, j1); tile_of(j, b, tb): clip and first frame of tile j.  Column
// tile cg + NWN i of the job's NT belongs to the waves with wave % NWN == cg (TPW tiles each, their W_p digits in registers for the
// whole launch); the CW / NWN waves of a column share the tile's 16-row blocks.  Per tile: coefficient tile -> obuf (three exact digit
// products, recombine3, * dq + bias), barrier, the coefficient rows leave once (a wave per frame, whole rows; the module API's last
// `all_layer_outputs` entry), the deep filter from LDS (deepfilter_pass_kernel's expressions), barrier.  Every output element is
// computed by ONE thread from the same expressions, so how the elements are dealt does not reach the results.
template <int TPW, int KS, int CW, class Params, class TileOf>
__device__ __forceinline__ void pdf_compute_waves(const Params& p, const PdfJob& jb, const PdfTile& L, int FT, int NWN, char* smem, int j0, int j1,
                                                  TileOf tile_of) {
    constexpr int KP = KS * 64, SROW = KP + 16;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, q = lane >> 4;
    const int U = jb.U, P = jb.P, N = P, NT = jb.NT;
    const int F = p.F, T = p.T, S = p.S, t1 = p.t1;
    const int MRT = L.MRT, LDF = L.LDF, nb = L.nb, XW = L.XW, SBUF = L.SBUF, SLOTB = L.SLOTB;
    float* obuf = reinterpret_cast<float*>(smem + L.obuf_off);
    const int* rowoff = reinterpret_cast<const int*>(smem + L.rowoff_off);
    const int fbin0 = jb.lo + jb.k0 * jb.fc;
    const int MW = CW / NWN;
    const int cg = wave % NWN, mw = wave / NWN;
    const bool worker = mw < MW;
    // ---- W_p tiles of this wave -> registers, once (spike_proj_fast_body's deal)
    v4i W[TPW][KS][3];
    v4f dqv[TPW], bv[TPW];
    int col[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int ct = cg + NWN * i;
        const bool have = worker && (TPW == 1 || ct < NT);  // (TPW = 1: NWN = NT, every column has its tile)
        col[i] = have ? ct * 16 + q * 4 : -1;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const size_t tile = (size_t)d * NT + (have ? ct : 0);
                W[i][ks][d] = *reinterpret_cast<const v4i*>(jb.w + ((tile * KS + ks) * 64 + lane) * 16);
            }
        dqv[i] = *reinterpret_cast<const v4f*>(jb.dq + (have ? col[i] : 0));
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[i][r] = (jb.bias && have && col[i] + r < N) ? jb.bias[col[i] + r] : 0.0f;
    }
    __syncthreads();
    constexpr int CT = CW * 64;                      // compute threads
    const int tt = tid & (FT - 1), slot0 = tid / FT, nslot = CT / FT;
    const int Q = (U * P) >> 2;                      // 16-byte units of a frame's coefficient rows
    int slot = 0;
    for (int j = j0; j < j1; ++j) {
        int b, tb;
        tile_of(j, b, tb);
        const char* sl = smem + slot * SLOTB;
        const int8_t* sbuf = reinterpret_cast<const int8_t*>(sl);
        const float2* xc = reinterpret_cast<const float2*>(sl + SBUF);
        // ---- matrix phase: coefficient tile -> obuf
        if (worker) {
            for (int mi = mw; mi < MRT; mi += MW) {
                const int8_t* sr = sbuf + (mi * 16 + n) * SROW + q * 16;
                v4i bfr[KS];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) bfr[ks] = *reinterpret_cast<const v4i*>(sr + ks * 64);
                const int ro = rowoff[mi * 16 + n];
#pragma unroll
                for (int i = 0; i < TPW; ++i) {
                    if (TPW > 1 && col[i] < 0) continue;
                    v4i a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0}, a2 = {0, 0, 0, 0};
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        a0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(W[i][ks][0], bfr[ks], a0, 0, 0, 0);
                        a1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(W[i][ks][1], bfr[ks], a1, 0, 0, 0);
                        a2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(W[i][ks][2], bfr[ks], a2, 0, 0, 0);
                    }
                    if (ro >= 0) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (col[i] + r < N) obuf[ro + col[i] + r] = recombine3(a0[r], a1[r], a2[r]) * dqv[i][r] + bv[i][r];
                    }
                }
            }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_s_barrier();
        // ---- the coefficient rows leave once
        if (jb.y) {
            for (int fl = wave; fl < FT; fl += CW) {
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
        // ---- deep filter from LDS
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
                        // (plain stores: the two 16-frame halves of a 256-byte run are written by consecutive tiles and merge in the L2 --
                        //  as non-temporal stores the lean strict forward measured 1 % slower)
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

// Bins no group covers (at least Nyquist) pass through untouched (MODEL:461-470): (clip, 64-frame tile) units `first`, `first + stride`,
// ... by a workgroup of 64 x `waves` threads.
template <class Params>
__device__ __forceinline__ void pdf_passthrough(const Params& p, int first, int stride, int waves) {
    const int tid = threadIdx.x, tt = tid & 63, fs = tid >> 6;
    const int ntile = (p.t1 - p.t0 + 63) / 64, tiles = p.B * ntile;
    for (int tl = first; tl < tiles; tl += stride) {
        const int b = tl / ntile, t = p.t0 + (tl - b * ntile) * 64 + tt;
        if (t >= p.t1) continue;
        for (int f = p.fcov + fs; f < p.F; f += waves) {
            const float2 xv = *reinterpret_cast<const float2*>(p.stft + (((size_t)b * p.F + f) * p.T + t) * 2);
            for (int s_ = 0; s_ < p.S; ++s_) {
                const size_t o = (((size_t)b * p.S + s_) * p.F + f) * p.T + t;
                *reinterpret_cast<float2*>(p.enh + 2 * o) = xv;
                if (p.mag) p.mag[o] = fast_abs2(xv.x, xv.y);
            }
        }
    }
}

// =====================================================================================================
// host side
// =====================================================================================================
struct PdfCaps {
    int nv, nx;    // 16-byte spike vectors and spectrum elements the loader waves hold per tile (loaders x slots per lane x 64)
    int cw;        // compute waves
    int max_tpw;   // column tiles per compute wave
    int max_jobs;
};

// sfsn_proj_deepfilter's checks of the groups in their order and its deal of units over jobs: the largest number of units per job that
// fits the prefetch slots and `lds_cap`, one more pass over the group's units until it does.  job[0 .. n): the jobs (block ranges not
// yet dealt), grp: their groups, wt: the bytes a tile of theirs moves (spikes in, coefficient rows out, spectrum in, enhanced spectrum
// + magnitude out), lds: the largest tile; lo: the first bin no group covers.
template <class Job>
static inline int pdf_split_groups(const sfsn_projdf_group* groups, int n_groups, int B, int S, int KS, const PdfCaps& c, size_t lds_cap,
                                   Job* job, int& n, int* grp, double* wt, size_t& lds, int& lo) {
    n = 0; lds = 0; lo = 0;
    for (int i = 0; i < n_groups; ++i) {
        const sfsn_projdf_group& g = groups[i];
        if (!g.spikes_i8 || !g.w_packed || !g.w_dq || g.n_units <= 0 || g.fc <= 0 || g.df <= 0) return SFSN_EINVAL;
        if (!aligned16(g.spikes_i8) || !aligned16(g.w_packed) || !aligned16(g.w_dq) || !aligned16(g.proj)) return SFSN_EINVAL;
        const int P = 2 * g.fc * g.df * S, NT = (P + 15) / 16;
        if (P % 4) return SFSN_EUNSUPPORTED;
        if ((NT + c.cw - 1) / c.cw > c.max_tpw) return SFSN_EUNSUPPORTED;
        int U = g.n_units;
        auto fits = [&](int u) {
            return PDF_FT * u * (KS * 4) <= c.nv && u * g.fc * (PDF_FT + g.df - 1) <= c.nx && g.df <= 200 &&
                   PdfTile(KS, PDF_FT, u, P, g.fc, g.df).bytes <= lds_cap;
        };
        while (U > 1 && !fits(U)) {
            const int np = (g.n_units + U - 1) / U + 1;  // one more pass
            U = (g.n_units + np - 1) / np;
        }
        if (!fits(U)) return SFSN_EUNSUPPORTED;
        for (int k0 = 0; k0 < g.n_units; k0 += U) {
            if (n >= c.max_jobs) return SFSN_EUNSUPPORTED;
            Job& d = job[n];
            d.s = g.spikes_i8; d.w = g.w_packed; d.dq = g.w_dq; d.bias = g.bias; d.y = g.proj;
            d.R = B * g.n_units; d.N = g.n_units; d.k0 = k0; d.U = (g.n_units - k0 < U) ? g.n_units - k0 : U;
            d.fc = g.fc; d.df = g.df; d.lo = lo; d.P = P; d.NT = NT;
            const size_t l = PdfTile(KS, PDF_FT, d.U, P, g.fc, g.df).bytes;
            if (l > lds) lds = l;
            grp[n] = i;
            wt[n] = (double)PDF_FT * d.U * (KS * 64 + (d.y ? P * 4.0 : 0.0)) + (double)d.U * g.fc * PDF_FT * (8.0 + S * 12.0);
            ++n;
        }
        lo += g.n_units * g.fc;
    }
    return SFSN_OK;
}
#endif
