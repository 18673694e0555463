// sfsn_pair16.hip -- layers 0 and 1 of a two-layer sub-band stack at 16 rows per workgroup in ONE launch (gfx950 only):
// sfsn_gsn_layer_scan_l01.
//
// With few hardware queues a forward is a serial chain of launches that each hold a fraction of the CUs, and the two
// longest links of bench.py's timed region are the 16-row scans of sub-band layers 0 and 1, back to back only because they are two
// launches: layer 1 needs frame t of layer 0 only at frame t.  This kernel carries the workgroups of both: every workgroup runs the role
// its per-layer launch would have run (scan3y_role / round 2's body for layer 0, scan3j_role for layer 1: sfsn_scan3j_dev.h,
// sfsn_scan_dev.h), in the publishing / gated forms the 8-row stack launch uses (sfsn_scan3_dev.h), each role with its own LDS layout
// from offset 0.  Same instructions on the same operands: bit-identical to sfsn_gsn_layer_scan_l0 + sfsn_gsn_layer_scan_fused.
//
// Block order: layer-0 fused-x segments, layer-0 input-term segments, padding up to a multiple of eight, then the layer-1 segments in the
// same segment order.  Both layers tile a segment's rows in blocks of 16 from the segment's first workgroup, so the producer of layer-1
// block i is layer-0 block i alone (n_in = 1), eight-aligned block ranges put the two on the same XCD (workgroups go to the XCDs round
// robin: the hand-off stays within one L2), and every consumer has a HIGHER block index than its producer.  That is the deadlock-freedom
// argument of sfsn_scan_dev.h (StackLink): workgroups are dispatched in index order, so a resident consumer's producer is resident or has
// finished, and a producer never waits for anybody.  Where more forwards are in flight than the chip holds workgroups, the consumers of a
// launch simply start late and find everything published; no case arises in which a resident workgroup waits for one that has not
// been dispatched.  Every spin is bounded all the same (error word, garbage output, reported by the host).
// Every workgroup (padding blocks too) ends in stack_exit_counters: the last one zeroes the counters for the next launch on the scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "sfsn.h"

#include "sfsn_scan_dev.h"
#include "sfsn_scan3_dev.h"
#include "sfsn_scan3j_dev.h"
#include "sfsn_host.h"
#include "sfsn_scan_host.h"

struct PairParams {
    unsigned* prog;  // [0] error word, [1] workgroups that have exited, [2 + block] frames published by that workgroup
    int nblocks;     // grid size (padding blocks included)
    int n0;          // layer-0 workgroups: blocks [0, n0)
    int n0pad;       // first layer-1 block (n0 rounded up to a multiple of eight); blocks [n0, n0pad) only count themselves out
    int lag;         // frames a consumer lets its producer run ahead between polls
    int exit_off;    // byte offset of the exit word in the dynamic LDS allocation (behind every role's layout)
};

// p0: the layer-0 segments (fused-x first, tile0 = block index; lsplit = the fused-x role's); p1: the layer-1 segments (tile0 counted from
// the first layer-1 block; lsplit = the fused-input role's).  OFF: scan3j_role's form for 14 tiles without an fp32 spike tensor.
template <int KS, int TL, int OUT, int OFF = 0>
__global__ __launch_bounds__(1024) void gsn_scan_l01_kernel(const ScanParams p0, const ScanParams p1, const PairParams pp) {
    extern __shared__ __attribute__((aligned(16))) char scan_smem[];
    int* exit_word = reinterpret_cast<int*>(scan_smem + pp.exit_off);
    const int b = (int)blockIdx.x;
    StackLink lk;
    lk.in = nullptr; lk.n_in = 0; lk.out = nullptr; lk.err = pp.prog; lk.lag = pp.lag; lk.dbg = nullptr;
    if (b < pp.n0) {
        // ---- layer 0: publishes the frames whose int8 rows are complete in its own counter
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
            constexpr int NW = 16;  // round 2's body, one output tile per wave (gsn_scan_l0_kernel), in its publishing form
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
    } else if (b >= pp.n0pad) {
        // ---- layer 1: its loader wave gates every frame on the counter of the layer-0 workgroup that owns the same 16 rows
        const int b1 = b - pp.n0pad;
        int s = 0;
        for (int i = 1; i < p1.nseg; ++i)
            if (b1 >= p1.seg[i].tile0) s = i;
        const ScanSegDev& sg = p1.seg[s];
        lk.in = pp.prog + 2 + b1; lk.n_in = 1;
        Scan3jRole rl;
        rl.spikes_in = sg.spikes_in; rl.w_ih = sg.w_ih; rl.w_ih_dq = sg.w_ih_dq; rl.w_hh = sg.w_hh; rl.w_dq = sg.w_dq; rl.bias = sg.bias;
        rl.bn_alpha = sg.bn_alpha; rl.bn_beta = sg.bn_beta; rl.h_state = sg.h_state; rl.c_state = sg.c_state;
        rl.spikes_f32 = sg.spikes_f32; rl.spikes_i8 = sg.spikes_i8; rl.R = sg.R; rl.row0 = (b1 - sg.tile0) * 16;
        rl.count = sg.count; rl.lsplit = p1.lsplit;
        scan3j_role<KS, TL, OUT, OFF, true>(rl, scan_smem, p1.T, p1.H, p1.NT, &lk);
    }
    stack_exit_counters(pp, exit_word);
}

// Each list gets the answers of its own entry point, for the list at fault and in the order x, z, layer 1 (sfsn_scan_host.h); then what
// ties the lists together.  See include/sfsn.h.
extern "C" int sfsn_gsn_layer_scan_l01(const sfsn_scan_segment* segs_x, const sfsn_fused_x* fin_x, int n_x, const sfsn_scan_segment* segs_z,
                                       int n_z, const sfsn_scan_segment* segs1, const sfsn_fused_input* fin1, int T, int H, int shared, int lag,
                                       void* scratch, size_t scratch_bytes, void* stream) {
    if (n_x < 0 || n_z < 0 || n_x > SFSN_MAX_SEGMENTS || n_z > SFSN_MAX_SEGMENTS || n_x + n_z == 0 || T < 0 || H <= 0 || lag < 0) return SFSN_EINVAL;
    if ((n_x > 0 && (!segs_x || !fin_x)) || (n_z > 0 && !segs_z) || !segs1 || !fin1 || !scratch) return SFSN_EINVAL;
    if (H % 16 != 0 || H <= 128 || H > 256) return SFSN_EUNSUPPORTED;  // (the range of the fused-x and the fused-input entry points)
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
    if (NT > 14 || getenv("SFSN_FUSED_V2") || getenv("SFSN_SCAN_V2")) return SFSN_EUNSUPPORTED;  // (round 2's bodies at 512 threads)
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
    // ---- the lists together: layer 1 reads what layer 0 writes, block for block
    int rows = 0;
    for (int i = 0; i < n0; ++i) {
        if (p1.seg[i].spikes_in != p0.seg[i].spikes_i8 || p1.seg[i].R != p0.seg[i].R) return SFSN_EINVAL;
        rows += p0.seg[i].R;
    }
    if (tiles1 != tiles_z) return SFSN_EINVAL;  // (cannot happen with equal row counts)
    if ((reinterpret_cast<uintptr_t>(scratch) & 3u) || scratch_bytes < sfsn_stack_scratch_bytes(2, n0, rows)) return SFSN_EINVAL;
    if (T == 0) return SFSN_OK;
    p0.nseg = n0; p0.T = T; p0.H = H; p0.NT = NT;
    p1.nseg = n0; p1.T = T; p1.H = H; p1.NT = NT;
    p0.lsplit = sfsn_knob("SFSN_S3Y_LSPLIT", SFSN_S3Y_LSPLIT, 0, 14);
    p1.lsplit = sfsn_knob("SFSN_S3J_LSPLIT", SFSN_S3J_LSPLIT, 0, 14);
    PairParams pp;
    pp.prog = static_cast<unsigned*>(scratch);
    pp.n0 = tiles_z; pp.n0pad = (tiles_z + 7) & ~7; pp.nblocks = pp.n0pad + tiles1; pp.lag = lag;
    const int KS = (H + 63) / 64;
    const bool tl = (H & 63) != 0 && (H & 63) <= 32;
    // layer 1 as sfsn_gsn_layer_scan_fused launches it: 14 tiles without an fp32 spike tensor take the OFF form (SFSN_S3J_OFF as there)
    const int offm = getenv("SFSN_S3J_OFF") ? atoi(getenv("SFSN_S3J_OFF")) : 1;
    const bool off = NT == 14 && KS == 4 && tl && (offm == 2 || (offm == 1 && out == 2));
    const int lds_x = KS == 3 ? Scan3yCfg<3, 2>::lds_bytes(NT) : Scan3yCfg<4, 2>::lds_bytes(NT);
    const int lds_j = KS == 3 ? Scan3jCfg<3>::lds_bytes(NT) : (off ? Scan3jCfg<4>::lds_bytes_off(NT) : Scan3jCfg<4>::lds_bytes(NT));
    hipStream_t st = static_cast<hipStream_t>(stream);
#define L01_CASE(KS_, TL_, OUT_, OFF_)                                                                                     \
    if (KS == KS_ && (int)tl == TL_ && out == OUT_ && (int)off == OFF_) {                                                  \
        const int lds_z = ScanCfg<1, KS_, 16, 1, OUT_, 0>::LDS_BYTES;                                                      \
        int lds = lds_x > lds_z ? lds_x : lds_z;                                                                           \
        lds = ((lds > lds_j ? lds : lds_j) + 15) & ~15;                                                                    \
        pp.exit_off = lds;                                                                                                 \
        if (lds + 16 > 160 * 1024 - 64) return SFSN_EUNSUPPORTED;                                                          \
        return launch_lds<gsn_scan_l01_kernel<KS_, TL_, OUT_, OFF_>>(dim3(pp.nblocks), dim3(1024), lds + 16, st, p0, p1, pp); \
    }
    L01_CASE(3, 0, 2, 0) L01_CASE(3, 0, 3, 0) L01_CASE(3, 1, 2, 0) L01_CASE(3, 1, 3, 0) L01_CASE(4, 1, 2, 0) L01_CASE(4, 1, 3, 0)
    L01_CASE(4, 1, 2, 1) L01_CASE(4, 1, 3, 1)
#undef L01_CASE
    return SFSN_EUNSUPPORTED;
}
