// sfsn_pair_dev.h -- what a workgroup of a 16-row scan launch runs, written once for every kernel that carries it (gfx950 only):
// the segment of a block, the roles of sfsn_scan3j_dev.h built from a segment, and the two dispatches
//   layer0_role16: scan3y_role for a segment with feature rows (x_in), round 2's body at one tile per wave for one with an input term;
//   layer1_role16: scan3j_role.
// Callers: gsn_scan_fused3_kernel / gsn_scan_fusedx3_kernel / gsn_scan_l0_kernel (sfsn_kernels.hip: plain, no link),
// gsn_scan_l01_kernel (sfsn_pair16.hip: layer 0 publishes, layer 1 is gated), gsn_scan_l01e_kernel (sfsn_pair16e.hip: layer 1 publishes
// too).  Everything is forced inline and the forms are template arguments: each kernel keeps the registers, LDS and size it had with
// a copy of its own (scripts/device_code_digest.py compares them symbol for symbol; profiles/pair_launch_refactor.md).
#ifndef SFSN_PAIR_DEV_H
#define SFSN_PAIR_DEV_H
#include "sfsn_scan_dev.h"
#include "sfsn_scan3_dev.h"
#include "sfsn_scan3j_dev.h"

// The segment that holds block `block`: the last one whose first block (tile0) is not above it.
__device__ __forceinline__ int scan_segment_of(const ScanParams& p, int block) {
    int s = 0;
    for (int i = 1; i < p.nseg; ++i)
        if (block >= p.seg[i].tile0) s = i;
    return s;
}

__device__ __forceinline__ Scan3yRole scan3y_role_of(const ScanSegDev& sg, int row0, int lsplit, int stagger) {
    Scan3yRole rl;
    rl.x = sg.x_in; rl.w_ih = sg.w_ih_f32; rl.I = sg.I; rl.w_hh = sg.w_hh; rl.w_dq = sg.w_dq; rl.bias = sg.bias;
    rl.bn_alpha = sg.bn_alpha; rl.bn_beta = sg.bn_beta; rl.h_state = sg.h_state; rl.c_state = sg.c_state;
    rl.spikes_f32 = sg.spikes_f32; rl.spikes_i8 = sg.spikes_i8; rl.R = sg.R; rl.row0 = row0;
    rl.count = sg.count; rl.lsplit = lsplit; rl.stagger = stagger;
    return rl;
}

__device__ __forceinline__ Scan3jRole scan3j_role_of(const ScanSegDev& sg, int row0, int lsplit, int stagger) {
    Scan3jRole rl;
    rl.spikes_in = sg.spikes_in; rl.w_ih = sg.w_ih; rl.w_ih_dq = sg.w_ih_dq; rl.w_hh = sg.w_hh; rl.w_dq = sg.w_dq; rl.bias = sg.bias;
    rl.bn_alpha = sg.bn_alpha; rl.bn_beta = sg.bn_beta; rl.h_state = sg.h_state; rl.c_state = sg.c_state;
    rl.spikes_f32 = sg.spikes_f32; rl.spikes_i8 = sg.spikes_i8; rl.R = sg.R; rl.row0 = row0;
    rl.count = sg.count; rl.lsplit = lsplit; rl.stagger = stagger;
    return rl;
}

// A segment with feature rows, its 16 rows from row0: scan3y_role.  p0.lsplit and p0.stagger are that role's.
// (the k-chunk count is compile time: a wave-uniform `if` around operand loads makes hipcc drain lgkmcnt at every merge)
template <int KS, int TL, int OUT, bool PUB>
__device__ __forceinline__ void scan3y_role16(const ScanParams& p0, const ScanSegDev& sg, int row0, char* smem, const StackLink* lk) {
    const Scan3yRole rl = scan3y_role_of(sg, row0, p0.lsplit, p0.stagger);
    if (sg.I > 32) scan3y_role<KS, TL, OUT, 2, PUB>(rl, smem, p0.T, p0.H, p0.NT, lk);
    else scan3y_role<KS, TL, OUT, 1, PUB>(rl, smem, p0.T, p0.H, p0.NT, lk);
}

// Layer 0, block `block` of p0 (fused-x segments first).  The choice of role is wave-uniform (one segment per workgroup) and each role
// keeps its own LDS layout from offset 0.  PUB = false: lk is null and round 2's body is what gsn_scan_kernel<1, KS, 16, 1, OUT, 0>
// runs; PUB = true: the frames whose int8 rows are complete are published in lk->out (scan3y_role<PUB> / scan_body's FLG = 2).
template <int KS, int TL, int OUT, bool PUB>
__device__ __forceinline__ void layer0_role16(const ScanParams& p0, int block, char* smem, const StackLink* lk) {
    const ScanSegDev& sg = p0.seg[scan_segment_of(p0, block)];
    const int row0 = (block - sg.tile0) * 16;
    if (sg.x_in != nullptr) {
        scan3y_role16<KS, TL, OUT, PUB>(p0, sg, row0, smem, lk);
    } else {
        constexpr int NW = 16;  // one output tile per wave, NT <= 14: waves NT .. 15 own none
        constexpr int FLG = PUB ? 2 : 0;
        const int tid = threadIdx.x, lane = tid & 63;
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        const int n = lane & 15, q = lane >> 4;
        const int R = sg.R;
        const int rowc = (row0 + n < R) ? row0 + n : R - 1;
        scan_prologue<1, KS, NW, 1, OUT, 0>(sg, smem, tid, p0.H, p0.NT, R, row0, 16);
        if (wave < p0.NT)
            scan_body<1, KS, NW, 1, OUT, 0, 1, FLG>(sg.zin, sg.w_hh, sg.spikes_f32, sg.spikes_i8, nullptr, sg.h_state, sg.c_state, smem, p0.T,
                                                    p0.H, p0.NT, R, row0, rowc, n, q, tid, wave, 16, lk, nullptr, sg.count);
        else
            scan_body<1, KS, NW, 1, OUT, 0, 0, FLG>(sg.zin, sg.w_hh, sg.spikes_f32, sg.spikes_i8, nullptr, sg.h_state, sg.c_state, smem, p0.T,
                                                    p0.H, p0.NT, R, row0, rowc, n, q, tid, wave, 16, lk, nullptr, sg.count);
    }
}

// Layer 1 (any layer with a fused input), block `block1` of p1: scan3j_role.  OFF / GATED / PUB: its forms; p1.lsplit and p1.stagger are its own.
template <int KS, int TL, int OUT, int OFF, bool GATED, bool PUB>
__device__ __forceinline__ void layer1_role16(const ScanParams& p1, int block1, char* smem, const StackLink* lk) {
    const ScanSegDev& sg = p1.seg[scan_segment_of(p1, block1)];
    const Scan3jRole rl = scan3j_role_of(sg, (block1 - sg.tile0) * 16, p1.lsplit, p1.stagger);
    scan3j_role<KS, TL, OUT, OFF, GATED, PUB>(rl, smem, p1.T, p1.H, p1.NT, lk);
}
#endif
