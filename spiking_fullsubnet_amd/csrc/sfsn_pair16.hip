// sfsn_pair16.hip -- layers 0 and 1 of a two-layer sub-band stack at 16 rows per workgroup in ONE launch (gfx950 only):
// sfsn_gsn_layer_scan_l01.
//
// With few hardware queues a forward is a serial chain of launches that each hold a fraction of the CUs, and the two
// longest links of bench.py's timed region are the 16-row scans of sub-band layers 0 and 1, back to back only because they are two
// launches: layer 1 needs frame t of layer 0 only at frame t.  This kernel carries the workgroups of both: every workgroup runs the role
// its per-layer launch would have run (layer0_role16 / layer1_role16, sfsn_pair_dev.h: the functions gsn_scan_l0_kernel and
// gsn_scan_fused3_kernel call), in the publishing / gated forms the 8-row stack launch uses (sfsn_scan3_dev.h), each role with its own
// LDS layout from offset 0.  Same instructions on the same operands: bit-identical to sfsn_gsn_layer_scan_l0 + sfsn_gsn_layer_scan_fused.
// This unit states the two-tier launch: the block ranges, the link of each tier and the launch parameters; the checks of the lists,
// the form rule, the LDS size and the case dispatch are sfsn_scan_host.h's, shared with sfsn_pair16e.hip.
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
#include "sfsn_pair_dev.h"
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
        lk.out = pp.prog + 2 + b;
        layer0_role16<KS, TL, OUT, true>(p0, b, scan_smem, &lk);
    } else if (b >= pp.n0pad) {
        // ---- layer 1: its loader wave gates every frame on the counter of the layer-0 workgroup that owns the same 16 rows
        const int b1 = b - pp.n0pad;
        lk.in = pp.prog + 2 + b1; lk.n_in = 1;
        layer1_role16<KS, TL, OUT, OFF, true, false>(p1, b1, scan_smem, &lk);
    }
    stack_exit_counters(pp, exit_word);
}

// The answers and their order: pair_lists_each, then pair_lists_together (sfsn_scan_host.h).  See include/sfsn.h.
extern "C" int sfsn_gsn_layer_scan_l01(const sfsn_scan_segment* segs_x, const sfsn_fused_x* fin_x, int n_x, const sfsn_scan_segment* segs_z,
                                       int n_z, const sfsn_scan_segment* segs1, const sfsn_fused_input* fin1, int T, int H, int shared, int lag,
                                       void* scratch, size_t scratch_bytes, void* stream) {
    PairLists pl;
    int rc = pair_lists_each(segs_x, fin_x, n_x, segs_z, n_z, segs1, fin1, T, H, shared, lag, scratch, pl);
    if (rc == SFSN_OK) rc = pair_lists_together(pl, T, H, scratch, scratch_bytes);
    if (rc != SFSN_OK || T == 0) return rc;
    PairParams pp;
    pp.prog = static_cast<unsigned*>(scratch);
    pp.n0 = pl.tiles0; pp.n0pad = (pl.tiles0 + 7) & ~7; pp.nblocks = pp.n0pad + pl.tiles1; pp.lag = lag;
    hipStream_t st = static_cast<hipStream_t>(stream);
    SFSN_PAIR_LAUNCH(gsn_scan_l01_kernel, pl, pp, 0, st, pl.p0, pl.p1, pp)
}
