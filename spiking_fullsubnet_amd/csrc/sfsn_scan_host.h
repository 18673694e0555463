// Host-only: the per-segment checks of the per-layer scan entry points and the segments as the device sees them (ScanSegDev), shared by
// the units that launch those scans (sfsn_kernels.hip, sfsn_pair16.hip): a launch that carries several kinds of segment gives each list
// the answers of the list's own entry point.  Include behind sfsn_scan_dev.h and sfsn_host.h.  Nothing here reaches the device code.
#pragma once
#include "sfsn_host.h"
#include "sfsn_scan_dev.h"

// The per-segment checks of sfsn_gsn_layer_scan, and the segments as the device sees them in dev[0 .. n_segs) (block indices from
// `tiles` on): shared with sfsn_gsn_layer_scan_l0 / _l01, which must give the same answers.
static inline int zin_segments(const sfsn_scan_segment* segs, int n_segs, int out, int rpw, ScanSegDev* dev, int& tiles) {
    for (int i = 0; i < n_segs; ++i) {
        const sfsn_scan_segment& s = segs[i];
        if (check_segment(s, out, SEG_NEED_ZIN | SEG_MEMBRANE) != SFSN_OK) return SFSN_EINVAL;
        ScanSegDev& d = dev[i];
        copy_segment(d, s, 0);
        d.membrane = s.membrane; d.tile0 = tiles;
        d.x_in = nullptr; d.w_ih_f32 = nullptr; d.I = 0;  // (what tells the two kinds of segment apart in gsn_scan_l0_kernel)
        tiles += (s.R + rpw - 1) / rpw;
    }
    return SFSN_OK;
}

// The per-segment checks of sfsn_gsn_layer_scan_fused_x in their order, and the segments as the device sees them in dev[0 .. n_segs)
// (16 rows per workgroup, block indices from `tiles` on): shared with sfsn_gsn_layer_scan_l0 / _l01, which must give the same answers.
static inline int fused_x_segments(const sfsn_scan_segment* segs, const sfsn_fused_x* fin, int n_segs, int out, ScanSegDev* dev, int& tiles, int& imax) {
    for (int i = 0; i < n_segs; ++i) {
        const sfsn_scan_segment& s = segs[i];
        if (check_segment(s, out, SEG_NO_ZIN | SEG_DEFER_ALIGN) != SFSN_OK || !fin[i].x || !fin[i].w_ih) return SFSN_EINVAL;
        if (fin[i].I <= 0 || fin[i].I > 64 || fin[i].I % 2 != 0 || s.R % 16 != 0) return SFSN_EUNSUPPORTED;  // (answers before alignment)
        if (!aligned16(fin[i].x) || !segment_aligned(s, SEG_NO_ZIN)) return SFSN_EINVAL;
        ScanSegDev& d = dev[i];
        copy_segment(d, s, SEG_NO_ZIN);
        d.membrane = nullptr; d.tile0 = tiles;
        d.spikes_in = nullptr; d.w_ih = nullptr; d.w_ih_dq = nullptr;
        d.x_in = fin[i].x; d.w_ih_f32 = fin[i].w_ih; d.I = fin[i].I;
        if (fin[i].I > imax) imax = fin[i].I;
        tiles += s.R / 16;
    }
    return SFSN_OK;
}

// The per-segment checks of sfsn_gsn_layer_scan_fused, and the segments as the device sees them in dev[0 .. n_segs) (16 rows per
// workgroup, block indices from `tiles` on): shared with sfsn_gsn_layer_scan_l01, which must give the same answers.
static inline int fused_segments(const sfsn_scan_segment* segs, const sfsn_fused_input* fin, int n_segs, int out, ScanSegDev* dev, int& tiles) {
    for (int i = 0; i < n_segs; ++i) {
        const sfsn_scan_segment& s = segs[i];
        if (check_segment(s, out, SEG_NO_ZIN) != SFSN_OK) return SFSN_EINVAL;
        if (!fin[i].spikes_in || !fin[i].w_ih || !fin[i].w_ih_dq || !aligned16(fin[i].spikes_in) || !aligned16(fin[i].w_ih)) return SFSN_EINVAL;
        ScanSegDev& d = dev[i];
        copy_segment(d, s, SEG_NO_ZIN);
        d.membrane = nullptr; d.tile0 = tiles;
        d.spikes_in = fin[i].spikes_in; d.w_ih = fin[i].w_ih; d.w_ih_dq = fin[i].w_ih_dq;
        tiles += (s.R + 15) / 16;
    }
    return SFSN_OK;
}
