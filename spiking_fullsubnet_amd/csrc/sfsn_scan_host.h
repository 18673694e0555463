// Host-only: the per-segment checks of the per-layer scan entry points and the segments as the device sees them (ScanSegDev), shared by
// the units that launch those scans (sfsn_kernels.hip, sfsn_pair16.hip, sfsn_pair16e.hip): a launch that carries several kinds of segment
// gives each list the answers of the list's own entry point.  Below them what the launches with more than one role share: the form
// rule of scan3j_role, the roles' LDS size, the two stages of the pair lists and the case dispatch.  Nothing here reaches the device code.
#pragma once
#include "sfsn_host.h"
#include "sfsn_scan_dev.h"
#include "sfsn_scan3j_dev.h"

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

// =====================================================================================================
// The 16-row launches that carry more than one role (gsn_scan_l0_kernel, gsn_scan_l01_kernel, gsn_scan_l01e_kernel): what their
// entry points share.
// =====================================================================================================
// scan3j_role's form for 14 tiles (sfsn_scan3j_dev.h): SFSN_S3J_OFF = 0 / 1 / 2: never / without an fp32 spike tensor only (default:
// the measurements are at sfsn_gsn_layer_scan_fused) / always (A/B runs).
static inline bool s3j_off_form(int NT, int KS, bool tl, int out) {
    const int offm = getenv("SFSN_S3J_OFF") ? atoi(getenv("SFSN_S3J_OFF")) : 1;
    return NT == 14 && KS == 4 && tl && (offm == 2 || (offm == 1 && out == 2));
}
// The stagger of the 16-row roles' compute waves (sfsn_scan3j_dev.h): wave slots in head order (bits 0-3) and at priority 1 (bits
// 4-7).  SFSN_S3J_STAGGER=<order mask>[,<priority mask>] is read on every call, in every build (tests switch it inside one process).
static inline int s3j_stagger() {
    int order = SFSN_S3J_STAGGER_ORDER, prio = SFSN_S3J_STAGGER_PRIO;
    if (const char* e = getenv("SFSN_S3J_STAGGER")) {
        char* end = nullptr;
        order = (int)strtol(e, &end, 0);
        prio = (end && *end == ',') ? (int)strtol(end + 1, nullptr, 0) : 0;
    }
    return (order & 15) | ((prio & 15) << 4);
}
// Dynamic LDS of a layer-0 workgroup (the larger of scan3y_role's layout and round 2's), and of a workgroup that may run any role of
// a layers 0+1 launch or `more` bytes of another one (rounded to 16: the exit word sits behind it).
template <int KS, int OUT>
static inline int layer0_lds_bytes(int NT) {
    const int lds_x = Scan3yCfg<KS, 2>::lds_bytes(NT), lds_z = ScanCfg<1, KS, 16, 1, OUT, 0>::LDS_BYTES;
    return lds_x > lds_z ? lds_x : lds_z;
}
template <int KS, int OUT>
static inline int pair_lds_bytes(int NT, bool off, int more) {
    const int lds_j = off ? Scan3jCfg<KS>::lds_bytes_off(NT) : Scan3jCfg<KS>::lds_bytes(NT);
    int lds = layer0_lds_bytes<KS, OUT>(NT);
    lds = lds > lds_j ? lds : lds_j;
    return ((lds > more ? lds : more) + 15) & ~15;
}

// The lists of sfsn_gsn_layer_scan_l01 / _l01_projdf as the device sees them, and what selects the kernel.
struct PairLists {
    ScanParams p0, p1;   // layer 0 (fused-x segments first, tile0 = block index) and layer 1 (tile0 from the first layer-1 block)
    int n0;              // segments per layer
    int out, NT, KS;
    bool tl, off;        // the kernels' TL and OFF (s3j_off_form)
    int tiles0, tiles1;  // workgroups of layer 0 / layer 1
};

// Stage one, each list alone: the scalar arguments, then every list with the answers of its own entry point, for the list at fault
// and in the order x, z, layer 1, and the output set they must share.  T: the frames of the launch.
static inline int pair_lists_each(const sfsn_scan_segment* segs_x, const sfsn_fused_x* fin_x, int n_x, const sfsn_scan_segment* segs_z, int n_z,
                                  const sfsn_scan_segment* segs1, const sfsn_fused_input* fin1, int T, int H, int shared, int lag,
                                  const void* scratch, PairLists& pl) {
    if (n_x < 0 || n_z < 0 || n_x > SFSN_MAX_SEGMENTS || n_z > SFSN_MAX_SEGMENTS || n_x + n_z == 0 || T < 0 || H <= 0 || lag < 0) return SFSN_EINVAL;
    if ((n_x > 0 && (!segs_x || !fin_x)) || (n_z > 0 && !segs_z) || !segs1 || !fin1 || !scratch) return SFSN_EINVAL;
    if (H % 16 != 0 || H <= 128 || H > 256) return SFSN_EUNSUPPORTED;  // (the range of the fused-x and the fused-input entry points)
    ScanParams &p0 = pl.p0, &p1 = pl.p1;
    p0.wg_times = nullptr; p0.rpw = 16; p0.w16 = 0;
    p1.wg_times = nullptr; p1.rpw = 16; p1.w16 = 0;
    pl.n0 = n_x + n_z;
    // ---- layer 0, the fused-x list
    int tiles = 0, imax = 0;
    const int out = 2 | ((n_x > 0 ? segs_x[0].spikes_f32 : segs_z[0].spikes_f32) ? 1 : 0);
    const int rc = fused_x_segments(segs_x, fin_x, n_x, out, p0.seg, tiles, imax);
    if (rc != SFSN_OK) return rc;
    pl.NT = H / 16;
    if (pl.NT > 14 || getenv("SFSN_FUSED_V2") || getenv("SFSN_SCAN_V2")) return SFSN_EUNSUPPORTED;  // (round 2's bodies at 512 threads)
    // ---- layer 0, the input-term list
    ScanSegDev zdev[SFSN_MAX_SEGMENTS];
    pl.tiles0 = tiles;
    if (n_z > 0) {
        const int out_z = 2 | (segs_z[0].spikes_f32 ? 1 : 0) | (segs_z[0].membrane ? 4 : 0);
        if (out_z == 6) return SFSN_EUNSUPPORTED;
        if (zin_segments(segs_z, n_z, out_z, 16, zdev, pl.tiles0) != SFSN_OK) return SFSN_EINVAL;
        if ((out_z & 4) || out_z != out) return SFSN_EUNSUPPORTED;
    }
    if (!shared || pl.n0 > SFSN_MAX_SEGMENTS) return SFSN_EUNSUPPORTED;
    for (int i = 0; i < n_z; ++i) p0.seg[n_x + i] = zdev[i];
    // ---- layer 1
    const int out1 = 2 | (segs1[0].spikes_f32 ? 1 : 0);
    pl.tiles1 = 0;
    if (fused_segments(segs1, fin1, pl.n0, out1, p1.seg, pl.tiles1) != SFSN_OK) return SFSN_EINVAL;
    if (out1 != out) return SFSN_EUNSUPPORTED;
    pl.out = out;
    return SFSN_OK;
}

// Stage two, the lists together: layer 1 reads what layer 0 writes, block for block, and the scratch holds a counter per block; then
// what the launch is made with.
static inline int pair_lists_together(PairLists& pl, int T, int H, const void* scratch, size_t scratch_bytes) {
    ScanParams &p0 = pl.p0, &p1 = pl.p1;
    int rows = 0;
    for (int i = 0; i < pl.n0; ++i) {
        if (p1.seg[i].spikes_in != p0.seg[i].spikes_i8 || p1.seg[i].R != p0.seg[i].R) return SFSN_EINVAL;
        rows += p0.seg[i].R;
    }
    if (pl.tiles1 != pl.tiles0) return SFSN_EINVAL;  // (cannot happen with equal row counts)
    if ((reinterpret_cast<uintptr_t>(scratch) & 3u) || scratch_bytes < sfsn_stack_scratch_bytes(2, pl.n0, rows)) return SFSN_EINVAL;
    p0.nseg = pl.n0; p0.T = T; p0.H = H; p0.NT = pl.NT;
    p1.nseg = pl.n0; p1.T = T; p1.H = H; p1.NT = pl.NT;
    p0.lsplit = sfsn_knob("SFSN_S3Y_LSPLIT", SFSN_S3Y_LSPLIT, 0, 14);
    p1.lsplit = sfsn_knob("SFSN_S3J_LSPLIT", SFSN_S3J_LSPLIT, 0, 14);
    p0.stagger = p1.stagger = s3j_stagger();
    pl.KS = (H + 63) / 64;
    pl.tl = (H & 63) != 0 && (H & 63) <= 32;
    // layer 1 as sfsn_gsn_layer_scan_fused launches it
    pl.off = s3j_off_form(pl.NT, pl.KS, pl.tl, pl.out);
    return SFSN_OK;
}

// The launch: KERNEL<KS, TL, OUT, OFF> for the lists `pl`, params `pp` (exit_off is set here), `more` bytes of LDS another role of
// the launch asks for, the kernel's arguments behind it.
#define SFSN_PAIR_CASE(KERNEL, KS_, TL_, OUT_, OFF_, pl, pp, more, st, ...)                                                \
    if (pl.KS == KS_ && (int)pl.tl == TL_ && pl.out == OUT_ && (int)pl.off == OFF_) {                                       \
        const int lds = pair_lds_bytes<KS_, OUT_>(pl.NT, pl.off, more);                                                     \
        pp.exit_off = lds;                                                                                                  \
        if (lds + 16 > 160 * 1024 - 64) return SFSN_EUNSUPPORTED;                                                           \
        return launch_lds<KERNEL<KS_, TL_, OUT_, OFF_>>(dim3(pp.nblocks), dim3(1024), lds + 16, st, __VA_ARGS__);           \
    }
#define SFSN_PAIR_LAUNCH(KERNEL, pl, pp, more, st, ...)                                                                    \
    SFSN_PAIR_CASE(KERNEL, 3, 0, 2, 0, pl, pp, more, st, __VA_ARGS__) SFSN_PAIR_CASE(KERNEL, 3, 0, 3, 0, pl, pp, more, st, __VA_ARGS__) \
    SFSN_PAIR_CASE(KERNEL, 3, 1, 2, 0, pl, pp, more, st, __VA_ARGS__) SFSN_PAIR_CASE(KERNEL, 3, 1, 3, 0, pl, pp, more, st, __VA_ARGS__) \
    SFSN_PAIR_CASE(KERNEL, 4, 1, 2, 0, pl, pp, more, st, __VA_ARGS__) SFSN_PAIR_CASE(KERNEL, 4, 1, 3, 0, pl, pp, more, st, __VA_ARGS__) \
    SFSN_PAIR_CASE(KERNEL, 4, 1, 2, 1, pl, pp, more, st, __VA_ARGS__) SFSN_PAIR_CASE(KERNEL, 4, 1, 3, 1, pl, pp, more, st, __VA_ARGS__) \
    return SFSN_EUNSUPPORTED;
