"""The schedule of a forward and the stack rule as pure functions (engine.plan_forward, engine.stack_rule): no GPU, no engine.

Every expected value below is worked out by hand from the rules (the arithmetic is in the comments), with 256 compute units:
  * overlapped when not pipelined, overlap_chunks > 1, no offline / cumulative norm, no seq_chunk below T, T >= 96 * overlap_chunks;
  * its first chunk round(0.24 T / 8) * 8 frames (at most T // 2), the rest cut evenly: ceil((T - first) / (chunks - 1));
  * with the default settings, T >= 256 and fewer than 600 sub-band rows: chunks of round(f T / 8) * 8 for f = .36, .32, .32, the last
    one taking what is left;
  * sub-band rows = B * 13 for the baseline_m geometry (8 + 3 + 2 units per clip).
"""
import dataclasses

import pytest

from spiking_fullsubnet_amd.engine import ForwardPlan, PathSpec, plan_forward, stack_rule

N_CU = 256

LIVE = PathSpec(front="live", n_fft=512, fdrc=0.5, fb_in=64, fb_hidden=320, fb_layers=2, fb_proj=64, sb_hidden=224, sb_layers=2,
                cutoffs=[0, 32, 128, 256], ctr=[4, 32, 64], nbr=[15, 15, 15], ctr_fb=[4, 32, 64], nbr_fb=[0, 0, 0], df=[5, 3, 1],
                shared=True, bn=True)  # 8 + 3 + 2 = 13 units per clip: 832 sub-band rows at B = 64, 416 at B = 32
# baseline_l's sub-band geometry: 16 + 24 + 2 + 1 = 43 units per clip (2752 rows at B = 64), hidden size 256
LARGE = dataclasses.replace(LIVE, sb_hidden=256, cutoffs=[0, 32, 128, 192, 256], ctr=[2, 4, 32, 64], nbr=[15] * 4, ctr_fb=[2, 4, 32, 64],
                            nbr_fb=[0] * 4, df=[5, 3, 1, 1])


def plan(spec=LIVE, B=64, T=1000, pipeline=None, n_cu=N_CU, **attrs) -> ForwardPlan:
    return plan_forward(spec, B, T, pipeline, n_cu, **attrs)


def test_the_specs_have_the_rows_the_cases_name():
    assert sum(LIVE.units(g) for g in range(LIVE.n_groups)) == 13 and sum(LARGE.units(g) for g in range(LARGE.n_groups)) == 43


@pytest.mark.parametrize("B,T,bounds", [
    (64, 1000, [(0, 240), (240, 380), (620, 380)]),  # 832 rows: first = round(30.0) * 8 = 240, rest = ceil(760 / 2) = 380
    (32, 1000, [(0, 360), (360, 320), (680, 320)]),  # 416 rows < 600: round(45.0) * 8, round(40.0) * 8, 1000 - 680
    (64, 288, [(0, 72), (72, 108), (180, 108)]),     # first = round(8.64) * 8 = 72, rest = ceil(216 / 2) = 108
    (32, 288, [(0, 104), (104, 96), (200, 88)]),     # round(12.96) * 8 = 104, round(11.52) * 8 = 96, 288 - 200
    (64, 300, [(0, 72), (72, 114), (186, 114)]),     # first = round(9.0) * 8 = 72, rest = ceil(228 / 2) = 114
], ids=["832rows-T1000", "416rows-T1000", "832rows-T288", "416rows-T288", "832rows-T300"])
def test_overlapped_chunks_with_default_settings(B, T, bounds):
    p = plan(B=B, T=T)
    assert p.overlap and p.staged and not p.pipeline
    assert list(p.bounds) == bounds
    assert p.nt_max == max(n for _, n in bounds)
    assert (p.rpw_fb, p.rpw_sb) == (0, 0)


def test_below_96_frames_per_chunk_there_is_no_overlap():
    p = plan(T=287)  # 287 < 96 * 3
    assert not p.overlap and not p.staged and not p.pipeline
    assert list(p.bounds) == [(0, 287)] and p.nt_max == 287


def test_equal_chunks_when_the_first_is_not_set_apart():
    p = plan(overlap_chunks=4, overlap_first=0)  # ceil(1000 / 4)
    assert p.overlap and list(p.bounds) == [(0, 250), (250, 250), (500, 250), (750, 250)] and p.nt_max == 250


def test_explicit_first_chunk_and_explicit_fractions():
    p = plan(overlap_first=100)  # rest = ceil(900 / 2) = 450
    assert p.overlap and list(p.bounds) == [(0, 100), (100, 450), (550, 450)]
    p = plan(overlap_first=800)  # at most T // 2
    assert list(p.bounds) == [(0, 500), (500, 250), (750, 250)]
    p = plan(overlap_fracs=[0.5, 0.25, 0.25])  # round(62.5) = 62 (to even) -> 496; round(31.25) * 8 = 248; 1000 - 744
    assert p.overlap and list(p.bounds) == [(0, 496), (496, 248), (744, 256)]
    p = plan(B=32, overlap_chunks=2)  # the (.36, .32, .32) rule is for three chunks: first = 240, rest = 760
    assert list(p.bounds) == [(0, 240), (240, 760)]
    p = plan(B=32, T=250, overlap_chunks=2)  # first = round(7.5) * 8 = 64 (to even), rest = 186
    assert list(p.bounds) == [(0, 64), (64, 186)]


def test_seq_chunk_excludes_the_overlap():
    p = plan(seq_chunk=128)
    assert not p.overlap and not p.staged
    assert len(p.bounds) == 8 and p.bounds[0] == (0, 128) and p.bounds[-1] == (896, 104) and p.nt_max == 128
    assert plan(seq_chunk=1000).overlap  # (a chunk of the whole sequence is no chunking)


@pytest.mark.parametrize("B", [4, 64])
def test_pipelined_schedule(B):
    p = plan(B=B, pipeline=True, pipeline_chunk=128)
    assert p.pipeline and p.staged and not p.overlap
    assert (p.rpw_fb, p.rpw_sb) == (16, 16) and p.nt_max == 128
    assert len(p.bounds) == 8 and p.bounds[-1] == (896, 104)
    # the default: opt-in, and only from two chunks on
    assert not plan(B=B).pipeline
    assert plan(B=B, pipeline_default=True, pipeline_chunk=500).pipeline and not plan(B=B, pipeline_default=True, pipeline_chunk=501).pipeline
    assert not plan(B=B, pipeline=False, pipeline_default=True).pipeline


@pytest.mark.parametrize("B", [4, 64])
def test_offline_norms_never_overlap(B):
    for spec in (dataclasses.replace(LIVE, front="frozen", laplace=True), dataclasses.replace(LIVE, front="frozen", laplace=True, gaussian=True)):
        p = plan(spec, B=B)
        assert not p.overlap and not p.staged and list(p.bounds) == [(0, 1000)]
        assert plan(spec, B=B, pipeline=True).pipeline  # (its layer pairs may still be pipelined)


@pytest.mark.parametrize("B", [4, 64])
def test_cumulative_norm_runs_in_single_stream_order(B):
    spec = dataclasses.replace(LIVE, front="frozen", cum_laplace=True)
    for asked in (None, True):
        p = plan(spec, B=B, pipeline=asked, pipeline_default=True)
        assert not p.pipeline and not p.overlap and not p.staged and list(p.bounds) == [(0, 1000)]


def test_sub_band_rows_per_workgroup_are_promoted_when_eight_rows_exceed_the_chip():
    assert plan(LARGE).rpw_sb == 16  # 2752 rows: 344 eight-row workgroups > 256 compute units
    assert plan(dataclasses.replace(LARGE, cutoffs=LIVE.cutoffs, ctr=LIVE.ctr, nbr=LIVE.nbr, ctr_fb=LIVE.ctr_fb, nbr_fb=LIVE.nbr_fb,
                                    df=LIVE.df)).rpw_sb == 0  # 832 rows: 104 workgroups
    assert plan(LARGE, B=47).rpw_sb == 0 and plan(LARGE, B=48).rpw_sb == 16  # 2021 rows: 253 workgroups; 2064 rows: 258
    assert plan(LARGE, n_cu=344).rpw_sb == 0
    assert plan(LARGE, rows_per_wg=(0, 8)).rpw_sb == 8 and plan(LARGE, fuse_input=False).rpw_sb == 0
    assert plan(dataclasses.replace(LARGE, shared=False)).rpw_sb == 0
    assert plan(dataclasses.replace(LARGE, sb_hidden=128)).rpw_sb == 0  # (the fused-input kernels start above 128)
    assert plan(LARGE).rpw_fb == 0


# Forced stack launches (stack_scan=True) on the overlapped schedule: both stacks side by side must fit the chip.  Workgroups of a
# stack as the check counts them, nl = 2: (2 * (scan + 7)) // 8 * 8 + (proj + 7) // 8 * 8, scan = sum ceil(R / rp) with rp = 4 (full
# band) / 8 (sub-band), proj = sum ceil(R / 16) for the full-band stack (H > 256) and for a wide sub-band stack, else 0.
#   B = 48, wide: fb scan 12, proj 3 -> 38 // 8 * 8 + 10 // 8 * 8 = 32 + 8 = 40; sb rows 384 / 144 / 96: scan 48 + 18 + 12 = 78,
#       proj 24 + 9 + 6 = 39 -> 170 // 8 * 8 + 46 // 8 * 8 = 168 + 40 = 208; together 248 <= 256
#   B = 49, wide: fb scan 13, proj 4 -> 40 + 8 = 48; sb rows 392 / 147 / 98: scan 49 + 19 + 13 = 81, proj 25 + 10 + 7 = 42
#       -> 176 + 48 = 224; together 272 > 256
#   B = 60, narrow: fb scan 15, proj 4 -> 44 // 8 * 8 + 8 = 48; sb rows 480 / 180 / 120: scan 60 + 23 + 15 = 98 -> 210 // 8 * 8 = 208,
#       proj 0 -> 0; together 256 <= 256
#   B = 64, narrow: fb scan 16, proj 4 -> 46 // 8 * 8 + 8 = 48; sb scan 64 + 24 + 16 = 104 -> 222 // 8 * 8 = 216; together 264 > 256
@pytest.mark.parametrize("B,wide,n_cu,overlap", [(48, True, 256, True), (49, True, 256, False), (48, True, 247, False), (49, True, 272, True),
                                                 (60, False, 256, True), (64, False, 256, False), (64, False, 264, True)])
def test_forced_stacks_overlap_only_where_both_fit_the_chip(B, wide, n_cu, overlap):
    p = plan(B=B, n_cu=n_cu, stack_scan=True, stack_wide=wide, stack_rows_per_wg={"fb": 4, "sb": 8})
    assert p.overlap == overlap and p.staged == overlap
    assert list(p.bounds) == ([(0, 240), (240, 380), (620, 380)] if overlap else [(0, 1000)])  # (624 rows and more: the 0.24 T lead-in)
    # the rule "auto" and stacks that are not both forced never get to the check
    assert plan(B=B, n_cu=n_cu, stack_scan="auto", stack_wide=wide).overlap
    assert plan(B=B, n_cu=n_cu, stack_scan=False, stack_wide=wide).overlap
    assert plan(dataclasses.replace(LIVE, shared=False), B=B, n_cu=n_cu, stack_scan=True, stack_wide=wide).overlap
    assert plan(B=B, n_cu=n_cu, stack_scan=True, stack_wide=wide, want_membrane=True).overlap


def test_forced_stack_rows_per_workgroup_enter_the_check():
    # B = 64, narrow, 16 rows per sub-band workgroup: sb scan 32 + 12 + 8 = 52 -> 118 // 8 * 8 = 112; with the full band's 48: 160
    assert plan(stack_scan=True, stack_wide=False, stack_rows_per_wg={"fb": 4, "sb": 16}).overlap
    assert not plan(stack_scan=True, stack_wide=False).overlap  # (a fresh engine's 4 / 8 rows: 264 workgroups)


# ---- the stack rule ----------------------------------------------------------------------------------------------------------------
RS = [512, 192, 128]  # the sub-band rows of baseline_m at B = 64


def rule(H=224, Rs=RS, n_groups=None, shared=True, nl=2, want_membrane=False, stack_scan="auto", stack_wide=True, fb_auto=4, pair_scan=True,
         rows_per_wg=(0, 0), alone=True, n_cu=N_CU):
    return stack_rule(shared, nl, H, len(Rs) if n_groups is None else n_groups, Rs, want_membrane, stack_scan, stack_wide, fb_auto, pair_scan,
                      rows_per_wg, alone, n_cu)


def test_stack_rule_full_band():
    assert rule(H=320, Rs=[64]) == (True, False, 4)  # 16 workgroups per layer * 2 + 4 PROJ workgroups = 36 <= 256
    assert rule(H=320, Rs=[64], n_cu=35) == (False, False, 4)
    assert rule(H=320, Rs=[64], alone=False, rows_per_wg=(16, 16)) == (True, False, 4)  # (neither is the full-band stack's business)


def test_stack_rule_sub_band_pair_launch_needs_the_chip_to_itself():
    assert rule() == (True, False, 8)  # 2 * (64 + 24 + 16) = 208 workgroups <= 256 - 40
    assert rule(rows_per_wg=(0, 8)) == (True, False, 8)
    # 832 rows: neither <= 256 nor <= 512 -- without the pair launch the per-layer scans
    assert rule(alone=False) == (False, False, 0)
    assert rule(rows_per_wg=(16, 16)) == (False, False, 0)
    assert rule(pair_scan=False) == (False, False, 0)
    assert rule(H=256) == (False, False, 0)
    assert rule(n_cu=247) == (False, False, 0)  # 208 > 247 - 40


def test_stack_rule_sub_band_without_the_pair_launch():
    assert rule(Rs=[128, 48, 32], pair_scan=False) == (True, True, 8)   # 208 rows <= 256: the wide flavour
    assert rule(Rs=[256, 96, 64], pair_scan=False) == (True, False, 8)  # 416 rows <= 512: narrow
    assert rule(Rs=[128, 48, 32], alone=False) == (True, True, 8)
    assert rule(Rs=[316, 116, 81], pair_scan=False) == (False, False, 0)  # 513 rows


def test_stack_rule_where_there_is_no_stack_launch():
    for kw in (dict(want_membrane=True), dict(shared=False), dict(stack_scan=False), dict(nl=1), dict(n_groups=9)):  # 9 * 3 roles > 24
        assert rule(**kw) == (False, False, 0)
    for kw in (dict(want_membrane=True), dict(shared=False), dict(stack_scan=False), dict(nl=1)):
        assert rule(H=320, Rs=[64], **kw) == (False, False, 0)


def test_stack_rule_forced():
    assert rule(stack_scan=True) == (True, True, None)  # (rows per workgroup: the engine's stack_rows_per_wg)
    assert rule(stack_scan=True, stack_wide=False, alone=False, rows_per_wg=(16, 16)) == (True, False, None)
    assert rule(stack_scan=True, want_membrane=True) == (False, False, 0)
