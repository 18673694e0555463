"""Every scan family through the C ABI against tests/scanref.py's fp64 reference and derived bound, on the case table that leaves the
mild regime (saturated integer sums, corner digits, sigmoid tails, row scales over 106 binades, exact-zero membranes, BatchNorm scales of
either sign).  test_scanref_host.py validates reference, bound and cases on the CPU; this file only runs kernels.

Which arguments select which kernel (read from layer_scan_impl, sfsn_gsn_layer_scan_fused* in sfsn_kernels.hip and stack_scan_impl in
sfsn_stack.hip; out = 2 | fp32 spikes | 4 membrane):
  sfsn_gsn_layer_scan     separate gates and H > 256                                   -> gsn_scan_stream_kernel            ("stream")
                          shared, H <= 224, rows_per_wg 4 / 8, no membrane             -> gsn_scan3_kernel                  ("scan3")
                          separate, H <= 224, rows_per_wg 4, no membrane               -> gsn_scan3g_kernel                 ("scan3g")
                          anything else: a membrane output, 16 rows, H > 224           -> gsn_scan_kernel, round 2's body   ("scan_kernel";
                                                                                          rows_per_wg 4: its repacked epilogue; H = 320: KS = 5)
  sfsn_gsn_layer_scan_w16 what scan3 covers, weights packed with 16 bits               -> two-plane gsn_scan3_kernel        ("scan3_w16")
  sfsn_gsn_layer_scan_split  separate, H > 256                                          -> gsn_scan_split_kernel             ("split")
  sfsn_gsn_layer_scan_fused  H <= 224 -> gsn_scan_fused3_kernel (scan3j role; H = 224 without fp32 spikes, or SFSN_S3J_OFF=2: its OFF
                          form); H = 256 -> gsn_scan_fused_kernel (round 2's fused body, the integer form at K = 256)
  sfsn_gsn_layer_scan_fused_x  H <= 224 -> gsn_scan_fusedx3_kernel; H = 256 -> gsn_scan_fusedx_kernel
  sfsn_gsn_stack_scan     H <= 256, layers >= 1 with an input-term buffer ("wide")     -> gsn_stack_wide_kernel, 16-wave scans + PROJ roles
                          H <= 224, no buffer, 8 rows ("narrow")                        -> gsn_stack_wide_kernel, FUSED3 roles (scan3i)
                          H = 256, no buffer ("narrow")                                 -> gsn_stack_kernel, 8-wave fused-input roles
                          H = 320, 8 rows                                               -> gsn_stack_fb_kernel (scan3w); SFSN_STACK_FB3=0:
                                                                                          gsn_stack_kernel, round 2's bodies
  sfsn_gsn_stack_scan_x   H <= 224, 8 rows, no buffer, x given                          -> FUSEDX3 role (scan3x) + FUSED3 role

Per launch (scanref.compare's rule): spikes; membranes where the entry point has them; final c within the propagated bound on the rows that
did not diverge; final h = the last spikes; int8 spikes = fp32 spikes; padding columns zero; without the fp32 tensor the launch's counter =
the number of spikes; outputs start as NaN / 0x7f.  Per test: at most 2 % of the elements left unasserted.  Every test prints its worst
error / tolerance (profiles/scan_edges.md keeps the first run's figures).  Launches go one at a time on the default stream."""
import numpy as np
import pytest

import scanref as sr
from test_hip_parity import _run_fused, _run_fused_x, run_scan
from test_stack_scan import run_stack

pytestmark = pytest.mark.gpu

TS = (1, 2, 9)      # 9: odd and longer than the ring's lead of 6
RS = (5, 16, 37)    # a ragged block, one full block, three blocks with a ragged last
RS16 = (16, 48)     # where the entry point wants whole blocks
NAMES = list(sr.CASES)
_refs = {}


@pytest.fixture(scope="module")
def hip():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    assert L.sfsn_device_count() >= 1
    return L


def _ref(name, H, shared, kind, I=38, bits=24):
    """The full-size case (48 rows, 9 frames) and its reference, computed once; every launch uses a prefix of it."""
    key = (name, H, shared, kind, I, bits)
    if key not in _refs:
        p = sr.make_case(name, H, shared, kind, I, bits)
        _refs[key] = (p, sr.layer(p))
    return _refs[key]


class Tally:
    """Worst ratios and the unasserted share over the launches of one test."""

    def __init__(self, tag):
        self.tag, self.ratio, self.n, self.open, self.spikes = tag, 0.0, 0, 0.0, 0

    def check(self, ref, H, spk, s8, hT, cT, mem=None, t_up=None, where=""):
        tag = f"{self.tag} {where}"
        assert np.isin(spk, (0.0, 1.0)).all(), f"{tag}: fp32 spikes are not all 0 / 1 (a canary left?)"
        res = sr.compare(spk, ref, mem, t_up)
        assert res.ok, f"{tag}: {res.why}"
        np.testing.assert_array_equal(s8[:, :, :H], spk.astype(np.int8), err_msg=f"{tag}: int8 spikes")
        assert not s8[:, :, H:].any(), f"{tag}: padding columns"
        np.testing.assert_array_equal(hT, spk[-1], err_msg=f"{tag}: final h")
        fr = sr.final_ratio(cT, ref, res.t_valid)
        assert fr <= 1.0, f"{tag}: final c {fr:.3g} x the tolerance"
        self.ratio = max(self.ratio, res.ratio, fr)
        self.n += spk.size
        self.open += res.unasserted * spk.size
        self.spikes += int(spk.sum())
        return res

    def done(self, expect_spikes=True):
        share = self.open / max(self.n, 1)
        print(f"SCAN_EDGES {self.tag}: worst error / tolerance {self.ratio:.3f}, unasserted {share:.5f}")
        assert share <= 0.02, f"{self.tag}: {share:.4f} of the elements unasserted"
        assert self.spikes > 0 or not expect_spikes


# family, H, shared, rows_per_wg values, membrane, bits, split
LAYER = ([("scan_kernel", H, True, (16, 4), True, 24, False) for H in (64, 224, 256, 320)]
         + [("scan_kernel", H, False, (16, 4), True, 24, False) for H in (128, 224)]
         + [("scan3", H, True, (4, 8), False, 24, False) for H in (160, 224)]
         + [("scan3_w16", H, True, (4, 8), False, 16, False) for H in (160, 224)]
         + [("scan3g", 224, False, (4,), False, 24, False), ("stream", 320, False, (0,), True, 24, False),
            ("split", 320, False, (0,), True, 24, True)])


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("family,H,shared,rpws,mem,bits,split", LAYER,
                         ids=[f"{c[0]}-H{c[1]}-{'shared' if c[2] else 'separate'}" for c in LAYER])
def test_layer_scan(hip, family, H, shared, rpws, mem, bits, split, name):
    full, ref = _ref(name, H, shared, "zin", bits=bits)
    tally = Tally(f"{family} H={H} {'shared' if shared else 'separate'} {name}")
    for R in RS:
        for T in TS:
            p, r = sr.crop(full, T, R), sr.prefix(ref, T, R)
            for rpw in rpws:
                kw = dict(split=split, rows_per_wg=rpw, bits=bits, zin_has_bias=True, canary=True)
                spk, m, s8, hT, cT = run_scan(hip, p["zin"], p["W_hh"], p["bias"], p["alpha"], p["beta"], shared, p["h0"], p["c0"], want_mem=mem, **kw)
                tally.check(r, H, spk, s8, hT, cT, m, where=f"R={R} T={T} rows_per_wg={rpw}")
                if not mem and not split:  # counts only: the same kernel without its fp32 stores
                    lean = run_scan(hip, p["zin"], p["W_hh"], p["bias"], p["alpha"], p["beta"], shared, p["h0"], p["c0"], want_mem=False, want_spk=False,
                                    count=True, **kw)
                    np.testing.assert_array_equal(lean[2], s8, err_msg="counts only: int8 spikes")
                    np.testing.assert_array_equal(lean[4], cT, err_msg="counts only: final c")
                    assert lean[5] == int(spk.sum()), "counts only: the counter is not the number of spikes"
    tally.done()


def _sd(p):
    return dict(weight_hh=p["W_hh"], weight_ih=p.get("W_ih"), bias_ih=p["bias"])


def _pad(s_in, H):
    T, R, _ = s_in.shape
    out = np.zeros((T, R, (H + 63) // 64 * 64), np.int8)
    out[:, :, :H] = s_in
    return out


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("H,off", [(224, None), (224, "2"), (256, None)], ids=["scan3j-H224", "scan3j_off-H224", "fused_v2-H256"])
def test_fused_scan(hip, H, off, name, monkeypatch):
    full, ref = _ref(name, H, True, "spike")
    if off is not None:
        monkeypatch.setenv("SFSN_S3J_OFF", off)
    tally = Tally(f"fused{'' if off is None else ' S3J_OFF=' + off} H={H} {name}")
    for R in RS:
        for T in TS:
            p, r = sr.crop(full, T, R), sr.prefix(ref, T, R)
            args = (hip, _pad(p["s_in"], H), _sd(p), p["alpha"], p["beta"], p["h0"], p["c0"])
            spk, s8, hT, cT, _ = _run_fused(*args, canary=True)
            tally.check(r, H, spk, s8, hT, cT, where=f"R={R} T={T}")
            lean = _run_fused(*args, want_f32=False, canary=True)
            np.testing.assert_array_equal(lean[1], s8, err_msg="counts only: int8 spikes")
            np.testing.assert_array_equal(lean[3], cT, err_msg="counts only: final c")
            assert lean[0] is None and lean[4] == int(spk.sum()), "counts only: the counter is not the number of spikes"
    tally.done()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("I", [38, 64])
@pytest.mark.parametrize("H", [224, 256], ids=["scan3y-H224", "fusedx_v2-H256"])
def test_fused_x_scan(hip, H, I, name):
    full, ref = _ref(name, H, True, "x", I=I)
    tally = Tally(f"fused_x H={H} I={I} {name}")
    for R in RS16:
        for T in TS:
            p, r = sr.crop(full, T, R), sr.prefix(ref, T, R)
            args = (hip, p["x"], _sd(p), p["alpha"], p["beta"], p["h0"], p["c0"])
            spk, s8, hT, cT, _ = _run_fused_x(*args, canary=True)
            tally.check(r, H, spk, s8, hT, cT, where=f"R={R} T={T}")
            lean = _run_fused_x(*args, want_f32=False, canary=True)
            np.testing.assert_array_equal(lean[1], s8, err_msg="counts only: int8 spikes")
            np.testing.assert_array_equal(lean[3], cT, err_msg="counts only: final c")
            assert lean[0] is None and lean[4] == int(spk.sum()), "counts only: the counter is not the number of spikes"
    tally.done()


# flavour, H, run_stack's `wide`, SFSN_STACK_FB3, layer 0 from x
STACK = [("wide", 224, True, None, False), ("narrow_scan3i", 224, False, None, False), ("wide", 256, True, None, False),
         ("narrow_fused8", 256, False, None, False), ("scan3w", 320, True, None, False), ("fb_round2", 320, True, "0", False),
         ("x_scan3x", 224, False, None, True)]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("flavour,H,wide,fb3,from_x", STACK, ids=[f"{c[0]}-H{c[1]}" for c in STACK])
def test_stack_scan(hip, flavour, H, wide, fb3, from_x, name, monkeypatch):
    """Two layers in one launch.  Layer 1's reference runs on the REFERENCE's layer-0 spikes and is asserted, row by row, for the frames
    in which the kernel's layer 0 agreed with them (compare's t_up)."""
    full0, ref0 = _ref(name, H, True, "x" if from_x else "zin")
    key = (name, H, "layer1", from_x)
    if key not in _refs:
        p1 = sr.next_layer(full0, ref0, name)
        _refs[key] = (p1, sr.layer(p1))
    full1, ref1 = _refs[key]
    if fb3 is not None:
        monkeypatch.setenv("SFSN_STACK_FB3", fb3)
    tallies = [Tally(f"stack {flavour} H={H} layer {l} {name}") for l in range(2)]
    for R in (RS16 if from_x else RS):
        for T in TS:
            p0, p1 = sr.crop(full0, T, R), sr.crop(full1, T, R)
            cells = [(_sd(p0), p0["alpha"], p0["beta"], None), (_sd(p1), p1["alpha"], p1["beta"], None)]
            zin0 = [np.zeros((T, R, H), np.float32) if from_x else p0["zin"]]
            got = run_stack(hip, zin0, cells, T, H, 8, h0=[[p0["h0"]], [p1["h0"]]], c0=[[p0["c0"]], [p1["c0"]]], wide=wide,
                            xs=[p0["x"]] if from_x else None, zin_has_bias=True, canary=True)
            t_up = None
            for l, r in enumerate((sr.prefix(ref0, T, R), sr.prefix(ref1, T, R))):
                spk, s8, hT, cT = got[l][0]
                t_up = tallies[l].check(r, H, spk, s8, hT, cT, t_up=t_up, where=f"R={R} T={T}").t_valid
    for t in tallies:
        t.done()
