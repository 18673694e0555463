"""The 16-row IO-wave scans (sfsn_scan3j_dev.h: scan3j_role, both forms, and scan3y_role) at the smallest shapes that reach every form of
the compute waves' step loop, written with the experiment of profiles/scan_cell_unpacked.md (the cell without packed fp32; measured and
not kept) and kept for what did change there: scan3y_role's store split between its loader and its storer wave (SFSN_S3Y_LSPLIT).
Through the C ABI, for exact equality (fp32 and int8 spikes, final h / c, spike counts):

  sfsn_gsn_layer_scan_fused / _fused_x   against round 2's bodies (SFSN_FUSED_V2=1, read on every call) and against the two-call forms
                                         (sfsn_spike_proj / sfsn_input_proj_f32 + sfsn_gsn_layer_scan); with fp32 spikes and counts only
                                         (at H = 224 the OFF form), and both forms forced in both output sets (SFSN_S3J_OFF = 0 / 2)
  sfsn_gsn_layer_scan_l0 (+ _fused)      against round 2's bodies group by group
  sfsn_gsn_layer_scan_l01 at lag 4       against sfsn_gsn_layer_scan_l0 + sfsn_gsn_layer_scan_fused
  sfsn_gsn_layer_scan_l01_projdf         against sfsn_gsn_layer_scan_l01 + sfsn_proj_deepfilter (coefficient rows, spectrum, magnitude too)

The gated launches run twice on one scratch buffer, and the helpers assert after each that the error word and every hand-off counter
are 0.  Shapes: H = 224 (KS = 4 with the 32-wide tail step), 192 (KS = 3, none), 144 (KS = 3 with it); one full 16-row block, and two
blocks with the last one's rows partly beyond R for the fused role; T = 1 (the odd-T copy of the step alone), 2 (one loop trip), 3
(a trip and the odd step), 7; I = 38 (two bf16 k-chunks) and 30 (one).  Two cases of tests/scanref.py leave the mild regime:
`threshold` with its tiny shifts moved to the smallest subnormals (y on +-0.0 and on the values next to it: the `>= 0` edge) and
`tails` (|pre_f| up to ~120: exp2 overflows to inf and underflows to 0)."""
import numpy as np
import pytest

import scanref as sr
import test_l01_epilogue_one_launch as epi
import test_layers01_one_launch as l01
from test_hip_parity import _run_fused, _run_fused_x, make_layer, run_scan
from test_stack_scan import _input_proj, _spike_proj

pytestmark = pytest.mark.gpu

TS = (1, 2, 3, 7)
TMAX = max(TS)
NAMES = ("fp32 spikes", "int8 spikes", "h", "c", "count")


@pytest.fixture(scope="module")
def hip():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    assert L.sfsn_device_count() >= 1
    return L


def _same(new, old, tag, upto=5):
    for a, b, nm in list(zip(new, old, NAMES))[:upto]:
        if a is None or b is None:
            assert a is None and b is None, f"{tag}: {nm}"
        else:
            np.testing.assert_array_equal(a, b, err_msg=f"{tag}: {nm}")


def _pad(s_in, H):
    T, R, _ = s_in.shape
    out = np.zeros((T, R, (H + 63) // 64 * 64), np.int8)
    out[:, :, :H] = s_in
    return out


def _check_role(hip, run, args_of, zin, sd, alpha, beta, h0, c0, H, tag, monkeypatch, off_forms):
    """One case at every T: the touched role in both output sets against round 2's body and the two-call form on the prefix."""
    seen = False
    for T in TS:
        args = args_of(T)
        new = (run(hip, *args), run(hip, *args, want_f32=False))
        monkeypatch.setenv("SFSN_FUSED_V2", "1")
        old = (run(hip, *args), run(hip, *args, want_f32=False))
        monkeypatch.delenv("SFSN_FUSED_V2")
        _same(new[0], old[0], f"{tag} T={T} with fp32 spikes against round 2's body")
        _same(new[1], old[1], f"{tag} T={T} counts only against round 2's body")
        assert new[1][0] is None and new[1][4] == int(new[0][0].sum()), f"{tag} T={T}: the count is not the number of spikes written"
        spk, _, s8, hT, cT = run_scan(hip, zin[:T], sd["weight_hh"], sd["bias_ih"], alpha, beta, True, h0, c0, want_mem=False)
        _same(new[0], (spk, s8, hT, cT), f"{tag} T={T} against the two-call form", upto=4)
        assert not new[0][1][:, :, H:].any(), f"{tag} T={T}: padding columns"
        if off_forms:  # H = 224: the plain form without fp32 spikes and the OFF form with them
            for mode, f32 in (("0", False), ("2", True)):
                monkeypatch.setenv("SFSN_S3J_OFF", mode)
                _same(run(hip, *args, want_f32=f32), new[0 if f32 else 1], f"{tag} T={T} SFSN_S3J_OFF={mode} fp32 spikes {f32}")
                monkeypatch.delenv("SFSN_S3J_OFF")
        seen = seen or bool(new[0][1].any())
    return seen


@pytest.mark.parametrize("R", [16, 27])  # one full block; two blocks, the last one's rows 11 .. 15 beyond R
@pytest.mark.parametrize("H", [224, 192, 144])
def test_fused_scan(hip, H, R, monkeypatch):
    rng = np.random.default_rng(31 * H + R)
    sd, alpha, beta, _ = make_layer(rng, H, H, True, True)
    s_in = _pad(rng.random((TMAX, R, H)) < 0.25, H)
    h0 = (rng.random((R, H)) > 0.5).astype(np.float32)
    c0 = rng.standard_normal((R, H)).astype(np.float32)
    zin = _spike_proj(hip, s_in, sd["weight_ih"], H)
    assert _check_role(hip, _run_fused, lambda T: (s_in[:T], sd, alpha, beta, h0, c0), zin, sd, alpha, beta, h0, c0, H, f"fused H={H} R={R}",
                       monkeypatch, off_forms=H == 224)


@pytest.mark.parametrize("R", [16, 32])
@pytest.mark.parametrize("I", [38, 30])
@pytest.mark.parametrize("H", [224, 192, 144])
def test_fused_x_scan(hip, H, I, R, monkeypatch):
    rng = np.random.default_rng(1000 * I + 31 * H + R)
    sd, alpha, beta, _ = make_layer(rng, I, H, True, True)
    x = rng.standard_normal((TMAX, R, I)).astype(np.float32)
    h0 = (rng.random((R, H)) > 0.5).astype(np.float32)
    c0 = rng.standard_normal((R, H)).astype(np.float32)
    zin = _input_proj(hip, x, sd["weight_ih"])  # (T x R >= 64 rows: the bf16 form the role restates; a row's product does not depend on the others)
    assert _check_role(hip, _run_fused_x, lambda T: (x[:T], sd, alpha, beta, h0, c0), zin, sd, alpha, beta, h0, c0, H, f"fused_x H={H} I={I} R={R}",
                       monkeypatch, off_forms=False)


def _edge(name, H, kind):
    """tests/scanref.py's case at 7 frames of 27 rows (32 for the fused-x role), as test_scan_edges.py builds its launches' arguments."""
    p = sr.make_case(name, H, True, kind, I=38, R=32, T=TMAX)
    if name == "threshold":  # the tiny shifts become the smallest values either side of zero
        g2 = sr.threshold_groups(H)[1]
        p["beta"][g2] = np.where(np.arange(len(g2)) % 2 == 0, 1.0, -1.0).astype(np.float32) * np.float32(1.401298464324817e-45)
    return p


def _sd(p):
    return dict(weight_hh=p["W_hh"], weight_ih=p.get("W_ih"), bias_ih=p["bias"])


@pytest.mark.parametrize("name", ["threshold", "tails"])
@pytest.mark.parametrize("H", [224, 192])
def test_fused_scan_at_the_cell_s_edges(hip, H, name, monkeypatch):
    p = sr.crop(_edge(name, H, "spike"), TMAX, 27)
    s_in = _pad(p["s_in"], H)
    zin = _spike_proj(hip, s_in, p["W_ih"], H)
    _check_role(hip, _run_fused, lambda T: (s_in[:T], _sd(p), p["alpha"], p["beta"], p["h0"], p["c0"]), zin, _sd(p), p["alpha"], p["beta"],
                p["h0"], p["c0"], H, f"fused {name} H={H}", monkeypatch, off_forms=H == 224)
    _edge_was_met(hip, name, H, p, _run_fused(hip, s_in, _sd(p), p["alpha"], p["beta"], p["h0"], p["c0"]), zin)


@pytest.mark.parametrize("name", ["threshold", "tails"])
@pytest.mark.parametrize("H", [224, 192])
def test_fused_x_scan_at_the_cell_s_edges(hip, H, name, monkeypatch):
    p = _edge(name, H, "x")
    zin = _input_proj(hip, p["x"], p["W_ih"])
    _check_role(hip, _run_fused_x, lambda T: (p["x"][:T], _sd(p), p["alpha"], p["beta"], p["h0"], p["c0"]), zin, _sd(p), p["alpha"], p["beta"],
                p["h0"], p["c0"], H, f"fused_x {name} H={H}", monkeypatch, off_forms=False)
    _edge_was_met(hip, name, H, p, _run_fused_x(hip, p["x"], _sd(p), p["alpha"], p["beta"], p["h0"], p["c0"]), zin)


def _edge_was_met(hip, name, H, p, got, zin):
    """The case did reach the edge it is named for (else it would tell nothing about it)."""
    spk = got[0]
    if name == "threshold":
        g1, g2, g3 = sr.threshold_groups(H)
        assert spk[:, :, g1].all() and spk[:, :, g3].all(), "y = +-0.0 must spike"
        assert spk[:, :, g2[::2]].all() and not spk[:, :, g2[1::2]].any(), "the smallest values either side of zero"
    else:
        pre = zin[0] + p["bias"][:H]  # frame 0's forget-gate input without the recurrent term (|rec| is a few units)
        # exp2(-pre_f log2 e): inf above 2^128 (pre_f < -88.8), 0 below 2^-149 (pre_f > 103.3)
        assert (pre > 106).any() and (pre < -92).any(), "exp2 neither underflows to 0 nor overflows to inf in this case"
        assert np.isfinite(got[3]).all()


# a fused-x group of one block (I = 38) and one of two blocks (I = 30), an input-term group whose second block is half full; 8 clips
FX, ZS, B = [(38, 16), (30, 32)], [24], 8


@pytest.mark.parametrize("H", [224, 192, 144])
def test_l0_l01_and_the_epilogue_launch(hip, H, monkeypatch):
    gx, gz = l01._case(52000 + H, H, FX, ZS)
    scratch = l01._scratch(hip, gx, gz)
    seen = False
    for T in TS:
        for f32 in (True, False):
            tag = f"H={H} T={T} fp32 spikes {f32}"
            monkeypatch.setenv("SFSN_FUSED_V2", "1")
            old = l01._run(hip, gx, [], False, f32, [0, T]) + l01._run(hip, [], gz, False, f32, [0, T])  # round 2's bodies, group by group
            monkeypatch.delenv("SFSN_FUSED_V2")
            per_layer = l01._run(hip, gx, gz, False, f32, [0, T])  # sfsn_gsn_layer_scan_l0 + sfsn_gsn_layer_scan_fused
            l01._same(per_layer, old, f"{tag}: l0 + fused against round 2's bodies")
            for rep in range(2):
                pair = l01._run(hip, gx, gz, True, f32, [0, T], lag=4, scratch=scratch)
                l01._same(pair, per_layer, f"{tag}: l01 run {rep} against l0 + fused")
            two = epi._run(hip, gx, gz, B, 1, False, f32, [0, T], ("cell", H), lag=4, scratch=scratch)
            for rep in range(2):
                one = epi._run(hip, gx, gz, B, 1, True, f32, [0, T], ("cell", H), lag=4, scratch=scratch)
                epi._same(one, two, f"{tag}: l01_projdf run {rep} against l01 + proj_deepfilter")
            for k, r in enumerate(pair):  # the epilogue launch's layers are the pair launch's
                np.testing.assert_array_equal(one[f"group {k} layer 1 s8"], r[6], err_msg=f"{tag}: group {k}")
                np.testing.assert_array_equal(one[f"group {k} layer 1 c"], r[8], err_msg=f"{tag}: group {k}")
            seen = seen or all(r[1].any() and r[6].any() for r in pair)
    assert seen, "the case cannot tell a launch that writes nothing"
