"""The stagger of the 16-row scan roles' compute waves (SFSN_S3J_STAGGER=<order mask>[,<priority mask>], sfsn_scan3j_dev.h): wave slots
in the order mask pass the step barrier before the input product of the next frame instead of behind it, slots in the priority mask run
at priority 1.  Neither changes an instruction's operands, so every setting must give setting 0's results bit for bit.  Through the C
ABI: sfsn_gsn_layer_scan_fused_x + sfsn_gsn_layer_scan_fused (a fused-x group alone), sfsn_gsn_layer_scan_l0 + sfsn_gsn_layer_scan_fused
(with an input-term group whose last block is ragged), sfsn_gsn_layer_scan_l01 and sfsn_gsn_layer_scan_l01_projdf; fp32 spikes, int8
rows, final h / c, spike counts, and for the epilogue launch the coefficient rows, the enhanced spectrum and its magnitude.  The gated
launches run twice in a row on one scratch buffer, and the helpers assert after every launch that the error word and every progress
counter are 0.  A setting whose two orders passed different numbers of barriers would hang instead of failing: both orders execute one
barrier per step by construction (one loop body, the barrier on either side of the product)."""
import pytest

import test_l01_epilogue_one_launch as epi
import test_layers01_one_launch as l01

pytestmark = pytest.mark.gpu

# 0: every slot's barrier behind the product, no priority; None: the built-in default (no variable set); every slot in head order;
# slots 1 and 3; slots 2 and 3 in head order with slots 0 and 1 at priority 1
SETTINGS = ("0", None, "15", "10", "12,3")
# the ring wraps at D = 7 (prologue A = 6 frames): below / at / above it, odd and even counts with two steps per trip, prologues longer
# than the clip, two wraps, many wraps
TS = (1, 2, 5, 6, 7, 8, 13, 14, 15, 64)
TS_COUNTS = (2, 7, 15, 64)  # ... without an fp32 spike tensor (the counting storer; at H = 224 the OFF form, which keeps setting 0's order)
TS_LAG0 = (8, 64)           # ... with the hand-off lag 0 beside the default 4
B = 8                       # clips of the epilogue launch: 2 and 3 units per clip
FX, ZS = [(38, 16)], [24]   # a fused-x group of one block (I = 38: two k-chunks), an input-term group with a ragged second block


@pytest.fixture(scope="module")
def hip():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    assert L.sfsn_device_count() >= 1
    return L


def _launches(hip, H, T, f32, lags, cuts=None):
    """Every launch of one (H, T, output mode) under the stagger setting of the environment, as {name: results}."""
    gx, gz = l01._case(9100 + H, H, FX, ZS)
    cuts = cuts or [0, T]
    out = {"fused_x + fused": l01._run(hip, gx, [], False, f32, cuts), "l0 + fused": l01._run(hip, gx, gz, False, f32, cuts)}
    scratch = l01._scratch(hip, gx, gz)
    for lag in lags:
        for rep in range(2):
            out[f"l01 lag {lag} run {rep}"] = l01._run(hip, gx, gz, True, f32, cuts, lag=lag, scratch=scratch)
            if len(cuts) == 2:
                out[f"l01_projdf lag {lag} run {rep}"] = epi._run(hip, gx, gz, B, 1, True, f32, cuts, ("stagger", H), lag=lag, scratch=scratch)
    return out


_REF = {}


def _ref(hip, H, T, f32, lags, monkeypatch):
    """Setting 0's results: computed once per case, shared by the settings, never written to."""
    key = (H, T, f32, lags)
    if key not in _REF:
        monkeypatch.setenv("SFSN_S3J_STAGGER", "0")
        _REF[key] = _launches(hip, H, T, f32, lags)
    return _REF[key]


def _set(monkeypatch, setting):
    if setting is None:
        monkeypatch.delenv("SFSN_S3J_STAGGER", raising=False)
    else:
        monkeypatch.setenv("SFSN_S3J_STAGGER", setting)


def _same(new, old, tag):
    assert new.keys() == old.keys()
    for name in new:
        if isinstance(new[name], dict):
            epi._same(new[name], old[name], f"{tag} {name}")
        else:
            l01._same(new[name], old[name], f"{tag} {name}")


@pytest.mark.parametrize("setting", SETTINGS[1:], ids=lambda s: "default" if s is None else s)
@pytest.mark.parametrize("H", [224, 192, 144])  # 14 tiles + a tail k-step; 12 tiles, none; 9 tiles: slot 2 holds one compute wave, slot 3 none
def test_every_setting_equals_setting_0(hip, H, setting, monkeypatch):
    wrote = False
    for T in TS:
        for f32 in ((True, False) if T in TS_COUNTS else (True,)):
            lags = (4, 0) if T in TS_LAG0 else (4,)
            old = _ref(hip, H, T, f32, lags, monkeypatch)
            _set(monkeypatch, setting)
            new = _launches(hip, H, T, f32, lags)
            _same(new, old, f"H={H} SFSN_S3J_STAGGER={setting} T={T} fp32 spikes {f32}:")
            wrote = wrote or all(r[1].any() and r[6].any() for r in new["fused_x + fused"])
    assert wrote, "the case cannot tell a launch that writes nothing"


@pytest.mark.parametrize("setting", SETTINGS[1:], ids=lambda s: "default" if s is None else s)
@pytest.mark.parametrize("H", [224, 192])
def test_carried_state_5_plus_6_frames_against_11(hip, H, setting, monkeypatch):
    old = _ref(hip, H, 11, True, (4,), monkeypatch)
    _set(monkeypatch, setting)
    new = _launches(hip, H, 11, True, (4,), cuts=[0, 5, 11])
    for name in new:
        l01._same(new[name], old[name], f"H={H} SFSN_S3J_STAGGER={setting} 5 + 6 frames against 11: {name}")


def test_masks_beyond_the_four_slots_and_mixed_masks(hip, monkeypatch):
    """Masks wider than the four slots are cut to them (hexadecimal is read too); order and priority on disjoint slots."""
    old = _ref(hip, 224, 15, True, (4,), monkeypatch)
    for setting in ("0x1ff,0x1ff", "5,10", "0"):
        _set(monkeypatch, setting)
        _same(_launches(hip, 224, 15, True, (4,)), old, f"SFSN_S3J_STAGGER={setting}")
