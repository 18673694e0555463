"""sfsn_gsn_layer_scan_l0 without a GPU: what it answers to bad arguments, before any launch.  For every case whose fault lies in one
of the two lists the answer equals that of the list's own entry point (sfsn_gsn_layer_scan_fused_x, sfsn_gsn_layer_scan at 16 rows per
workgroup) for the same list; what only the pair can get wrong (output sets that differ, an empty list, too many segments together)
is SFSN_EUNSUPPORTED: the caller makes the two calls.  EVERY call in this file is refused by an argument check -- none reaches a
launch (the pointers are host addresses)."""
import ctypes

import pytest

from spiking_fullsubnet_amd import _lib
from spiking_fullsubnet_amd._lib import SFSN_EINVAL, SFSN_EUNSUPPORTED, FusedX, ScanSegment

_BUF = ctypes.create_string_buffer(1 << 16)
_BASE = (ctypes.addressof(_BUF) + 255) & ~255


def _a(k, off=0):
    """A 16-byte aligned host address (slot k), plus `off` bytes."""
    return _BASE + 256 * k + off


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _lists(n_x=1, n_z=1, f32=True, R_x=32, R_z=24, I=38):
    sx, sz, fin = (ScanSegment * max(n_x, 1))(), (ScanSegment * max(n_z, 1))(), (FusedX * max(n_x, 1))()
    for k, s in enumerate(list(sx) + list(sz)):
        s.w_hh, s.w_dq, s.bias, s.bn_alpha, s.bn_beta, s.h_state, s.c_state = (_a(20 * k + j) for j in range(7))
        s.spikes_i8, s.spikes_f32, s.membrane, s.spike_count = _a(20 * k + 7), _a(20 * k + 8) if f32 else None, None, None
    for s, f in zip(sx, fin):
        s.zin, s.R = None, R_x
        f.x, f.w_ih, f.I = _a(200), _a(201), I
    for s in sz:
        s.zin, s.R = _a(202), R_z
    return sx, fin, sz


def _l0(L, sx, fin, sz, n_x=1, n_z=1, T=4, H=224, shared=1):
    return L.sfsn_gsn_layer_scan_l0(sx, fin, n_x, sz, n_z, T, H, shared, None)


def test_the_entry_point_is_exported_and_declared():
    assert "sfsn_gsn_layer_scan_l0" in _lib.EXPORTS and hasattr(_lib.lib(), "sfsn_gsn_layer_scan_l0")


def _break_x(name):
    """A pair of lists whose fused-x list has the named fault, and the entry point's own answer to it."""
    sx, fin, sz = _lists()
    H = 224
    if name == "null w_hh":
        sx[0].w_hh = None
    elif name == "null x":
        fin[0].x = None
    elif name == "null fused-x weights":
        fin[0].w_ih = None
    elif name == "null int8 spikes":
        sx[0].spikes_i8 = None
    elif name == "misaligned x":
        fin[0].x = _a(200, 4)
    elif name == "misaligned h":
        sx[0].h_state = _a(5, 8)
    elif name == "odd I":
        fin[0].I = 37
    elif name == "odd I and misaligned x":  # (SFSN_EUNSUPPORTED answers before the alignment checks)
        fin[0].I, fin[0].x = 37, _a(200, 4)
    elif name == "I > 64":
        fin[0].I = 66
    elif name == "I = 0":
        fin[0].I = 0
    elif name == "R % 16 != 0":
        sx[0].R = 24
    elif name == "R = 0":
        sx[0].R = 0
    elif name == "membrane on the fused-x side":
        sx[0].membrane = _a(9)
    elif name == "H = 320":
        H = 320
    elif name == "H = 128":
        H = 128
    elif name == "H = 200":
        H = 200
    else:
        raise KeyError(name)
    return sx, fin, sz, H


X_FAULTS = {"null w_hh": SFSN_EINVAL, "null x": SFSN_EINVAL, "null fused-x weights": SFSN_EINVAL, "null int8 spikes": SFSN_EINVAL,
            "misaligned x": SFSN_EINVAL, "misaligned h": SFSN_EINVAL, "odd I": SFSN_EUNSUPPORTED, "odd I and misaligned x": SFSN_EUNSUPPORTED,
            "I > 64": SFSN_EUNSUPPORTED, "I = 0": SFSN_EUNSUPPORTED, "R % 16 != 0": SFSN_EUNSUPPORTED, "R = 0": SFSN_EINVAL,
            "membrane on the fused-x side": SFSN_EINVAL, "H = 320": SFSN_EUNSUPPORTED, "H = 128": SFSN_EUNSUPPORTED, "H = 200": SFSN_EUNSUPPORTED}


@pytest.mark.parametrize("name", list(X_FAULTS))
def test_a_fault_in_the_fused_x_list_gets_that_entry_points_answer(L, name):
    sx, fin, sz, H = _break_x(name)
    own = L.sfsn_gsn_layer_scan_fused_x(sx, fin, 1, 4, H, None)
    assert own == X_FAULTS[name]  # (refused: nothing was launched)
    assert _l0(L, sx, fin, sz, H=H) == own


def _break_z(name):
    sx, fin, sz = _lists()
    if name == "null zin":
        sz[0].zin = None
    elif name == "null bias":
        sz[0].bias = None
    elif name == "misaligned zin":
        sz[0].zin = _a(202, 8)
    elif name == "misaligned fp32 spikes":
        sz[0].spikes_f32 = _a(8, 4)
    elif name == "R = 0":
        sz[0].R = 0
    elif name == "membrane without fp32 spikes":
        sz[0].spikes_f32, sz[0].membrane = None, _a(9)
    else:
        raise KeyError(name)
    return sx, fin, sz


Z_FAULTS = {"null zin": SFSN_EINVAL, "null bias": SFSN_EINVAL, "misaligned zin": SFSN_EINVAL, "misaligned fp32 spikes": SFSN_EINVAL,
            "R = 0": SFSN_EINVAL, "membrane without fp32 spikes": SFSN_EUNSUPPORTED}


@pytest.mark.parametrize("name", list(Z_FAULTS))
def test_a_fault_in_the_input_term_list_gets_that_entry_points_answer(L, name):
    sx, fin, sz = _break_z(name)
    own = L.sfsn_gsn_layer_scan(sz, 1, 4, 224, 1, 16, None)
    assert own == Z_FAULTS[name]  # (refused: nothing was launched)
    assert _l0(L, sx, fin, sz) == own


def test_null_lists_and_bad_counts(L):
    sx, fin, sz = _lists()
    assert L.sfsn_gsn_layer_scan_fused_x(None, fin, 1, 4, 224, None) == SFSN_EINVAL == _l0(L, None, fin, sz)
    assert L.sfsn_gsn_layer_scan_fused_x(sx, None, 1, 4, 224, None) == SFSN_EINVAL == _l0(L, sx, None, sz)
    assert L.sfsn_gsn_layer_scan(None, 1, 4, 224, 1, 16, None) == SFSN_EINVAL == _l0(L, sx, fin, None)
    assert L.sfsn_gsn_layer_scan_fused_x(sx, fin, -1, 4, 224, None) == SFSN_EINVAL == _l0(L, sx, fin, sz, n_x=-1)
    assert L.sfsn_gsn_layer_scan(sz, -1, 4, 224, 1, 16, None) == SFSN_EINVAL == _l0(L, sx, fin, sz, n_z=-1)
    assert L.sfsn_gsn_layer_scan_fused_x(sx, fin, 9, 4, 224, None) == SFSN_EINVAL == _l0(L, sx, fin, sz, n_x=9)
    assert L.sfsn_gsn_layer_scan_fused_x(sx, fin, 1, -1, 224, None) == SFSN_EINVAL == _l0(L, sx, fin, sz, T=-1)
    assert L.sfsn_gsn_layer_scan_fused_x(sx, fin, 1, 4, 0, None) == SFSN_EINVAL == _l0(L, sx, fin, sz, H=0)


def test_what_only_the_pair_can_get_wrong_is_unsupported(L, monkeypatch):
    """(each list alone is one its own entry point would launch: those are not called here)"""
    sx, fin, sz = _lists()
    assert _l0(L, sx, fin, sz, n_x=0) == SFSN_EUNSUPPORTED and _l0(L, sx, fin, sz, n_z=0) == SFSN_EUNSUPPORTED  # an empty list
    assert _l0(L, sx, fin, sz, shared=0) == SFSN_EUNSUPPORTED  # separate gate weights
    assert _l0(L, sx, fin, sz, H=240) == SFSN_EUNSUPPORTED  # 15 tiles: the fused-x list would take round 2's 512-thread body
    sz[0].spikes_f32 = None  # output sets that differ: fp32 spikes on the fused-x side only ...
    assert _l0(L, sx, fin, sz) == SFSN_EUNSUPPORTED
    sx, fin, sz = _lists(f32=False)
    sz[0].spikes_f32 = _a(150)  # ... and on the other side only
    assert _l0(L, sx, fin, sz) == SFSN_EUNSUPPORTED
    sx, fin, sz = _lists()
    sz[0].membrane = _a(151)  # a membrane output (with the fp32 spikes it needs)
    assert _l0(L, sx, fin, sz) == SFSN_EUNSUPPORTED
    sx, fin, sz = _lists(n_x=5, n_z=5)  # more than SFSN_MAX_SEGMENTS together
    assert _lib.MAX_SEGMENTS == 8 and _l0(L, sx, fin, sz, n_x=5, n_z=5) == SFSN_EUNSUPPORTED
    sx, fin, sz = _lists()
    for var in ("SFSN_SCAN_V2", "SFSN_FUSED_V2"):  # round 2's bodies asked for: read on every call
        monkeypatch.setenv(var, "1")
        assert _l0(L, sx, fin, sz) == SFSN_EUNSUPPORTED
        monkeypatch.delenv(var)
