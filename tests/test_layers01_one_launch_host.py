"""sfsn_gsn_layer_scan_l01 without a GPU: what it answers to bad arguments, before any launch.  For every case whose fault lies in one
of the three lists the answer equals that of the list's own entry point (sfsn_gsn_layer_scan_fused_x, sfsn_gsn_layer_scan at 16 rows
per workgroup, sfsn_gsn_layer_scan_fused) for the same list; what only the three together can get wrong is SFSN_EINVAL (layer 1 does
not read layer 0's int8 buffer, row counts differ, scratch too small) or SFSN_EUNSUPPORTED (output sets that differ, too many
segments: the caller makes the per-layer calls).  EVERY call in this file is refused by an argument check -- none reaches a launch
(the pointers are host addresses)."""
import ctypes

import pytest

from spiking_fullsubnet_amd import _lib
from spiking_fullsubnet_amd._lib import SFSN_EINVAL, SFSN_EUNSUPPORTED, FusedInput, FusedX, ScanSegment

_BUF = ctypes.create_string_buffer(1 << 17)
_BASE = (ctypes.addressof(_BUF) + 255) & ~255


def _a(k, off=0):
    """A 16-byte aligned host address (slot k), plus `off` bytes."""
    return _BASE + 256 * k + off


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _lists(n_x=1, n_z=1, f32=True, R_x=32, R_z=24, I=38):
    """The three lists of a call that would be launched: layer 1 reads layer 0's int8 buffers, segment for segment (x then z)."""
    sx, sz, fin = (ScanSegment * max(n_x, 1))(), (ScanSegment * max(n_z, 1))(), (FusedX * max(n_x, 1))()
    s1, fin1 = (ScanSegment * max(n_x + n_z, 1))(), (FusedInput * max(n_x + n_z, 1))()
    for k, s in enumerate(list(sx) + list(sz) + list(s1)):
        s.w_hh, s.w_dq, s.bias, s.bn_alpha, s.bn_beta, s.h_state, s.c_state = (_a(12 * k + j) for j in range(7))
        s.spikes_i8, s.spikes_f32, s.membrane, s.spike_count, s.zin = _a(12 * k + 7), _a(12 * k + 8) if f32 else None, None, None, None
    for s, f in zip(sx, fin):
        s.R = R_x
        f.x, f.w_ih, f.I = _a(400), _a(401), I
    for s in sz:
        s.zin, s.R = _a(402), R_z
    l0 = list(sx)[:n_x] + list(sz)[:n_z]
    for s, f, p in zip(s1, fin1, l0):
        s.R = p.R
        f.spikes_in, f.w_ih, f.w_ih_dq = p.spikes_i8, _a(403), _a(404)
    return sx, fin, sz, s1, fin1


def _l01(L, sx, fin, sz, s1, fin1, n_x=1, n_z=1, T=4, H=224, shared=1, lag=4, scratch=None, nbytes=None):
    rows = sum(s.R for s in list(sx)[:max(n_x, 0)]) + sum(s.R for s in list(sz)[:max(n_z, 0)])
    need = L.sfsn_stack_scratch_bytes(2, max(n_x + n_z, 1), max(rows, 1))
    return L.sfsn_gsn_layer_scan_l01(sx if n_x else None, fin if n_x else None, n_x, sz if n_z else None, n_z, s1, fin1, T, H, shared, lag,
                                     _a(450) if scratch is None else scratch, need if nbytes is None else nbytes, None)


def test_the_entry_point_is_exported_and_declared():
    assert "sfsn_gsn_layer_scan_l01" in _lib.EXPORTS and hasattr(_lib.lib(), "sfsn_gsn_layer_scan_l01")
    assert _lib.lib().sfsn_abi_version() == _lib.ABI_VERSION == 21  # (a new function alone does not bump it)


X_FAULTS = {"null w_hh": SFSN_EINVAL, "null x": SFSN_EINVAL, "misaligned x": SFSN_EINVAL, "misaligned h": SFSN_EINVAL,
            "odd I": SFSN_EUNSUPPORTED, "odd I and misaligned x": SFSN_EUNSUPPORTED, "I > 64": SFSN_EUNSUPPORTED,
            "R % 16 != 0": SFSN_EUNSUPPORTED, "R = 0": SFSN_EINVAL, "H = 128": SFSN_EUNSUPPORTED, "H = 272": SFSN_EUNSUPPORTED}


def _break_x(name, lists):
    sx, fin = lists[0], lists[1]
    H = 224
    if name == "null w_hh":
        sx[0].w_hh = None
    elif name == "null x":
        fin[0].x = None
    elif name == "misaligned x":
        fin[0].x = _a(400, 4)
    elif name == "misaligned h":
        sx[0].h_state = _a(5, 8)
    elif name == "odd I":
        fin[0].I = 37
    elif name == "odd I and misaligned x":  # (SFSN_EUNSUPPORTED answers before the alignment checks)
        fin[0].I, fin[0].x = 37, _a(400, 4)
    elif name == "I > 64":
        fin[0].I = 66
    elif name == "R % 16 != 0":
        sx[0].R = 24
    elif name == "R = 0":
        sx[0].R = 0
    elif name == "H = 128":
        H = 128
    elif name == "H = 272":
        H = 272
    else:
        raise KeyError(name)
    return H


@pytest.mark.parametrize("n_z", [1, 0])  # beside an input-term list, and as the only layer-0 list
@pytest.mark.parametrize("name", list(X_FAULTS))
def test_a_fault_in_the_fused_x_list_gets_that_entry_points_answer(L, name, n_z):
    lists = _lists(n_z=n_z)
    H = _break_x(name, lists)
    own = L.sfsn_gsn_layer_scan_fused_x(lists[0], lists[1], 1, 4, H, None)
    assert own == X_FAULTS[name]  # (refused: nothing was launched)
    assert _l01(L, *lists, n_z=n_z, H=H) == own


Z_FAULTS = {"null zin": SFSN_EINVAL, "null bias": SFSN_EINVAL, "misaligned zin": SFSN_EINVAL, "misaligned fp32 spikes": SFSN_EINVAL,
            "R = 0": SFSN_EINVAL, "membrane without fp32 spikes": SFSN_EUNSUPPORTED}


def _break_z(name, lists):
    sz = lists[2]
    if name == "null zin":
        sz[0].zin = None
    elif name == "null bias":
        sz[0].bias = None
    elif name == "misaligned zin":
        sz[0].zin = _a(402, 8)
    elif name == "misaligned fp32 spikes":
        sz[0].spikes_f32 = _a(8, 4)
    elif name == "R = 0":
        sz[0].R = 0
    elif name == "membrane without fp32 spikes":
        sz[0].spikes_f32, sz[0].membrane = None, _a(9)
    else:
        raise KeyError(name)


@pytest.mark.parametrize("name", list(Z_FAULTS))
def test_a_fault_in_the_input_term_list_gets_that_entry_points_answer(L, name):
    lists = _lists()
    _break_z(name, lists)
    own = L.sfsn_gsn_layer_scan(lists[2], 1, 4, 224, 1, 16, None)
    assert own == Z_FAULTS[name]  # (refused: nothing was launched)
    assert _l01(L, *lists) == own


F_FAULTS = ("null input spikes", "null packed weights", "null dequantisation", "misaligned input spikes", "misaligned packed weights",
            "null c", "misaligned int8 spikes", "R = 0", "membrane", "fp32 spikes in the second segment only")


def _break_1(name, lists):
    s1, fin1 = lists[3], lists[4]
    if name == "null input spikes":
        fin1[0].spikes_in = None
    elif name == "null packed weights":
        fin1[0].w_ih = None
    elif name == "null dequantisation":
        fin1[0].w_ih_dq = None
    elif name == "misaligned input spikes":
        fin1[0].spikes_in = fin1[0].spikes_in + 4
    elif name == "misaligned packed weights":
        fin1[0].w_ih = _a(403, 8)
    elif name == "null c":
        s1[1].c_state = None
    elif name == "misaligned int8 spikes":
        s1[1].spikes_i8 = s1[1].spikes_i8 + 4
    elif name == "R = 0":
        s1[0].R = 0
    elif name == "membrane":
        s1[0].membrane = _a(9)
    elif name == "fp32 spikes in the second segment only":
        s1[0].spikes_f32, s1[1].spikes_f32 = None, _a(10)
    else:
        raise KeyError(name)


@pytest.mark.parametrize("name", F_FAULTS)
def test_a_fault_in_the_layer_1_list_gets_that_entry_points_answer(L, name):
    lists = _lists(f32=name != "fp32 spikes in the second segment only")
    _break_1(name, lists)
    own = L.sfsn_gsn_layer_scan_fused(lists[3], lists[4], 2, 4, 224, None)
    assert own == SFSN_EINVAL  # (refused: nothing was launched)
    assert _l01(L, *lists) == own


def test_null_lists_and_bad_counts(L):
    sx, fin, sz, s1, fin1 = _lists()
    call = L.sfsn_gsn_layer_scan_l01
    need = L.sfsn_stack_scratch_bytes(2, 2, 56)
    assert L.sfsn_gsn_layer_scan_fused_x(None, fin, 1, 4, 224, None) == SFSN_EINVAL == call(None, fin, 1, sz, 1, s1, fin1, 4, 224, 1, 4, _a(450), need, None)
    assert L.sfsn_gsn_layer_scan_fused_x(sx, None, 1, 4, 224, None) == SFSN_EINVAL == call(sx, None, 1, sz, 1, s1, fin1, 4, 224, 1, 4, _a(450), need, None)
    assert L.sfsn_gsn_layer_scan(None, 1, 4, 224, 1, 16, None) == SFSN_EINVAL == call(sx, fin, 1, None, 1, s1, fin1, 4, 224, 1, 4, _a(450), need, None)
    assert L.sfsn_gsn_layer_scan_fused(None, fin1, 2, 4, 224, None) == SFSN_EINVAL == call(sx, fin, 1, sz, 1, None, fin1, 4, 224, 1, 4, _a(450), need, None)
    assert L.sfsn_gsn_layer_scan_fused(s1, None, 2, 4, 224, None) == SFSN_EINVAL == call(sx, fin, 1, sz, 1, s1, None, 4, 224, 1, 4, _a(450), need, None)
    assert call(sx, fin, 1, sz, 1, s1, fin1, 4, 224, 1, 4, None, need, None) == SFSN_EINVAL  # no scratch
    lists = (sx, fin, sz, s1, fin1)
    assert L.sfsn_gsn_layer_scan_fused_x(sx, fin, -1, 4, 224, None) == SFSN_EINVAL == _l01(L, *lists, n_x=-1)
    assert L.sfsn_gsn_layer_scan(sz, -1, 4, 224, 1, 16, None) == SFSN_EINVAL == _l01(L, *lists, n_z=-1)
    assert L.sfsn_gsn_layer_scan_fused_x(sx, fin, 9, 4, 224, None) == SFSN_EINVAL == _l01(L, *lists, n_x=9)
    assert L.sfsn_gsn_layer_scan_fused_x(sx, fin, 1, -1, 224, None) == SFSN_EINVAL == _l01(L, *lists, T=-1)
    assert L.sfsn_gsn_layer_scan_fused_x(sx, fin, 1, 4, 0, None) == SFSN_EINVAL == _l01(L, *lists, H=0)
    assert _l01(L, *lists, n_x=0, n_z=0) == SFSN_EINVAL  # no segment at all
    assert _l01(L, *lists, lag=-1) == SFSN_EINVAL


@pytest.mark.parametrize("H", [128, 256, 272])
def test_hidden_sizes_outside_the_16_row_io_wave_kernels_are_unsupported(L, H):
    """128: below the fused entry points' range; 256: 16 tiles (round 2's 512-thread bodies); 272: above it -- for every layer-0 layout"""
    for n_x, n_z in ((1, 1), (1, 0), (0, 1)):
        assert _l01(L, *_lists(n_x=n_x, n_z=n_z), n_x=n_x, n_z=n_z, H=H) == SFSN_EUNSUPPORTED


def test_what_ties_the_lists_together(L, monkeypatch):
    """(each list alone is one its own entry point would launch: those are not called here)"""
    lists = _lists()
    assert _l01(L, *lists, shared=0) == SFSN_EUNSUPPORTED  # separate gate weights
    assert _l01(L, *lists, H=240) == SFSN_EUNSUPPORTED  # 15 tiles
    lists[2][0].spikes_f32 = None  # output sets that differ: fp32 spikes on the fused-x side only ...
    assert _l01(L, *lists) == SFSN_EUNSUPPORTED
    lists = _lists(f32=False)
    lists[2][0].spikes_f32 = _a(350)  # ... on the input-term side only ...
    assert _l01(L, *lists) == SFSN_EUNSUPPORTED
    lists = _lists(f32=False)
    for s in lists[3]:
        s.spikes_f32 = _a(351)  # ... and in layer 1 only
    assert _l01(L, *lists) == SFSN_EUNSUPPORTED
    lists = _lists()
    lists[2][0].membrane = _a(352)  # a membrane output (with the fp32 spikes it needs)
    assert _l01(L, *lists) == SFSN_EUNSUPPORTED
    lists = _lists(n_x=5, n_z=5)  # more than SFSN_MAX_SEGMENTS in a layer
    assert _lib.MAX_SEGMENTS == 8 and _l01(L, *lists, n_x=5, n_z=5) == SFSN_EUNSUPPORTED
    lists = _lists()
    lists[4][1].spikes_in = lists[0][0].spikes_i8  # layer 1 of segment 1 reads segment 0's buffer
    assert _l01(L, *lists) == SFSN_EINVAL
    lists = _lists()
    lists[4][0].spikes_in = _a(353)  # ... or a buffer of its own
    assert _l01(L, *lists) == SFSN_EINVAL
    lists = _lists()
    lists[3][1].R = 40  # row counts differ
    assert _l01(L, *lists) == SFSN_EINVAL
    lists = _lists()
    need = L.sfsn_stack_scratch_bytes(2, 2, 56)
    assert _l01(L, *lists, nbytes=need - 4) == SFSN_EINVAL and _l01(L, *lists, nbytes=0) == SFSN_EINVAL  # scratch too small
    assert _l01(L, *lists, scratch=_a(450, 2)) == SFSN_EINVAL  # scratch not a word address
    for var in ("SFSN_SCAN_V2", "SFSN_FUSED_V2"):  # round 2's bodies asked for: read on every call
        monkeypatch.setenv(var, "1")
        assert _l01(L, *lists) == SFSN_EUNSUPPORTED
        monkeypatch.delenv(var)
