"""sfsn_gsn_layer_scan_l01_projdf without a GPU: what it answers to bad arguments, before any launch.  A fault in one of the four lists
gets the answer of the list's own entry point (sfsn_gsn_layer_scan_fused_x, sfsn_gsn_layer_scan at 16 rows per workgroup,
sfsn_gsn_layer_scan_fused, sfsn_proj_deepfilter) for the same list; what only the lists together can get wrong is SFSN_EINVAL.  EVERY
call in this file is refused by an argument check or asks for no frames -- none reaches a launch (the pointers are host addresses)."""
import pytest

from spiking_fullsubnet_amd import _lib
from spiking_fullsubnet_amd._lib import SFSN_EINVAL, SFSN_EUNSUPPORTED, ProjDfGroup
from test_layers01_one_launch_host import _a, _break_1, _break_x, _break_z, _lists, F_FAULTS, X_FAULTS, Z_FAULTS

B, F, T, H, HP = 2, 257, 40, 224, 256


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _groups(lists, t0=0, S=1):
    """One group per layer-1 segment (x then z): R = B * n_units rows, the segment's int8 buffer (which starts at frame t0)."""
    s1 = lists[3]
    arr = (ProjDfGroup * len(s1))()
    for g, s in zip(arr, s1):
        g.n_units, g.fc, g.df = s.R // B, 2, 3
        g.spikes_i8 = s.spikes_i8 - t0 * s.R * HP
        g.w_packed, g.w_dq, g.bias, g.proj = _a(460), _a(461), _a(462), _a(463)
    return arr


def _e(L, lists, groups, n_x=1, n_z=1, nt=4, H=H, shared=1, lag=4, scratch=None, nbytes=None, t0=0, n_groups=None, stft=_a(470), enh=_a(471),
       B=B, F=F, T=T, S=1):
    sx, fin, sz, s1, fin1 = lists
    rows = sum(s.R for s in list(sx or ())[:max(n_x, 0)]) + sum(s.R for s in list(sz or ())[:max(n_z, 0)])
    need = L.sfsn_stack_scratch_bytes(2, max(n_x + n_z, 1), max(rows, 1))
    return L.sfsn_gsn_layer_scan_l01_projdf(sx if n_x else None, fin if n_x else None, n_x, sz if n_z else None, n_z, s1, fin1, H, shared, lag,
                                            _a(450) if scratch is None else scratch, need if nbytes is None else nbytes, stft, B, F, T, S,
                                            groups, len(groups) if n_groups is None else n_groups, enh, _a(472), t0, nt, None)


def test_the_entry_point_is_exported_and_declared():
    assert "sfsn_gsn_layer_scan_l01_projdf" in _lib.EXPORTS and hasattr(_lib.lib(), "sfsn_gsn_layer_scan_l01_projdf")
    assert _lib.lib().sfsn_abi_version() == _lib.ABI_VERSION == 21  # (a new function alone does not bump it)


def test_no_frames_is_ok_and_launches_nothing(L):
    lists = _lists(R_z=24, R_x=32)
    assert _e(L, lists, _groups(lists), nt=0) == 0
    assert _e(L, lists, _groups(lists, t0=7), nt=0, t0=7) == 0


@pytest.mark.parametrize("name", list(X_FAULTS))
def test_a_fault_in_the_fused_x_list_gets_that_entry_points_answer(L, name):
    lists = _lists()
    groups = _groups(lists)
    Hh = _break_x(name, lists)
    own = L.sfsn_gsn_layer_scan_fused_x(lists[0], lists[1], 1, 4, Hh, None)
    assert own == X_FAULTS[name] and _e(L, lists, groups, H=Hh) == own


@pytest.mark.parametrize("name", list(Z_FAULTS))
def test_a_fault_in_the_input_term_list_gets_that_entry_points_answer(L, name):
    lists = _lists()
    groups = _groups(lists)
    _break_z(name, lists)
    own = L.sfsn_gsn_layer_scan(lists[2], 1, 4, 224, 1, 16, None)
    assert own == Z_FAULTS[name] and _e(L, lists, groups) == own


@pytest.mark.parametrize("name", F_FAULTS)
def test_a_fault_in_the_layer_1_list_gets_that_entry_points_answer(L, name):
    lists = _lists(f32=name != "fp32 spikes in the second segment only")
    groups = _groups(lists)
    _break_1(name, lists)
    own = L.sfsn_gsn_layer_scan_fused(lists[3], lists[4], 2, 4, 224, None)
    assert own == SFSN_EINVAL and _e(L, lists, groups) == own


def _break_g(name, g):
    S = 1
    if name == "null spikes":
        g[0].spikes_i8 = None
    elif name == "null packed weights":
        g[1].w_packed = None
    elif name == "misaligned spikes":
        g[0].spikes_i8 = g[0].spikes_i8 + 4
    elif name == "misaligned coefficient rows":
        g[1].proj = _a(463, 8)
    elif name == "no units":
        g[0].n_units = 0
    elif name == "P % 4 != 0":
        g[0].fc, g[0].df = 1, 3
    elif name == "P > 288":
        g[0].fc, g[0].df = 8, 19
    elif name == "more bins than F":
        g[0].fc = g[1].fc = 10  # (16 + 12 units: 280 bins)
    else:
        raise KeyError(name)
    return S


G_FAULTS = {"null spikes": SFSN_EINVAL, "null packed weights": SFSN_EINVAL, "misaligned spikes": SFSN_EINVAL,
            "misaligned coefficient rows": SFSN_EINVAL, "no units": SFSN_EINVAL, "P % 4 != 0": SFSN_EUNSUPPORTED, "P > 288": SFSN_EUNSUPPORTED,
            "more bins than F": SFSN_EINVAL}


@pytest.mark.parametrize("name", list(G_FAULTS))
def test_a_fault_in_the_groups_gets_that_entry_points_answer(L, name):
    lists = _lists()
    groups = _groups(lists)
    _break_g(name, groups)
    own = L.sfsn_proj_deepfilter(_a(470), B, F, T, 1, H, groups, 2, _a(471), _a(472), 0, 4, None)
    assert own == G_FAULTS[name] and _e(L, lists, groups) == own


def test_null_lists_and_bad_counts(L):
    lists = _lists()
    groups = _groups(lists)
    sx, fin, sz, s1, fin1 = lists
    assert _e(L, (None, fin, sz, s1, fin1), groups) == SFSN_EINVAL
    assert _e(L, (sx, fin, None, s1, fin1), groups) == SFSN_EINVAL
    call = L.sfsn_gsn_layer_scan_l01_projdf
    need = L.sfsn_stack_scratch_bytes(2, 2, 56)
    tail = (_a(470), B, F, T, 1, groups, 2, _a(471), _a(472), 0, 4, None)
    assert call(sx, fin, 1, sz, 1, None, fin1, H, 1, 4, _a(450), need, *tail) == SFSN_EINVAL
    assert call(sx, fin, 1, sz, 1, s1, None, H, 1, 4, _a(450), need, *tail) == SFSN_EINVAL
    assert call(sx, fin, 1, sz, 1, s1, fin1, H, 1, 4, None, need, *tail) == SFSN_EINVAL  # no scratch
    assert call(sx, fin, 1, sz, 1, s1, fin1, H, 1, 4, _a(450), need, _a(470), B, F, T, 1, None, 2, _a(471), _a(472), 0, 4, None) == SFSN_EINVAL
    assert L.sfsn_proj_deepfilter(None, B, F, T, 1, H, groups, 2, _a(471), _a(472), 0, 4, None) == SFSN_EINVAL == _e(L, lists, groups, stft=None)
    assert L.sfsn_proj_deepfilter(_a(470), B, F, T, 1, H, groups, 2, None, _a(472), 0, 4, None) == SFSN_EINVAL == _e(L, lists, groups, enh=None)
    assert L.sfsn_proj_deepfilter(_a(470), B, F, T, 1, H, groups, 0, _a(471), _a(472), 0, 4, None) == SFSN_EINVAL == _e(L, lists, groups, n_groups=0)
    assert L.sfsn_proj_deepfilter(_a(470), B, F, T, 1, H, groups, 2, _a(471), _a(472), 38, 4, None) == SFSN_EINVAL == _e(L, lists, groups, t0=38)
    assert L.sfsn_proj_deepfilter(_a(470), B, F, T, 0, H, groups, 2, _a(471), _a(472), 0, 4, None) == SFSN_EINVAL == _e(L, lists, groups, S=0)
    for kw in (dict(n_x=-1), dict(n_z=-1), dict(n_x=9), dict(nt=-1), dict(H=0), dict(n_x=0, n_z=0), dict(lag=-1), dict(t0=-1)):
        assert _e(L, lists, groups, **kw) == SFSN_EINVAL, kw


@pytest.mark.parametrize("Hh", [128, 256, 272])
def test_hidden_sizes_outside_the_16_row_io_wave_kernels_are_unsupported(L, Hh):
    for n_x, n_z in ((1, 1), (1, 0), (0, 1)):
        lists = _lists(n_x=n_x, n_z=n_z)
        assert _e(L, lists, _groups(lists), n_x=n_x, n_z=n_z, H=Hh) == SFSN_EUNSUPPORTED


def test_what_ties_the_lists_together(L):
    lists = _lists()
    assert _e(L, lists, _groups(lists), shared=0) == SFSN_EUNSUPPORTED  # separate gate weights
    assert _e(L, lists, _groups(lists), n_groups=1) == SFSN_EINVAL  # a layer-1 segment without a group
    groups = _groups(lists)
    groups[1].spikes_i8 = _a(480)  # a group that reads a buffer no layer-1 segment writes
    assert _e(L, lists, groups) == SFSN_EINVAL
    groups = _groups(lists)
    groups[1].spikes_i8 = groups[0].spikes_i8  # two groups on one segment
    assert _e(L, lists, groups) == SFSN_EINVAL
    groups = _groups(lists)
    groups[0].n_units += 1  # R != B * n_units
    assert _e(L, lists, groups) == SFSN_EINVAL
    assert _e(L, lists, _groups(lists), t0=3) == SFSN_EINVAL  # the groups' tensors must start t0 frames before the segments'
    assert _e(L, lists, _groups(lists, t0=3), t0=3, nt=0) == 0
    lists = _lists()
    lists[3][1].R = 40  # row counts of the layers differ
    assert _e(L, lists, _groups(_lists())) == SFSN_EINVAL
    lists = _lists()
    groups = _groups(lists)
    need = L.sfsn_stack_scratch_bytes(2, 2, 56)
    assert _e(L, lists, groups, nbytes=need - 4) == SFSN_EINVAL and _e(L, lists, groups, nbytes=0) == SFSN_EINVAL  # scratch too small
    assert _e(L, lists, groups, scratch=_a(450, 2)) == SFSN_EINVAL  # scratch not a word address
