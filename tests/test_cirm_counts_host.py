"""cIRM-GSN spike counts without a device: the two C-ABI exports of the counting hop, the host-only slot count, and the refusal of a
counting session on a module that is not on a HIP device."""
import ctypes

import pytest

from spiking_fullsubnet_amd import _lib as L
from spiking_fullsubnet_amd.modeling_cirm_gsn import Model

NEW = ("sfsn_fullband_hop_spike_slots", "sfsn_fullband_stream_hop_counted")
RECIPE = dict(Hp=272, nl=4, F=257, S=1, df=3, B=1, hop=1)


def _desc(**over):
    g = dict(RECIPE, **over)
    d = L.FullbandHopDesc()
    d.n_layers, d.Hp, d.B, d.F, d.S, d.df, d.hop, d.D = g["nl"], g["Hp"], g["B"], g["F"], g["S"], g["df"], g["hop"], g["df"] - 1
    d.unshared = g.get("unshared", 0)
    return d


def test_exports_and_prototypes():
    lib = L.lib()
    for name in NEW:
        assert name in L.EXPORTS
        assert hasattr(lib, name)
    assert lib.sfsn_fullband_hop_spike_slots.restype is ctypes.c_size_t
    assert list(lib.sfsn_fullband_hop_spike_slots.argtypes) == [ctypes.POINTER(L.FullbandHopDesc)]
    assert lib.sfsn_fullband_stream_hop_counted.restype is ctypes.c_int
    assert list(lib.sfsn_fullband_stream_hop_counted.argtypes) == [ctypes.POINTER(L.FullbandHopDesc), ctypes.c_void_p, ctypes.c_void_p]


def test_abi_version_did_not_move():
    assert L.ABI_VERSION == 21 and L.lib().sfsn_abi_version() == 21


@pytest.mark.parametrize("over", [dict(), dict(B=16), dict(Hp=32, nl=3, B=2), dict(Hp=32, nl=3, B=2, hop=5), dict(Hp=272, B=3, S=2)], ids=str)
def test_slot_count(over):
    d = _desc(**over)
    assert L.lib().sfsn_fullband_hop_spike_slots(ctypes.byref(d)) == d.n_layers * d.B * d.Hp // 4


@pytest.mark.parametrize("over", [dict(B=17), dict(unshared=1), dict(Hp=264), dict(nl=5), dict(hop=0)], ids=str)
def test_slot_count_of_an_uncovered_descriptor_is_zero(over):
    d = _desc(**over)
    assert L.lib().sfsn_fullband_hop_spike_slots(ctypes.byref(d)) == 0


def test_counted_launch_refuses_bad_slots_before_anything_else():
    """NULL and 4-byte-misaligned slots are SFSN_EINVAL whatever else the descriptor holds (decided on the host, no device needed)."""
    d = _desc()
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    a += -a % 4
    lib = L.lib()
    assert lib.sfsn_fullband_stream_hop_counted(ctypes.byref(d), None, None) == L.SFSN_EINVAL
    for off in (1, 2, 3):
        assert lib.sfsn_fullband_stream_hop_counted(ctypes.byref(d), ctypes.c_void_p(a + off), None) == L.SFSN_EINVAL
    # (aligned slots: the descriptor's own NULL pointers are the next refusal -- still no launch)
    assert lib.sfsn_fullband_stream_hop_counted(ctypes.byref(d), ctypes.c_void_p(a), None) == L.SFSN_EINVAL
    assert lib.sfsn_fullband_stream_hop_counted(None, ctypes.c_void_p(a), None) == L.SFSN_EINVAL


def test_cpu_module_refuses_a_counting_session():
    m = Model(n_fft=512, hop_length=128, win_length=512, fdrc=0.5, input_size=257, hidden_size=20, num_layers=2, proj_size=257,
              output_activate_function=False, df_order=3, bn=True, shared_weights=True, sequence_model="GSN", num_spks=1).eval()
    with pytest.raises(NotImplementedError, match="count_spikes"):
        m.streaming(count_spikes=True)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        m.streaming(count_spikes=True)
    with pytest.raises(NotImplementedError, match="resident"):
        m.streaming(count_spikes=True, resident=True)
