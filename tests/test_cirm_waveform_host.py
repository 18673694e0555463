"""Waveform mode of the cIRM-GSN hop without a device: the two new C-ABI exports, the host-only coverage check
``sfsn_fullband_wave_hop_check`` and the argument check of ``sfsn_fullband_stream_hop_wave`` that needs no device."""
import pytest

from spiking_fullsubnet_amd import _lib as L

NEW = ("sfsn_fullband_wave_hop_check", "sfsn_fullband_stream_hop_wave")
RECIPE = dict(Hp=272, nl=4, F=257, S=1, df=3, B=1, unshared=0)


def _check(**over):
    g = dict(RECIPE, **over)
    return L.lib().sfsn_fullband_wave_hop_check(g["Hp"], g["nl"], g["F"], g["S"], g["df"], g["B"], g["unshared"])


def test_exports():
    lib = L.lib()
    for name in NEW:
        assert name in L.EXPORTS
        assert hasattr(lib, name)
    assert L.ABI_VERSION == 21 and lib.sfsn_abi_version() == 21


@pytest.mark.parametrize("over", [dict(), dict(B=16), dict(S=2, df=5)], ids=str)
def test_coverage_accepts(over):
    assert _check(**over) == L.SFSN_OK
    g = dict(RECIPE, **over)  # what sfsn_fullband_hop_check says at hop = 1, D = df - 1
    assert L.lib().sfsn_fullband_hop_check(g["Hp"], g["nl"], g["F"], g["S"], g["df"], g["B"], 1, g["df"] - 1, 0) == L.SFSN_OK


@pytest.mark.parametrize("over", [dict(F=201), dict(F=320), dict(B=17), dict(unshared=1), dict(S=3), dict(df=6), dict(nl=5)], ids=str)
def test_coverage_refuses(over):
    assert _check(**over) == L.SFSN_EUNSUPPORTED


@pytest.mark.parametrize("over", [dict(B=0), dict(Hp=0), dict(nl=0), dict(F=0), dict(S=0), dict(df=0), dict(B=-1)], ids=str)
def test_coverage_invalid(over):
    assert _check(**over) == L.SFSN_EINVAL


def test_null_descriptor():
    assert L.lib().sfsn_fullband_stream_hop_wave(None, None) == L.SFSN_EINVAL


def test_descriptor_embeds_the_hop_descriptor():
    import ctypes
    assert L.FullbandWaveDesc.hop.offset == 0 and L.FullbandWaveDesc.hop.size == ctypes.sizeof(L.FullbandHopDesc)
    assert [n for n, _ in L.FullbandWaveDesc._fields_] == ["hop", "wave_in", "wave_state", "ola_state", "wave_out", "window", "spec_g",
                                                            "enh_g", "done"]
