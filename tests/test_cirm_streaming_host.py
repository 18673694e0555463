"""cIRM-GSN streaming without a device: the new C-ABI exports, the host-only coverage check of sfsn_fullband_stream_hop and the
refusals of ``modeling_cirm_gsn.Model.streaming`` that are decided before any device is needed."""
import ctypes

import pytest
import torch

from spiking_fullsubnet_amd import _lib as L
from spiking_fullsubnet_amd.modeling_cirm_gsn import Model

NEW = ("sfsn_fullband_hop_check", "sfsn_fullband_hop_scratch_bytes", "sfsn_fullband_stream_hop")
RECIPE = dict(Hp=272, nl=4, F=257, S=1, df=3, B=1, hop=1)


def _check(**over):
    g = dict(RECIPE, **over)
    D = g.pop("D", g["df"] - 1)
    return L.lib().sfsn_fullband_hop_check(g["Hp"], g["nl"], g["F"], g["S"], g["df"], g["B"], g["hop"], D, g.get("unshared", 0))


def _scratch_bytes(**over):
    g = dict(RECIPE, **over)
    d = L.FullbandHopDesc()
    d.n_layers, d.Hp, d.B, d.F, d.S, d.df, d.hop, d.D = g["nl"], g["Hp"], g["B"], g["F"], g["S"], g["df"], g["hop"], g["df"] - 1
    return L.lib().sfsn_fullband_hop_scratch_bytes(ctypes.byref(d))


def test_exports():
    lib = L.lib()
    for name in NEW:
        assert name in L.EXPORTS
        assert hasattr(lib, name)


def test_coverage_accepts_the_recipe():
    assert _check() == L.SFSN_OK
    assert _check(B=16) == L.SFSN_OK
    assert _check(hop=30) == L.SFSN_OK  # D + hop = 32
    assert _check(Hp=320, F=320, S=2, df=5, nl=1) == L.SFSN_OK
    assert _check(F=193) == L.SFSN_OK
    assert _scratch_bytes() >= 4 and _scratch_bytes(B=16) >= 4  # at least the error word


@pytest.mark.parametrize("over", [dict(B=17), dict(nl=5), dict(Hp=336), dict(hop=31), dict(unshared=1), dict(F=192), dict(F=321),
                                  dict(S=3), dict(df=6), dict(Hp=264)], ids=str)
def test_coverage_refuses(over):
    assert _check(**over) == L.SFSN_EUNSUPPORTED
    if "unshared" not in over:
        assert _scratch_bytes(**over) == 0


@pytest.mark.parametrize("over", [dict(hop=0), dict(B=0), dict(nl=0), dict(D=1)], ids=str)
def test_coverage_invalid(over):
    assert _check(**over) == L.SFSN_EINVAL


def _model(**over):
    kw = dict(n_fft=512, hop_length=128, win_length=512, fdrc=0.5, input_size=257, hidden_size=20, num_layers=2, proj_size=257,
              output_activate_function=False, df_order=3, bn=True, shared_weights=True, sequence_model="GSN", num_spks=1)
    kw.update(over)
    return Model(**kw).eval()


def test_streaming_refusals():
    with pytest.raises(NotImplementedError, match="LSTM"):
        _model(sequence_model="LSTM", bn=False, shared_weights=False).streaming()
    m = _model()
    with pytest.raises(RuntimeError, match="training mode"):
        m.train().streaming()
    m.eval()
    for opt in ("waveform", "host_io", "resident", "count_spikes"):
        with pytest.raises(NotImplementedError, match=opt):
            m.streaming(**{opt: True})
    with pytest.raises(ValueError, match="positive"):
        m.streaming(batch=0)
    with pytest.raises(ValueError, match="positive"):
        m.streaming(hop=0)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        m.streaming()  # parameters on the CPU
    assert not any(p.is_cuda for p in m.parameters())
