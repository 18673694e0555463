"""CPU checks behind tests/test_cirm_stream_io.py (``modeling_cirm_gsn.Model.streaming_outer``, ``sfsn_fullband_stream_hop_wave_io``):
the export, its prototype and ctypes mirror, the entry point's refusals in the header's order -- each answered by an argument check on a
descriptor of host addresses, before any device query -- and the factory's argument refusals beside the sibling's wording.  The
library's host side only."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IO = "sfsn_fullband_stream_hop_wave_io"
P = 1 << 20  # a non-NULL, 64-byte-aligned number that is no device address
TINY = dict(n_fft=512, hop_length=128, win_length=512, fdrc=0.5, input_size=257, hidden_size=20, num_layers=3, proj_size=257,
            output_activate_function=False, df_order=3, use_pre_layer_norm_fb=True, bn=True, shared_weights=True, sequence_model="GSN",
            num_spks=1)


def test_the_entry_point_is_exported_and_declared_without_an_abi_bump():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "sfsn.h")).read()
    assert IO in _lib.EXPORTS and hasattr(L, IO)
    fn = getattr(L, IO)
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.POINTER(_lib.FullbandWaveDesc), ctypes.POINTER(_lib.HopIo), ctypes.c_uint, ctypes.c_void_p]
    decl = re.search(r"\bint\s+" + IO + r"\s*\(([^;]*)\)\s*;", header)
    assert decl, f"{IO} is not declared in sfsn.h"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert [re.sub(r"\s+", " ", a) for a in args] == ["const sfsn_fullband_wave_desc* desc", "const sfsn_hop_io* io", "unsigned held_mask",
                                                      "void* stream"]
    assert re.search(r"#define\s+SFSN_ABI_VERSION\s+21\b", header) and _lib.ABI_VERSION == 21 and L.sfsn_abi_version() == 21
    # sfsn_hop_io is reused as it stands
    assert [n for n, _ in _lib.HopIo._fields_] == ["ratio", "format", "wave_in", "wave_out", "dec_state", "int_state", "taps", "phase_taps"]
    # the new unit is part of what the library is made of, in the Makefile's order
    names = [os.path.basename(p) for p in _lib._sources()]
    assert names[names.index("sfsn_hop_io.hip") + 1] == "sfsn_fullband_hop_io.hip"
    mk = open(os.path.join(ROOT, "spiking_fullsubnet_amd", "csrc", "Makefile")).read()
    assert "sfsn_hop_io.hip sfsn_fullband_hop_io.hip" in mk and "sfsn_fullband_hop_io.o: sfsn_fullband_hop.hip" in mk


def wave_desc(B=3, wave_state=P):
    from spiking_fullsubnet_amd import _lib
    w = _lib.FullbandWaveDesc()
    d = w.hop
    d.n_layers, d.Hp, d.B, d.F, d.S, d.df, d.hop, d.D, d.act, d.unshared = 3, 32, B, 257, 1, 3, 1, 2, 0, 0
    d.clip_start = P
    w.wave_state = wave_state
    return w


def io_of(ratio=3, fmt=1, **ptrs):
    from spiking_fullsubnet_amd import _lib
    io = _lib.HopIo()
    io.ratio, io.format = ratio, fmt
    for k in ("wave_in", "wave_out", "dec_state", "int_state", "taps", "phase_taps"):
        setattr(io, k, ptrs.get(k, P))
    return io


def test_the_refusals_come_in_the_stated_order_without_a_device():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    EINVAL, EUNSUP = _lib.SFSN_EINVAL, _lib.SFSN_EUNSUPPORTED

    def call(w, io, mask=0):
        return L.sfsn_fullband_stream_hop_wave_io(None if w is None else ctypes.byref(w), None if io is None else ctypes.byref(io), mask, None)

    ok = wave_desc()
    assert L.sfsn_fullband_wave_hop_check(32, 3, 257, 1, 3, 3, 0) == _lib.SFSN_OK
    # a descriptor the plain waveform launch refuses as unsupported tells the refusals in front of the launch from the launch's own
    big = wave_desc(B=17)
    assert L.sfsn_fullband_stream_hop_wave(ctypes.byref(big), None) == EUNSUP
    assert call(big, io_of()) == EUNSUP and call(big, io_of(1, 1)) == EUNSUP and call(big, io_of(1, 0)) == EUNSUP  # 6: the plain launch's code
    # 1: the ratio, before everything else (a NULL descriptor and an unknown format included)
    for ratio in (0, 2, 4, -3):
        assert call(big, io_of(ratio)) == EINVAL and call(None, io_of(ratio, 7)) == EINVAL and call(ok, io_of(ratio)) == EINVAL
    # 2: the format
    for fmt in (2, 7, -1):
        assert call(big, io_of(3, fmt)) == EINVAL and call(big, io_of(1, fmt)) == EINVAL and call(None, io_of(3, fmt)) == EINVAL
    # 3: the descriptor
    assert call(None, io_of()) == EINVAL and call(None, io_of(1, 0)) == EINVAL
    assert call(wave_desc(B=17, wave_state=None), io_of()) == EINVAL and call(wave_desc(B=17, wave_state=None), io_of(1, 0)) == EINVAL
    # 4: io's pointers -- the samples for every combination, the states and taps for ratio 3 only
    for k in ("wave_in", "wave_out"):
        for ratio, fmt in ((3, 1), (3, 0), (1, 1), (1, 0)):
            assert call(big, io_of(ratio, fmt, **{k: None})) == EINVAL, (k, ratio, fmt)
    for k in ("dec_state", "int_state", "taps", "phase_taps"):
        assert call(big, io_of(3, 1, **{k: None})) == EINVAL and call(big, io_of(3, 0, **{k: None})) == EINVAL, k
        assert call(big, io_of(1, 1, **{k: None})) == EUNSUP, k  # (ratio 1 has no filter: on to the launch's own refusal)
    # 5: the mask's checks, in front of the launch's own refusals
    for ratio, fmt in ((3, 1), (3, 0), (1, 1), (1, 0)):
        assert call(big, io_of(ratio, fmt), 1 << 17) == EINVAL  # a bit at or beyond B
        assert call(big, io_of(ratio, fmt), 1) == EUNSUP  # a fine mask: the launch's own code
        w = wave_desc(B=17)
        w.hop.clip_start = None  # a held clip needs an origin of its own
        assert call(w, io_of(ratio, fmt), 1) == EINVAL
        assert call(ok, io_of(ratio, fmt), 1 << 3) == EINVAL
    # 6: a geometry that is covered but whose pointers are not there: the plain launch's argument check, still no device
    assert L.sfsn_fullband_stream_hop_wave(ctypes.byref(ok), None) == EINVAL
    for ratio, fmt in ((3, 1), (3, 0), (1, 1), (1, 0)):
        assert call(ok, io_of(ratio, fmt)) == EINVAL and call(ok, io_of(ratio, fmt), 1) == EINVAL
    # io == NULL IS the held entry point
    for w, mask in ((big, 0), (big, 1), (big, 1 << 17), (ok, 0), (None, 0), (None, 1)):
        assert call(w, None, mask) == L.sfsn_fullband_stream_hop_wave_held(None if w is None else ctypes.byref(w), mask, None)


def test_the_factorys_argument_refusals_beside_the_siblings():
    import types
    from spiking_fullsubnet_amd.modeling_cirm_gsn import Model
    cirm = Model(**TINY).eval()
    assert list(inspect.signature(Model.streaming_outer).parameters) == ["self", "batch", "host_io", "resample", "sample_format"]
    sig = inspect.signature(Model.streaming_outer).parameters
    assert (sig["batch"].default, sig["host_io"].default, sig["resample"].default, sig["sample_format"].default) == (1, False, 3, "s16")

    def message(fn):
        with pytest.raises(ValueError) as e:
            fn()
        return str(e.value)

    from spiking_fullsubnet_amd import streaming
    for kw in (dict(resample=2), dict(resample=0), dict(sample_format="s24"), dict(resample=2, sample_format="s24")):
        mine = message(lambda: cirm.streaming_outer(batch=1, **kw))
        # (the sibling's session judges the two options before it looks into its engine)
        theirs = message(lambda: streaming.StreamingSession(types.SimpleNamespace(spec=None), batch=1, waveform=True, **kw))
        assert mine == theirs, kw
    assert "resample must be 1 or 3" in message(lambda: cirm.streaming_outer(resample=2))
    assert "sample_format" in message(lambda: cirm.streaming_outer(sample_format="s24"))
    assert "streaming(waveform=True)" in message(lambda: cirm.streaming_outer(resample=1, sample_format="f32"))
    assert "positive" in message(lambda: cirm.streaming_outer(batch=0))
    # the existing errors: a module on the CPU, an LSTM model
    with pytest.raises(NotImplementedError, match="no CPU path"):
        cirm.streaming_outer()
    with pytest.raises(NotImplementedError, match="LSTM"):
        Model(**dict(TINY, sequence_model="LSTM")).eval().streaming_outer()
    # streaming() keeps refusing both options exactly as it did, and points here
    with pytest.raises(NotImplementedError, match="resample=3"):
        cirm.streaming(batch=1, waveform=True, resample=3)
    with pytest.raises(NotImplementedError, match="sample_format='s16'"):
        cirm.streaming(batch=1, waveform=True, sample_format="s16")
    assert "streaming_outer" in Model.streaming.__doc__ and "follow-up" not in Model.streaming.__doc__


def test_the_session_class_carries_the_plain_defaults():
    from spiking_fullsubnet_amd import fullband_streaming as fs
    import torch
    cls = fs.FullbandStreamingSession
    assert (cls.resample, cls.sample_format, cls._io, cls._outer, cls._fmt_dtype) == (1, "f32", False, 128, torch.float32)
    params = inspect.signature(cls.__init__).parameters
    assert params["resample"].default == 1 and params["sample_format"].default == "f32"
    # the pinned signatures stay
    assert list(inspect.signature(cls.step_wave).parameters) == ["self", "samples", "copy"]
    assert list(inspect.signature(cls.step_wave_host).parameters) == ["self", "samples", "timeout_s"]
    assert list(inspect.signature(cls.catch_up_wave).parameters) == ["self", "samples", "clips"]
    assert IO in fs.__doc__ and "streaming_outer" in fs.__doc__
    with pytest.raises(ValueError, match="resample must be 1 or 3"):
        cls(None, resample=2)
    with pytest.raises(ValueError, match="sample_format"):
        cls(None, sample_format="u8")
    with pytest.raises(ValueError, match="waveform=True"):
        cls(None, resample=3)
