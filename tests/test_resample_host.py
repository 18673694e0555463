"""Outer samples (48 kHz, 16-bit PCM) of the waveform sessions, without a device: the filter design, the phase tables, the reference
and its bound (tests/resampleref.py) against an fp32 emulation and against mutants, the quantiser, the exports and the refusals the C
entry points answer before they touch a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import resampleref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_response_of_the_float64_design():
    h = rr.design64()
    pass_db = rr.response_db(h, np.arange(0.0, 6500.0 + 1, 50.0))
    stop_db = rr.response_db(h, np.arange(9500.0, 24000.0 + 1, 25.0))
    print(f"passband max |dB| {np.abs(pass_db).max():.6f}, 7 kHz {rr.response_db(h, [7000.0])[0]:.4f} dB, stopband max {stop_db.max():.2f} dB, "
          f"sum|h| {np.abs(h).sum():.4f}")
    assert np.abs(pass_db).max() <= 0.001
    assert stop_db.max() <= -80.0
    assert abs(np.abs(h).sum() - 1.939) < 1e-3
    assert np.allclose(h, h[::-1], rtol=0, atol=1e-18)  # linear phase: 47.5 samples of group delay


def test_library_taps_are_the_design_rounded_once():
    from spiking_fullsubnet_amd import spectral
    h, g = spectral.resample_taps_host()
    h_ref, g_ref = rr.taps()
    assert h.dtype == np.float32 and g.dtype == np.float32 and h.shape == (96,) and g.shape == (3, 32)
    assert np.array_equal(h, h_ref) and np.array_equal(g, g_ref)
    assert np.array_equal(g, (3.0 * rr.design64()).astype(np.float32).reshape(32, 3).T)


def test_phase_tables_sum_to_one():
    _, g = rr.taps()
    sums = g.astype(np.float64).sum(axis=1)
    print("phase sums", sums)
    assert np.all(np.abs(sums - 1.0) <= 1e-5)


def _cases():
    out = []
    for n_out in (1, 31, 32, 33, 128, 129):
        for name, x in rr.signals(2, 3 * n_out, seed=n_out).items():
            out.append((f"{name}-{n_out}", rr.as_float(x)))
    return out


def test_fp32_emulation_of_the_stated_order_is_inside_the_bound():
    h, g = rr.taps()
    rng = np.random.default_rng(5)
    for name, x in _cases():
        st = rng.standard_normal((x.shape[0], 96)).astype(np.float32)
        y, bound, _ = rr.down3(x, h, st)
        err = np.abs(rr.down3_f32(x, h, st).astype(np.float64) - y)
        assert np.all(err <= bound), (name, float((err - bound).max()))
        yy = x[:, : max(1, x.shape[1] // 3)]
        su = rng.standard_normal((yy.shape[0], 32)).astype(np.float32)
        z, zb, _ = rr.up3(yy, g, su)
        err = np.abs(rr.up3_f32(yy, g, su).astype(np.float64) - z)
        assert np.all(err <= zb), (name, float((err - zb).max()))


def test_chunked_reference_equals_one_shot():
    h, g = rr.taps()
    x = rr.signals(2, 3 * 128, seed=9)["noise"]
    y, _, s_end = rr.down3(x, h)
    st, parts = None, []
    for a, b in ((0, 3), (3, 123), (123, 384)):
        yp, _, st = rr.down3(x[:, a:b], h, st)
        parts.append(yp)
    assert np.array_equal(np.concatenate(parts, axis=1), y) and np.array_equal(st, s_end)
    z, _, u_end = rr.up3(y, g)
    st, parts = None, []
    for a, b in ((0, 1), (1, 41), (41, 128)):
        zp, _, st = rr.up3(y[:, a:b], g, st)
        parts.append(zp)
    assert np.array_equal(np.concatenate(parts, axis=1), z) and np.array_equal(st, u_end)


def test_bound_rejects_mutants():
    h, g = rr.taps()
    x = rr.signals(2, 3 * 128, seed=3)["noise"]
    st_d = np.random.default_rng(4).standard_normal((2, 96)).astype(np.float32)
    y, yb, _ = rr.down3(x, h, st_d)
    yin = y.astype(np.float32)
    st_u = np.random.default_rng(6).standard_normal((2, 32)).astype(np.float32)
    z, zb, _ = rr.up3(yin, g, st_u)

    def rejected(got, ref, bound):
        return bool(np.any(np.abs(got.astype(np.float64) - ref) > bound))

    assert not rejected(rr.up3_f32(yin, g, st_u), z, zb) and not rejected(rr.down3_f32(x, h, st_d), y, yb)
    mutants = {
        "taps reversed within a phase": rr.up3_f32(yin, g[:, ::-1], st_u),
        "phase index off by one": rr.up3_f32(yin, np.roll(g, 1, axis=0), st_u),
        "the gain 3 missing": rr.up3_f32(yin, (g / 3.0).astype(np.float32), st_u),
        "state shifted by one sample (up)": rr.up3_f32(yin, g, np.concatenate([st_u[:, 1:31], st_u[:, :1], st_u[:, 31:]], axis=1)),
        "state not carried (up)": rr.up3_f32(yin, g, None),
    }
    for name, got in mutants.items():
        assert rejected(got, z, zb), name
    down_mutants = {
        "state shifted by one sample (down)": rr.down3_f32(x, h, np.concatenate([st_d[:, 1:93], st_d[:, :1], st_d[:, 93:]], axis=1)),
        "state not carried (down)": rr.down3_f32(x, h, None),
        "decimation phase off by one": rr.down3_f32(np.concatenate([x[:, 1:], x[:, :1]], axis=1), h, st_d),
    }
    for name, got in down_mutants.items():
        assert rejected(got, y, yb), name


def test_quantiser_and_its_mutants():
    v = np.array([0.0, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768, 0.4 / 32768, 0.6 / 32768, 1.0, 1.5, -1.0, -1.5,
                  32766.5 / 32768, 32767.0 / 32768, np.nan, np.inf, -np.inf, 0.25, -0.75], dtype=np.float32)
    want = np.array([0, 0, 2, 2, 0, -2, 0, 1, 32767, 32767, -32768, -32768, 32766, 32767, 0, 32767, -32768, 8192, -24576], dtype=np.int16)
    assert np.array_equal(rr.quantise(v), want)
    fin = np.nan_to_num(v.astype(np.float64), nan=0.0, posinf=4.0, neginf=-4.0)
    mutants = {
        "truncation": np.clip(np.trunc(fin * 32768), -32768, 32767).astype(np.int16),
        "round half up": np.clip(np.floor(fin * 32768 + 0.5), -32768, 32767).astype(np.int16),
        "missing saturation": np.rint(fin * 32768).astype(np.int64).astype(np.int16),
        "scale 32767": np.clip(np.rint(fin * 32767), -32768, 32767).astype(np.int16),
    }
    for name, got in mutants.items():
        assert not np.array_equal(got, want), name
    s = np.arange(-32768, 32768, dtype=np.int16)  # int16 -> float -> int16 is the identity
    assert np.array_equal(rr.quantise(rr.as_float(s)), s)


def _header():
    with open(os.path.join(ROOT, "include", "sfsn.h")) as f:
        return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S))


def test_exports_prototypes_and_abi():
    from spiking_fullsubnet_amd import _lib
    hdr = _header()
    assert "#define SFSN_ABI_VERSION 21" in hdr and _lib.ABI_VERSION == 21
    assert "#define SFSN_SAMPLE_F32 0" in hdr and "#define SFSN_SAMPLE_S16 1" in hdr
    protos = [
        "int sfsn_resample_down3(const void* in, int in_format, int B, int n_out, long long in_stride, const float* taps , float* state , "
        "float* out , void* stream);",
        "int sfsn_resample_up3(const float* in , int R, int n_in, const float* phase_taps , float* state , void* out, int out_format, "
        "long long out_stride, void* stream);",
        "int sfsn_stream_hop_io(const sfsn_hop_desc* desc , const sfsn_hop_io* io , const uint64_t* held_bits , void* stream);",
    ]
    for p in protos:
        assert re.sub(r"\s+", " ", p) in hdr, p
    m = re.search(r"typedef struct \{([^}]*)\} sfsn_hop_io;", hdr)
    assert m and [f.split()[-1].lstrip("*") for f in m.group(1).split(";") if f.strip()] == \
        ["ratio", "format", "wave_in", "wave_out", "dec_state", "int_state", "taps", "phase_taps"]
    assert [n for n, _ in _lib.HopIo._fields_] == ["ratio", "format", "wave_in", "wave_out", "dec_state", "int_state", "taps", "phase_taps"]
    L = _lib.lib()
    assert L.sfsn_abi_version() == 21
    for name in ("sfsn_resample_down3", "sfsn_resample_up3", "sfsn_stream_hop_io"):
        assert name in _lib.EXPORTS and hasattr(L, name)


def test_refusals_without_a_device():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 512)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    E = _lib.SFSN_EINVAL
    assert L.sfsn_resample_down3(p, 2, 1, 1, 3, p, None, p, None) == E        # unknown format
    assert L.sfsn_resample_down3(None, 2, 0, 0, 0, None, None, None, None) == E
    assert L.sfsn_resample_down3(None, 0, 1, 1, 3, p, None, p, None) == E     # NULL in
    assert L.sfsn_resample_down3(p, 1, 0, 1, 3, p, None, p, None) == E        # B < 1
    assert L.sfsn_resample_down3(p, 1, 1, 0, 3, p, None, p, None) == E        # n_out < 1
    assert L.sfsn_resample_down3(p, 1, 1, 2, 5, p, None, p, None) == E        # in_stride < 3 n_out
    assert L.sfsn_resample_up3(p, 1, 1, p, None, p, -1, 3, None) == E         # unknown format
    assert L.sfsn_resample_up3(p, 1, 1, None, None, p, 0, 3, None) == E       # NULL phase_taps
    assert L.sfsn_resample_up3(p, 1, 2, p, None, p, 1, 5, None) == E          # out_stride < 3 n_in
    desc, io = _lib.HopDesc(), _lib.HopIo()
    io.ratio, io.format = 2, 0
    assert L.sfsn_stream_hop_io(ctypes.byref(desc), ctypes.byref(io), None, None) == E        # ratio
    io.ratio, io.format = 3, 7
    assert L.sfsn_stream_hop_io(ctypes.byref(desc), ctypes.byref(io), None, None) == E        # format
    io.format = 1
    assert L.sfsn_stream_hop_io(ctypes.byref(desc), ctypes.byref(io), None, None) == E        # not a waveform descriptor
    assert L.sfsn_stream_hop_io(None, ctypes.byref(io), None, None) == E
    desc.wave_state, desc.hop = p.value, 2
    assert L.sfsn_stream_hop_io(ctypes.byref(desc), ctypes.byref(io), None, None) == _lib.SFSN_EUNSUPPORTED  # hop != 1
    desc.hop = 1
    assert L.sfsn_stream_hop_io(ctypes.byref(desc), ctypes.byref(io), None, None) == E        # NULL io->wave_in
    io.wave_in = io.wave_out = p.value
    assert L.sfsn_stream_hop_io(ctypes.byref(desc), ctypes.byref(io), None, None) == E        # ratio 3: NULL states / taps
    # the order: the ratio is judged before the format, the format before the descriptor
    io.ratio, io.format = 2, 7
    assert L.sfsn_stream_hop_io(None, ctypes.byref(io), None, None) == E


def test_python_refusals_without_a_device():
    import torch
    from spiking_fullsubnet_amd import spectral
    with pytest.raises(ValueError, match="sample_format"):
        spectral.format_of("s24")
    assert spectral.format_of("s16")[1] == torch.int16 and spectral.format_of("f32")[1] == torch.float32
    with pytest.raises(RuntimeError, match=r"\[B, 3 n\]"):
        spectral.resample_down3(torch.zeros((1, 6)))
    with pytest.raises(ValueError, match="sample_format"):
        spectral.resample_up3(torch.zeros((1, 6)), sample_format="u8")
