"""CPU checks behind tests/test_stream_prime.py (``StreamingSession.prime`` / ``prime_wave``, ``sfsn_hop_prime``): the export, the
exactness condition of every (fixture, seed, prefix) the GPU file uses, and the index arithmetic of priming restated in numpy
(tests/primeref.py) -- origins with wrap, the frames c calls of samples complete, and what the last three frames leave in the
overlap-add accumulator, against the oracle's inverse STFT.  numpy, the oracle and the library's host side only."""
import ctypes
import os
import re

import numpy as np
import pytest

import hopref as hr
import primeref as pr
import scanref as sr
from oracle import model as om
from oracle.model import forward_from_stft, spec_from_frozen_kwargs, spec_from_live_kwargs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_the_entry_point_is_exported_and_declared():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    assert "sfsn_hop_prime" in _lib.EXPORTS and hasattr(L, "sfsn_hop_prime")
    header = open(os.path.join(ROOT, "include", "sfsn.h")).read()
    decl = re.search(r"\bint\s+sfsn_hop_prime\s*\(([^;]*)\)\s*;", header)
    assert decl, "sfsn_hop_prime is not declared in sfsn.h"
    assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == len(L.sfsn_hop_prime.argtypes) == 5
    assert L.sfsn_hop_prime.restype is ctypes.c_int
    # a new function alone does not bump the version; sfsn_hop_desc is what it was
    assert re.search(r"#define\s+SFSN_ABI_VERSION\s+21\b", header) and _lib.ABI_VERSION == 21 and L.sfsn_abi_version() == 21
    # the ctypes mirror of sfsn_prime_src: three ints, three pointers, five sequences of (three layers x two pointers + cum)
    assert ctypes.sizeof(_lib.PrimeSeq) == 8 * (2 * _lib.HOP_MAX_LAYERS + 1)
    assert ctypes.sizeof(_lib.PrimeSrc) == 16 + 3 * 8 + (1 + _lib.HOP_MAX_GROUPS) * ctypes.sizeof(_lib.PrimeSeq)


def test_null_arguments_are_refused_before_any_launch():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    desc, src, one = _lib.HopDesc(), _lib.PrimeSrc(), (ctypes.c_int * 1)(0)
    assert L.sfsn_hop_prime(None, one, 1, ctypes.byref(src), None) == _lib.SFSN_EINVAL
    assert L.sfsn_hop_prime(ctypes.byref(desc), None, 1, ctypes.byref(src), None) == _lib.SFSN_EINVAL
    assert L.sfsn_hop_prime(ctypes.byref(desc), one, 1, None, None) == _lib.SFSN_EINVAL
    assert L.sfsn_hop_prime(ctypes.byref(desc), one, 0, ctypes.byref(src), None) == _lib.SFSN_EINVAL
    # a descriptor sfsn_stream_hop would not run (all zeros: no groups) is not primed either
    assert L.sfsn_hop_prime(ctypes.byref(desc), one, 1, ctypes.byref(src), None) == _lib.SFSN_EUNSUPPORTED


# ---- the exactness condition ----------------------------------------------------------------------------------------------
def layer0_inputs(name, stft, seed=None):
    front, kw, _ = pr.FIXTURES[name]
    spec = spec_from_live_kwargs(kw) if front == "live" else spec_from_frozen_kwargs(kw)
    res = forward_from_stft(spec, pr.state_dict(name, seed), stft, precision="f64")
    return [np.asarray(res["fb_all"][0], F32)] + [np.asarray(a[0], F32) for a in res["sb_all"]]


def near_threshold(name, stft, first, seed=None):
    """The layer-0 membranes of frames >= first that lie within the "x32" bound of the threshold: (count, elements, smallest margin)."""
    n_near, n_all, margin = 0, 0, np.inf
    for hd, x in zip(pr.layer0_cells(name, seed), layer0_inputs(name, stft, seed)):
        ref = sr.layer(hr.layer_case(hd, x))
        y, tol = np.abs(ref["y"][first:]), ref["tol"][first:]
        assert np.isfinite(y).all() and np.isfinite(tol).all()
        n_near += int((y <= tol).sum())
        n_all += y.size
        with np.errstate(divide="ignore"):
            margin = min(margin, float((y / tol).min()))
    return n_near, n_all, margin


@pytest.mark.parametrize("name", sorted(pr.FIXTURES))
def test_no_layer0_membrane_of_the_spectral_cases_is_within_the_bound_of_the_threshold(name):
    """Every prefix length of the GPU file is at least one frame, so the frames behind a prefix are 1 .. T - 1 of every clip (the
    B = 1 sessions stream clip 0 of the same batch).  The cap is zero: a case that fails gets another seed, not a looser assertion."""
    n_near, n_all, margin = near_threshold(name, pr.spectra(name, pr.B_MAX), 1)
    print(f"PRIME_EXACT {name}: {n_near} of {n_all} layer-0 membranes within the bound, smallest |y| / tol {margin:.3g}")
    assert n_near == 0


@pytest.mark.parametrize("name", sorted(pr.WAVE_FIXTURES))
def test_no_layer0_membrane_of_the_waveform_cases_is_within_the_bound_of_the_threshold(name):
    w = pr.waves(name, pr.B_MAX)
    stft = om.stft(w)[:, :, :pr.CALLS - 1]  # the frames CALLS calls complete
    n_near, n_all, margin = near_threshold(name, stft, 0, pr.WAVE_FIXTURES[name])
    print(f"PRIME_EXACT {name} (waveform): {n_near} of {n_all} within the bound, smallest |y| / tol {margin:.3g}")
    assert n_near == 0


# ---- origins ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [1, 2, 3])
@pytest.mark.parametrize("k", [0, 1, 5, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 3, 2 ** 32 - 1])
def test_origin_arithmetic_wraps(k, hop):
    for n_launches in (1, 2, 9, 40, 1250):
        N = n_launches * hop
        org = pr.origin(k, N, hop)
        assert 0 <= org < 2 ** 32
        assert pr.frame_index_at(k, org) == N // hop            # the next launch computes frame index N / hop ...
        assert pr.frame_index_at(k, org) * hop == N              # ... with N frames before it
        assert org != k                                          # never the launch that reads the state as zero
        assert pr.frame_index_at((k + 7) % 2 ** 32, org) == N // hop + 7
        # what the session writes: the same 32 bits as a signed fill value
        from spiking_fullsubnet_amd.streaming import StreamingSession
        assert StreamingSession._as_i32(k - N // hop) % 2 ** 32 == org
    assert pr.origin(k, 0, hop) == k  # no frame yet (a waveform clip after one call): the next launch reads zero state, rightly


# ---- which frames exist ---------------------------------------------------------------------------------------------------
def test_frames_of_calls():
    assert pr.frames_of_calls(1) == []
    for c in range(2, 24):
        assert pr.frames_of_calls(c) == list(range(c - 1))
    # against the oracle's STFT: frames 0 .. c - 2 of c calls' samples do not change when more samples follow; the next two do
    rng = np.random.default_rng(5)
    w = rng.standard_normal((1, 128 * 9)).astype(F32)
    full = om.stft(w)
    for c in (2, 3, 5, 8):
        part = om.stft(w[:, :128 * c])
        assert part.shape[-1] == c + 1
        np.testing.assert_array_equal(part[:, :, :c - 1], full[:, :, :c - 1])
        assert not np.array_equal(part[:, :, c - 1], full[:, :, c - 1]) and not np.array_equal(part[:, :, c], full[:, :, c])


# ---- the overlap-add accumulator ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [0, 1, 2, 3, 4, 18])
def test_what_the_last_three_frames_leave_in_the_accumulator(M):
    feed = pr.ola_feed(M)
    assert feed[3] == [] and all(f >= max(0, M - 3) for j in feed for f, _ in feed[j])
    assert all([f for f, _ in feed[j]] == sorted(f for f, _ in feed[j]) for j in feed)  # ascending frame order
    assert [len(feed[j]) for j in range(4)] == [min(M, 3), min(M, 2), min(M, 1), 0]
    if M == 0:
        return
    # the oracle's inverse STFT of M + 3 frames whose last three are silent: its un-normalised sums at the padded positions
    # [128 M, 128 (M + 3)) are what the M real frames leave behind -- the accumulator's blocks 0 .. 2
    rng = np.random.default_rng(M)
    spec = (rng.standard_normal((1, 257, M + 3)) + 1j * rng.standard_normal((1, 257, M + 3))).astype(np.complex64)
    spec[:, :, M:] = 0
    win = om.hann_window(512).astype(np.float64)
    frames = np.fft.irfft(spec.astype(np.complex128).transpose(0, 2, 1), n=512, axis=-1)[0] * win  # [M + 3, 512]
    env = np.zeros(128 * (M + 2) + 512)
    for t in range(M + 3):
        env[128 * t:128 * t + 512] += win * win
    want = om.istft(spec, length=128 * (M + 2))[0].astype(np.float64)  # samples n = padded position n + 256
    for j in range(3):
        got = np.zeros(128)
        for f, blk in feed[j]:
            got += frames[f, 128 * blk:128 * (blk + 1)]
        pos = 128 * (M + j)  # padded position of the block's first sample
        if pos - 256 < 0:
            continue  # (trimmed by the inverse STFT: M = 1, block 0)
        np.testing.assert_allclose(got / env[pos:pos + 128], want[pos - 256:pos - 128], rtol=0, atol=1e-5)
