"""CPU checks behind tests/test_stream_advance.py (``StreamingSession.advance`` / ``advance_wave``, ``sfsn_hop_seed`` /
``sfsn_hop_advance``): the exports, the refusals that need no device, and the index arithmetic of a backlog restated in numpy -- the
origin of a continued clip with wrap, which frames of [history | new] become the session's history for N < D, N = D and N > D, and
the order in which the overlap-add accumulator takes carried partial sums and new frames (generalising ``primeref.ola_feed``),
against the oracle's inverse STFT.  The exactness condition of the inputs is tests/test_stream_prime_host.py's: the GPU file uses the
same fixtures, seeds, spectra and waves.  numpy, the oracle and the library's host side only."""
import ctypes
import os
import re

import numpy as np
import pytest

import primeref as pr
from oracle import model as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAMES = ("sfsn_hop_seed", "sfsn_hop_advance")


def test_the_entry_points_are_exported_and_declared():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "sfsn.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name)
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl, f"{name} is not declared in sfsn.h"
        fn = getattr(L, name)
        assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == len(fn.argtypes) == 5
        assert fn.restype is ctypes.c_int
    # new functions alone do not bump the version
    assert re.search(r"#define\s+SFSN_ABI_VERSION\s+21\b", header) and _lib.ABI_VERSION == 21 and L.sfsn_abi_version() == 21
    # the ctypes mirrors: sfsn_seed_dst = four ints, two pointers, five sequences of (three layers x two pointers + cum);
    # sfsn_advance_src = four ints, four pointers, five sfsn_prime_seq
    assert ctypes.sizeof(_lib.SeedSeq) == 8 * (2 * _lib.HOP_MAX_LAYERS + 1)
    assert ctypes.sizeof(_lib.SeedDst) == 16 + 2 * 8 + (1 + _lib.HOP_MAX_GROUPS) * ctypes.sizeof(_lib.SeedSeq)
    assert ctypes.sizeof(_lib.AdvanceSrc) == 16 + 4 * 8 + (1 + _lib.HOP_MAX_GROUPS) * ctypes.sizeof(_lib.PrimeSeq)
    # the exactness statement and the layout are in the header
    doc = header[header.index("sfsn_hop_seed: the offline kernels' START tensors"):header.index("typedef struct sfsn_seed_layer")]
    for word in ("h[k & 1]", "cum[k & 1]", "ADDED to", "wave_tail", "N < D keeps the tail", "Exactness", "bit for bit", "SFSN_EUNSUPPORTED"):
        assert word in doc, word
    from spiking_fullsubnet_amd.streaming import StreamingSession
    for m in (StreamingSession.advance, StreamingSession.advance_wave):
        assert "bit for bit" in StreamingSession.advance.__doc__ and m.__doc__


def test_null_and_bad_arguments_are_refused_before_any_launch():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    desc, one = _lib.HopDesc(), (ctypes.c_int * 1)(0)
    for fn, arg in ((L.sfsn_hop_seed, _lib.SeedDst()), (L.sfsn_hop_advance, _lib.AdvanceSrc())):
        assert fn(None, one, 1, ctypes.byref(arg), None) == _lib.SFSN_EINVAL
        assert fn(ctypes.byref(desc), None, 1, ctypes.byref(arg), None) == _lib.SFSN_EINVAL
        assert fn(ctypes.byref(desc), one, 1, None, None) == _lib.SFSN_EINVAL
        assert fn(ctypes.byref(desc), one, 0, ctypes.byref(arg), None) == _lib.SFSN_EINVAL
        assert fn(ctypes.byref(desc), one, -1, ctypes.byref(arg), None) == _lib.SFSN_EINVAL
        # a descriptor sfsn_stream_hop would not run (all zeros: no groups) is refused as such
        assert fn(ctypes.byref(desc), one, 1, ctypes.byref(arg), None) == _lib.SFSN_EUNSUPPORTED


# ---- origins ------------------------------------------------------------------------------------------------------------------
def moved_back(org, N, hop):
    """clip_start of a clip with origin `org` after a backlog of N frames (uint32 arithmetic)."""
    return (org - N // hop) % (1 << 32)


def as_i32(v):
    v %= 1 << 32
    return v - (1 << 32) if v >= 1 << 31 else v


@pytest.mark.parametrize("hop", [1, 2, 3])
@pytest.mark.parametrize("k", [0, 1, 5, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 3, 2 ** 32 - 3, 2 ** 32 - 1])
def test_origin_arithmetic_wraps(k, hop):
    from spiking_fullsubnet_amd import clip_select
    from spiking_fullsubnet_amd.streaming import StreamingSession
    for age in (0, 1, 7, 40, 2 ** 31 - 5):  # launches the clip has made when launch k is next
        org = (k - age) % (1 << 32)
        assert pr.frame_index_at(k, org) == age
        for n_launches in (1, 2, 9, 40, 1250):
            N = n_launches * hop
            new = moved_back(org, N, hop)
            assert 0 <= new < 2 ** 32
            assert pr.frame_index_at(k, new) == age + n_launches          # launch k continues n_launches frame indices further ...
            assert pr.frame_index_at(k, new) * hop == age * hop + N      # ... with N frames more before it
            assert new != k                                              # never the launch that reads the state as zero
            assert pr.frame_index_at((k + 7) % 2 ** 32, new) == age + n_launches + 7
            # what the session does: a subtraction on the int32 tensor that holds the origins, wrapping like the hardware's
            i32 = np.array([StreamingSession._as_i32(org)], dtype=np.int32)
            with np.errstate(over="ignore"):
                i32 -= np.int32(n_launches)
            assert int(i32[0]) % 2 ** 32 == new and as_i32(new) == int(i32[0])
            assert clip_select.as_i32(new) == as_i32(new) and StreamingSession._as_i32 is clip_select.as_i32  # (the sessions' own)
            if age == 0:
                assert new == pr.origin(k, N, hop)  # a fresh clip: prime's formula


# ---- the history a backlog leaves -------------------------------------------------------------------------------------------------
def history_after(hist, new, D):
    """The session's last D frames after `new` [.., N] behind `hist` [.., D]: the last D frames of [history | new]."""
    return np.concatenate([hist, new], -1)[..., -D:] if D else hist[..., :0]


@pytest.mark.parametrize("D", [1, 2, 4])
def test_history_composition(D):
    rng = np.random.default_rng(D)
    hist = rng.standard_normal((3, 5, D)).astype(F32)
    for N in sorted({1, max(D - 1, 1), D, D + 1, 3 * D + 2}):
        new = rng.standard_normal((3, 5, N)).astype(F32)
        got = history_after(hist, new, D)
        # frame by frame, what N single steps leave: shift by one, append
        want = hist.copy()
        for t in range(N):
            want = np.concatenate([want[..., 1:], new[..., t:t + 1]], -1)
        np.testing.assert_array_equal(got, want)
        if N < D:  # the tail of the old history stays in front
            np.testing.assert_array_equal(got[..., :D - N], hist[..., N:])
            np.testing.assert_array_equal(got[..., D - N:], new)
        else:
            np.testing.assert_array_equal(got, new[..., N - D:])
        # the launch's index: frame d of the new history is frame T - D + d of the T = D + N frame buffer
        T = D + N
        buf = np.concatenate([hist, new], -1)
        for d in range(D):
            np.testing.assert_array_equal(got[..., d], buf[..., T - D + d])
    # a fresh clip's history is zeros: N < D leaves zeros in front, as a short prefix does when priming
    got = history_after(np.zeros_like(hist), new[..., :1], D)
    assert not got[..., :D - 1].any() and np.array_equal(got[..., D - 1:], new[..., :1])


# ---- which frames the new samples complete ------------------------------------------------------------------------------------
def test_frame_j_of_the_backlog_is_the_centred_frame_j_plus_2_of_context_and_samples():
    rng = np.random.default_rng(7)
    w = rng.standard_normal((1, 128 * 12)).astype(F32)
    full = om.stft(w)  # frame f covers samples [128 f - 256, 128 f + 256)
    for m, c in ((1, 1), (1, 3), (2, 2), (4, 5), (7, 1)):
        # after m calls the STFT state's last 384 samples are samples [128 m - 384, 128 m), zeros before the utterance's first
        ctx = np.zeros((1, 384), F32)
        have = min(384, 128 * m)
        ctx[:, 384 - have:] = w[:, 128 * m - have:128 * m]
        buf = np.concatenate([ctx, w[:, 128 * m:128 * (m + c)]], -1)
        got = om.stft(buf)
        assert got.shape[-1] == c + 4
        for j in range(c):  # the clip's frame m - 1 + j: it ends with the samples of call m + j
            np.testing.assert_array_equal(got[:, :, j + 2], full[:, :, m - 1 + j])
        assert pr.frames_of_calls(m + c)[len(pr.frames_of_calls(m)):] == list(range(max(m - 1, 0), m + c - 1))


# ---- the overlap-add accumulator with carried partial sums ----------------------------------------------------------------------
def ola_feed_from(M, c):
    """primeref.ola_feed generalised: a clip whose accumulator holds what frames 0 .. M - 1 left (block j = padded positions
    [128 (M + j), 128 (M + j + 1))) takes the frames M .. M + c - 1.  Returns (outputs, left): outputs[i] = the terms of the block
    the i-th new frame completes (padded positions [128 (M + i), ..)), left[j] = the terms of block j of the accumulator afterwards;
    a term is ("carry", j) -- block j of the carried accumulator, always FIRST -- or (frame, block of that frame's 512 samples), the
    new frames in ascending order."""
    acc = {j: ([("carry", j)] if j < 3 and M > 0 else []) for j in range(4)}
    outputs = []
    for f in range(M, M + c):
        for j in range(4):
            acc[j] = acc[j] + [(f, j)]
        outputs.append(acc[0])
        acc = {0: acc[1], 1: acc[2], 2: acc[3], 3: []}
    return outputs, acc


@pytest.mark.parametrize("M", [0, 1, 2, 3, 6])
@pytest.mark.parametrize("c", [1, 2, 3, 4, 5, 19])
def test_the_accumulator_takes_carried_sums_first_then_new_frames_in_ascending_order(M, c):
    outputs, left = ola_feed_from(M, c)
    assert left[3] == [] and len(outputs) == c
    for terms in outputs + list(left.values()):
        assert [t for t in terms if t[0] == "carry"] == terms[:1 if terms and terms[0][0] == "carry" else 0]  # carried sums first
        frames = [t[0] for t in terms if t[0] != "carry"]
        assert frames == sorted(frames)                                                                      # ascending frames
    # expanded into frames, the carried blocks are primeref.ola_feed(M)'s and the result is primeref.ola_feed(M + c)'s
    old = pr.ola_feed(M)

    def expand(terms):
        out = []
        for t in terms:
            out += old[t[1]] if t[0] == "carry" else [t]
        return out

    want = pr.ola_feed(M + c)
    for j in range(4):
        assert expand(left[j]) == want[j], (j, expand(left[j]), want[j])
    for i, terms in enumerate(outputs):
        t = M + i  # the frame that completes the block: frames t - 3 .. t, oldest first
        assert expand(terms) == [(f, t - f) for f in range(max(0, t - 3), t + 1)]
    # in numbers, against the oracle's inverse STFT of all M + c frames: block i divided by the envelope of the frames that exist
    rng = np.random.default_rng(100 * M + c)
    n_fr = M + c
    spec = (rng.standard_normal((1, 257, n_fr + 3)) + 1j * rng.standard_normal((1, 257, n_fr + 3))).astype(np.complex64)
    spec[:, :, n_fr:] = 0
    win = om.hann_window(512).astype(np.float64)
    frames = np.fft.irfft(spec.astype(np.complex128).transpose(0, 2, 1), n=512, axis=-1)[0] * win
    want = om.istft(spec, length=128 * (n_fr + 2))[0].astype(np.float64)  # sample n = padded position n + 256
    for i, terms in enumerate(outputs):
        t = M + i
        if t < 2:
            continue  # (the part the inverse STFT trims: the launch writes zeros)
        got = sum(frames[f, 128 * blk:128 * (blk + 1)] for f, blk in expand(terms))
        env = sum(win[128 * q:128 * (q + 1)] ** 2 for q in range(4) if t - q >= 0)
        np.testing.assert_allclose(got / env, want[128 * t - 256:128 * t - 128], rtol=0, atol=1e-5)
