"""CPU checks behind tests/test_stream_advance_ragged.py (``StreamingSession.advance_ragged`` / ``advance_wave_ragged``,
``sfsn_hop_advance_ragged``): the export, every refusal (on a session object without a device: the refusals come before any device
work), the length checks beside what ``advance`` says for the same fault, and the per-clip gather of the hand-back launch restated
in numpy -- which spike / membrane row a clip takes, which frames of [history | new | padding] become its history, which samples its
STFT state, where the overlap-add recurrence stops -- each against the equal-length restatement of tests/test_stream_advance_host.py
at ``N_b = N`` and against the single-clip call of ``N_b`` frames below it.  numpy, torch on the CPU and the library's host side only."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import primeref as pr
from test_stream_advance_host import as_i32, history_after, moved_back, ola_feed_from

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAME = "sfsn_hop_advance_ragged"


def test_the_entry_point_is_exported_and_declared():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "sfsn.h")).read()
    assert NAME in _lib.EXPORTS and hasattr(L, NAME)
    decl = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", header)
    assert decl, f"{NAME} is not declared in sfsn.h"
    fn = getattr(L, NAME)
    assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == len(fn.argtypes) == 5
    assert fn.restype is ctypes.c_int
    # a new function and new structs alone do not bump the version
    assert re.search(r"#define\s+SFSN_ABI_VERSION\s+21\b", header) and _lib.ABI_VERSION == 21 and L.sfsn_abi_version() == 21
    # the ctypes mirror: five ints (padded to the pointers' alignment), five pointers, five sequences of three (spikes, membrane) pairs
    assert ctypes.sizeof(_lib.RaggedSeq) == 8 * 2 * _lib.HOP_MAX_LAYERS
    assert ctypes.sizeof(_lib.AdvanceRaggedSrc) == 24 + 5 * 8 + (1 + _lib.HOP_MAX_GROUPS) * ctypes.sizeof(_lib.RaggedSeq)
    assert _lib.AdvanceRaggedSrc.frames.offset == 24
    # the older structs are what they were
    assert ctypes.sizeof(_lib.AdvanceSrc) == 16 + 4 * 8 + (1 + _lib.HOP_MAX_GROUPS) * ctypes.sizeof(_lib.PrimeSeq)
    doc = header[header.index("sfsn_hop_advance with a backlog of ITS OWN LENGTH"):header.index("typedef struct sfsn_ragged_layer")]
    for word in ("h[k & 1]", "row N_b - 1", "membrane", "N_b < D keeps the tail", "[0, N_b)", "384 + 128 N_b", "ITS OWN N_b / hop",
                 "SFSN_NORM_CUMLAPLACE", "SFSN_EUNSUPPORTED", "SFSN_EINVAL", "without an ABI bump"):
        assert word in doc, word
    from spiking_fullsubnet_amd.streaming import StreamingSession
    for m in (StreamingSession.advance_ragged, StreamingSession.advance_wave_ragged):
        assert m.__doc__ and "ValueError" in m.__doc__
    assert "bit for bit" in StreamingSession.advance_ragged.__doc__


def test_null_and_bad_arguments_are_refused_before_any_launch():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    desc, one, arg = _lib.HopDesc(), (ctypes.c_int * 1)(0), _lib.AdvanceRaggedSrc()
    fn = L.sfsn_hop_advance_ragged
    assert fn(None, one, 1, ctypes.byref(arg), None) == _lib.SFSN_EINVAL
    assert fn(ctypes.byref(desc), None, 1, ctypes.byref(arg), None) == _lib.SFSN_EINVAL
    assert fn(ctypes.byref(desc), one, 1, None, None) == _lib.SFSN_EINVAL
    assert fn(ctypes.byref(desc), one, 0, ctypes.byref(arg), None) == _lib.SFSN_EINVAL
    assert fn(ctypes.byref(desc), one, -1, ctypes.byref(arg), None) == _lib.SFSN_EINVAL
    # a descriptor sfsn_stream_hop would not run (all zeros: no groups) is refused as such
    assert fn(ctypes.byref(desc), one, 1, ctypes.byref(arg), None) == _lib.SFSN_EUNSUPPORTED


# ---- the refusals of the two methods: all of them come before any device work --------------------------------------------------
class _Spec:
    def __init__(self, cum):
        self.cum_laplace, self.num_spks = cum, 1


class _Eng:
    def __init__(self, cum):
        self.spec = _Spec(cum)


def session(B=3, hop=2, waveform=False, resident=False, cum=False, calls=1):
    """A StreamingSession with the fields the argument checks read and no device behind it."""
    from spiking_fullsubnet_amd.streaming import StreamingSession
    s = object.__new__(StreamingSession)
    s.B, s.hop, s.F, s.dev = B, hop, 257, torch.device("cpu")
    s.waveform, s.resident, s.eng = waveform, resident, _Eng(cum)
    s.frames_done, s._wave_calls = 0, calls
    s._clip_f0, s._clip_c0 = np.zeros(B, np.int64), np.zeros(B, np.int64)
    return s


def spectrum(n, N):
    return torch.zeros((n, 257, N), dtype=torch.complex64)


def test_what_advance_ragged_refuses():
    x = spectrum(3, 8)
    with pytest.raises(NotImplementedError, match="resident"):
        session(resident=True).advance_ragged(x, [2, 4, 8])
    with pytest.raises(NotImplementedError, match="resident"):
        session(resident=True, waveform=True).advance_wave_ragged(torch.zeros((3, 512)), [128, 256, 512])
    with pytest.raises(NotImplementedError, match=r"one `advance` call per length"):
        session(cum=True).advance_ragged(x, [2, 4, 8])
    with pytest.raises(NotImplementedError, match=r"one `advance` call per length"):
        session(cum=True, waveform=True, hop=1).advance_wave_ragged(torch.zeros((3, 512)), [128, 256, 512])
    # a mode mismatch, as the siblings
    with pytest.raises(RuntimeError, match="advance_wave_ragged"):
        session(waveform=True).advance_ragged(x, [2, 4, 8])
    with pytest.raises(RuntimeError, match="waveform=True"):
        session().advance_wave_ragged(torch.zeros((3, 512)), [128, 256, 512])
    s = session()
    with pytest.raises(RuntimeError):
        s.advance_ragged(x.real.contiguous(), [2, 4, 8])  # dtype
    with pytest.raises(RuntimeError):
        s.advance_ragged(x[:, :100], [2, 4, 8])           # bins
    with pytest.raises(RuntimeError):
        s.advance_ragged(x[:2], [2, 4])                   # two rows for a session of three
    with pytest.raises(RuntimeError):
        session(waveform=True).advance_wave_ragged(torch.zeros((3, 512), dtype=torch.float64), [128, 256, 512])
    # the clip list: clip_indices' errors, as advance
    with pytest.raises(IndexError):
        s.advance_ragged(x[:1], [2], clips=[3])
    with pytest.raises(ValueError, match="distinct"):
        s.advance_ragged(x[:2], [2, 4], clips=[1, 1])
    with pytest.raises(TypeError):
        s.advance_ragged(x[:1], [2], clips=[0.5])
    # a wrong count of lengths
    with pytest.raises(ValueError, match="2 lengths for 3 clips"):
        s.advance_ragged(x, [2, 4])
    with pytest.raises(ValueError, match="3 lengths for 2 clips"):
        s.advance_ragged(x[:2], [2, 4, 8], clips=[2, 0])
    # the lengths, naming the clip (of the session, not the row)
    with pytest.raises(ValueError, match=r"clip 2\b.*3 frames is not a positive multiple of the session's hop \(2\)"):
        s.advance_ragged(x[:2], [4, 3], clips=[0, 2])
    with pytest.raises(ValueError, match=r"clip 0\b.*0 frames"):
        s.advance_ragged(x, [0, 4, 8])
    with pytest.raises(ValueError, match=r"clip 1\b.*1 frames"):
        s.advance_ragged(x, [2, 1, 8])                    # below one launch
    with pytest.raises(ValueError, match=r"clip 1\b.*10 frames.*hold 8"):
        s.advance_ragged(x, [2, 10, 8])                   # above the tensor's
    with pytest.raises(ValueError, match="CPU"):
        s.advance_ragged(x, torch.tensor([2, 4, 8], device="meta"))
    with pytest.raises(ValueError, match="not an integer"):
        s.advance_ragged(x, [2, 4.0, 8])
    w = session(waveform=True, hop=1)
    with pytest.raises(ValueError, match=r"clip 1\b.*200 samples is not a positive multiple of 128"):
        w.advance_wave_ragged(torch.zeros((3, 512)), [128, 200, 512])
    with pytest.raises(ValueError, match=r"clip 2\b.*640 samples.*hold 512"):
        w.advance_wave_ragged(torch.zeros((3, 512)), [128, 256, 640])
    with pytest.raises(ValueError, match=r"clip 0\b.*0 samples"):
        w.advance_wave_ragged(torch.zeros((3, 512)), [0, 256, 512])
    # a waveform clip with no call in its utterance, as advance_wave says it
    w = session(waveform=True, hop=1)
    w._clip_c0[1] = 1
    with pytest.raises(ValueError, match=r"clip 1\b.*prime_wave"):
        w.advance_wave_ragged(torch.zeros((3, 512)), [128, 256, 512])
    with pytest.raises(ValueError, match=r"clip 0\b.*prime_wave"):
        session(waveform=True, hop=1, calls=0).advance_wave_ragged(torch.zeros((3, 512)), [128, 256, 512])
    # nothing above moved a clip
    assert s.clip_frames.tolist() == [0, 0, 0] and w.clip_calls.tolist() == [1, 0, 1]


@pytest.mark.parametrize("hop", [1, 2, 3])
def test_the_length_checks_say_what_advance_says_for_the_same_fault(hop):
    from spiking_fullsubnet_amd.clip_select import check_frames, check_samples, clip_lengths
    dev = torch.device("cpu")
    for N in (0, 1, 2, 3, 4, 5, 6, 7, 12):
        theirs = None
        try:
            check_frames("advance", spectrum(1, N), 1, 257, dev, hop)
        except ValueError as e:
            theirs = str(e)
        mine = None
        try:
            assert clip_lengths("advance_ragged", [N], [5], hop, f"the session's hop ({hop})", 12, "frames") == [N]
        except ValueError as e:
            mine = str(e)
        assert (mine is None) == (theirs is None), (N, hop, mine, theirs)
        if theirs is not None:
            assert mine == theirs.replace("advance: ", "advance_ragged: clip 5: "), (mine, theirs)
    for Ls in (0, 64, 128, 200, 256, 384):
        theirs = None
        try:
            check_samples("advance_wave", torch.zeros((1, Ls)), 1, dev)
        except ValueError as e:
            theirs = str(e)
        mine = None
        try:
            assert clip_lengths("advance_wave_ragged", torch.tensor([Ls]), [2], 128, "128", 384, "samples") == [Ls]
        except ValueError as e:
            mine = str(e)
        assert (mine is None) == (theirs is None), (Ls, mine, theirs)
        if theirs is not None:
            assert mine == theirs.replace("advance_wave: ", "advance_wave_ragged: clip 2: "), (mine, theirs)
    # every accepted form of the lengths
    for form in ([2 * hop, hop], (2 * hop, hop), np.array([2 * hop, hop]), torch.tensor([2 * hop, hop]), torch.tensor([2 * hop, hop], dtype=torch.int32)):
        assert clip_lengths("advance_ragged", form, [0, 1], hop, f"the session's hop ({hop})", 2 * hop, "frames") == [2 * hop, hop]
    for bad in (7, "12", torch.tensor([[hop]]), torch.tensor([1.0]), [True]):
        with pytest.raises(ValueError):
            clip_lengths("advance_ragged", bad, [0], hop, f"the session's hop ({hop})", 12, "frames")


# ---- the per-clip gather of the hand-back launch, restated --------------------------------------------------------------------------
def toy_scan(x, c0):
    """A causal recurrence with a threshold: per frame the membrane after the frame and the spike -- (mem [N, ..], spk [N, ..], c_state)."""
    c, mem, spk = c0.copy(), [], []
    for t in range(x.shape[0]):
        c = (F32(0.75) * c + x[t]).astype(F32)
        s = (c > 1).astype(np.int8)
        c = (c - s).astype(F32)
        mem.append(c.copy())
        spk.append(s)
    return np.stack(mem), np.stack(spk), c


def take_rows(mem, spk, lens):
    """What the launch takes per clip: row N_b - 1 of the spikes (h) and of the membrane tap (c); mem, spk: [Nmax, clips, H]."""
    b = np.arange(len(lens))
    last = np.asarray(lens) - 1
    return spk[last, b], mem[last, b]


def test_each_clip_takes_the_spike_and_membrane_row_of_its_own_last_frame():
    rng = np.random.default_rng(3)
    Nmax, B, H = 12, 4, 8
    x = rng.standard_normal((Nmax, B, H)).astype(F32)
    c0 = rng.standard_normal((B, H)).astype(F32)
    mem, spk, c_end = toy_scan(x, c0)
    # N_b = N for everybody: the equal-length launch's rows -- the last frame's spikes and c_state
    h, c = take_rows(mem, spk, [Nmax] * B)
    np.testing.assert_array_equal(h, spk[Nmax - 1])
    np.testing.assert_array_equal(c, c_end)
    # different lengths over a padded batch (padding: zeros, as the session writes it): each clip's rows are those of its single-clip
    # run of N_b frames, and c_state of the padded run is NOT (it is the membrane after the last padded frame)
    lens = [1, 5, 12, 8]
    xp = x.copy()
    for b, n in enumerate(lens):
        xp[n:, b] = 0
    memp, spkp, c_pad = toy_scan(xp, c0)
    h, c = take_rows(memp, spkp, lens)
    for b, n in enumerate(lens):
        m1, s1, c1 = toy_scan(x[:n, b:b + 1], c0[b:b + 1])
        np.testing.assert_array_equal(h[b], s1[n - 1, 0])
        np.testing.assert_array_equal(c[b], c1[0])
        assert n == Nmax or not np.array_equal(c_pad[b], c1[0])
    # the spike counts run over [0, N_b) only
    counts = [int(spkp[:n, b].sum()) for b, n in enumerate(lens)]
    assert counts == [int(toy_scan(x[:n, b:b + 1], c0[b:b + 1])[1].sum()) for b, n in enumerate(lens)]


def history_ragged(buf, lead, n_b, D):
    """The launch's index: the D frames that end with frame lead + N_b - 1 of the clip's [history | new | padding] row."""
    return buf[..., lead + n_b - D:lead + n_b] if D else buf[..., :0]


@pytest.mark.parametrize("D", [1, 2, 4])
def test_history_composition_at_each_clips_own_end(D):
    rng = np.random.default_rng(10 + D)
    Nmax = 3 * D + 2
    hist = rng.standard_normal((5, D)).astype(F32)
    new = rng.standard_normal((5, Nmax)).astype(F32)
    buf = np.concatenate([hist, new], -1)
    np.testing.assert_array_equal(history_ragged(buf, D, Nmax, D), history_after(hist, new, D))  # N_b = N: the equal-length launch
    for n_b in sorted({1, max(D - 1, 1), D, D + 1, Nmax - 1}):
        padded = buf.copy()
        padded[..., D + n_b:] = np.nan  # (what lies behind the clip's end is never read)
        got = history_ragged(padded, D, n_b, D)
        np.testing.assert_array_equal(got, history_after(hist, new[..., :n_b], D))
        if n_b < D:  # the tail of the old history stays in front
            np.testing.assert_array_equal(got[..., :D - n_b], hist[..., n_b:])
            np.testing.assert_array_equal(got[..., D - n_b:], new[..., :n_b])
    # a longer lead than D (rows of T > D + Nmax frames): the index counts from the row's end
    lead = D + 3
    wide = np.concatenate([rng.standard_normal((5, 3)).astype(F32), buf], -1)
    np.testing.assert_array_equal(history_ragged(wide, lead, 2, D), history_after(hist, new[..., :2], D))


def test_the_stft_state_ends_with_each_clips_own_last_sample():
    rng = np.random.default_rng(5)
    cmax = 6
    ctx = rng.standard_normal(384).astype(F32)
    smp = rng.standard_normal(128 * cmax).astype(F32)
    row = np.concatenate([ctx, smp])
    for c in range(1, cmax + 1):
        end = 384 + 128 * c
        got = row[end - 512:end]
        np.testing.assert_array_equal(got, np.concatenate([ctx, smp[:128 * c]])[-512:])  # advance_wave's tail of a backlog of c calls
        assert end - 512 >= 0
    np.testing.assert_array_equal(row[384 + 128 * cmax - 512:], row[-512:])  # N_b = N


def ola_feed_ragged(M, n_max, n_b):
    """The launch's loop: the carried sums, then the clip's own frames M .. M + N_b - 1 in ascending order; blocks N_b .. Nmax - 1 are
    written as zeros (None) and add nothing.  (outputs per block, what the accumulator holds afterwards.)"""
    acc = {j: ([("carry", j)] if j < 3 and M > 0 else []) for j in range(4)}
    outputs = []
    for t in range(n_max):
        if t >= n_b:
            outputs.append(None)
            continue
        for j in range(4):
            acc[j] = acc[j] + [(M + t, j)]
        outputs.append(acc[0])
        acc = {0: acc[1], 1: acc[2], 2: acc[3], 3: []}
    return outputs, acc


@pytest.mark.parametrize("M", [0, 1, 2, 3, 6])
def test_the_overlap_add_recurrence_stops_at_each_clips_own_last_frame(M):
    n_max = 19
    assert ola_feed_ragged(M, n_max, n_max) == ola_feed_from(M, n_max)  # N_b = N: the equal-length launch
    for n_b in (1, 2, 3, 4, 5, 18):
        outputs, left = ola_feed_ragged(M, n_max, n_b)
        want_out, want_left = ola_feed_from(M, n_b)
        assert outputs[:n_b] == want_out and outputs[n_b:] == [None] * (n_max - n_b)
        assert left == want_left


@pytest.mark.parametrize("hop", [1, 2])
@pytest.mark.parametrize("k", [0, 5, 2 ** 31 + 3, 2 ** 32 - 3])
def test_each_origin_moves_back_by_its_own_launches(k, hop):
    ages = [0, 1, 7, 40]
    lens = [n * hop for n in (1, 17, 40, 9)]
    orgs = [(k - a) % (1 << 32) for a in ages]
    # the session's operation: an int32 tensor minus an int32 tensor of the clips' own launch counts, wrapping
    i32 = torch.tensor([as_i32(o) for o in orgs], dtype=torch.int32)
    i32.sub_(torch.tensor(lens, dtype=torch.int32) // hop)
    for a, n, o, got in zip(ages, lens, orgs, i32.tolist()):
        new = moved_back(o, n, hop)
        assert got % 2 ** 32 == new and pr.frame_index_at(k, new) == a + n // hop and new != k
        if a == 0:
            assert new == pr.origin(k, n, hop)
