"""CPU checks behind tests/test_cirm_catchup_ragged.py (``FullbandStreamingSession.catch_up_ragged`` / ``catch_up_wave_ragged``,
``sfsn_fullband_hop_advance_ragged``): the export, every ``SFSN_EINVAL`` of the entry point (otherwise valid dummy arguments with exactly
one defect, so that the return comes before any launch), every refusal of the two methods on a session object without a device beside
what ``catch_up`` / ``catch_up_wave`` raise for the same fault, and the per-clip gather of the hand-back launch restated in numpy --
which spike / membrane row a clip takes, which frames of [history | new | padding] become its history, which samples its STFT state
(both kinds of waveform clip), where the overlap-add recurrence stops (a fresh clip and a clip without a call included) and how far
each origin moves -- each against the equal-length restatement at ``N_b = N`` and the single-clip call of ``N_b`` frames.  numpy, torch
on the CPU and the library's host side only."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_cirm_catchup_host import Dummy, _set, age_at
from test_stream_advance_ragged_host import history_ragged, take_rows, toy_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAME = "sfsn_fullband_hop_advance_ragged"


def test_the_entry_point_is_exported_and_declared():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "sfsn.h")).read()
    assert NAME in _lib.EXPORTS and hasattr(L, NAME)
    decl = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", header)
    assert decl, f"{NAME} is not declared in sfsn.h"
    fn = getattr(L, NAME)
    assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == len(fn.argtypes) == 8
    assert fn.restype is ctypes.c_int
    # a new function and a new struct alone do not bump the version
    assert re.search(r"#define\s+SFSN_ABI_VERSION\s+21\b", header) and _lib.ABI_VERSION == 21 and L.sfsn_abi_version() == 21
    # the ctypes mirror: five ints (padded to the pointers' alignment), six pointers, four layers of a (spikes, membrane) pair
    S = _lib.FullbandAdvanceRaggedSrc
    assert ctypes.sizeof(S) == 24 + 6 * 8 + _lib.FULLBAND_HOP_MAX_LAYERS * 16
    assert S.frames.offset == 24 and S.window.offset == 64 and S.layer.offset == 72
    # the older structs are what they were
    assert ctypes.sizeof(_lib.FullbandAdvanceSrc) == 16 + 5 * 8 + _lib.FULLBAND_HOP_MAX_LAYERS * 16
    assert ctypes.sizeof(_lib.AdvanceRaggedSrc) == 24 + 5 * 8 + (1 + _lib.HOP_MAX_GROUPS) * ctypes.sizeof(_lib.RaggedSeq)
    doc = header[header.index("sfsn_fullband_hop_advance with a backlog of ITS OWN LENGTH"):
                 header.index("typedef struct sfsn_fullband_advance_ragged_src")]
    for word in ("h[k & 1]", "hist_ri[k & 1]", "row N_b - 1", "membrane", "N_b < D keeps the tail", "[0, N_b)", "384 + 128 N_b",
                 "WITHOUT A CALL", "ONE HOP LATER", "384 + 128 (N_b + 1)", "[0, Nmax]", "N_b / hop", "no atomics", "SFSN_EUNSUPPORTED",
                 "SFSN_EINVAL", "without an ABI bump"):
        assert word in doc, word
    from spiking_fullsubnet_amd.fullband_streaming import FullbandStreamingSession as S
    for m in (S.catch_up_ragged, S.catch_up_wave_ragged):
        assert m.__doc__ and "ValueError" in m.__doc__
    assert "bit for bit" in S.catch_up_ragged.__doc__
    for name in ("prime", "prime_wave", "advance", "advance_wave", "advance_ragged", "advance_wave_ragged"):
        assert not hasattr(S, name)  # (the sibling's names stay the sibling's)


# ---- refusals of the entry point before any launch ---------------------------------------------------------------------------------
class RaggedDummy(Dummy):
    """tests/test_cirm_catchup_host.py's descriptor with a ragged source: every pointer a non-NULL, 64-byte-aligned number that is no
    device address -- a call that got as far as a launch could not succeed, so SFSN_EINVAL proves the return came before it."""

    def __init__(self, wave=False, counted=False, hop=1):
        super().__init__(wave=wave, counted=counted, hop=hop)
        r = self.rsrc = self.lib.FullbandAdvanceRaggedSrc()
        r.Bp, r.Nmax, r.b0, r.T, r.frames, r.stft_ri = 2, 2 * hop, 0, 2 + 2 * hop, self.P, self.P
        if wave:
            r.wave_stride, r.enh_ri, r.wave_ctx, r.wave_out, r.window = 384 + 128 * 2, self.P, self.P, self.P, self.P
        for l in range(3):
            r.layer[l].spikes_i8, r.layer[l].membrane = self.P, self.P

    def ragged(self, desc=True, clips=True, src=True, n=None):
        return getattr(self.L, NAME)(ctypes.byref(self.desc) if desc else None, self.slots, self.wstate, self.ola,
                                     self.arr() if clips else None, len(self.clips) if n is None else n,
                                     ctypes.byref(self.rsrc) if src else None, None)


P = Dummy.P
DEFECTS = [  # (waveform mode, the one defect: a path into the RaggedDummy and the value put there)
    (False, ("clips",), [0, 3]),              # an index outside [0, B)
    (False, ("clips",), [0, -1]),
    (False, ("clips",), [2, 2]),              # listed twice
    (False, ("clips",), [0, 1, 2, 0]),        # more clips than the session has
    (False, ("rsrc", "b0"), 1),               # b0 + n_clips > Bp
    (False, ("rsrc", "Bp"), 1),
    (False, ("rsrc", "b0"), -1),
    (False, ("rsrc", "Nmax"), 0),             # Nmax < hop
    (True, ("rsrc", "Nmax"), 0),              # ... in waveform mode too: the longest clip has a frame
    (False, ("rsrc", "Nmax"), -1),
    (False, ("rsrc", "T"), 3),                # T < D + Nmax
    (False, ("rsrc", "frames"), None),
    (False, ("rsrc", "frames"), P + 2),
    (False, ("rsrc", "stft_ri"), None),
    (False, ("rsrc", "stft_ri"), P + 4),
    (False, ("rsrc", "layer", 0, "spikes_i8"), None),
    (False, ("rsrc", "layer", 0, "spikes_i8"), P + 2),
    (False, ("rsrc", "layer", 2, "membrane"), None),
    (False, ("rsrc", "layer", 1, "membrane"), P + 8),
    (False, ("desc", "layer", 1, "c"), None),
    (False, ("desc", "layer", 2, "c"), P + 4),
    (False, ("desc", "layer", 0, "h", 0), None),  # (launch_index 4: the half launch 4 reads)
    (False, ("desc", "hist_ri", 0), None),
    (False, ("desc", "hist_ri", 0), P + 4),
    (True, ("desc", "clip_start"), None),     # the waveform launch takes every clip's kind and frame index from it
    (True, ("ola",), None),                   # one of wave_state / ola_state NULL
    (True, ("ola",), ctypes.c_void_p(P + 4)),
    (True, ("wstate",), ctypes.c_void_p(P + 2)),
    (True, ("rsrc", "wave_ctx"), None),
    (True, ("rsrc", "wave_ctx"), P + 2),
    (True, ("rsrc", "wave_stride"), 384 + 128 * 2 - 1),
    (True, ("rsrc", "wave_stride"), 0),
    (True, ("rsrc", "window"), None),
    (True, ("rsrc", "window"), P + 2),
    (True, ("rsrc", "enh_ri"), None),
    (True, ("rsrc", "enh_ri"), P + 4),
    (True, ("rsrc", "wave_out"), None),
    (True, ("rsrc", "wave_out"), P + 4),
]


@pytest.mark.parametrize("wave,path,value", DEFECTS, ids=[f"{'wave' if v else 'spec'}-{'.'.join(map(str, p))}-"
                                                           f"{x if not isinstance(x, ctypes.c_void_p) else x.value}" for v, p, x in DEFECTS])
def test_each_einval_returns_before_any_launch(wave, path, value):
    d = RaggedDummy(wave=wave)
    _set(d, path, value)
    assert d.ragged() == d.lib.SFSN_EINVAL


def test_nulls_counts_hop_multiples_and_unsupported():
    for wave in (False, True):
        d = RaggedDummy(wave=wave)
        E, U = d.lib.SFSN_EINVAL, d.lib.SFSN_EUNSUPPORTED
        assert d.ragged(desc=False) == E and d.ragged(clips=False) == E and d.ragged(src=False) == E
        assert d.ragged(n=0) == E and d.ragged(n=-1) == E
    d = RaggedDummy(hop=2)
    d.rsrc.Nmax = 3  # Nmax % hop
    assert d.ragged() == E
    d = RaggedDummy(hop=2)
    d.rsrc.Nmax, d.rsrc.T = 1, 8  # Nmax < hop
    assert d.ragged() == E
    # a descriptor the coverage check refuses; spike slots together with the waveform state: as sfsn_fullband_hop_advance
    for field, value in (("Hp", 336), ("B", 17), ("unshared", 1), ("F", 129)):
        d = RaggedDummy()
        setattr(d.desc, field, value)
        assert d.ragged() == d.advance() == U, field
    d = RaggedDummy(wave=True)
    d.desc.F = 321
    assert d.ragged() == d.advance() == U
    d = RaggedDummy(wave=True, counted=True)
    assert d.ragged() == d.advance() == U
    d = RaggedDummy(counted=True)
    d.slots = ctypes.c_void_p(P + 2)
    assert d.ragged() == d.advance() == E


# ---- the refusals of the two methods: all of them come before any device work, each beside the sibling's ---------------------------
def session(B=3, hop=2, waveform=False, calls=1):
    """A FullbandStreamingSession with the fields the argument checks read and no device behind it."""
    from spiking_fullsubnet_amd.fullband_streaming import FullbandStreamingSession
    s = object.__new__(FullbandStreamingSession)
    s.B, s.hop, s.F, s.dev = B, hop, 257, torch.device("cpu")
    s.waveform, s.host_io = waveform, False
    s.frames_done, s._calls = 0, calls
    s._clip_f0, s._clip_c0 = np.zeros(B, np.int64), np.zeros(B, np.int64)
    return s


def spectrum(n, N):
    return torch.zeros((n, 257, N), dtype=torch.complex64)


def raised(fn):
    try:
        fn()
    except Exception as e:  # noqa: BLE001
        return type(e), str(e)
    return None, None


def test_each_refusal_is_the_siblings():
    x, w = spectrum(3, 8), torch.zeros((3, 512))
    s, ws = session(), session(waveform=True, hop=1)
    # (the sibling's call, ours, how the sibling's text becomes ours)
    cases = [
        # the wrong kind of session
        (lambda: ws.catch_up(x), lambda: ws.catch_up_ragged(x, [2, 4, 8]), ("catch_up_wave(samples)", "catch_up_wave_ragged(samples, lengths)")),
        (lambda: s.catch_up_wave(w), lambda: s.catch_up_wave_ragged(w, [128, 256, 512]), None),
        # dtype, bins, device, rows != len(clips)
        (lambda: s.catch_up(x.real.contiguous()), lambda: s.catch_up_ragged(x.real.contiguous(), [2, 4, 8]), None),
        (lambda: s.catch_up(x[:, :100]), lambda: s.catch_up_ragged(x[:, :100], [2, 4, 8]), None),
        (lambda: s.catch_up(x.to("meta")), lambda: s.catch_up_ragged(x.to("meta"), [2, 4, 8]), None),
        (lambda: s.catch_up(x[:2]), lambda: s.catch_up_ragged(x[:2], [2, 4]), ("catch_up:", "catch_up_ragged:")),
        (lambda: s.catch_up(x[:2], clips=[1]), lambda: s.catch_up_ragged(x[:2], [2, 4], clips=[1]), ("catch_up:", "catch_up_ragged:")),
        (lambda: ws.catch_up_wave(w.double()), lambda: ws.catch_up_wave_ragged(w.double(), [128, 256, 512]), None),
        (lambda: ws.catch_up_wave(w.to("meta")), lambda: ws.catch_up_wave_ragged(w.to("meta"), [128, 256, 512]), None),
        (lambda: ws.catch_up_wave(w[:2]), lambda: ws.catch_up_wave_ragged(w[:2], [128, 256]), ("catch_up_wave:", "catch_up_wave_ragged:")),
        # the clip list: clip_indices' errors
        (lambda: s.catch_up(x[:1], clips=[3]), lambda: s.catch_up_ragged(x[:1], [2], clips=[3]), None),
        (lambda: s.catch_up(x[:2], clips=[1, 1]), lambda: s.catch_up_ragged(x[:2], [2, 4], clips=[1, 1]), ("catch_up:", "catch_up_ragged:")),
        (lambda: s.catch_up(x[:1], clips=[0.5]), lambda: s.catch_up_ragged(x[:1], [2], clips=[0.5]), None),
        (lambda: s.catch_up(x[:0], clips=[]), lambda: s.catch_up_ragged(x[:0], [], clips=[]), ("catch_up:", "catch_up_ragged:")),
        (lambda: ws.catch_up_wave(w[:1], clips=[-1]), lambda: ws.catch_up_wave_ragged(w[:1], [128], clips=[-1]), None),
        (lambda: ws.catch_up_wave(w[:2], clips=[0, 0]), lambda: ws.catch_up_wave_ragged(w[:2], [128, 256], clips=[0, 0]),
         ("catch_up_wave:", "catch_up_wave_ragged:")),
        (lambda: ws.catch_up_wave(w[:1], clips=[True]), lambda: ws.catch_up_wave_ragged(w[:1], [128], clips=[True]), None),
        # a tensor's width that is no multiple of 128
        (lambda: ws.catch_up_wave(w[:, :200]), lambda: ws.catch_up_wave_ragged(w[:, :200], [128, 128, 128]),
         ("catch_up_wave:", "catch_up_wave_ragged:")),
    ]
    for i, (theirs, ours, swap) in enumerate(cases):
        (t_type, t_text), (o_type, o_text) = raised(theirs), raised(ours)
        assert t_type is not None and o_type is t_type, (i, t_type, o_type, o_text)
        assert o_text == (t_text.replace(*swap) if swap else t_text), (i, t_text, o_text)
    assert raised(cases[0][0])[0] is RuntimeError and raised(cases[1][0])[0] is RuntimeError and raised(cases[2][0])[0] is RuntimeError
    # a length that the single-clip call would refuse for its tensor: the same words, naming the clip (of the session, not the row)
    for hop in (1, 2, 3):
        s = session(hop=hop)
        for N in (0, 1, 2, 3, 4, 5, 7):
            t_type, t_text = raised(lambda: s.catch_up(spectrum(1, N), clips=[2]) if N % hop or N < hop else None)
            o_type, o_text = raised(lambda: s.catch_up_ragged(spectrum(2, 12), [N, 12], clips=[2, 0]) if N % hop or N < hop else None)
            assert o_type is t_type and (t_type is None or (t_type is ValueError and o_text == t_text.replace("catch_up: ", "catch_up_ragged: clip 2: ")))
    for Ls in (0, 64, 200):
        t_type, t_text = raised(lambda: ws.catch_up_wave(torch.zeros((1, Ls)), clips=[1]))
        o_type, o_text = raised(lambda: ws.catch_up_wave_ragged(w[:2], [Ls, 512], clips=[1, 2]))
        assert t_type is o_type is ValueError and o_text == t_text.replace("catch_up_wave: ", "catch_up_wave_ragged: clip 1: ")
    s = session()
    # a wrong count of lengths; above the tensor's; not integers; a device tensor
    with pytest.raises(ValueError, match="2 lengths for 3 clips"):
        s.catch_up_ragged(x, [2, 4])
    with pytest.raises(ValueError, match="3 lengths for 2 clips"):
        s.catch_up_ragged(x[:2], [2, 4, 8], clips=[2, 0])
    with pytest.raises(ValueError, match=r"clip 1\b.*10 frames.*hold 8"):
        s.catch_up_ragged(x, [2, 10, 8])
    with pytest.raises(ValueError, match=r"clip 2\b.*640 samples.*hold 512"):
        ws.catch_up_wave_ragged(w, [128, 256, 640])
    with pytest.raises(ValueError, match="not an integer"):
        s.catch_up_ragged(x, [2, 4.0, 8])
    with pytest.raises(ValueError, match="CPU"):
        s.catch_up_ragged(x, torch.tensor([2, 4, 8], device="meta"))
    # the two kinds of waveform clip in one call: catch_up_wave's ValueError, word for word
    mixed = session(waveform=True, hop=1)
    mixed._clip_c0[1] = 1  # clip 1 has made no call, clips 0 and 2 one
    t_type, t_text = raised(lambda: mixed.catch_up_wave(w))
    o_type, o_text = raised(lambda: mixed.catch_up_wave_ragged(w, [128, 256, 512]))
    assert t_type is o_type is ValueError and o_text == t_text and "clip 1" in t_text and "clip 0" in t_text
    o_type, o_text = raised(lambda: mixed.catch_up_wave_ragged(w[:2], [512, 256], clips=[2, 1]))
    assert o_type is ValueError and o_text == raised(lambda: mixed.catch_up_wave(w[:2], clips=[2, 1]))[1]
    # nothing above moved a clip
    assert s.clip_frames().tolist() == [0, 0, 0] and ws.clip_calls().tolist() == [1, 1, 1] and mixed.clip_calls().tolist() == [1, 0, 1]


# ---- the per-clip gather of the hand-back launch, restated --------------------------------------------------------------------------
def test_each_clip_takes_the_spike_and_membrane_row_of_its_own_last_frame():
    rng = np.random.default_rng(13)
    Nmax, B, H = 12, 4, 8
    x = rng.standard_normal((Nmax, B, H)).astype(F32)
    c0 = rng.standard_normal((B, H)).astype(F32)
    mem, spk, c_end = toy_scan(x, c0)
    h, c = take_rows(mem, spk, [Nmax] * B)  # N_b = N: sfsn_fullband_hop_advance's rows -- the last frame's spikes and c_state
    np.testing.assert_array_equal(h, spk[Nmax - 1])
    np.testing.assert_array_equal(c, c_end)
    lens = [1, 5, 12, 8]
    xp = x.copy()
    for b, n in enumerate(lens):
        xp[n:, b] = 0  # (the padding as the session writes it)
    memp, spkp, c_pad = toy_scan(xp, c0)
    h, c = take_rows(memp, spkp, lens)
    for b, n in enumerate(lens):
        m1, s1, c1 = toy_scan(x[:n, b:b + 1], c0[b:b + 1])
        np.testing.assert_array_equal(h[b], s1[n - 1, 0])
        np.testing.assert_array_equal(c[b], c1[0])
        assert n == Nmax or not np.array_equal(c_pad[b], c1[0])  # the scan's own end state is not the clip's
        assert int(spkp[:n, b].sum()) == int(s1.sum())             # the counts run over [0, N_b) only
    # the per-kernel tier's index into the [T][n][.] buffers: frame D + N_b - 1
    D = 2
    full = np.concatenate([np.full((D, B, H), np.nan, F32), memp])
    np.testing.assert_array_equal(full[np.asarray(lens) + D - 1, np.arange(B)], c)


def history_steps(hist, new, D):
    """What single steps leave: shift by one, append."""
    want = hist.copy()
    for t in range(new.shape[-1]):
        want = np.concatenate([want[..., 1:], new[..., t:t + 1]], -1)
    return want


@pytest.mark.parametrize("D", [1, 2, 4])
def test_history_composition_at_each_clips_own_end(D):
    rng = np.random.default_rng(20 + D)
    Nmax = 3 * D + 2
    hist = rng.standard_normal((5, D)).astype(F32)
    new = rng.standard_normal((5, Nmax)).astype(F32)
    buf = np.concatenate([hist, new], -1)
    np.testing.assert_array_equal(history_ragged(buf, D, Nmax, D), history_steps(hist, new, D))  # N_b = N
    for n_b in sorted({1, max(D - 1, 1), D, D + 1, Nmax - 1}):
        padded = buf.copy()
        padded[..., D + n_b:] = np.nan  # (what lies behind the clip's end is never read)
        got = history_ragged(padded, D, n_b, D)
        np.testing.assert_array_equal(got, history_steps(hist, new[..., :n_b], D))
        # the launch's own index: frame d <- frame T - Nmax + N_b - D + d
        T = D + Nmax
        np.testing.assert_array_equal(got, np.stack([padded[..., T - Nmax + n_b - D + d] for d in range(D)], -1))
        if n_b < D:  # the tail of the old history stays in front
            np.testing.assert_array_equal(got[..., :D - n_b], hist[..., n_b:])
            np.testing.assert_array_equal(got[..., D - n_b:], new[..., :n_b])
    # the per-kernel tier keeps D + hop frames: the window that ends with the clip's own last frame (N_b >= hop: the row has them)
    for hop in (1, 2):
        Th = D + hop
        for n_b in range(hop, Nmax + 1, hop):
            np.testing.assert_array_equal(buf[..., D + n_b - Th:D + n_b][..., hop:], history_steps(hist, new[..., :n_b], D))


def state_window(row, n_b, nocall, stride):
    """The launch's window: the 512 samples that end at 384 + 128 N_b -- one hop later for the clip without a call -- held inside the row."""
    end = min(384 + 128 * (n_b + int(nocall)), stride)
    assert end - 512 >= 0
    return row[end - 512:end]


def test_the_stft_state_window_of_both_kinds_of_clip():
    rng = np.random.default_rng(6)
    cmax = 6
    smp = rng.standard_normal(128 * cmax).astype(F32)
    # a clip that has made a call: [384 of its STFT state | new samples], c_b calls = c_b frames
    ctx = rng.standard_normal(384).astype(F32)
    row = np.concatenate([ctx, smp])
    for c in range(1, cmax + 1):
        got = state_window(row, c, False, len(row))
        np.testing.assert_array_equal(got, np.concatenate([ctx, smp[:128 * c]])[-512:])  # catch_up_wave's tail of a backlog of c calls
    # a clip without a call: [384 zeros | new samples], c_b calls = c_b - 1 frames, and the state ends 128 c_b samples into the row
    row0 = np.concatenate([np.zeros(384, F32), smp])
    for c in range(1, cmax + 1):
        got = state_window(row0, c - 1, True, len(row0))
        np.testing.assert_array_equal(got, np.concatenate([np.zeros(384, F32), smp[:128 * c]])[-512:])
        if c == 1:  # no frame at all: what the first call alone leaves -- 384 zeros, then its 128 samples
            np.testing.assert_array_equal(got, np.concatenate([np.zeros(384, F32), smp[:128]]))
    # frame j of such a clip is the centred frame j + 3 of the row: it ends with sample 128 (j + 2) of the new ones, inside the clip
    for c in range(2, cmax + 1):
        assert 128 * ((c - 2) + 1) + 512 - 384 == 128 * c
    # a frame count past the row (a wrong array): the window stays inside
    assert len(state_window(row0, cmax, True, len(row0))) == 512


def ola_feed(age, n_max, n_b):
    """The launch's loop for a clip of frame index ``age`` at its first new frame (0: fresh; -1: no call yet, its first new frame is
    frame 0 too): the carried sums unless fresh, then the clip's own frames in ascending order; blocks N_b .. Nmax - 1 are written as
    zeros (None).  A block is muted while the frame index is < 2.  (outputs per block, what the accumulator holds afterwards.)"""
    fresh = age <= 0
    fi0 = 0 if fresh else age
    acc = {j: ([] if fresh or j == 3 else [("carry", j)]) for j in range(4)}
    outputs = []
    for t in range(n_max):
        if t >= n_b:
            outputs.append(None)
            continue
        for j in range(4):
            acc[j] = acc[j] + [(fi0 + t, j)]
        outputs.append(acc[0] if fi0 + t >= 2 else "muted")
        acc = {0: acc[1], 1: acc[2], 2: acc[3], 3: []}
    return outputs, acc


@pytest.mark.parametrize("age", [-1, 0, 1, 2, 3, 6])
def test_the_overlap_add_recurrence_stops_at_each_clips_own_last_frame(age):
    n_max = 19
    whole, left_whole = ola_feed(age, n_max, n_max)
    assert None not in whole
    for n_b in ([0] if age == -1 else []) + [1, 2, 3, 4, 5, 18]:
        outputs, left = ola_feed(age, n_max, n_b)
        # over its own frames the clip's blocks are those of the longer run: the recurrence is causal
        assert outputs[:n_b] == whole[:n_b] and outputs[n_b:] == [None] * (n_max - n_b)
        # ... and what stays in the accumulator is what a run that ends there leaves: frames N_b - 3 .. N_b - 1, the carried sums while
        # they have not left yet
        assert left == ola_feed(age, n_b, n_b)[1]
        first = max(age, 0)
        assert left[0] == ([("carry", n_b)] if age > 0 and n_b < 3 else []) + [(first + t, n_b - t) for t in range(max(n_b - 3, 0), n_b)]
        assert left[3] == []
    # a fresh clip and a clip without a call carry nothing in: their first frames are muted like an utterance's
    for a in (-1, 0):
        out, _ = ola_feed(a, 4, 4)
        assert out[:2] == ["muted", "muted"] and out[2] == [(0, 2), (1, 1), (2, 0)]
    assert ola_feed(-1, 5, 0) == ([None] * 5, {0: [], 1: [], 2: [], 3: []})  # no frame: zeros to the accumulator


@pytest.mark.parametrize("hop", [1, 2])
@pytest.mark.parametrize("k", [0, 5, 2 ** 31 + 3, 2 ** 32 - 3])
def test_each_origin_moves_back_by_its_own_launches(k, hop):
    from spiking_fullsubnet_amd.fullband_streaming import FullbandStreamingSession as S
    ages = [0, 1, 7, 40]
    lens = [n * hop for n in (1, 17, 40, 9)]
    orgs = [(k - a) % (1 << 32) for a in ages]
    # the session's operation: an int32 tensor minus an int32 tensor of the clips' own launch counts, wrapping
    i32 = torch.tensor([S._as_i32(o) for o in orgs], dtype=torch.int32)
    for i in range(4):
        i32[i:i + 1].sub_(torch.tensor(lens, dtype=torch.int32)[i:i + 1] // hop)
    for a, n, got in zip(ages, lens, i32.tolist()):
        assert age_at(k, got % 2 ** 32) == a + n // hop and age_at((k + 3) % 2 ** 32, got % 2 ** 32) == a + n // hop + 3
        assert got % 2 ** 32 != k  # never again the launch that reads the state as zero
    if hop == 1:  # waveform mode: a clip without a call (age -1) moves back by its calls, one more than its frames
        for calls in (1, 2, 9):
            org = (k + 1) % (1 << 32)
            t = torch.tensor([S._as_i32(org)], dtype=torch.int32)
            t.sub_(torch.tensor([(calls - 1) + 1], dtype=torch.int32))
            assert age_at(k, int(t[0]) % 2 ** 32) == calls - 1  # the frame index of its next call's frame
