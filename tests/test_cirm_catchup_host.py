"""CPU checks behind tests/test_cirm_catchup.py (``FullbandStreamingSession.catch_up`` / ``catch_up_wave``, ``sfsn_fullband_hop_seed`` /
``sfsn_fullband_hop_advance``): the exports, the index arithmetic of a backlog restated in numpy -- which frames of [history | new]
become the session's history, and the origin of a continued clip in uint32 with the launch counter near 2^32, the waveform clip
without a call (age -1) and more calls than launches made -- and every ``SFSN_EINVAL`` of the two entry points, each called with
otherwise valid dummy arguments and exactly one defect, so that it returns before any launch.  numpy and the library's host side only."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAMES = {"sfsn_fullband_hop_seed": 7, "sfsn_fullband_hop_advance": 8}
PINNED = ("prime", "prime_wave", "advance", "advance_wave")


def test_the_entry_points_are_exported_and_declared():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "sfsn.h")).read()
    for name, nargs in NAMES.items():
        assert name in _lib.EXPORTS and hasattr(L, name)
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl, f"{name} is not declared in sfsn.h"
        fn = getattr(L, name)
        assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == len(fn.argtypes) == nargs
        assert fn.restype is ctypes.c_int
    # new functions alone do not bump the version
    assert re.search(r"#define\s+SFSN_ABI_VERSION\s+21\b", header) and _lib.ABI_VERSION == 21 and L.sfsn_abi_version() == 21
    # the ctypes mirrors: four ints, two pointers, four layers of two pointers; four ints, five pointers, four layers of two pointers
    assert ctypes.sizeof(_lib.FullbandSeedDst) == 16 + 2 * 8 + _lib.FULLBAND_HOP_MAX_LAYERS * 16
    assert ctypes.sizeof(_lib.FullbandAdvanceSrc) == 16 + 5 * 8 + _lib.FULLBAND_HOP_MAX_LAYERS * 16
    doc = header[header.index("sfsn_fullband_hop_seed: the offline kernels' START tensors"):header.index("typedef struct sfsn_fullband_seed_dst")]
    for word in ("h[k & 1]", "hist_ri[k & 1]", "ADDED to", "wave_tail", "N < D keeps the tail", "k + 1", "no layer-0 reservation", "SFSN_EUNSUPPORTED"):
        assert word in doc, word


def test_the_session_has_the_new_methods_and_none_of_the_pinned_names():
    from spiking_fullsubnet_amd import fullband_streaming as fs
    cls = fs.FullbandStreamingSession
    for name in ("catch_up", "catch_up_wave"):
        assert callable(getattr(cls, name)) and "bit for bit" in getattr(cls, name).__doc__.lower()
    for name in PINNED:  # (tests/test_stream_prime.py, test_stream_advance.py and test_cirm_migrate.py pin their absence)
        assert not hasattr(cls, name) and name not in cls.__dict__
    assert "__getattr__" not in cls.__dict__
    assert "catch_up" in fs.__doc__ and "have no ``prime``" not in fs.__doc__ and "no ``prime``" not in cls.export_state.__doc__


# ---- the history a backlog leaves -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 4])
def test_history_composition(D):
    rng = np.random.default_rng(D)
    hist = rng.standard_normal((3, 5, D)).astype(F32)
    for N in sorted({1, max(D - 1, 1), D, D + 1}):
        new = rng.standard_normal((3, 5, N)).astype(F32)
        T = D + N
        buf = np.concatenate([hist, new], -1)  # [history | new], the launch's source rows
        got = np.stack([buf[..., T - D + d] for d in range(D)], -1)  # adv_hist: frame d <- frame T - D + d
        want = hist.copy()
        for t in range(N):  # what N single steps leave: shift by one, append
            want = np.concatenate([want[..., 1:], new[..., t:t + 1]], -1)
        np.testing.assert_array_equal(got, want)
        if N < D:  # the tail of the old history stays in front
            np.testing.assert_array_equal(got[..., :D - N], hist[..., N:])
            np.testing.assert_array_equal(got[..., D - N:], new)
        else:
            np.testing.assert_array_equal(got, new[..., N - D:])


# ---- origins ----------------------------------------------------------------------------------------------------------------------
def age_at(k, org):
    """The launch's frame index of a clip: (int)(k - clip_start), an unsigned difference read as int32."""
    d = (k - org) % (1 << 32)
    return d - (1 << 32) if d >= 1 << 31 else d


@pytest.mark.parametrize("k", [0, 1, 5, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 3, 2 ** 32 - 1])
def test_origin_arithmetic_wraps(k):
    from spiking_fullsubnet_amd.fullband_streaming import FullbandStreamingSession as S
    for age in (-1, 0, 1, 7, 2 ** 31 - 5):  # -1: the waveform clip whose first call is launch k
        org = (k - age) % (1 << 32)
        assert age_at(k, org) == age
        for back in (1, 2, 9, 1250) + ((k + 1, k + 77) if k <= 5 else ()):  # launches replaced; more of them than launches made so far
            if age + back + 7 >= 2 ** 31:
                continue  # (a frame index is an int32)
            new = (org - back) % (1 << 32)
            assert age_at(k, new) == age + back and age_at((k + 7) % 2 ** 32, new) == age + back + 7
            assert age_at(k, new) >= 0  # never again the launch that reads the state as zero, nor a first call
            # what the session does: a subtraction on the int32 tensor that holds the origins, wrapping like the hardware's
            i32 = np.array([S._as_i32(org)], dtype=np.int32)
            with np.errstate(over="ignore"):
                i32 -= np.array(back % (1 << 32), dtype=np.uint32).astype(np.int32)
            assert int(i32[0]) % 2 ** 32 == new
    # the kernels' rule for "reads as zero": the unsigned distance origin - k is at most span (1 in waveform mode: k and k + 1)
    for span in (0, 1):
        for age in (-2, -1, 0, 1, 5):
            fresh = ((k - age) % 2 ** 32 - k) % 2 ** 32 <= span
            assert fresh == (age == 0 or (span == 1 and age == -1))


# ---- refusals before any launch ---------------------------------------------------------------------------------------------------
class Dummy:
    """A descriptor the coverage checks accept and argument structs whose every pointer is a non-NULL, 64-byte-aligned number that is
    no device address: a call that got as far as a launch could not succeed, so SFSN_EINVAL proves the return came before it."""
    P = 1 << 20

    def __init__(self, wave=False, counted=False, hop=1):
        from spiking_fullsubnet_amd import _lib
        self.lib, self.L, self.wave = _lib, _lib.lib(), wave
        d = self.desc = _lib.FullbandHopDesc()
        d.n_layers, d.Hp, d.B, d.F, d.S, d.df, d.hop, d.D, d.act, d.unshared = 3, 32, 3, 257, 1, 3, hop, 2, 0, 0
        assert self.L.sfsn_fullband_hop_check(d.Hp, d.n_layers, d.F, d.S, d.df, d.B, d.hop, d.D, 0) == _lib.SFSN_OK
        for l in range(3):
            d.layer[l].h[0], d.layer[l].h[1], d.layer[l].c = self.P, self.P, self.P
        d.hist_ri[0], d.hist_ri[1], d.clip_start, d.launch_index = self.P, self.P, self.P, 4
        self.slots = ctypes.c_void_p(self.P) if counted else None
        self.wstate = ctypes.c_void_p(self.P) if wave else None
        self.ola = ctypes.c_void_p(self.P) if wave else None
        self.clips = [0, 2]
        dst = self.dst = _lib.FullbandSeedDst()
        dst.Bp, dst.T, dst.b0, dst.wave_stride, dst.stft_ri = 2, 2 + 2 * hop, 0, 384 + 256, self.P
        dst.wave_ctx = self.P if wave else None
        src = self.src = _lib.FullbandAdvanceSrc()
        src.Bp, src.N, src.b0, src.T, src.stft_ri = 2, 2 * hop, 0, 2 + 2 * hop, self.P
        if wave:
            src.enh_ri, src.wave_tail, src.wave_out, src.window = self.P, self.P, self.P, self.P
        for l in range(3):
            dst.layer[l].h, dst.layer[l].c = self.P, self.P
            src.layer[l].spikes_i8, src.layer[l].c = self.P, self.P

    def arr(self):
        return (ctypes.c_int * max(len(self.clips), 1))(*self.clips)

    def seed(self, desc=True, clips=True, dst=True, n=None):
        return self.L.sfsn_fullband_hop_seed(ctypes.byref(self.desc) if desc else None, self.slots, self.wstate, self.arr() if clips else None,
                                             len(self.clips) if n is None else n, ctypes.byref(self.dst) if dst else None, None)

    def advance(self, desc=True, clips=True, src=True, n=None):
        return self.L.sfsn_fullband_hop_advance(ctypes.byref(self.desc) if desc else None, self.slots, self.wstate, self.ola,
                                                self.arr() if clips else None, len(self.clips) if n is None else n,
                                                ctypes.byref(self.src) if src else None, None)


def _set(obj, path, value):
    for name in path[:-1]:
        obj = getattr(obj, name) if isinstance(name, str) else obj[name]
    if isinstance(path[-1], str):
        setattr(obj, path[-1], value)
    else:
        obj[path[-1]] = value


# (which call, waveform mode, the one defect: a path into the Dummy and the value put there)
DEFECTS = [
    ("both", False, ("clips",), [0, 3]),            # an index outside [0, B)
    ("both", False, ("clips",), [0, -1]),
    ("both", False, ("clips",), [2, 2]),            # listed twice
    ("seed", False, ("dst", "b0"), 1),              # b0 + n_clips > Bp
    ("seed", False, ("dst", "Bp"), 1),
    ("seed", False, ("dst", "b0"), -1),
    ("advance", False, ("src", "b0"), 1),
    ("advance", False, ("src", "Bp"), 1),
    ("advance", False, ("src", "N"), 0),            # N < hop
    ("advance", False, ("src", "N"), -1),
    ("advance", True, ("src", "N"), -1),            # waveform mode: N < 0
    ("advance", False, ("src", "T"), 3),            # T < D + N
    ("seed", False, ("dst", "T"), 1),               # T < D
    ("seed", True, ("dst", "wave_stride"), 383),
    ("seed", True, ("dst", "wave_ctx"), None),
    ("seed", True, ("desc", "clip_start"), None),   # the waveform launches take every frame index from it
    ("advance", True, ("desc", "clip_start"), None),
    ("advance", True, ("ola",), None),              # one of wave_state / ola_state NULL
    ("advance", True, ("src", "wave_tail"), None),
    ("advance", True, ("src", "window"), None),
    ("advance", True, ("src", "enh_ri"), None),
    ("advance", True, ("src", "wave_out"), None),
    ("seed", False, ("dst", "stft_ri"), None),
    ("advance", False, ("src", "stft_ri"), None),
    ("seed", False, ("dst", "layer", 1, "h"), None),
    ("seed", False, ("dst", "layer", 2, "c"), None),
    ("advance", False, ("src", "layer", 0, "spikes_i8"), None),
    ("advance", False, ("src", "layer", 2, "c"), None),
    ("both", False, ("desc", "layer", 1, "c"), None),
    ("both", False, ("desc", "layer", 0, "h", 0), None),  # (launch_index 4: the half launch 4 reads)
    ("both", False, ("desc", "hist_ri", 0), None),
    # misalignment: h, c 16 bytes; stft_ri, enh_ri, wave_out, ola_state 8; the others 4
    ("seed", False, ("dst", "layer", 0, "h"), Dummy.P + 8),
    ("seed", False, ("dst", "layer", 0, "c"), Dummy.P + 8),
    ("advance", False, ("src", "layer", 0, "c"), Dummy.P + 8),
    ("advance", False, ("src", "layer", 0, "spikes_i8"), Dummy.P + 2),
    ("both", False, ("desc", "layer", 2, "c"), Dummy.P + 4),
    ("both", False, ("desc", "hist_ri", 0), Dummy.P + 4),
    ("seed", False, ("dst", "stft_ri"), Dummy.P + 4),
    ("advance", False, ("src", "stft_ri"), Dummy.P + 4),
    ("advance", True, ("src", "enh_ri"), Dummy.P + 4),
    ("advance", True, ("src", "wave_out"), Dummy.P + 4),
    ("advance", True, ("ola",), ctypes.c_void_p(Dummy.P + 4)),
    ("advance", True, ("src", "wave_tail"), Dummy.P + 2),
    ("seed", True, ("dst", "wave_ctx"), Dummy.P + 2),
    ("seed", True, ("wstate",), ctypes.c_void_p(Dummy.P + 2)),
]


@pytest.mark.parametrize("which,wave,path,value", DEFECTS, ids=[f"{w}-{'wave' if v else 'spec'}-{'.'.join(map(str, p))}-{x if not isinstance(x, ctypes.c_void_p) else x.value}"
                                                                 for w, v, p, x in DEFECTS])
def test_each_einval_returns_before_any_launch(which, wave, path, value):
    d = Dummy(wave=wave)
    _set(d, path, value)
    EINVAL = d.lib.SFSN_EINVAL
    if which in ("seed", "both"):
        assert d.seed() == EINVAL
    if which in ("advance", "both"):
        assert d.advance() == EINVAL


def test_nulls_counts_hop_multiples_and_unsupported():
    for wave in (False, True):
        d = Dummy(wave=wave)
        E, U = d.lib.SFSN_EINVAL, d.lib.SFSN_EUNSUPPORTED
        for fn, arg in ((d.seed, "dst"), (d.advance, "src")):
            assert fn(desc=False) == E and fn(clips=False) == E and fn(**{arg: False}) == E
            assert fn(n=0) == E and fn(n=-1) == E
    d = Dummy(hop=2)
    d.src.N = 3  # N % hop
    assert d.advance() == d.lib.SFSN_EINVAL
    d = Dummy(hop=2)
    d.src.N, d.src.T = 1, 8  # N < hop
    assert d.advance() == d.lib.SFSN_EINVAL
    # a descriptor the coverage check refuses; spike slots together with the waveform state
    for field, value in (("Hp", 336), ("B", 17), ("unshared", 1), ("F", 129)):
        d = Dummy()
        setattr(d.desc, field, value)
        assert d.seed() == U and d.advance() == U, field
    d = Dummy(wave=True)
    d.desc.F = 321
    assert d.seed() == U and d.advance() == U
    d = Dummy(wave=True, counted=True)
    assert d.seed() == U and d.advance() == U
    d = Dummy(counted=True)
    d.slots = ctypes.c_void_p(Dummy.P + 2)
    assert d.seed() == d.lib.SFSN_EINVAL and d.advance() == d.lib.SFSN_EINVAL
