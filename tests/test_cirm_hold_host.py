"""CPU checks behind tests/test_cirm_hold.py (``FullbandStreamingSession.tick`` / ``tick_wave`` / ``tick_wave_host``,
``sfsn_fullband_stream_hop_held`` / ``sfsn_fullband_stream_hop_wave_held``): the exports and their ctypes mirrors, the contract's
wording in include/sfsn.h, the mask's refusals -- each answered by an argument check on a descriptor of host addresses, before any
device query -- the session's new names, and the one mask word ``clip_select.held_masks`` makes for a batch the hop kernel takes.
The library's host side only."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELD, WAVE_HELD = "sfsn_fullband_stream_hop_held", "sfsn_fullband_stream_hop_wave_held"
PINNED = ("prime", "prime_wave", "advance", "advance_wave")
P = 1 << 20  # a non-NULL, 64-byte-aligned number that is no device address


def test_the_entry_points_are_exported_and_declared_without_an_abi_bump():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "sfsn.h")).read()
    want = {HELD: [ctypes.POINTER(_lib.FullbandHopDesc), ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p],
            WAVE_HELD: [ctypes.POINTER(_lib.FullbandWaveDesc), ctypes.c_uint, ctypes.c_void_p]}
    for name, argtypes in want.items():
        assert name in _lib.EXPORTS and hasattr(L, name)
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl, f"{name} is not declared in sfsn.h"
        fn = getattr(L, name)
        assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == len(fn.argtypes) == len(argtypes)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == argtypes
    assert re.search(r"#define\s+SFSN_ABI_VERSION\s+21\b", header) and _lib.ABI_VERSION == 21 and L.sfsn_abi_version() == 21
    # the contract is in the header: every row of the per-row rules, the origin rule, the return codes
    doc = header[header.index("The cIRM-GSN hop with HELD clips"):header.index("int " + HELD)]
    for word in ("h[(k + 1) & 1] row <- the bytes of h[k & 1] row", "not written", "not added to, nor zeroed", "every tile gathers all rows",
                 "hist_ri[(k + 1) & 1] rows <- hist_ri[k & 1] rows", "no shift", "D == 0", "written as zero", "with their tag",
                 "not shifted", "does not take the samples", "not touched", "a host that spins on the words returns",
                 "clip_start[b] += 1", "Nobody waits", "word 3", "kernel arguments", "NaN included", "no wait is added",
                 "held_mask == 0 IS the existing launch", "SFSN_EINVAL", "the plain launch's code", "sfsn_fullband_hop_scratch_bytes stays 64"):
        assert word in doc, word
    # the sibling's header points here (and keeps the words tests/test_stream_hold_host.py looks for)
    sib = header[header.index("sfsn_stream_hop with HELD clips"):header.index("int sfsn_stream_hop_held")]
    assert HELD in sib


def covered(B=3, hop=1):
    from spiking_fullsubnet_amd import _lib
    d = _lib.FullbandHopDesc()
    d.n_layers, d.Hp, d.B, d.F, d.S, d.df, d.hop, d.D, d.act, d.unshared = 3, 32, B, 257, 1, 3, hop, 2, 0, 0
    d.clip_start = P
    return d


def wave_of(d):
    from spiking_fullsubnet_amd import _lib
    w = _lib.FullbandWaveDesc()
    ctypes.memmove(ctypes.byref(w.hop), ctypes.byref(d), ctypes.sizeof(d))
    return w


def test_the_masks_refusals_are_answered_without_a_device():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    EINVAL, EUNSUP = _lib.SFSN_EINVAL, _lib.SFSN_EUNSUPPORTED
    held = lambda d, mask, slots=None: L.sfsn_fullband_stream_hop_held(None if d is None else ctypes.byref(d), slots, mask, None)  # noqa: E731
    wheld = lambda w, mask: L.sfsn_fullband_stream_hop_wave_held(None if w is None else ctypes.byref(w), mask, None)  # noqa: E731
    for B in (1, 3, 16):
        d = covered(B)
        assert L.sfsn_fullband_hop_check(d.Hp, d.n_layers, d.F, d.S, d.df, d.B, d.hop, d.D, 0) == _lib.SFSN_OK
        for mask in (1 << B, 1 | 1 << B, 1 << 31, 0xFFFFFFFF):  # a bit at or beyond B
            assert held(d, mask) == EINVAL and held(d, mask, ctypes.c_void_p(P)) == EINVAL and wheld(wave_of(d), mask) == EINVAL, (B, mask)
        d.clip_start = None  # a held clip needs an origin of its own
        for mask in (1, (1 << B) - 1):
            assert held(d, mask) == EINVAL and wheld(wave_of(d), mask) == EINVAL, (B, mask)
    for mask in (1, 1 << 15):  # a NULL descriptor
        assert held(None, mask) == EINVAL and wheld(None, mask) == EINVAL
    # a descriptor the plain launch refuses gets the plain launch's code, with and without a bit set
    seen = set()
    cases = [covered(B=17), covered(hop=31), covered()]
    cases[2].D = 1  # D != df - 1
    for d in cases:
        want = L.sfsn_fullband_stream_hop(ctypes.byref(d), None)
        assert want in (EINVAL, EUNSUP)  # (an argument check: nothing was launched)
        assert L.sfsn_fullband_stream_hop_counted(ctypes.byref(d), ctypes.c_void_p(P), None) == want
        for mask in (0, 1, 2):
            assert held(d, mask) == want and held(d, mask, ctypes.c_void_p(P)) == want, mask
            assert held(d, mask, ctypes.c_void_p(P + 2)) == (EINVAL if mask == 0 else want)  # (the plan answers before the slots are looked at)
        seen.add(want)
    assert seen == {EINVAL, EUNSUP}
    w = wave_of(covered(B=17))
    assert wheld(w, 1) == L.sfsn_fullband_stream_hop_wave(ctypes.byref(w), None) == wheld(w, 0) == EUNSUP
    # held_mask == 0 IS the plain launch: its refusals, NULL descriptor included
    assert held(None, 0) == L.sfsn_fullband_stream_hop(None, None) == EINVAL and wheld(None, 0) == EINVAL
    # misaligned spike slots on a descriptor the plan accepts
    assert held(covered(), 1, ctypes.c_void_p(P + 2)) == EINVAL
    assert L.sfsn_fullband_hop_scratch_bytes(ctypes.byref(covered())) == 64


def test_the_session_has_the_three_methods_and_none_of_the_pinned_names():
    from spiking_fullsubnet_amd import fullband_streaming as fs
    cls = fs.FullbandStreamingSession
    for name, first in (("tick", "frames"), ("tick_wave", "samples"), ("tick_wave_host", "samples")):
        m = getattr(cls, name)
        params = list(inspect.signature(m).parameters)
        assert params[:3] == ["self", first, "clips"] and "held" in m.__doc__.lower(), name
    assert list(inspect.signature(cls.tick).parameters)[3] == "copy" and list(inspect.signature(cls.tick_wave_host).parameters)[3] == "timeout_s"
    # step* keep their signatures (tests/test_stream_hold.py pins `step`)
    assert list(inspect.signature(cls.step).parameters) == ["self", "frames", "copy"]
    assert list(inspect.signature(cls.step_wave).parameters) == ["self", "samples", "copy"]
    assert list(inspect.signature(cls.step_wave_host).parameters) == ["self", "samples", "timeout_s"]
    for name in PINNED:
        assert not hasattr(cls, name) and name not in cls.__dict__
    assert "__getattr__" not in cls.__dict__
    assert "tick_wave_host" in fs.__doc__ and "held" in fs.__doc__.lower() and HELD in fs.__doc__


@pytest.mark.parametrize("B", [1, 3, 16])
def test_the_mask_of_a_batch_the_hop_kernel_takes_is_one_word(B):
    from spiking_fullsubnet_amd.clip_select import held_masks
    lists = [[], [0], [B - 1], list(range(B)), list(range(0, B, 2)), list(range(1, B, 2)), [B - 1, 0, 0]]
    for active in lists:
        got_active, held, words = held_masks(active, B, [(0, B)], "tick")
        assert got_active == sorted(set(active)) and held == [b for b in range(B) if b not in active]
        assert len(words) == 1 and len(words[0]) == 1
        assert words[0][0] == ((1 << B) - 1) & ~sum(1 << b for b in set(active))  # the complement of the active list
        assert words[0][0] >> B == 0  # no bit at or beyond B: what the launch refuses
    with pytest.raises(ValueError, match=rf"tick: clip index {B} out of range for a session of {B} clips"):
        held_masks([0, B], B, [(0, B)], "tick")
    for wrong in ([0.5], [True], "0", 1):
        with pytest.raises(TypeError):
            held_masks(wrong, B, [(0, B)], "tick")
