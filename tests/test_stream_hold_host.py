"""CPU checks behind tests/test_stream_hold.py (``step(frames, clips=...)`` / ``step_wave`` / ``step_wave_host`` with held clips,
``sfsn_stream_hop_held``): the export and its declaration, every refusal that an argument check answers (no call below launches --
a descriptor that passes all checks is never handed to a launch entry point here), the per-part mask words against a numpy
restatement, the properties of THE hold schedule (tests/holdref.py) on the launches it really makes, and the origin arithmetic of a
held clip (+ 1 per hold, unsigned, across the 2^32 wrap) restated with ``primeref.origin`` / ``frame_index_at``.  numpy and the
library's host side only."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import holdref as hd
import primeref as pr
import refweights as rw
from test_stream_migrate_host import A, hop_desc  # descriptors the hop's plan accepts, built on the host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sfsn_stream_hop_held"


def words(*v):
    return (ctypes.c_uint64 * len(v))(*v)


# ---- the export ---------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_exported_and_declared_without_an_abi_bump():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "sfsn.h")).read()
    assert NAME in _lib.EXPORTS and hasattr(L, NAME)
    decl = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", header)
    assert decl, f"{NAME} is not declared in sfsn.h"
    fn = getattr(L, NAME)
    assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == len(fn.argtypes) == 3
    assert fn.restype is ctypes.c_int and fn.argtypes[1] is ctypes.POINTER(ctypes.c_uint64)
    # a new function alone does not bump the version, and no struct changed
    assert re.search(r"#define\s+SFSN_ABI_VERSION\s+21\b", header) and _lib.ABI_VERSION == 21 and L.sfsn_abi_version() == 21
    # the contract is in the header: what is and is not written, the origin rule, the return codes
    doc = header[header.index("sfsn_stream_hop with HELD clips"):header.index("int " + NAME)]
    for word in ("h[(k + 1) & 1] <- the bytes of h[k & 1]", "cum[(k + 1) & 1] <- cum[k & 1]", "not shifted", "not touched", "written as zero",
                 "done   written", "clip_start[b] += 1", "Nobody waits", "kernel arguments", "SFSN_EINVAL", "SFSN_EUNSUPPORTED", "NaN included"):
        assert word in doc, word
    from spiking_fullsubnet_amd.streaming import StreamingSession
    for m in (StreamingSession.step, StreamingSession.step_wave, StreamingSession.step_wave_host):
        assert "clips" in inspect.signature(m).parameters and inspect.signature(m).parameters["clips"].default is None
        assert "held" in m.__doc__.lower()


# ---- refusals: every call is answered by an argument check ------------------------------------------------------------------------
def launchable(**kw):
    """A descriptor that passes the plan and the scratch check (host addresses: it is only ever given to calls that an argument
    check on the mask refuses)."""
    d = hop_desc(rw.LIVE_TINY, **kw)
    d.scratch, d.scratch_bytes = A, 1 << 30
    return d


def test_a_descriptor_the_sibling_refuses_gets_the_siblings_code():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    no_scratch = hop_desc(rw.LIVE_TINY, B=3)  # scratch == NULL: SFSN_EINVAL
    no_scratch.clip_start = A
    small = launchable(B=3)
    small.scratch_bytes = 8
    no_input = launchable(B=3)
    no_input.inp_ri = None
    cases = [None, _lib.HopDesc(), hop_desc(rw.LIVE_TINY, hop=31), no_scratch, small, no_input]
    seen = set()
    for d in cases:
        ref = None if d is None else ctypes.byref(d)
        want = L.sfsn_stream_hop(ref, None)
        assert want in (_lib.SFSN_EINVAL, _lib.SFSN_EUNSUPPORTED)  # (an argument check: nothing was launched)
        for bits in (None, words(0), words(1), words(8)):
            assert L.sfsn_stream_hop_held(ref, bits, None) == want
        seen.add(want)
    assert seen == {_lib.SFSN_EINVAL, _lib.SFSN_EUNSUPPORTED}


def test_the_masks_own_refusals():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    EINVAL, EUNSUP = _lib.SFSN_EINVAL, _lib.SFSN_EUNSUPPORTED
    d = launchable(B=3)
    d.clip_start = A
    ref = ctypes.byref(d)
    assert L.sfsn_stream_hop_held(ref, words(1 << 3), None) == EINVAL            # bit B
    assert L.sfsn_stream_hop_held(ref, words(1 | 1 << 63), None) == EINVAL       # the word's last bit
    d65 = launchable(B=65)
    d65.clip_start = A
    assert L.sfsn_stream_hop_held(ctypes.byref(d65), words(0, 2), None) == EINVAL  # bit 65 of a 65-clip descriptor
    assert L.sfsn_stream_hop_held(ctypes.byref(d65), words(1, 1 << 5), None) == EINVAL
    # a held clip needs an origin of its own
    d0 = launchable(B=3)
    assert not d0.clip_start
    for bits in (words(1), words(7), words(2)):
        assert L.sfsn_stream_hop_held(ctypes.byref(d0), bits, None) == EINVAL
    # more clips than the argument block carries (256)
    big = launchable(B=257)
    big.clip_start = A
    assert L.sfsn_stream_hop_held(ctypes.byref(big), words(1, 0, 0, 0, 0), None) == EUNSUP
    assert L.sfsn_stream_hop_held(ctypes.byref(big), words(0, 0, 0, 0, 1), None) == EUNSUP


# ---- the mask words -------------------------------------------------------------------------------------------------------------
def masks_numpy(active, B, bounds):
    held = np.ones(B, dtype=bool)
    held[list(active)] = False
    out = []
    for b0, nb in bounds:
        bits = np.zeros(-(-nb // 64) * 64, dtype=np.uint8)
        bits[:nb] = held[b0:b0 + nb]
        out.append(np.packbits(bits, bitorder="little").view("<u8").tolist())
    return np.flatnonzero(held).tolist(), out


@pytest.mark.parametrize("B,bounds", [(3, [(0, 3)]), (3, [(0, 2), (2, 1)]), (64, [(0, 64)]), (64, [(0, 40), (40, 24)]), (65, [(0, 65)]),
                                      (65, [(0, 64), (64, 1)]), (65, [(0, 33), (33, 32)]), (130, [(0, 130)]), (130, [(0, 70), (70, 60)]),
                                      (130, [(0, 44), (44, 44), (88, 42)])])
def test_mask_words_against_numpy(B, bounds):
    from spiking_fullsubnet_amd.clip_select import held_masks
    rng = np.random.default_rng(B + len(bounds))
    cut = bounds[1][0] if len(bounds) > 1 else B // 2
    lists = [[], [0], [B - 1], list(range(B)), [max(cut - 1, 0)], [min(cut, B - 1)], [max(cut - 1, 0), min(cut, B - 1)],
             [b for b in range(B) if not bounds[0][0] <= b < bounds[0][0] + bounds[0][1]],           # the first part held as a whole
             [b for b in range(B) if b % 64 in (0, 63)], sorted(rng.choice(B, size=max(B // 3, 1), replace=False).tolist())]
    for active in lists:
        got_active, held, got = held_masks(active, B, bounds, "step")
        want_held, want = masks_numpy(active, B, bounds)
        assert got_active == sorted(set(active)) and held == want_held
        assert got == want, (active, bounds)
        assert [len(w) for w in got] == [-(-nb // 64) for _, nb in bounds]
        for (b0, nb), w in zip(bounds, got):  # no bit at or beyond the part's clips: what the launch refuses
            assert sum(x << (64 * i) for i, x in enumerate(w)) >> nb == 0
    # an empty list: everybody is held
    _, held, got = held_masks([], B, bounds, "step")
    assert held == list(range(B))
    assert [sum(x << (64 * i) for i, x in enumerate(w)) for w in got] == [(1 << nb) - 1 for _, nb in bounds]
    # duplicates are merged; tensors and arrays are taken
    import torch
    assert held_masks([1, 1, 0], B, bounds, "step")[0] == [0, 1]
    assert held_masks(torch.tensor([1, 0]), B, bounds, "step") == held_masks(np.array([0, 1]), B, bounds, "step") == held_masks([0, 1], B, bounds, "step")


def test_mask_errors_name_the_offending_index():
    from spiking_fullsubnet_amd.clip_select import held_masks
    import torch
    for bad, B in ((3, 3), (-1, 3), (130, 130), (64, 64)):
        with pytest.raises(ValueError, match=rf"clip index {bad} out of range for a session of {B} clips"):
            held_masks([0, bad], B, [(0, B)], "step")
    for wrong in ([0.0], [True], torch.tensor([0.5]), torch.zeros((1, 1), dtype=torch.long), "01", 1):
        with pytest.raises(TypeError):
            held_masks(wrong, 3, [(0, 3)], "step")


# ---- the schedule ---------------------------------------------------------------------------------------------------------------
def test_the_schedule_holds_every_clip_where_it_can_go_wrong():
    assert hd.B == 3 and 14 <= len(hd.TICKS) <= 18
    assert all(sorted(set(a)) == a and all(0 <= b < hd.B for b in a) for a in hd.TICKS)
    la = hd.launches()
    assert [k for _, k, _, _ in la] == list(range(len(la))) and len(la) == sum(1 for a in hd.TICKS if a)
    assert sum(1 for a in hd.TICKS if not a) == 1                                   # one tick advances nobody
    held_at = {b: [k for _, k, _, held in la if b in held] for b in range(hd.B)}
    for b in range(hd.B):
        assert any(k % 2 == 0 for k in held_at[b]) and any(k % 2 == 1 for k in held_at[b]), b   # both launch parities
        assert any(k + 1 in held_at[b] for k in held_at[b]), b                                     # two launches in a row
    assert held_at[0][:2] == [0, 1] and 0 not in la[0][2] and 0 not in la[1][2]     # clip 0: held before it has run
    (t_reset, who), = hd.RESET_BEFORE.items()
    assert who == [2] and t_reset == 10
    first_after = next(x for x in la if x[0] >= t_reset)
    assert 2 in first_after[3]                                                      # clip 2: held in the launch that would restart it
    D = max(pr.df_reach(n) for n in pr.FIXTURES)
    for b in range(hd.B):
        last = max(t for t, a in enumerate(hd.TICKS) if b not in a)
        assert all(b in a for a in hd.TICKS[last + 1:]) and len(hd.TICKS) - last - 1 >= D + 3, b
    # the feed: every clip takes its frames in order, one index per active tick; the control resets clip 2 at the matching call
    seen = [0] * hd.B
    for t, fed in hd.feed():
        assert sorted(fed) == hd.TICKS[t]
        for b, j in fed.items():
            assert j == seen[b]
            seen[b] += 1
    assert seen == hd.active_ticks() and len(set(seen)) == 1  # (a control of the same batch serves all three clips)
    assert hd.resets() == {2: sum(2 in a for a in hd.TICKS[:10])} and 0 < hd.resets()[2] < seen[2]
    assert pr.T >= 2 * max(seen) and pr.CALLS >= max(seen)    # the fixtures' inputs cover it at hop 2


@pytest.mark.parametrize("hop", [1, 2])
@pytest.mark.parametrize("k0", [0, 5, 2 ** 31 - 2, 2 ** 31 + 3, 2 ** 32 - 3, 2 ** 32 - 1])
def test_a_held_clips_origin_moves_on_by_one_launch(k0, hop):
    """The session's and the launch's arithmetic restated: clip_start[b] += 1 (unsigned) in a launch that holds b; a reset writes the
    next launch's index.  Then every launch gives an active clip the frame index = its active launches since its utterance began,
    whatever happened in between -- i.e. its origin is that of a clip primed with those frames at that launch."""
    M = 1 << 32
    org = [k0] * hd.B                      # a session whose next launch has index k0 (as after reset())
    age = [0] * hd.B                       # active launches of the clip's current utterance
    k = k0
    for t, active in enumerate(hd.TICKS):
        for b in hd.RESET_BEFORE.get(t, []):
            org[b], age[b] = k % M, 0      # (reset(clips): frame 0 is the next launch)
        if not active:
            continue                       # nothing is launched: no index is spent
        for b in range(hd.B):
            if b in active:
                assert pr.frame_index_at(k % M, org[b]) == age[b]
                assert pr.frame_index_at(k % M, org[b]) * hop == age[b] * hop       # frames_before of the cumulative norm
                age[b] += 1
            else:
                before = pr.frame_index_at(k % M, org[b])
                org[b] = (org[b] + 1) % M
                assert 0 <= org[b] < M and pr.frame_index_at((k + 1) % M, org[b]) == before == age[b]  # the next launch sees it where it was
                assert (age[b] == 0) == (org[b] == (k + 1) % M)                     # a restart that was due is due in the next launch
        k += 1
        for b in range(hd.B):
            assert org[b] == pr.origin(k % M, age[b] * hop, hop)
    assert age[:2] == hd.active_ticks()[:2] and age[2] == hd.active_ticks()[2] - hd.resets()[2]
    # the int32 tensor the session keeps the origins in: add_(1) wraps like the hardware's unsigned add
    from spiking_fullsubnet_amd.clip_select import as_i32
    for v in (0, 2 ** 31 - 1, 2 ** 32 - 1):
        i32 = np.array([as_i32(v)], dtype=np.int32)
        with np.errstate(over="ignore"):
            i32 += np.int32(1)
        assert int(i32[0]) % M == (v + 1) % M
