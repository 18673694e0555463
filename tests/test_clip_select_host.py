"""The host-side bookkeeping of the streaming sessions (spiking_fullsubnet_amd/clip_select.py), on the CPU: which clips a call names,
slot order, runs, launch chunks, the int32 form of a launch index and the argument checks of the calls that take recorded input."""
import numpy as np
import pytest
import torch

from spiking_fullsubnet_amd.clip_select import (as_i32, check_frames, check_samples, clip_indices, part_runs, runs, runs_by,
                                                slot_order)

B = 4
ONE_D = "clips: a 1-D tensor or a sequence of clip indices"
INTEGER = "clips: integer clip indices"

# the modes of clip_indices' table (what, duplicates, empty), and StreamingSession.reset's late merge
MODES = {"reset": ("reset", "merge", "ok"), "reset_late": ("reset", "merge_late", "ok"), "set_norm_stats": ("set_norm_stats", "refuse", "ok"),
         "prime": ("prime", "refuse", "refuse"), "spike_summary": ("clips", "merge", "refuse")}


def out_of_range(i):
    return IndexError, f"clip index {i} out of range for a session of {B} clips"


def expectations(what, duplicates, empty):
    """[(input, expected list or (exception type, message))] for one mode."""
    merge = duplicates != "refuse"
    nothing = [] if empty == "ok" else (ValueError, f"{what}: no clip selected")

    def pick(merged, kept):
        return merged if merge else kept

    return [
        ([2, 0], pick([0, 2], [2, 0])),
        ((3, 1), pick([1, 3], [3, 1])),
        (range(1, 4), [1, 2, 3]),
        (np.array([3, 0], dtype=np.int64), pick([0, 3], [3, 0])),
        (torch.tensor([1, 0]), pick([0, 1], [1, 0])),
        (torch.tensor([], dtype=torch.int64), nothing),
        (torch.zeros((1, 1), dtype=torch.long), (TypeError, ONE_D)),
        (np.zeros((2, 2), dtype=np.int64), (TypeError, ONE_D)),
        ("01", (TypeError, ONE_D)),
        (5, (TypeError, ONE_D)),
        ([True], (TypeError, INTEGER)),
        ([0.5], (TypeError, INTEGER)),
        ([-1], out_of_range(-1)),
        ([B], out_of_range(B)),
        ([0, B + 5], out_of_range(B + 5)),
        # two indices out of range: a merge in front of the range check meets the smallest first, every other mode the caller's first
        ([B + 5, -1], out_of_range(-1 if duplicates == "merge" else B + 5)),
        ([1, 1], pick([1], (ValueError, f"{what}: clip indices must be distinct"))),
        ([3, 1, 3], pick([1, 3], (ValueError, f"{what}: clip indices must be distinct"))),
        ([], nothing),
        (None, [0, 1, 2, 3]),
    ]


@pytest.mark.parametrize("mode", sorted(MODES))
def test_clip_indices_in_every_mode(mode):
    what, duplicates, empty = MODES[mode]
    for clips, want in expectations(what, duplicates, empty):
        if isinstance(want, list):
            got = clip_indices(clips, B, what, duplicates=duplicates, empty=empty)
            assert got == want and all(type(i) is int for i in got), (mode, clips, got)
        else:
            with pytest.raises(want[0]) as e:
                clip_indices(clips, B, what, duplicates=duplicates, empty=empty)
            assert type(e.value) is want[0] and str(e.value) == want[1], (mode, clips, str(e.value))


def test_clip_list_is_the_refusing_mode():
    from spiking_fullsubnet_amd.clip_state import clip_list
    for clips, want in expectations("export_state", "refuse", "refuse"):
        if isinstance(want, list):
            assert clip_list(clips, B, "export_state") == want
        else:
            with pytest.raises(want[0]) as e:
                clip_list(clips, B, "export_state")
            assert str(e.value) == want[1]


def test_slot_order():
    for idx in ([0], [0, 1, 2], [1, 5, 9]):
        assert slot_order(idx) == (idx, None)
    rng = np.random.default_rng(0)
    for n in (2, 3, 7, 40):
        idx = rng.permutation(100)[:n].tolist()
        if idx == sorted(idx):
            idx.reverse()
        ordered, order = slot_order(idx)
        assert ordered == sorted(idx) and ordered == [idx[j] for j in order]
        inv = np.empty(n, dtype=np.int64)
        inv[order] = np.arange(n)  # what the sessions do on the device
        rows = np.array(idx)
        assert (rows[order][inv] == rows).all() and sorted(order) == list(range(n))


def test_runs():
    assert runs([]) == [] and runs_by([], []) == []
    assert runs([7]) == [(7, 1)] and runs_by([7], ["a"]) == [(7, 1, "a")]
    assert runs([3, 4, 5, 6]) == [(3, 4)]
    assert runs([0, 2, 4]) == [(0, 1), (2, 1), (4, 1)]
    assert runs([0, 1, 2, 5, 6, 9]) == [(0, 3), (5, 2), (9, 1)]
    assert runs([5, 6, 2, 3]) == [(5, 2), (2, 2)]  # (consecutive means: the predecessor plus one)
    assert runs_by([0, 1, 2, 5, 6, 9], [4] * 6) == [(0, 3, 4), (5, 2, 4), (9, 1, 4)]
    # a key change inside a consecutive stretch starts a run; so does an index that is no successor, whatever its key
    assert runs_by([0, 1, 2, 3, 4], [7, 7, 8, 8, 7]) == [(0, 2, 7), (2, 2, 8), (4, 1, 7)]
    assert runs_by([2, 3, 3, 4], [1, 1, 1, 1]) == [(2, 2, 1), (3, 2, 1)]
    assert runs_by([4, 2, 3], [0, 0, -1]) == [(4, 1, 0), (2, 1, 0), (3, 1, -1)]


def removed_chunk_loop(idx, bounds, limit=256):
    """What the sessions' own loops over the parts produced for ascending ``idx``: per part the positions of its clips, in chunks."""
    out = []
    for p, (b0, nb) in enumerate(bounds):
        pos = [j for j, b in enumerate(idx) if b0 <= b < b0 + nb]
        for j0 in range(0, len(pos), limit):
            out.append((p, pos[j0], [idx[j] - b0 for j in pos[j0:j0 + limit]]))
    return out


def covered(result, bounds):
    return [bounds[p][0] + i for p, _, local in result for i in local]


def test_part_runs():
    bounds = [(0, 32), (32, 32), (64, 6)]
    idx = [0, 1, 5, 31, 32, 40, 63, 64, 69]
    got = part_runs(idx, bounds)
    assert got == [(0, 0, [0, 1, 5, 31]), (1, 4, [0, 8, 31]), (2, 7, [0, 5])]
    assert got == removed_chunk_loop(idx, bounds) and covered(got, bounds) == idx
    # the caller's order (export / import): every change of part starts a run, at the position where it happens
    idx = [33, 2, 3, 65, 64, 0, 40]
    got = part_runs(idx, bounds)
    assert got == [(1, 0, [1]), (0, 1, [2, 3]), (2, 3, [1, 0]), (0, 5, [0]), (1, 6, [8])]
    assert covered(got, bounds) == idx
    got = part_runs([69, 0, 32, 1], bounds)
    assert [r[:2] for r in got] == [(2, 0), (0, 1), (1, 2), (0, 3)] and covered(got, bounds) == [69, 0, 32, 1]
    # more clips of one part than a launch takes
    one = [(0, 600)]
    got = part_runs(list(range(600)), one)
    assert [(p, j0, len(local)) for p, j0, local in got] == [(0, 0, 256), (0, 256, 256), (0, 512, 88)]
    assert got == removed_chunk_loop(list(range(600)), one) and covered(got, one) == list(range(600))
    # ascending selections against the removed loop, chunk limits that cut inside parts included
    rng = np.random.default_rng(1)
    for bounds, limit in ((bounds, 256), (bounds, 5), ([(0, 300), (300, 300)], 256), ([(0, 7)], 3), ([(0, 1), (1, 1), (2, 1)], 256)):
        total = sum(nb for _, nb in bounds)
        for _ in range(20):
            idx = sorted(rng.permutation(total)[:rng.integers(1, total + 1)].tolist())
            got = part_runs(idx, bounds, limit)
            assert got == removed_chunk_loop(idx, bounds, limit) and covered(got, bounds) == idx
            assert all(idx[j0] == bounds[p][0] + local[0] and len(local) <= limit for p, j0, local in got)
    assert part_runs([], bounds) == []


def test_as_i32():
    for v, want in ((0, 0), (1, 1), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31, -2 ** 31), (2 ** 32 - 1, -1), (2 ** 32 + 5, 5), (-3, -3),
                    (-2 ** 31 - 1, 2 ** 31 - 1)):
        assert as_i32(v) == want and -2 ** 31 <= as_i32(v) < 2 ** 31
        assert as_i32(v) % 2 ** 32 == v % 2 ** 32
        assert int(np.array([as_i32(v)], dtype=np.int32).view(np.uint32)[0]) == v % 2 ** 32  # the word a fill writes


def test_check_frames():
    cpu, F, hop = torch.device("cpu"), 5, 2
    good = torch.zeros((3, F, 6), dtype=torch.complex64)
    assert check_frames("prime", good, 3, F, cpu, hop) == 6
    assert check_frames("advance", good[..., :2], 3, F, cpu, hop) == 2
    for bad in (good.to(torch.complex128), torch.zeros((3, F, 6)), torch.zeros((3, F + 1, 6), dtype=torch.complex64)):
        with pytest.raises(RuntimeError) as e:
            check_frames("prime", bad, 3, F, cpu, hop)
        assert str(e.value) == f"expected complex64 (3, {F}, 'N') on cpu, got {bad.dtype} {tuple(bad.shape)} on cpu"
    with pytest.raises(RuntimeError, match="on meta$"):
        check_frames("prime", good.to("meta"), 3, F, cpu, hop)
    for what, N in (("prime", 0), ("catch_up", 1), ("advance", 3), ("advance", 7)):
        with pytest.raises(ValueError) as e:
            check_frames(what, torch.zeros((3, F, N), dtype=torch.complex64), 3, F, cpu, hop)
        assert str(e.value) == f"{what}: {N} frames is not a positive multiple of the session's hop (2)"
    assert check_frames("prime", torch.zeros((1, F, 1), dtype=torch.complex64), 1, F, cpu, 1) == 1


def test_check_samples():
    cpu = torch.device("cpu")
    assert check_samples("prime_wave", torch.zeros((2, 128)), 2, cpu) == 128
    assert check_samples("advance_wave", torch.zeros((2, 640)), 2, cpu) == 640
    for bad in (torch.zeros((2, 128), dtype=torch.float64), torch.zeros((2, 128), dtype=torch.int16)):
        with pytest.raises(RuntimeError) as e:
            check_samples("prime_wave", bad, 2, cpu)
        assert str(e.value) == f"expected float32 (2, '128 * c') on cpu, got {bad.dtype} (2, 128) on cpu"
    with pytest.raises(RuntimeError, match="on meta$"):
        check_samples("prime_wave", torch.zeros((2, 128), device="meta"), 2, cpu)
    for what, Ls in (("prime_wave", 0), ("catch_up_wave", 100), ("advance_wave", 129), ("advance_wave", 383)):
        with pytest.raises(ValueError) as e:
            check_samples(what, torch.zeros((2, Ls)), 2, cpu)
        assert str(e.value) == f"{what}: {Ls} samples is not a positive multiple of 128"
