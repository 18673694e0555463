"""Host-side bookkeeping the streaming sessions share: which clips a call names, in which order its launches take them, which
stream-ordered fills / copies and which launch chunks that makes, and the argument checks of the calls that take recorded input.

Pure functions of lists and integers (torch only for ``isinstance`` and tensor attributes): no device work, no session object.
``streaming.StreamingSession`` and ``fullband_streaming.FullbandStreamingSession`` call them; tests/test_clip_select_host.py runs
them on the CPU.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch


def clip_indices(clips, B: int, what: str, *, duplicates: str, empty: str) -> List[int]:
    """The clip indices a call names, checked: ``clips`` is a sequence, a 1-D numpy array or a 1-D tensor of integers (no bools) in
    ``[0, B)``; ``None`` is every clip, ``list(range(B))``.

    ``duplicates``: ``"refuse"`` raises ``ValueError(f"{what}: clip indices must be distinct")`` and keeps the caller's order;
    ``"merge"`` returns ``sorted(set(...))``, and the range check sees the sorted indices; ``"merge_late"`` is ``"merge"`` with the
    range check on the caller's order (the ``IndexError`` names the first index out of range that the check meets).
    ``empty``: ``"ok"`` returns ``[]``; ``"refuse"`` raises ``ValueError(f"{what}: no clip selected")``.

    ==========================================  ==========  =============================  ============
    Call                                        Duplicates  Empty list                     Order
    ==========================================  ==========  =============================  ============
    ``reset(clips)``                            merge [1]_  no-op                          sorted
    ``set_norm_stats``                          refuse      return                         caller order
    ``prime*``, ``advance*``, ``catch_up*``,    refuse      ``"{what}: no clip selected"``  caller order
    ``export_state``, ``import_state``
    ``spike_summary`` (``what="clips"``)        merge       ``"clips: no clip selected"``   sorted
    ``step*(clips=)`` (``held_masks``) [2]_     merge       every clip is held             sorted
    ==========================================  ==========  =============================  ============

    .. [1] ``StreamingSession.reset``: ``merge_late``; ``FullbandStreamingSession.reset``: ``merge``.
    .. [2] ``merge_late``; an index out of range is re-raised as a ``ValueError`` with the same wording.
    """
    assert duplicates in ("refuse", "merge", "merge_late") and empty in ("ok", "refuse")
    if clips is None:
        return list(range(B))
    array = isinstance(clips, (torch.Tensor, np.ndarray))
    if (array and clips.ndim != 1) or isinstance(clips, (str, bytes)) or not hasattr(clips, "__iter__"):
        raise TypeError("clips: a 1-D tensor or a sequence of clip indices")
    items = clips.tolist() if array else list(clips)
    if any(isinstance(i, bool) or not isinstance(i, (int, np.integer)) for i in items):
        raise TypeError("clips: integer clip indices")
    idx = [int(i) for i in items]
    if duplicates == "merge":
        idx = sorted(set(idx))
    bad = [i for i in idx if not 0 <= i < B]
    if bad:
        raise IndexError(f"clip index {bad[0]} out of range for a session of {B} clips")
    if duplicates == "merge_late":
        idx = sorted(set(idx))
    elif len(set(idx)) != len(idx):
        raise ValueError(f"{what}: clip indices must be distinct")
    if not idx and empty == "refuse":
        raise ValueError(f"{what}: no clip selected")
    return idx


def slot_order(idx: Sequence[int]) -> Tuple[List[int], Optional[List[int]]]:
    """``(idx sorted, order)`` with ``sorted[j] == idx[order[j]]``; ``order`` is None where ``idx`` ascends already (the launches
    take clips in slot order: the caller's rows go through ``order`` first, the results through its inverse)."""
    order = sorted(range(len(idx)), key=idx.__getitem__)
    return [idx[j] for j in order], (None if order == list(range(len(idx))) else order)


def runs_by(indices: Sequence[int], keys: Sequence) -> List[tuple]:
    """``[(first, count, key), ...]``: ``indices`` cut into runs of consecutive ones (each its predecessor plus one) with equal
    ``keys`` -- one stream-ordered fill per run (clips that moved together share an age)."""
    out: List[list] = []
    for i, k in zip(indices, keys):
        if out and out[-1][0] + out[-1][1] == i and out[-1][2] == k:
            out[-1][1] += 1
        else:
            out.append([i, 1, k])
    return [tuple(r) for r in out]


def runs(ascending: Sequence[int]) -> List[Tuple[int, int]]:
    """``[(first, count), ...]``: runs of consecutive indices (one stream-ordered fill / copy per run)."""
    return [(first, count) for first, count, _ in runs_by(ascending, [None] * len(ascending))]


def part_runs(idx: Sequence[int], bounds: Sequence[Tuple[int, int]], limit: int = 256) -> List[Tuple[int, int, List[int]]]:
    """``[(part number, first position, local clip indices), ...]``: ``idx`` cut into runs of consecutive POSITIONS whose clips
    lie in one part (``bounds[p] = (b0, nb)``: part p holds the clips ``[b0, b0 + nb)``; local index = clip - b0), ``limit`` clips at
    most -- what one launch with clip indices in its arguments takes: consecutive rows of the caller's tensor, one part.  Every
    change of part starts a run; where ``idx`` ascends, a part's runs follow each other."""
    out: List[Tuple[int, int, List[int]]] = []
    for j, b in enumerate(idx):
        p = next(p for p, (b0, nb) in enumerate(bounds) if b0 <= b < b0 + nb)
        if out and out[-1][0] == p and len(out[-1][2]) < limit:
            out[-1][2].append(b - bounds[p][0])
        else:
            out.append((p, j, [b - bounds[p][0]]))
    return out


def held_masks(clips, B: int, bounds: Sequence[Tuple[int, int]], what: str) -> Tuple[List[int], List[int], List[List[int]]]:
    """``step(..., clips=)``: the clips that take this hop and the ones that are HELD, as ``(active, held, words)`` -- ``active`` =
    ``clips`` checked like ``reset(clips)``'s (duplicates merged, sorted), ``held`` = every other clip of the batch, ``words[p]`` = the
    mask ``sfsn_stream_hop_held`` takes for part p (``bounds[p] = (b0, nb)``, as for ``part_runs``): ``ceil(nb / 64)`` 64-bit words, bit
    ``b - b0`` of the part's mask set for a held clip b.  An empty list holds everybody (all-held masks).  An index out of range is a
    ``ValueError`` that names it (``clip_indices``' wording); a wrong type is ``clip_indices``' ``TypeError``."""
    # this runs in front of every tick's launch: a plain list of ints inside the batch -- the everyday call -- is taken without the
    # per-item checks (anything else goes through clip_indices, which raises what it always raises)
    active = sorted(set(clips)) if type(clips) is list and set(map(type, clips)) <= {int} else None
    if active is None or (active and not 0 <= active[0] <= active[-1] < B):
        try:
            active = clip_indices(clips, B, what, duplicates="merge_late", empty="ok")
        except IndexError as e:
            raise ValueError(f"{what}: {e}") from None
    held = sorted(set(range(B)).difference(active))
    mask = sum(1 << b for b in held)  # bit b = clip b is held
    words = [[((mask >> b0) & ((1 << nb) - 1)) >> (64 * i) & 0xFFFFFFFFFFFFFFFF for i in range((nb + 63) // 64)] for b0, nb in bounds]
    return active, held, words


def as_i32(v: int) -> int:
    """A launch index (uint32, wrapping) as the int32 a fill writes."""
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def check_frames(what: str, stft: torch.Tensor, n: int, F: int, dev, hop: int) -> int:
    """``stft``: recorded frames of ``n`` clips, complex64 [n, F, N] on ``dev`` with ``N`` a positive multiple of ``hop``; returns N."""
    if stft.device != dev or stft.dtype != torch.complex64 or stft.shape[1] != F:
        raise RuntimeError(f"expected complex64 {(n, F, 'N')} on {dev}, got {stft.dtype} {tuple(stft.shape)} on {stft.device}")
    N = stft.shape[2]
    if N < hop or N % hop != 0:
        raise ValueError(f"{what}: {N} frames is not a positive multiple of the session's hop ({hop})")
    return N


def clip_lengths(what: str, lengths, idx: Sequence[int], unit: int, unit_text: str, most: int, noun: str) -> List[int]:
    """The per-clip lengths of a ragged backlog (``advance_ragged``: ``noun`` = "frames", ``unit`` = the session's hop;
    ``advance_wave_ragged``: "samples", 128): a sequence or a CPU integer tensor with one value per listed clip ``idx[i]``, each a
    positive multiple of ``unit`` (``unit_text``: how the message names it) and at most ``most``, what the tensor's rows hold.
    ``ValueError`` naming the clip, in ``check_frames`` / ``check_samples``' wording for the same fault; returns the list of ints."""
    if torch.is_tensor(lengths):
        if lengths.device.type != "cpu":
            raise ValueError(f"{what}: the lengths are a sequence or a CPU integer tensor (a device tensor would cost a "
                             f"synchronisation), got a tensor on {lengths.device}")
        if lengths.dim() != 1 or lengths.dtype.is_floating_point or lengths.dtype.is_complex or lengths.dtype == torch.bool:
            raise ValueError(f"{what}: the lengths are a 1-D integer tensor, got {lengths.dtype} {tuple(lengths.shape)}")
        lengths = lengths.tolist()
    elif isinstance(lengths, (str, bytes)) or not hasattr(lengths, "__iter__"):
        raise ValueError(f"{what}: the lengths are a sequence or a CPU integer tensor with one value per clip")
    vals = list(lengths)
    if len(vals) != len(idx):
        raise ValueError(f"{what}: {len(vals)} lengths for {len(idx)} clips")
    out = []
    for b, v in zip(idx, vals):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{what}: clip {b}: the length {v!r} is not an integer")
        v = int(v)
        if v < unit or v % unit != 0:
            raise ValueError(f"{what}: clip {b}: {v} {noun} is not a positive multiple of {unit_text}")
        if v > most:
            raise ValueError(f"{what}: clip {b}: {v} {noun}, the tensor's rows hold {most}")
        out.append(v)
    return out


def check_samples(what: str, samples: torch.Tensor, n: int, dev) -> int:
    """``samples``: recorded samples of ``n`` clips, float32 [n, Ls] on ``dev`` with ``Ls`` a positive multiple of 128; returns Ls."""
    if samples.device != dev or samples.dtype != torch.float32:
        raise RuntimeError(f"expected float32 {(n, '128 * c')} on {dev}, got {samples.dtype} {tuple(samples.shape)} on {samples.device}")
    Ls = samples.shape[1]
    if Ls < 128 or Ls % 128 != 0:
        raise ValueError(f"{what}: {Ls} samples is not a positive multiple of 128")
    return Ls
