"""``ClipState``: the carried state of some clips of a streaming session, outside the session.

``session.export_state(clips)`` returns one; ``other.import_state(state, clips)`` puts its rows into slots of the same or another
session, where the clips continue bit for bit (``streaming.StreamingSession``, ``fullband_streaming.FullbandStreamingSession``).  A
state is a ``uint8`` blob ``[n, bytes]`` -- one self-contained row per clip -- plus what the host keeps per clip: the frames (waveform
sessions: the calls) of its utterance and, for a frozen model with given statistics, its ``NormStats`` rows.

Blob layouts.  Every section starts at a multiple of 16 bytes; ``sections()`` names them.

* One-launch tier: the layout ``include/sfsn.h`` states for ``sfsn_hop_state_export`` / ``sfsn_fullband_hop_state_export``, written and
  read by one launch (``csrc/sfsn_state.hip``) and free of launch parity.  Spiking-FullSubNet: ``fb.l0.h``, ``fb.l0.c``, ... ,
  ``sb0.l0.h``, ... (int8 ``[units][H]`` last spikes, float32 ``[units][H]`` membranes per sequence and layer), ``cum`` (running sums
  of the cumulative norm, all sequences), ``slots`` (spike counts, all sequences and layers), ``hist`` (the last ``D`` noisy frames of
  the covered bins), ``wave`` (the last 512 samples), ``ola`` (``[S][512]`` overlap-add sums).  cIRM-GSN: ``l0.h``, ``l0.c``, ... ,
  ``slots``, ``hist``, ``wave``, ``ola``.
* Per-kernel tier (``StreamingSession`` with ``one_launch=False``) and graph tier (``FullbandStreamingSession``): the clip's rows of
  everything a later step reads before it writes, gathered and scattered with stream-ordered tensor copies -- per sequence and layer
  the float32 ``(h, c)`` rows ``[units][H]`` (``fb.l0.h`` ...; cIRM: ``l0.h`` ... of width ``Hp``), ``hist`` (complex64
  ``[F][D + hop]``, the session's whole window) and, when the session counts, ``rows`` (int64 per layer).  The int8 spike rings
  (``s8``) are not carried: a step writes its ``hop`` frames of them before anything reads them, and the recurrence takes the last
  spikes from ``h``.

A state moves only between sessions of equal ``signature`` (model kind, every geometry number, tier, hop, waveform, counting, norm
kind): ``check_signature`` raises a ``ValueError`` that names the first difference.  WEIGHTS ARE NOT PART OF THE SIGNATURE: importing a
clip into a session of another model of the same geometry is the caller's decision (an A/B of two checkpoints on one call, say).

All attributes are tensors, numpy arrays and tuples: ``torch.save(state, f)`` / ``torch.load(f, weights_only=False)`` round-trip it.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from .clip_select import clip_indices


def _pad16(n: int) -> int:
    return (n + 15) // 16 * 16


def layout_of(sizes: Sequence[Tuple[str, int]]) -> Tuple[Tuple[Tuple[str, int, int], ...], int]:
    """``((name, start, stop), ...), bytes`` of sections of the given sizes laid out in order, each at a multiple of 16."""
    out, off = [], 0
    for name, n in sizes:
        off = _pad16(off)
        out.append((name, off, off + n))
        off += n
    return tuple(out), _pad16(off)


def hop_sections(seqs, cum: bool, counted: bool, fcov: int, D: int, wave: bool, S: int):
    """Sections of ``sfsn_hop_state_export``'s blob.  ``seqs``: ``(name, units, H, layers)`` per sequence, full-band first."""
    sizes = []
    for name, units, H, nl in seqs:
        for l in range(nl):
            sizes += [(f"{name}.l{l}.h", units * H), (f"{name}.l{l}.c", units * H * 4)]
    if cum:  # (each sequence's sums start at a multiple of 16; the section spans them all)
        sizes.append(("cum", sum(_pad16(units * 4) for _, units, _, _ in seqs[:-1]) + seqs[-1][1] * 4))
    if counted:
        sizes.append(("slots", sum(units * H * nl for _, units, H, nl in seqs)))
    if D > 0 and fcov > 0:
        sizes.append(("hist", fcov * D * 8))
    if wave:
        sizes += [("wave", 2048), ("ola", S * 2048)]
    return layout_of(sizes)


def fullband_sections(nl: int, Hp: int, counted: bool, F: int, D: int, wave: bool, S: int):
    """Sections of ``sfsn_fullband_hop_state_export``'s blob."""
    sizes = []
    for l in range(nl):
        sizes += [(f"l{l}.h", Hp), (f"l{l}.c", Hp * 4)]
    if counted:
        sizes.append(("slots", nl * Hp))
    if D > 0:
        sizes.append(("hist", F * D * 8))
    if wave:
        sizes += [("wave", 2048), ("ola", S * 2048)]
    return layout_of(sizes)


def gather_rows(parts, sel: torch.Tensor, nbytes: int, layout) -> torch.Tensor:
    """The per-kernel tiers' export: ``parts`` = ``(name, t)`` with ``t`` a ``[B, n]`` view of a session tensor; rows ``sel`` of each,
    as bytes, at the section's place of a new ``[len(sel), nbytes]`` blob.  Stream-ordered copies, no synchronisation."""
    blob = torch.zeros((sel.numel(), nbytes), dtype=torch.uint8, device=sel.device)
    for (name, t), (lname, a, b) in zip(parts, layout):
        assert name == lname
        blob[:, a:b] = t.index_select(0, sel).contiguous().view(torch.uint8).view(sel.numel(), -1)
    return blob


def scatter_rows(parts, sel: torch.Tensor, blob: torch.Tensor, layout) -> None:
    """The per-kernel tiers' import: the inverse of ``gather_rows`` (rows of ``blob`` into rows ``sel`` of every tensor)."""
    for (name, t), (lname, a, b) in zip(parts, layout):
        assert name == lname
        t.index_copy_(0, sel, blob[:, a:b].contiguous().view(t.dtype).view(sel.numel(), -1))


def clip_list(clips, B: int, what: str):
    """Clip indices of an export / import / backlog call: ``clip_select.clip_indices``, distinct, at least one, caller's order."""
    return clip_indices(clips, B, what, duplicates="refuse", empty="refuse")


def new_blob(n: int, nbytes: int, layout, device) -> torch.Tensor:
    """The ``[n, nbytes]`` blob an export launch writes: no fill launch in front of it where the sections tile the row; the padding
    between sections reads as zero."""
    alloc = torch.empty if sum(b - a for _, a, b in layout) == nbytes else torch.zeros
    return alloc((n, nbytes), dtype=torch.uint8, device=device)


class ClipState:
    """``len(state)`` clips' state.  ``blob`` uint8 ``[n, bytes]``; ``frames`` int64 ``[n]`` (numpy), the frames of each clip's utterance;
    ``calls`` int64 ``[n]`` or None, waveform sessions' calls; ``stats`` None or the clips' statistics as a tuple
    ``(mu_fb, mu_sb, sd_fb, sd_sb)`` of tensors / None on the blob's device; ``signature`` a tuple of ``(field, value)`` pairs;
    ``layout`` a tuple of ``(section, start, stop)``."""

    def __init__(self, blob: torch.Tensor, frames, calls, stats, signature, layout):
        if not torch.is_tensor(blob) or blob.dtype != torch.uint8 or blob.dim() != 2:
            raise TypeError("ClipState: blob is a uint8 tensor [n, bytes]")
        self.blob = blob
        self.frames = np.asarray(frames, dtype=np.int64).reshape(-1).copy()
        self.calls = None if calls is None else np.asarray(calls, dtype=np.int64).reshape(-1).copy()
        self.stats = None if stats is None else tuple(stats)
        self.signature = tuple((str(k), v) for k, v in signature)
        self.layout = tuple((str(n), int(a), int(b)) for n, a, b in layout)
        n = blob.shape[0]
        if self.frames.shape[0] != n or (self.calls is not None and self.calls.shape[0] != n):
            raise ValueError(f"ClipState: {n} blob rows, {self.frames.shape[0]} frame counts")
        if self.stats is not None and any(t is not None and t.shape[-1] != n for t in self.stats):
            raise ValueError(f"ClipState: statistics of another number of clips than the {n} blob rows")

    def __len__(self) -> int:
        return self.blob.shape[0]

    @property
    def device(self) -> torch.device:
        return self.blob.device

    def sections(self) -> Dict[str, Tuple[int, int]]:
        """``{name: (start, stop)}``: the byte range of every section inside one clip's blob row."""
        return {n: (a, b) for n, a, b in self.layout}

    def select(self, rows) -> "ClipState":
        """The state of rows ``rows`` (a sequence of row indices, in that order); a copy."""
        idx = [int(i) for i in (rows.tolist() if isinstance(rows, (torch.Tensor, np.ndarray)) else rows)]
        bad = [i for i in idx if not 0 <= i < len(self)]
        if bad:
            raise IndexError(f"row {bad[0]} out of range for a state of {len(self)} clips")
        sel = torch.tensor(idx, dtype=torch.long).to(self.blob.device, non_blocking=True)
        stats = None if self.stats is None else tuple(None if t is None else t.index_select(-1, sel) for t in self.stats)
        return ClipState(self.blob.index_select(0, sel), self.frames[idx], None if self.calls is None else self.calls[idx], stats,
                         self.signature, self.layout)

    def to(self, device) -> "ClipState":
        """The state on ``device``: ``"cpu"`` parks the clips in host memory, a HIP device brings them back or moves them to another
        GPU.  (The copy to the host blocks, as ``Tensor.to`` does; the way back is stream-ordered.)"""
        device = torch.device(device)
        stats = None if self.stats is None else tuple(None if t is None else t.to(device) for t in self.stats)
        return ClipState(self.blob.to(device), self.frames, self.calls, stats, self.signature, self.layout)

    def clone(self) -> "ClipState":
        stats = None if self.stats is None else tuple(None if t is None else t.clone() for t in self.stats)
        return ClipState(self.blob.clone(), self.frames, self.calls, stats, self.signature, self.layout)

    def check_signature(self, signature) -> None:
        """``ValueError`` naming the first field in which ``signature`` (a session's) differs from this state's."""
        mine, theirs = dict(self.signature), dict((str(k), v) for k, v in signature)
        for k in list(mine) + [k for k in theirs if k not in mine]:
            if k not in mine or k not in theirs or mine[k] != theirs[k]:
                raise ValueError(f"import_state: the state's {k} ({mine.get(k, 'absent')!r}) differs from the session's "
                                 f"({theirs.get(k, 'absent')!r}); a state moves only between sessions of equal signature")

    def __repr__(self) -> str:
        return f"ClipState({len(self)} clips x {self.blob.shape[1]} bytes on {self.blob.device}, frames={self.frames.tolist()})"


def check_import(state, idx, dev, what: str = "import_state") -> None:
    """The refusals every session's import shares: type, device, row count."""
    if not isinstance(state, ClipState):
        raise TypeError(f"{what}: expected a ClipState, got {type(state).__name__}")
    dev = torch.device(dev)
    same = state.device.type == dev.type and (dev.type == "cpu" or dev.index is None or state.device.index is None or
                                               state.device.index == dev.index)
    if not same:
        raise RuntimeError(f"{what}: the state is on {state.device}, the session on {dev}: call state.to({str(dev)!r}) first")
    if len(state) != len(idx):
        raise RuntimeError(f"{what}: a state of {len(state)} clips for {len(idx)} clip indices")


def import_clips(state, clips, B: int, dev, signature, layout, nbytes: int) -> list:
    """What every session's ``import_state`` does first: the clip indices (``clip_list``), then the refusals in their order -- the
    state's type, device and row count, its signature against the session's, its blob layout against the session's."""
    idx = clip_list(clips, B, "import_state")
    check_import(state, idx, dev)
    state.check_signature(signature)
    if state.layout != layout or state.blob.shape[1] != nbytes:
        raise ValueError("import_state: the state's blob layout is not this session's")
    return idx
