"""Ragged batches: clips of different lengths, zero-padded into one batch, each computed as if it ran alone.

The model is causal, so frames ``t < T_b`` of a padded clip are already those of the clip alone; what depends on where a clip
ends sits at the edges of the path (inverse STFT, the offline norms' statistics, spike counts) and takes per-clip lengths through
the ``*_ragged`` calls of the C ABI (``csrc/sfsn_ragged.hip``).  This module holds the host side: the length checks, the upload,
and the per-clip views of what a ragged forward returns.

``T_b = 1 + L_b // hop`` is the frame count of a clip of ``L_b`` samples (``torch.stft(center=True)``).

Entry points: ``model.forward_ragged(waves, lengths)``, ``model.forward_stft(stft, frames=...)``,
``Separator.norm_stats(x, lengths=...)``; per-clip results: ``clip_layers``.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from .engine import SpikeSummary


def _as_ints(values, what: str) -> List[int]:
    if torch.is_tensor(values):
        if values.device.type != "cpu":
            raise ValueError(f"{what}: expected a sequence or a CPU int tensor (a device tensor would cost a synchronisation), "
                             f"got a tensor on {values.device}")
        if values.dim() != 1 or values.dtype.is_floating_point or values.dtype.is_complex or values.dtype == torch.bool:
            raise ValueError(f"{what}: expected a 1-D integer tensor, got {values.dtype} {tuple(values.shape)}")
        values = values.tolist()
    out = []
    for b, v in enumerate(values):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{what}[{b}] = {v!r} is not an integer")
        out.append(int(v))
    return out


def frames_of(lengths: Sequence[int], hop: int) -> List[int]:
    """Frame counts of clips of the given lengths in samples: ``T_b = 1 + L_b // hop``."""
    return [1 + int(L) // hop for L in lengths]


def check_lengths(lengths, batch: int, max_len: int, hop: int, gaussian: bool = False) -> List[int]:
    """The clips' lengths in samples as a list of ints; ``ValueError`` naming the clip for a wrong count, ``L_b < 1``,
    ``L_b > max_len`` or -- ``gaussian``: offline_gaussian_norm's unbiased deviation needs two frames -- ``L_b < hop``."""
    lens = _as_ints(lengths, "lengths")
    if len(lens) != batch:
        raise ValueError(f"lengths: expected one length per clip ({batch}), got {len(lens)}")
    for b, L in enumerate(lens):
        if L < 1 or L > max_len:
            raise ValueError(f"lengths[{b}] = {L}: clip {b} must have between 1 and {max_len} samples (the padded length)")
        if gaussian and L < hop:
            raise ValueError(f"lengths[{b}] = {L}: clip {b} is shorter than one hop ({hop} samples), a single frame -- "
                             "offline_gaussian_norm's standard deviation needs two")
    return lens


def check_frames(frames, batch: int, max_frames: int, gaussian: bool = False) -> List[int]:
    """The clips' frame counts as a list of ints; ``ValueError`` naming the clip for a wrong count, ``T_b < 1``, ``T_b > max_frames``
    or (``gaussian``) ``T_b < 2``."""
    fr = _as_ints(frames, "frames")
    if len(fr) != batch:
        raise ValueError(f"frames: expected one frame count per clip ({batch}), got {len(fr)}")
    for b, T in enumerate(fr):
        if T < 1 or T > max_frames:
            raise ValueError(f"frames[{b}] = {T}: clip {b} must have between 1 and {max_frames} frames (the padded batch's)")
        if gaussian and T < 2:
            raise ValueError(f"frames[{b}] = {T}: clip {b} has a single frame -- offline_gaussian_norm's standard deviation needs two")
    return fr


def upload(values: Sequence[int], device) -> torch.Tensor:
    """int32 device tensor of the values (any nesting ``torch.tensor`` takes), copied from pinned memory on the current stream:
    no host synchronisation."""
    return torch.tensor(values, dtype=torch.int32).pin_memory().to(device, non_blocking=True)


class ClipSpikeSummary(SpikeSummary):
    """What ``layer_outputs="counts"`` puts in place of one spike tensor of a ragged batch: per-clip spike counts ``counts`` [B]
    (int64, on the device), each over the clip's own ``frames[b]`` frames, and the shape ``(T, R, H)`` the padded tensor has.
    ``clip(b)`` is the ``SpikeSummary`` the clip-alone forward returns: clip b's count, shape ``(T_b, R / B, H)``.  As a whole it
    reads as a ``SpikeSummary`` of the batch's valid part: ``count`` is the total, ``rate()`` its mean over the valid elements."""

    def __init__(self, counts: torch.Tensor, shape, frames: Sequence[int]):
        self.counts, self.shape, self.frames = counts, torch.Size(shape), tuple(int(t) for t in frames)
        if self.shape[1] % len(self.frames):
            raise ValueError(f"{self.shape[1]} rows do not divide into {len(self.frames)} clips")
        self.rows_per_clip = self.shape[1] // len(self.frames)

    @property
    def count(self) -> torch.Tensor:
        return self.counts.sum()

    def numel(self) -> int:  # valid elements only
        return sum(self.frames) * self.rows_per_clip * self.shape[2]

    def clip(self, b: int) -> SpikeSummary:
        return SpikeSummary(self.counts[b], (self.frames[b], self.rows_per_clip, self.shape[2]))

    def __repr__(self):
        return f"ClipSpikeSummary(shape={tuple(self.shape)}, clips={len(self.frames)})"


def clip_layers(fb_all, sb_all, b: int, lengths_or_frames, hop: Optional[int] = None):
    """Clip b's ``(fb_all, sb_all)`` of a ragged forward, in the form the forward of that clip alone returns.

    ``lengths_or_frames``: the clips' frame counts -- or, with ``hop=``, their lengths in samples (``T_b = 1 + L_b // hop``).

    * ``layer_outputs="tensors"``: every entry ``[T, B * n, C]`` becomes the view ``[:T_b, b * n:(b + 1) * n]``.  (The frames
      ``>= T_b`` of the batch's tensors are left as the model computed them on the padding -- spikes of a network fed zeros, not
      zeros: slice before averaging, which is what this function does.)
    * ``layer_outputs="counts"``: every ``ClipSpikeSummary`` becomes ``clip(b)``, a ``SpikeSummary`` with clip b's count and shape
      ``(T_b, n, H)``, so ``metric.compute_synops`` / ``compute_neuronops`` give clip b's numbers unchanged.
    * ``None`` entries (``layer_outputs="none"``) stay ``None``.
    """
    vals = _as_ints(lengths_or_frames, "lengths_or_frames")
    frames = vals if hop is None else frames_of(vals, hop)
    B = len(frames)
    if not 0 <= b < B:
        raise IndexError(f"clip {b} of a batch of {B}")
    Tb = frames[b]

    def one(x):
        if x is None:
            return None
        if isinstance(x, ClipSpikeSummary):
            if x.frames != tuple(frames):
                raise ValueError(f"the summary was counted with frames {x.frames}, not {tuple(frames)}")
            return x.clip(b)
        if isinstance(x, SpikeSummary):
            raise ValueError("a SpikeSummary of a whole batch has no per-clip counts: run the forward with frames= / forward_ragged")
        T, R = x.shape[0], x.shape[1]
        if R % B or Tb > T:
            raise ValueError(f"a [{T}, {R}, ...] tensor does not hold {B} clips with {Tb} frames in clip {b}")
        n = R // B
        return x[:Tb, b * n:(b + 1) * n]

    return [one(x) for x in fb_all], [[one(x) for x in outs] for outs in sb_all]
