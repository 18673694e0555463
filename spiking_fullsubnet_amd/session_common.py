"""What ``streaming.StreamingSession`` and ``fullband_streaming.FullbandStreamingSession`` do in the same way, written once.

``SessionCommon`` is a state-less mixin: no ``__init__``, no attributes of its own, nothing to override.  Its methods read the
attributes both sessions carry under the same names (``eng``, ``dev``, ``B``, ``F``, ``D``, ``hop``, ``waveform``, ``inp`` / ``hist`` /
``_tmp``, ``_owner``, ``_clip_f0`` / ``_clip_c0``, ``frames_done``, ``_state_parts()``, ``_make_state_layout()``) and take everything
the two name or shape differently as an argument.  Neither session inherits from the other, and no public method lives here: what a
session offers (``prime`` / ``advance`` on one, ``tick`` / ``catch_up`` on the other) is its own class's business.

``row_count_jobs`` builds the ``sfsn_spike_count_rows`` job arrays of both sessions' per-kernel tiers (tests/test_session_common_host.py).
"""
from __future__ import annotations

import ctypes

import torch

from ._lib import MAX_COUNT_TENSORS, RowCount, check
from .clip_select import as_i32, clip_indices, runs_by
from .clip_state import gather_rows, scatter_rows


def row_count_jobs(tensors_with_rows_per_clip, counts, T=None, R=None) -> list:
    """The ``RowCount`` arrays of one per-clip spike count: job i counts ``tensors_with_rows_per_clip[i] = (int8 spikes [T][R][HP],
    rows per clip)`` into ``counts[i]`` (int64, one word per clip); ``MAX_COUNT_TENSORS`` jobs per array at most, one
    ``sfsn_spike_count_rows`` launch each.  ``T`` / ``R``: frames / rows to count over where they are not the tensors' own."""
    jobs = []
    for i0 in range(0, len(tensors_with_rows_per_clip), MAX_COUNT_TENSORS):
        chunk = tensors_with_rows_per_clip[i0:i0 + MAX_COUNT_TENSORS]
        arr = (RowCount * len(chunk))()
        for j, (t, rows_per_clip) in enumerate(chunk):
            arr[j].spikes_i8, arr[j].HP, arr[j].rows_per_clip = t.data_ptr(), t.shape[2], rows_per_clip
            arr[j].T, arr[j].R = (t.shape[0] if T is None else T), (t.shape[1] if R is None else R)
            arr[j].counts = counts[i0 + j].data_ptr()
        jobs.append(arr)
    return jobs


class SessionCommon:
    _as_i32 = staticmethod(as_i32)  # a launch index (uint32) as the int32 a fill writes

    def _check_owner(self) -> None:
        """A whole ``reset()``: the module the engine was packed from must still own this engine."""
        owner = self._owner() if self._owner is not None else None
        if owner is not None and owner.engine() is not self.eng:
            raise RuntimeError("the module's parameters (or device) changed after this streaming session was created: its packed "
                               "weights are stale -- create a new session with module.streaming(...)")

    # ---- the per-kernel sequence ----------------------------------------------------------------------------------------------------
    def _shift_history(self, ri: torch.Tensor, st) -> None:
        """The first thing a hop of the per-kernel sequence enqueues (``ri``: ``hist`` as real pairs, ``st``: the stream's handle):
        the history window moves on by ``hop`` frames and ``inp`` becomes its last ``hop``."""
        D, hop = self.D, self.hop
        if D + hop <= 16:  # history shift + append in one launch
            check(self.eng.lib.sfsn_hist_shift(ctypes.c_void_p(ri.data_ptr()), ctypes.c_void_p(torch.view_as_real(self.inp).data_ptr()),
                                               self.B * self.F, D, hop, st), "sfsn_hist_shift")
        else:
            if D > 0:
                self._tmp[:, :, :D].copy_(self.hist[:, :, hop:hop + D])
                self.hist[:, :, :D].copy_(self._tmp[:, :, :D])
            self.hist[:, :, D:].copy_(self.inp)

    def _capture(self, after_warmup=None) -> None:
        """``_enqueue()`` into a HIP graph (``_graph``).  ``after_warmup``: called once behind the synchronised warm-up hops."""
        side = torch.cuda.Stream(device=self.dev)
        side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(side):
            for _ in range(2):  # module loading, function attributes and allocator warm-up happen outside the capture
                self._enqueue()
        torch.cuda.current_stream(self.dev).wait_stream(side)
        torch.cuda.synchronize(self.dev)
        if after_warmup is not None:
            after_warmup()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._enqueue()
        self._graph = g
        self.reset()

    def _clip_rows(self, idx) -> torch.Tensor:
        """Clip indices as the int64 index tensor of a stream-ordered row copy."""
        return torch.tensor(idx, dtype=torch.long).to(self.dev, non_blocking=True)

    def _save_held(self, held):
        """In front of a hop that holds ``held``: their rows of everything a step reads before it writes (export_state's sections)
        are put aside -- stream-ordered row copies, the ones export_state / import_state of this tier make."""
        sel = self._clip_rows(held)
        parts = self._state_parts()
        return sel, parts, [t.index_select(0, sel) for _, t in parts]

    def _restore_held(self, saved, outputs) -> None:
        """Behind that hop: the rows ``_save_held`` put aside go back, and the held clips' rows of ``outputs`` are zero."""
        sel, parts, rows = saved
        for (_, t), r in zip(parts, rows):
            t.index_copy_(0, sel, r)
        for out in outputs:
            if out is not None:
                out.index_fill_(0, sel, 0)

    def _export_rows(self, idx, nbytes: int, layout) -> torch.Tensor:
        return gather_rows(self._state_parts(), self._clip_rows(idx), nbytes, layout)

    def _import_rows(self, idx, state, blob, layout) -> None:
        scatter_rows(self._state_parts(), self._clip_rows(idx), blob, layout)
        self._clip_f0[idx] = self.frames_done - state.frames

    # ---- the one-launch hop ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def _error_words_follow(holders) -> None:
        """Behind a launch, every ~256 frames: each holder's error word (``scratch[0]``) follows the launches into its pinned
        ``err``, which a later launch looks at without blocking."""
        for h in holders:
            h["err"].copy_(h["scratch"][:1], non_blocking=True)
            h["err_pending"] = True

    def _fill_origins(self, origin, launch_index: int, local, state, j0: int = 0) -> None:
        """Behind a state import: the next launch gives clip ``local[i]`` (an index into ``origin``) the frame index row ``j0 + i``
        of ``state`` had at export -- a waveform clip's is its calls minus one (-1: its first call is still to come).  Fills behind
        the queued launches, one per run of consecutive clips of one age (clips that moved together)."""
        ages = [int(state.calls[j0 + i]) - 1 if self.waveform else int(state.frames[j0 + i]) // self.hop for i in range(len(local))]
        for b0, m, age in runs_by(local, ages):
            origin[b0:b0 + m].fill_(self._as_i32(launch_index - age))

    # ---- bookkeeping ----------------------------------------------------------------------------------------------------------------
    def _held_bookkeeping(self, held) -> None:
        """After a launch that held ``held``: their utterances began one hop (waveform: one call) later, so that ``clip_frames`` /
        ``clip_calls`` stay what they were."""
        self._clip_f0[held] += self.hop
        if self.waveform:
            self._clip_c0[held] += 1

    def _state_layout(self):
        """((section, start, stop), ...), bytes of one clip's blob in this session's tier (clip_state.py); fixed at construction."""
        cached = getattr(self, "_layout", None)
        if cached is None:
            cached = self._layout = self._make_state_layout()
        return cached

    def _summary_clips(self, clips, clip_frames):
        """``spike_summary``'s selection: ``(clip indices, the frames T every one of them has seen)``; ``clip_frames``: int64 [B]."""
        if not self.count_spikes:
            raise RuntimeError("open the session with count_spikes=True to count spikes")
        idx = clip_indices(clips, self.B, "clips", duplicates="merge", empty="refuse")
        frames = clip_frames[idx]
        if (frames != frames[0]).any():
            raise ValueError(f"spike_summary: the selected clips have seen different numbers of frames {frames.tolist()}; select "
                             "clips whose utterances are equally long")
        return idx, int(frames[0])
