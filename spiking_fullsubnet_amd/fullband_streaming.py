"""Frame-by-frame (streaming) execution of the cIRM-GSN model (``modeling_cirm_gsn.Model``).

The model is causal after the STFT: the features of a frame (``|X|^fdrc``, a LayerNorm over the bins of that frame) need the frame
only, the GSN cells carry ``(h, c)``, and the deep filter reaches back ``df - 1`` frames of the noisy spectrum with zeros before
frame 0.  A session keeps, on the device, the ``(h, c)`` of every layer at the padded size ``Hp = ceil16(H)`` and ``df - 1`` frames
of input history; every ``step`` computes ``hop`` new frames.  Outputs are bit-identical to ``FullbandEngine.forward_stft`` on the
concatenated input (tests/test_cirm_streaming.py).

Two ways to run a hop:

* the per-kernel sequence (``one_launch=False``): exactly the launches of ``FullbandEngine.forward_stft``
  (``FullbandEngine._launch_frames``) restricted to the ``hop`` new frames behind the history, behind one history-shift launch;
  captured once into a HIP graph when ``graph=True``.  Covers every GSN configuration the engine covers.
* ``sfsn_fullband_stream_hop`` (``one_launch=True``; csrc/sfsn_fullband_hop.hip): the whole hop in ONE launch.  Covers shared gate
  weights, ``Hp <= 320``, up to 4 layers, ``193 <= F <= 320``, ``S <= 2``, ``df <= 5``, ``df - 1 + hop <= 32``, ``B <= 16``
  (include/sfsn.h); outside that ``one_launch=True`` raises ``NotImplementedError`` and ``"auto"`` takes the per-kernel sequence.

``one_launch="auto"`` picks the tier ``AUTO_ONE_LAUNCH`` names where the hop kernel covers the session (profiles/cirm_streaming.md
has the measurement behind the setting).

Per-clip utterances: ``reset(clips=[...])`` restarts some clips of a batched session while the others go on bit for bit.  The
one-launch hop gives every clip its own origin (the launch at which its utterance began) and reads a restarted clip's state and
history as zero in that launch; the per-kernel sequence zeroes the clips' rows with stream-ordered fills.  Neither synchronises.

Waveform sessions (``waveform=True``): ``step_wave(samples [B, 128])`` returns ``[B, S, 128]`` enhanced samples, the frame's STFT, the
hop and the inverse STFT with its overlap-add state in ONE ``sfsn_fullband_stream_hop_wave`` launch, bit-identical to ``model(wave)``
(tests/test_cirm_waveform.py).  Call c of an utterance returns the samples that entered with call c - 3 (centred 512-point frames
need 256 samples of look-ahead, the overlap-add another hop); the first three calls return zeros.  Every call is a launch: a clip's
first call only moves its samples into the STFT state (the kernel's k == -1), so every clip's origin is the launch after its next one.
With ``host_io=True``, ``step_wave_host`` takes and returns CPU tensors: the launch reads the samples from pinned host memory and
writes the enhanced samples and a completion word per (clip, speaker) back into pinned host memory, no copy launch and no stream
synchronisation.  Waveform sessions exist on the one-launch kernel only (``hop == 1``, 512-point frames with hop 128, ``B <= 16``,
shared gate weights); anything else has no waveform tier and raises ``NotImplementedError``.

Spike counts (``count_spikes=True``, spectrum sessions): the session counts every layer's spikes per clip as it runs, and
``spike_summary(clips)`` returns them in the form of the offline forward's ``want_counts`` list, so that
``metric.compute_synops(session.spike_summary([b]), [], shared_weights=...)`` is clip b's SynOPs.  The one-launch hop adds each
launch's spikes into per-lane slots (``sfsn_fullband_stream_hop_counted``, still one launch per hop; a restarted clip's slots read as
zero); the per-kernel sequence ends with one per-clip count launch (``sfsn_spike_count_rows``), captured with the rest.

Moving a clip: ``export_state(clips)`` / ``import_state(state, clips)`` copy the clips' carried state out of the session (a
``clip_state.ClipState``) and into slots of this or another session of the same geometry and tier, where the clips continue bit for bit:
one launch each way on the one-launch kernel (``sfsn_fullband_hop_state_export`` / ``_import``, csrc/sfsn_state.hip), row copies in the
per-kernel sequence; stream-ordered, no synchronisation.

A backlog: ``catch_up(stft, clips)`` / ``catch_up_wave(samples, clips)`` run recorded frames of some clips through the OFFLINE kernels
(``FullbandEngine._launch_frames``) from the state the clips carry and hand the end state back: what ``N / hop`` calls of ``step``
(``c`` calls of ``step_wave``) would have returned and left, bit for bit, at offline speed -- a clip that joins mid-call, reconnects
after a stall or switches from a file to live input.  One launch each way on the one-launch kernel (``sfsn_fullband_hop_seed`` /
``sfsn_fullband_hop_advance``, csrc/sfsn_prime.hip), row copies in the per-kernel sequence; stream-ordered, no synchronisation.  A
fresh clip reads as zero state, so ``reset(clips); catch_up(prefix, clips)`` is the warm start from a recorded prefix (the sibling's
``prime``; its four method names are not defined here).

A backlog of its own length per clip: ``catch_up_ragged(stft, frames, clips)`` / ``catch_up_wave_ragged(samples, lengths, clips)`` equal the
single-clip ``catch_up`` / ``catch_up_wave`` calls bit for bit in one call: one padded forward on the per-layer scans with the per-frame
membrane tap and the length-aware epilogue, and a hand-back launch that takes every clip's rows at its own last frame
(``sfsn_fullband_hop_advance_ragged``; the per-kernel sequence gathers the same rows).

Held ticks: ``tick(frames, clips)`` / ``tick_wave(samples, clips)`` / ``tick_wave_host(samples, clips)`` advance only the listed clips
of the batch; every other clip is HELD: its input row may hold anything (NaN included), its output row is zero, and its state, spike
counts, ``clip_frames()`` and ``clip_calls()`` stay what they were, so that its next active call continues its utterance bit for bit
(tests/test_cirm_hold.py).  A server whose clips' frames arrive with jitter ticks with the clips that are ready.  The one-launch hop
holds clips inside the one launch it makes anyway (``sfsn_fullband_stream_hop_held`` / ``_wave_held``: the mask travels by value in the
kernel arguments, a held row's state stores are suppressed, ``h`` and the deep-filter history cross the launch parity unchanged, and the
last workgroup to finish moves the held clips' origins on by one launch; no fill, no copy, no second kernel); the per-kernel sequence
saves the held clips' rows of its state before the replay and puts them back after it.  ``clips=None`` or every clip listed is the call
``step*`` makes; an empty list launches nothing.  These are names of their own beside ``step`` / ``step_wave`` / ``step_wave_host``,
whose signatures stay (the sibling's sessions take ``clips=`` on ``step*`` itself); profiles/cirm_hold.md has the measurement.

Outer samples (``Model.streaming_outer(resample=3, sample_format="s16")``; the sibling's ``streaming(waveform=True, resample=...,
sample_format=...)``): a waveform session whose samples are ``[B, 128 * resample]`` of float32 or int16, in and out -- 48 kHz and 16-bit
PCM as a sound card delivers them, converted inside the same one launch (``sfsn_fullband_stream_hop_wave_io``,
csrc/sfsn_fullband_hop_io.hip: the STFT role decimates in front of the frame, the inverse-STFT role interpolates and quantises behind
it; the device bodies and the filters are the sibling's).  Call by call the result is ``Q(U3(control(D3(x * 2**-15))))`` with
``control`` a plain waveform session on the same calls, bit for bit what ``spectral.resample_down3``, that session and
``spectral.resample_up3`` give with their states carried per clip (tests/test_cirm_stream_io.py).  ``step_wave`` / ``tick_wave`` and
their ``_host`` forms, ``reset(clips)`` (no extra launch: a clip's first call reads its decimator row as zero, a muted call writes
its interpolator rows as zero), ``export_state`` / ``import_state`` (sections ``"dec"`` / ``"int"`` behind the launch's blob) and
``catch_up_wave`` (the stand-alone resamplers around the model-rate backlog) carry the filters with the clip;
``catch_up_wave_ragged`` refuses such sessions.  The delay is three calls plus 95 outer samples.

Not covered here: ``resident`` sessions, ``count_spikes`` together with ``waveform``, waveform sessions beyond 16 clips or with
separate gate weights, ragged backlogs in outer samples, and LSTM models.
"""
from __future__ import annotations

import ctypes
import dataclasses
import time
import weakref
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib, ragged, spectral
from ._lib import FullbandHopDesc, FullbandWaveDesc, HopIo, check
from .clip_select import check_frames, check_samples, clip_indices, clip_lengths, held_masks, runs
from .clip_state import ClipState, clip_list, fullband_sections, import_clips, layout_of, new_blob
from .engine import SpikeSummary
from .fullband_engine import FullbandEngine
from .session_common import SessionCommon, row_count_jobs

# what one_launch="auto" takes where sfsn_fullband_stream_hop covers the session: the tier that measured faster at the recipe
# geometry, B = 1, hop = 1 (profiles/cirm_streaming.md)
AUTO_ONE_LAUNCH = True


def hop_covers(engine: FullbandEngine, batch: int, hop: int) -> bool:
    """sfsn_fullband_stream_hop's coverage of a session of this engine (the library's host-only check; 16-bit weights are the
    engine's own mode and use the same digit images)."""
    spec = engine.spec
    rc = engine.lib.sfsn_fullband_hop_check(engine.Hp, spec.layers, engine.F, spec.num_spks, spec.df, batch, hop, spec.df - 1,
                                            0 if spec.shared else 1)
    if rc == _lib.SFSN_EUNSUPPORTED:
        return False
    check(rc, "sfsn_fullband_hop_check")
    return True


def wave_refusal(engine: FullbandEngine, batch: int, hop: int, frame=None) -> Optional[str]:
    """The first thing about a waveform session that sfsn_fullband_stream_hop_wave does not cover, or None.  ``frame``: the module's
    ``(n_fft, hop_length, win_length)`` (None: taken to be the engine's n_fft with hop n_fft / 4)."""
    spec = engine.spec
    n_fft, hop_length, win_length = frame if frame is not None else (spec.n_fft, spec.n_fft // 4, spec.n_fft)
    if hop != 1:
        return f"hop={hop}: a waveform session computes one frame (128 new samples) per call"
    if (n_fft, hop_length, win_length) != (512, 128, 512):
        return (f"n_fft={n_fft}, hop_length={hop_length}, win_length={win_length}: the in-launch transforms are 512-point frames with hop "
                "128 (other frame sizes have no waveform tier)")
    rc = engine.lib.sfsn_fullband_wave_hop_check(engine.Hp, spec.layers, engine.F, spec.num_spks, spec.df, batch, 0 if spec.shared else 1)
    if rc == _lib.SFSN_EUNSUPPORTED:
        if not spec.shared:
            return "shared_weights=False: separate gate weights have no waveform tier"
        if batch > 16:
            return f"B={batch}: more than 16 clips have no waveform tier"
        return (f"Hp={engine.Hp}, layers={spec.layers}, F={engine.F}, S={spec.num_spks}, df={spec.df}: outside "
                "sfsn_fullband_wave_hop_check's coverage (include/sfsn.h)")
    check(rc, "sfsn_fullband_wave_hop_check")
    return None


class FullbandStreamingSession(SessionCommon):
    """``step(frames [B, F, hop] complex64) -> (enh_stft [B, S, F, hop], enh_mag [B, S, F, hop] or None when S > 1)``;
    ``waveform=True``: ``step_wave(samples [B, 128] float32) -> [B, S, 128]`` (``host_io=True``: ``step_wave_host``, CPU tensors);
    ``count_spikes=True``: ``spike_summary(clips)`` (spectrum sessions); ``resample=3`` / ``sample_format="s16"`` (waveform sessions,
    ``Model.streaming_outer``): the samples are ``[B, 128 * resample]`` of float32 or int16, in and out."""

    # the plain session's samples (the constructor replaces them for resample=3 / sample_format="s16")
    resample, sample_format, _io, _outer, _fmt_code, _fmt_dtype = 1, "f32", False, 128, 0, torch.float32

    def __init__(self, engine: FullbandEngine, batch: int = 1, hop: int = 1, graph: bool = True, one_launch="auto", owner=None,
                 waveform: bool = False, host_io: bool = False, frame=None, count_spikes: bool = False, resample: int = 1,
                 sample_format: str = "f32"):
        if batch < 1 or hop < 1:
            raise ValueError("batch and hop must be positive")
        # outer samples (waveform sessions): `resample` times the model's rate, as float32 or 16-bit PCM; (1, "f32") is the plain session
        if resample not in (1, 3):
            raise ValueError(f"resample must be 1 or 3 (the session's samples at the model's rate or at three times it), got {resample!r}")
        self._fmt_code, self._fmt_dtype = spectral.format_of(sample_format)
        self.resample, self.sample_format = int(resample), sample_format
        self._outer = 128 * self.resample  # samples per clip and call, each way
        self._io = self.resample != 1 or sample_format != "f32"
        if self._io and not waveform:
            raise ValueError("resample / sample_format go with waveform=True")
        if one_launch not in ("auto", True, False):
            raise ValueError("one_launch must be 'auto', True or False")
        self.waveform, self.host_io = bool(waveform), bool(host_io)
        if self.host_io and not self.waveform:
            raise ValueError("host_io goes with waveform=True")
        # count_spikes: per-clip spike counts of every layer (spike_summary) -- the one-launch hop keeps them in its slots (`_hop["slots"]`),
        # the per-kernel sequence in `_rows` [layers, B] int64, filled by one sfsn_spike_count_rows launch per step
        self.count_spikes = bool(count_spikes)
        self._rows = None
        if self.count_spikes and self.waveform:
            raise NotImplementedError("count_spikes=True with waveform=True: sfsn_fullband_stream_hop_wave has no counted form (count on a "
                                      "spectrum session)")
        if self.waveform:
            if one_launch is False:
                raise ValueError("waveform=True runs on the one-launch kernel only (one_launch='auto' or True)")
            why = wave_refusal(engine, batch, hop, frame)
            if why is not None:
                raise NotImplementedError(f"waveform=True: {why}")
            one_launch = True
        spec = engine.spec
        self.eng, self.B, self.hop = engine, batch, hop
        self._owner = weakref.ref(owner) if owner is not None else None
        dev = self.dev = engine.device
        self.F, self.S = engine.F, spec.num_spks
        self.D = D = spec.df - 1  # frames of input history the deep filter reaches back
        self.Th = D + hop
        self.launches: Dict[str, int] = {}
        self.frames_done = 0
        self._clip_f0 = np.zeros(batch, dtype=np.int64)
        self._calls = 0  # waveform sessions: step_wave / step_wave_host calls (= launches) since the last whole reset
        self._clip_c0 = np.zeros(batch, dtype=np.int64)
        self._graph: Optional[torch.cuda.CUDAGraph] = None
        self._hop = None
        self._catch_up_ws: Dict[tuple, dict] = {}  # the offline launches' scratch of the last few backlog sizes (catch_up)
        covered = hop_covers(engine, batch, hop)
        if one_launch is True and not covered:
            raise NotImplementedError(
                f"sfsn_fullband_stream_hop does not cover this session (shared={spec.shared}, Hp={engine.Hp}, layers={spec.layers}, "
                f"F={engine.F}, S={spec.num_spks}, df={spec.df}, B={batch}, hop={hop}; coverage: include/sfsn.h) -- use "
                "one_launch='auto' or False for the per-kernel sequence")
        self.one_launch = covered and (AUTO_ONE_LAUNCH if one_launch == "auto" else bool(one_launch))
        self.inp = None if self.waveform else torch.zeros((batch, self.F, hop), dtype=torch.complex64, device=dev)
        with torch.cuda.device(dev):
            if self.one_launch:
                self._build_hop()
            else:
                self._build_sequence()
                if graph:
                    self._capture(lambda: engine._errors.poll(block=True))  # (the warm-up launches' error words)

    def _count(self, what: str) -> None:
        self.launches[what] = self.launches.get(what, 0) + 1

    # ---- the one-launch hop ---------------------------------------------------------------------------------------------------------
    def _build_hop(self) -> None:
        eng, spec, dev = self.eng, self.eng.spec, self.dev
        B, F, S, hop, D, Hp, HP8, nl = self.B, self.F, self.S, self.hop, self.D, eng.Hp, eng.HP8, spec.layers
        f32 = dict(dtype=torch.float32, device=dev)
        i8 = dict(dtype=torch.int8, device=dev)
        # carried state (zero = the start of an utterance) and the launch's tagged work buffers
        st = dict(h=[torch.zeros((2, B, HP8), **i8) for _ in range(nl)], c=[torch.zeros((B, Hp), **f32) for _ in range(nl)],
                  hist=torch.zeros((2, B, F, max(D, 1), 2), **f32))
        work = dict(spikes=[torch.zeros((hop, B, HP8), **i8) for _ in range(nl)], z0=torch.zeros((hop, B, Hp, 2), **f32))
        enh = torch.zeros((B, S, F, hop, 2), **f32)
        mag = torch.zeros((B, S, F, hop), **f32) if S == 1 else None
        origin = torch.zeros((B,), dtype=torch.int32, device=dev)  # the launch index of every clip's frame 0
        wd = FullbandWaveDesc() if self.waveform else None
        d = wd.hop if wd is not None else FullbandHopDesc()
        for l, layer in enumerate(eng.layers):
            o = d.layer[l]
            if l > 0:
                o.w_ih, o.w_ih_dq = layer.w_ih_q[0][0].data_ptr(), layer.w_ih_q[0][1].data_ptr()
            o.w_hh, o.w_hh_dq, o.bias = layer.w_hh_q.data_ptr(), layer.w_hh_dq.data_ptr(), layer.bias.data_ptr()
            o.bn_alpha, o.bn_beta = layer.alpha.data_ptr(), layer.beta.data_ptr()
            o.h[0], o.h[1], o.c, o.spikes = st["h"][l][0].data_ptr(), st["h"][l][1].data_ptr(), st["c"][l].data_ptr(), work["spikes"][l].data_ptr()
        d.n_layers, d.Hp, d.B, d.F, d.S, d.df, d.hop, d.D, d.act, d.unshared = nl, Hp, B, F, S, spec.df, hop, D, spec.act, 0
        d.fdrc, d.ln_eps = spec.fdrc, 1e-5
        d.w_ih0 = eng.layers[0].w_ih_f32.data_ptr()
        if eng.ln_w is not None:
            d.ln_w, d.ln_b = eng.ln_w.data_ptr(), eng.ln_b.data_ptr()
        d.w_p, d.w_p_dq, d.b_p = eng.proj_q.data_ptr(), eng.proj_dq.data_ptr(), eng.proj_b.data_ptr()
        d.inp_ri = self.inp.data_ptr() if self.inp is not None else None
        d.hist_ri[0], d.hist_ri[1] = st["hist"][0].data_ptr(), st["hist"][1].data_ptr()
        d.enh_ri, d.enh_mag, d.z0 = enh.data_ptr(), (mag.data_ptr() if mag is not None else None), work["z0"].data_ptr()
        d.clip_start = origin.data_ptr()
        nbytes = eng.lib.sfsn_fullband_hop_scratch_bytes(ctypes.byref(d))
        assert nbytes, "sfsn_fullband_hop_check accepted this geometry"
        scratch = torch.zeros((nbytes // 4,), dtype=torch.int32, device=dev)  # word 0: the error word
        d.scratch, d.scratch_bytes, d.launch_index = scratch.data_ptr(), nbytes, 0
        slots = None
        if self.count_spikes:  # running spike counts, one word per lane that writes 4 neurons of a clip row (include/sfsn.h)
            n = eng.lib.sfsn_fullband_hop_spike_slots(ctypes.byref(d))
            assert n == nl * B * (Hp // 4), (n, nl, B, Hp)
            slots = torch.zeros((n,), dtype=torch.int32, device=dev)
        self._hop = dict(desc=d, ref=ctypes.byref(d), st=st, work=work, enh=torch.view_as_complex(enh), mag=mag, origin=origin,
                         scratch=scratch, slots=slots, err=torch.zeros((1,), dtype=torch.int32).pin_memory(), err_pending=False)
        if wd is not None:
            self._build_wave(wd)

    def _build_wave(self, wd: FullbandWaveDesc) -> None:
        """The waveform state, the granule scratch (zeroed once) and, with host_io, the pinned buffers the launch reads and writes."""
        B, F, S, dev, h = self.B, self.F, self.S, self.dev, self._hop
        f32 = dict(dtype=torch.float32, device=dev)
        n, dt = self._outer, self._fmt_dtype
        wv = dict(state=torch.zeros((B, 512), **f32), ola=torch.zeros((B, S, 512), **f32), out=torch.zeros((B, S, n), dtype=dt, device=dev),
                  window=torch.hann_window(512, **f32), spec_g=torch.zeros((B, F, 4), **f32), enh_g=torch.zeros((B, S, F, 4), **f32))
        wd.wave_state, wd.ola_state, wd.wave_out, wd.window = (wv[k].data_ptr() for k in ("state", "ola", "out", "window"))
        wd.spec_g, wd.enh_g = wv["spec_g"].data_ptr(), wv["enh_g"].data_ptr()
        wd.wave_in = wv["out"].data_ptr()  # (set per call)
        if self.host_io:  # pinned host memory the kernel reads / writes directly (device-reachable at the same address)
            host = dict(inp=torch.zeros((B, n), dtype=dt).pin_memory(), out=torch.zeros((B, S, n), dtype=dt).pin_memory(),
                        done=torch.zeros((B * S,), dtype=torch.int32).pin_memory())
            host["done_np"] = host["done"].numpy()
            wd.wave_in, wd.wave_out, wd.done = host["inp"].data_ptr(), host["out"].data_ptr(), host["done"].data_ptr()
            wv["host"] = host
        io = None
        if self._io:  # the launch goes through sfsn_fullband_stream_hop_wave_io: the descriptor's own sample pointers are ignored
            io = HopIo()
            io.ratio, io.format, io.wave_in, io.wave_out = self.resample, self._fmt_code, wd.wave_in, wd.wave_out
            if self.resample == 3:  # the two filters' carried samples and taps (include/sfsn.h: sfsn_hop_io)
                wv.update(dec=torch.zeros((B, 96), **f32), int=torch.zeros((B * S, 32), **f32))
                wv["taps"], wv["phase_taps"] = spectral.resample_taps(dev)
                io.dec_state, io.int_state = wv["dec"].data_ptr(), wv["int"].data_ptr()
                io.taps, io.phase_taps = wv["taps"].data_ptr(), wv["phase_taps"].data_ptr()
        h["origin"].fill_(1)  # every clip's first call is launch 0: its frame 0 is launch 1
        h.update(wave=wv, wdesc=wd, wref=ctypes.byref(wd), io=io, io_ref=None if io is None else ctypes.byref(io))

    def _launch(self, name: str, *args) -> None:
        """One launch of the hop's entry point ``name`` (``args``: everything in front of the stream) on torch's current stream."""
        h = self._hop
        if h["err_pending"] and int(h["err"][0]) != 0:  # written behind an earlier launch; no blocking here
            self.check_errors()
        with torch.cuda.device(self.dev):  # the C ABI launches on the calling thread's current device
            rc = getattr(self.eng.lib, name)(*args, ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream))
        if rc:
            check(rc, name)
        d = h["desc"]
        d.launch_index = (d.launch_index + 1) & 0xFFFFFFFF
        self._count("hop")

    def _launch_wave(self, wave_in_ptr: int, held_mask: int = 0) -> None:
        """One waveform launch; ``held_mask`` (tick_wave*): bit b = clip b is held -- the held entry point, still one launch."""
        h = self._hop
        if h["io"] is not None:  # outer samples: the io entry point, held or not -- still one launch
            h["io"].wave_in = wave_in_ptr
            self._launch("sfsn_fullband_stream_hop_wave_io", h["wref"], h["io_ref"], held_mask)
        else:
            h["wdesc"].wave_in = wave_in_ptr
            if held_mask:
                self._launch("sfsn_fullband_stream_hop_wave_held", h["wref"], held_mask)
            else:
                self._launch("sfsn_fullband_stream_hop_wave", h["wref"])
        self._calls += 1
        if self._calls % 256 == 0:  # every 256 launches the error word follows them into pinned memory
            self._error_words_follow((h,))

    def step_wave(self, samples: torch.Tensor, copy: bool = True) -> torch.Tensor:
        """Waveform streaming (``waveform=True``): ``samples`` float32 [B, 128], contiguous, on the device -- the next 8 ms of every
        clip, read in place in stream order.  Returns enhanced samples [B, S, 128]: call c of a clip's utterance returns the samples
        that entered with its call c - 3; a clip's first three calls return zeros.  One launch per call.  ``copy=False``: a view of the
        session's buffer, valid until the next call.  A session with outer samples (``Model.streaming_outer``) takes
        ``[B, 128 * resample]`` of float32 or int16 and returns ``[B, S, 128 * resample]`` of the same format, converted inside the
        same launch; a wrong shape or dtype is refused with a message that names the options."""
        if not self.waveform:
            raise RuntimeError("open the session with waveform=True")
        if self.host_io:
            raise RuntimeError("this session was opened with host_io=True: use step_wave_host(samples)")
        return self._call_wave(samples, None, copy)

    def _call_wave(self, samples: torch.Tensor, hold, copy: bool) -> torch.Tensor:
        """``step_wave`` (``hold=None``) / ``tick_wave`` (``hold``: ``_hold``'s ``(active, held, mask)``) behind their refusals."""
        if (samples.device != self.dev or samples.dtype != self._fmt_dtype or tuple(samples.shape) != (self.B, self._outer)
                or not samples.is_contiguous() or samples.data_ptr() % 8 != 0):
            raise RuntimeError(f"expected contiguous {self._sample_kind()} {(self.B, self._outer)} on {self.dev}, got {samples.dtype} "
                               f"{tuple(samples.shape)} on {samples.device}")
        out = self._hop["wave"]["out"]
        if hold is None:
            self._launch_wave(samples.data_ptr())
        elif not hold[0]:  # nobody makes this call
            return torch.zeros_like(out)
        else:
            self._launch_wave(samples.data_ptr(), hold[2])
            self._held_bookkeeping(hold[1])
        return out.clone() if copy else out

    def _sample_kind(self) -> str:
        """The session's samples as an error message names them: the dtype, and for outer samples the options behind it."""
        if not self._io:
            return "float32"
        return f"{self._fmt_dtype} (resample={self.resample}, sample_format={self.sample_format!r})".replace("torch.", "")

    def step_wave_host(self, samples, timeout_s: float = 2.0) -> torch.Tensor:
        """Waveform streaming with the samples on the HOST (``waveform=True, host_io=True``): ``samples`` = float32 [B, 128] CPU tensor
        (or anything ``torch.as_tensor`` takes).  The launch reads them from pinned host memory and writes the enhanced samples and a
        completion word per (clip, speaker) back into pinned host memory; the caller's thread spins on the words -- no copy launch,
        no stream synchronisation.  Returns a CPU tensor [B, S, 128] (a view of the session's pinned buffer, valid until the next
        call); same three-call delay as ``step_wave``."""
        if not self.host_io:
            raise RuntimeError("open the session with waveform=True, host_io=True")
        return self._call_wave_host(samples, None, timeout_s)

    def _call_wave_host(self, samples, hold, timeout_s: float) -> torch.Tensor:
        """``step_wave_host`` (``hold=None``) / ``tick_wave_host`` (``hold``: ``_hold``'s) behind their refusal."""
        host = self._hop["wave"]["host"]
        if hold is not None and not hold[0]:  # nobody makes this call
            return torch.zeros_like(host["out"])
        if self._io:
            given = torch.as_tensor(samples)
            if given.dtype != self._fmt_dtype or given.numel() != self.B * self._outer:
                raise RuntimeError(f"expected {str(self._fmt_dtype).replace('torch.', '')} {(self.B, self._outer)} (resample={self.resample}, "
                                   f"sample_format={self.sample_format!r}), got {given.dtype} {tuple(given.shape)}")
            host["inp"].copy_(given.reshape(self.B, self._outer))
        else:
            host["inp"].copy_(torch.as_tensor(samples, dtype=torch.float32).reshape(self.B, 128))
        target = (self._hop["desc"].launch_index + 1) & 0xFFFFFFFF
        if hold is None:
            self._launch_wave(host["inp"].data_ptr())
        else:
            self._launch_wave(host["inp"].data_ptr(), hold[2])
            self._held_bookkeeping(hold[1])
        self._wait_done(target, timeout_s)
        return host["out"]

    def _wait_done(self, target: int, timeout_s: float) -> None:
        """Spin until every (clip, speaker) completion word of a host_io session reads ``target`` (the launch's index + 1)."""
        done, t_end, t_soft = self._hop["wave"]["host"]["done_np"], None, None
        while (int(done.min()) & 0xFFFFFFFF) != target or (int(done.max()) & 0xFFFFFFFF) != target:  # (uint32 compare: the index wraps)
            if t_end is None:
                t_end = time.perf_counter() + timeout_s
                t_soft = t_end - timeout_s + 0.02
            elif t_soft is not None and time.perf_counter() > t_soft:
                # 20 ms without the words (a hop takes tens of microseconds): a hand-off wait inside the launch has probably expired --
                # the launch has ended by now, its error word says so, and check_errors() raises it
                t_soft = None
                self.check_errors()
            elif time.perf_counter() > t_end:
                raise RuntimeError("sfsn_fullband_stream_hop_wave: no completion word from the launch (see check_errors())")

    # ---- the per-kernel sequence ----------------------------------------------------------------------------------------------------
    def _build_sequence(self) -> None:
        eng, spec, dev = self.eng, self.eng.spec, self.dev
        B, F, S, Th, Hp, nl = self.B, self.F, self.S, self.Th, eng.Hp, spec.layers
        f32 = dict(dtype=torch.float32, device=dev)
        self.hist = torch.zeros((B, F, Th), dtype=torch.complex64, device=dev)
        self._tmp = torch.zeros((B, F, max(self.D, 1)), dtype=torch.complex64, device=dev)
        self._stack = eng._use_stack(B)
        self._ws = eng._make_workspace(B, self.hop, Th, self._stack)
        self._x = torch.empty((Th, B, F), **f32)
        self._flat = torch.zeros((nl, 2, B, Hp), **f32)
        self._states = [(self._flat[l, 0], self._flat[l, 1]) for l in range(nl)]
        self.enh = torch.zeros((B, S, F, Th), dtype=torch.complex64, device=dev)
        self.enh_mag = torch.zeros((B, S, F, Th), **f32) if S == 1 else None
        self._row_jobs = []
        if self.count_spikes:  # the workspace's int8 spikes [Th][B][HP8], one row per clip; frames [D, D + hop) are this step's
            self._rows = torch.zeros((nl, B), dtype=torch.int64, device=dev)
            self._row_jobs = row_count_jobs([(t, 1) for t in self._ws["s8"]], self._rows)

    def _enqueue(self) -> None:
        """One hop on torch's current stream: the history shift, then the offline forward's launches on frames [D, D + hop)."""
        eng, B, D, hop = self.eng, self.B, self.D, self.hop
        with torch.cuda.device(self.dev):
            st = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
            ri = torch.view_as_real(self.hist)
            self._shift_history(ri, st)
            before = dict(eng.launches)
            eng._launch_frames(ri, B, self.Th, D, hop, self._stack, self._ws, self._x, self._states, [None] * len(self._states), None,
                               torch.view_as_real(self.enh), self.enh_mag)
            for arr in self._row_jobs:  # count_spikes: the new frames' spikes per clip (one launch up to 16 layers; capturable)
                check(eng.lib.sfsn_spike_count_rows(arr, len(arr), D, hop, st), "sfsn_spike_count_rows")
                eng._count("spike_count")
            self._last = {k: v - before.get(k, 0) for k, v in eng.launches.items() if v != before.get(k, 0)}

    # ---- the session ----------------------------------------------------------------------------------------------------------------
    def step(self, frames: torch.Tensor, copy: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """``frames``: complex64 [B, F, hop] on the device.  Returns the enhanced frames and (one speaker) their magnitudes; with
        ``copy=False`` the returned tensors are views of the session's buffers, valid until the next ``step``.  The one-launch hop
        reads ``frames`` in place, in stream order: do not overwrite it before the stream has passed this step."""
        if self.waveform:
            raise RuntimeError("this session was opened with waveform=True: use step_wave(samples)")
        return self._call(frames, None, copy)

    def _call(self, frames: torch.Tensor, hold, copy: bool) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """``step`` (``hold=None``) / ``tick`` (``hold``: ``_hold``'s ``(active, held, mask)``) behind their refusals."""
        if frames.device != self.dev or frames.dtype != torch.complex64 or tuple(frames.shape) != (self.B, self.F, self.hop):
            raise RuntimeError(f"expected complex64 {(self.B, self.F, self.hop)} on {self.dev}, got {frames.dtype} {tuple(frames.shape)} "
                               f"on {frames.device}")
        h = self._hop
        if h is not None:
            e, m = h["enh"], h["mag"]
        else:
            e, m = self.enh[..., self.D:], (self.enh_mag[..., self.D:] if self.enh_mag is not None else None)
        if hold is not None and not hold[0]:  # nobody advances
            return torch.zeros_like(e), (torch.zeros_like(m) if m is not None else None)
        if h is not None:
            if not (frames.is_contiguous() and frames.data_ptr() % 8 == 0):
                self.inp.copy_(frames)
                frames = self.inp
            h["desc"].inp_ri = frames.data_ptr()  # read in place: no staging copy in front (the held rows too, into nothing that stays)
            slots = h["slots"]
            if hold is not None:  # the held entry point, still one launch: bit b of the mask = clip b is held
                self._launch("sfsn_fullband_stream_hop_held", h["ref"], ctypes.c_void_p(slots.data_ptr()) if slots is not None else None,
                             hold[2])
            elif slots is not None:
                self._launch("sfsn_fullband_stream_hop_counted", h["ref"], ctypes.c_void_p(slots.data_ptr()))
            else:
                self._launch("sfsn_fullband_stream_hop", h["ref"])
            if (self.frames_done + self.hop) % 256 < self.hop:  # every ~256 frames the error word follows the launches into pinned memory
                self._error_words_follow((h,))
        else:
            saved = None if hold is None else self._save_held(hold[1])
            self.inp.copy_(frames)
            if self._graph is not None:
                self._graph.replay()
            else:
                self.eng._errors.poll()  # the eager launches' error words, looked at without blocking
                self._enqueue()
            for k, v in self._last.items():
                self.launches[k] = self.launches.get(k, 0) + v
            if saved is not None:
                self._restore_held(saved, (e, m))
        self.frames_done += self.hop
        if hold is not None:
            self._held_bookkeeping(hold[1])
        if copy:
            return e.clone(), (m.clone() if m is not None else None)
        return e, m

    # ---- held ticks: a call that advances only some clips of the batch ------------------------------------------------------------
    def _hold(self, clips, what: str):
        """``clips`` of a tick: None where nobody is held (``clips=None`` or every clip listed); otherwise ``(active, held, mask)``
        with bit b of ``mask`` set for a held clip b (clip_select.held_masks: duplicates merged, ``ValueError`` naming an index out of
        range, ``TypeError`` for wrong types)."""
        if clips is None:
            return None
        active, held, words = held_masks(clips, self.B, [(0, self.B)], what)
        if not held:
            return None
        return active, held, words[0][0]  # (the mask is the one-launch tier's: B <= 16 there, one word)

    def tick(self, frames: torch.Tensor, clips, copy: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """``step`` for a tick on which only ``clips`` (a sequence or 1-D tensor of clip indices; duplicates merged) have new frames:
        they take the hop, every other clip is HELD -- its rows of ``frames`` may hold anything (NaN included), its output rows are
        zero, and its state, spike counts and ``clip_frames()`` are what they were: its next active call continues its utterance
        bit for bit.  Shapes do not change.  The one-launch tier holds the clips inside the one launch it makes anyway
        (``sfsn_fullband_stream_hop_held``: the mask travels in the kernel arguments, no fill, no copy, no second kernel); the
        per-kernel tier saves the held clips' rows of its state before the replay and puts them back after it (stream-ordered row
        copies).  ``clips=None`` or every clip listed: exactly ``step(frames, copy)``.  An empty list advances nobody: nothing is
        launched, nothing changes, zeros are returned.  ``ValueError``: an index out of range (named); ``TypeError``: wrong types."""
        if self.waveform:
            raise RuntimeError("this session was opened with waveform=True: use step_wave(samples)")
        return self._call(frames, self._hold(clips, "tick"), copy)

    def tick_wave(self, samples: torch.Tensor, clips, copy: bool = True) -> torch.Tensor:
        """``step_wave`` for a tick on which only ``clips`` have new samples: they make this call, every other clip is HELD -- its
        row of ``samples`` is ignored (NaN included), it gets zeros, its state and ``clip_calls()`` stay, and its next active call
        returns what that call would have returned (the three-call delay line counts the clip's OWN calls).  A clip may be held at
        the session's first call and before it has ever run: it simply makes its first call later.  One
        ``sfsn_fullband_stream_hop_wave_held`` launch.  ``clips=None`` or every clip listed: exactly ``step_wave(samples, copy)``;
        an empty list launches nothing and returns zeros."""
        if not self.waveform:
            raise RuntimeError("open the session with waveform=True")
        if self.host_io:
            raise RuntimeError("this session was opened with host_io=True: use step_wave_host(samples)")
        return self._call_wave(samples, self._hold(clips, "tick_wave"), copy)

    def tick_wave_host(self, samples, clips, timeout_s: float = 2.0) -> torch.Tensor:
        """``step_wave_host`` with HELD clips (``tick_wave``'s rules, CPU tensors in and out): the launch writes the held clips'
        completion words too, so the wait on the words ends as it always does.  ``clips=None`` or every clip listed: exactly
        ``step_wave_host(samples, timeout_s)``; an empty list launches nothing and returns zeros."""
        if not self.host_io:
            raise RuntimeError("open the session with waveform=True, host_io=True")
        return self._call_wave_host(samples, self._hold(clips, "tick_wave_host"), timeout_s)

    def reset(self, clips=None) -> None:
        """Back to the start of an utterance: zero (h, c), zero history and zero spike counts.  ``clips`` (a sequence or 1-D tensor of
        clip indices): only these clips restart, at their next step; the others go on as if nothing happened.  Ordered with the steps
        on torch's current stream, no synchronisation.  ``clips=None``: the whole session (also checks the error word and that the
        module's parameters have not changed since the session packed them)."""
        if clips is not None:
            self._reset_clips(clips)
            return
        self._check_owner()
        if self._hop is not None:
            self.check_errors()
            h = self._hop
            for t in h["st"]["h"] + h["st"]["c"] + [h["st"]["hist"]]:
                t.zero_()
            if self.waveform:  # every clip's next call is its first (no frame yet): its frame 0 is the launch after the next
                h["wave"]["state"].zero_()
                h["wave"]["ola"].zero_()
                if self.resample == 3:  # (a whole reset only: reset(clips) leaves the filters to the hop's first-call and mute rules)
                    h["wave"]["dec"].zero_()
                    h["wave"]["int"].zero_()
                h["origin"].fill_(self._as_i32(h["desc"].launch_index + 1))
            else:
                h["origin"].fill_(self._as_i32(h["desc"].launch_index))  # every clip's frame 0 is the next launch
            if h["slots"] is not None:
                h["slots"].zero_()
        else:
            self._flat.zero_()
            self.hist.zero_()
            if self._rows is not None:
                self._rows.zero_()
        self.frames_done = 0
        self._clip_f0[:] = 0
        self._calls = 0
        self._clip_c0[:] = 0

    def _reset_clips(self, clips) -> None:
        idx = clip_indices(clips, self.B, "reset", duplicates="merge", empty="ok")
        if not idx:
            return
        self._clip_f0[idx] = self.frames_done
        self._clip_c0[idx] = self._calls
        if self._hop is not None:  # (a fill behind the queued launches: none of them sees the new origin)
            # the launch that computes the clips' frame 0: the next one -- in waveform mode the one after (the next call is the
            # clips' first, which has no frame yet).  Spike slots: read as zero in that launch, as h and c are
            org = self._as_i32(self._hop["desc"].launch_index + (1 if self.waveform else 0))
            for b in idx:
                self._hop["origin"][b:b + 1].fill_(org)
            return
        for b in idx:  # the per-kernel sequence: the clips' rows of the states and their history, in stream order
            self._flat[:, :, b].zero_()
            self.hist[b].zero_()
            if self._rows is not None:
                self._rows[:, b].zero_()

    # ---- a backlog on running clips: the offline kernels from the carried state, their end state back into the session -----------
    def _catch_up_workspace(self, n: int, N: int, T: int, stack: bool) -> dict:
        """The offline launches' scratch for a backlog of N frames of n clips (kept for the next backlog of that size: the int8
        spikes' pad columns stay zero, every stack launch leaves its counters zeroed)."""
        cache = self._catch_up_ws
        key = (n, N, stack, torch.cuda.current_stream(self.dev).cuda_stream)
        ws = cache.get(key)
        if ws is None:
            if len(cache) >= 4:
                cache.clear()
            ws = cache[key] = self.eng._make_workspace(n, max(N, 1), T, stack)
        return ws

    def _catch_up_run(self, idx, stft=None, samples=None, nocall: bool = False, lens=None):
        """``idx``: distinct clip indices in the caller's order; ``stft`` complex64 [len(idx), F, N], or (waveform mode) ``samples``
        float32 [len(idx), 128 c] contiguous, ``nocall``: the clips have made no call in their utterance.  Returns (enh [n, S, F, N],
        mag or None) or the waveform blocks [n, S, 128 c].  Everything on torch's current stream.  ``lens`` (``catch_up_ragged``):
        clip ``idx[i]`` has ``lens[i]`` of the N frames (waveform mode: of the c calls) and the rest of its row is padding -- the same
        seed, the padding zeroed, one forward with the membrane tap and every clip's end taken at its own last frame
        (``_take_ragged``)."""
        eng, spec, dev, L = self.eng, self.eng.spec, self.dev, self.eng.lib
        n, hop, D, F, S, nl, Hp, HP8 = len(idx), self.hop, self.D, self.F, self.S, spec.layers, eng.Hp, eng.HP8
        f32 = dict(dtype=torch.float32, device=dev)
        c = samples.shape[1] // 128 if samples is not None else 0
        N = stft.shape[-1] if samples is None else c - int(nocall)  # (a clip's first call makes no frame)
        T = D + N
        arr = (ctypes.c_int * n)(*idx)
        h = self._hop
        with torch.cuda.device(dev):
            st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            flat = torch.empty((nl, 2, n, Hp), **f32)  # the offline kernels' (h, c) of the listed clips
            buf = torch.empty((n, F, max(T, 1)), dtype=torch.complex64, device=dev)  # [history | new]
            ri = torch.view_as_real(buf)
            wbuf = None
            if samples is not None:  # [384 samples of context | the new samples]
                wbuf = (torch.empty if N else torch.zeros)((n, 384 + 128 * c), **f32)
            if h is not None:
                slots, wstate, ola = self._state_pointers()
            if N and h is None:
                # the per-kernel sequence: the clips' rows of its states and the last D frames of its history window
                sel = torch.tensor(idx, dtype=torch.long).to(dev, non_blocking=True)
                flat.copy_(self._flat.index_select(2, sel))
                if D:
                    buf[:, :, :D].copy_(self.hist.index_select(0, sel)[:, :, hop:])
            elif N:
                dst = _lib.FullbandSeedDst()
                dst.Bp, dst.T, dst.b0 = n, T, 0
                if D:
                    dst.stft_ri = ri.data_ptr()
                if wbuf is not None:
                    dst.wave_ctx, dst.wave_stride = wbuf.data_ptr(), wbuf.shape[1]
                for l in range(nl):
                    dst.layer[l].h, dst.layer[l].c = flat[l, 0].data_ptr(), flat[l, 1].data_ptr()
                rc = L.sfsn_fullband_hop_seed(h["ref"], slots, wstate, arr, n, ctypes.byref(dst), st)
                if rc:
                    check(rc, "sfsn_fullband_hop_seed")
                self._count("seed")
            ws = enh = mag = None
            if samples is not None:
                wbuf[:, 384:].copy_(samples)
            if N:
                if samples is not None:
                    from . import spectral
                    # frame j of the backlog covers samples [128 j, 128 j + 512) of the buffer, the centred frame j + 2 -- behind a
                    # first call, whose samples make no frame, [128 (j + 1), ..): the centred frame j + 3
                    lead = 3 if nocall else 2
                    stft = spectral.stft(wbuf, 512, 128)[:, :, lead:lead + N]
                if lens is not None:  # (N >= 1: the longest clip has a frame)
                    return self._run_ragged(idx, [v - int(nocall) for v in lens] if samples is not None else lens, stft, buf, flat, wbuf,
                                            sel if h is None else None, nocall)
                buf[:, :, D:].copy_(stft)
                stack = eng._use_stack(n)
                ws = self._catch_up_workspace(n, N, T, stack)
                x = torch.empty((T, n, F), **f32)
                states = [(flat[l, 0], flat[l, 1]) for l in range(nl)]
                enh = torch.empty((n, S, F, T, 2), **f32)
                mag = torch.empty((n, S, F, T), **f32) if S == 1 else None
                if not torch.cuda.is_current_stream_capturing():
                    eng._errors.poll()
                eng._launch_frames(ri, n, T, D, N, stack, ws, x, states, [None] * nl, None, enh, mag)
            if h is None:
                self._flat.index_copy_(2, sel, flat)
                self.hist.index_copy_(0, sel, buf[:, :, T - self.Th:])  # the last D + hop frames of [history | new] (N >= hop)
                if self._rows is not None:  # the new frames' spikes per clip, added to the clips' counts
                    tmp = torch.zeros((nl, n), dtype=torch.int64, device=dev)
                    for jobs in row_count_jobs([(t, 1) for t in ws["s8"]], tmp, T=T, R=n):
                        check(L.sfsn_spike_count_rows(jobs, len(jobs), D, N, st), "sfsn_spike_count_rows")
                        eng._count("spike_count")
                    self._rows.index_add_(1, sel, tmp)
                return torch.view_as_complex(enh)[..., D:].contiguous(), (mag[..., D:].contiguous() if mag is not None else None)
            src = _lib.FullbandAdvanceSrc()
            src.Bp, src.N, src.b0, src.T = n, N, 0, T
            if N:
                src.stft_ri = ri.data_ptr()
                for l in range(nl):  # (the new frames of the workspace's [T][n][HP8] spikes)
                    src.layer[l].spikes_i8, src.layer[l].c = ws["s8"][l].data_ptr() + D * n * HP8, flat[l, 1].data_ptr()
            wo = None
            if samples is not None:
                tail = wbuf[:, -512:].contiguous()
                src.wave_tail, src.window = tail.data_ptr(), h["wave"]["window"].data_ptr()
                if N:
                    wo = torch.empty((n, S, 128 * N), **f32)
                    src.enh_ri, src.wave_out = enh.data_ptr(), wo.data_ptr()
            rc = L.sfsn_fullband_hop_advance(h["ref"], slots, wstate, ola, arr, n, ctypes.byref(src), st)
            if rc:
                check(rc, "sfsn_fullband_hop_advance")
            self._count("advance")
            # the clips' origins move back by the launches replaced (32-bit wrap-around, as the launch's unsigned difference), behind
            # the queued launches: the next launch continues that many frame indices further
            back = c if samples is not None else N // hop
            for b0, m in runs(sorted(idx)):  # (one op per run of consecutive clips)
                h["origin"][b0:b0 + m].sub_(back)
            if samples is None:
                return torch.view_as_complex(enh)[..., D:].contiguous(), (mag[..., D:].contiguous() if mag is not None else None)
            if not nocall:
                return wo
            lead0 = torch.zeros((n, S, 128), **f32)  # (the first call's block)
            return torch.cat([lead0, wo], -1) if wo is not None else lead0

    def _run_ragged(self, idx, own, stft, buf, flat, wbuf, sel, nocall: bool):
        """The rest of ``_catch_up_run`` with per-clip lengths, behind the seed: ``own[i]`` new frames of clip ``idx[i]`` (0: a clip
        without a call whose backlog is its first call alone) in rows of ``Nmax = stft.shape[-1]`` frames.  ``buf`` [n, F, D + Nmax]
        holds the history, ``flat`` the clips' (h, c), ``wbuf`` the waveform context rows or None, ``sel`` the clips as a device index
        (per-kernel tier).  The padding is zeroed whatever the caller left there (the scans run over it: nothing of it may be NaN);
        ONE forward on the per-layer launches with the membrane tap and the length-aware epilogue; then every clip's rows at its own
        last frame go back into the session -- ``sfsn_fullband_hop_advance_ragged`` on the one-launch tier, stream-ordered gathers
        on the per-kernel tier -- and its origin moves back by its own launches."""
        eng, spec, dev, L = self.eng, self.eng.spec, self.dev, self.eng.lib
        n, hop, D, F, S, nl, Hp, HP8 = len(idx), self.hop, self.D, self.F, self.S, spec.layers, eng.Hp, eng.HP8
        f32 = dict(dtype=torch.float32, device=dev)
        N = stft.shape[-1]
        T = D + N
        h = self._hop
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        fdev = ragged.upload(own, dev)  # (pinned, on the current stream: no synchronisation)
        keep = torch.arange(N, device=dev).unsqueeze(0) < fdev.unsqueeze(1)
        buf[:, :, D:].copy_(torch.where(keep.unsqueeze(1), stft, torch.zeros((), dtype=stft.dtype, device=dev)))
        ws = self._catch_up_workspace(n, N, T, False)
        x = torch.empty((T, n, F), **f32)
        states = [(flat[l, 0], flat[l, 1]) for l in range(nl)]  # (left after the last PADDED frame: not read again)
        spk = [torch.empty((T, n, Hp), **f32) for _ in range(nl)]
        mem = [torch.empty((T, n, Hp), **f32) for _ in range(nl)]
        enh = torch.empty((n, S, F, T, 2), **f32)
        mag = torch.empty((n, S, F, T), **f32) if S == 1 else None
        ends = fdev + D  # each clip's frames within its [history | new] row
        if not torch.cuda.is_current_stream_capturing():
            eng._errors.poll()
        eng._launch_frames(torch.view_as_real(buf), n, T, D, N, False, ws, x, states, spk, None, enh, mag, frames_dev=ends, mem=mem,
                           own_frames=own)
        if h is None:
            last = (ends - 1).long()  # (own >= hop >= 1 on spectrum sessions, the only ones of this tier)
            rows = torch.arange(n, device=dev)
            for l in range(nl):
                self._flat[l, 0].index_copy_(0, sel, spk[l][last, rows])
                self._flat[l, 1].index_copy_(0, sel, mem[l][last, rows])
            for j, b in enumerate(idx):  # the D + hop frames that end with the clip's own last one
                self.hist[b].copy_(buf[j, :, D + own[j] - self.Th:D + own[j]])
            if self._rows is not None:  # each clip's own frames' spikes, added to its counts
                tmp = torch.zeros((nl, n), dtype=torch.int64, device=dev)
                for jobs in row_count_jobs([(t, 1) for t in ws["s8"]], tmp, T=T, R=n):
                    check(L.sfsn_spike_count_rows_ragged(jobs, len(jobs), D, N, ctypes.c_void_p(ends.data_ptr()), n, st),
                          "sfsn_spike_count_rows_ragged")
                    eng._count("spike_count")
                self._rows.index_add_(1, sel, tmp)
            return torch.view_as_complex(enh)[..., D:].contiguous(), (mag[..., D:].contiguous() if mag is not None else None)
        slots, wstate, ola = self._state_pointers()
        src = _lib.FullbandAdvanceRaggedSrc()
        src.Bp, src.Nmax, src.b0, src.T = n, N, 0, T
        src.frames, src.stft_ri = fdev.data_ptr(), torch.view_as_real(buf).data_ptr()
        for l in range(nl):  # (the new frames of the [T][n][.] buffers)
            src.layer[l].spikes_i8, src.layer[l].membrane = ws["s8"][l].data_ptr() + D * n * HP8, mem[l].data_ptr() + D * n * Hp * 4
        wo = None
        if wbuf is not None:
            wo = torch.empty((n, S, 128 * N), **f32)
            src.wave_ctx, src.wave_stride, src.window = wbuf.data_ptr(), wbuf.shape[1], h["wave"]["window"].data_ptr()
            src.enh_ri, src.wave_out = enh.data_ptr(), wo.data_ptr()
        arr = (ctypes.c_int * n)(*idx)
        rc = L.sfsn_fullband_hop_advance_ragged(h["ref"], slots, wstate, ola, arr, n, ctypes.byref(src), st)
        if rc:
            check(rc, "sfsn_fullband_hop_advance_ragged")
        self._count("advance_ragged")
        # every clip's origin moves back by ITS OWN launches replaced (32-bit wrap-around, as the launch's unsigned difference), behind
        # the queued launches
        back = ragged.upload([v + int(nocall) for v in own] if wbuf is not None else [v // hop for v in own], dev)
        for i, b in enumerate(idx):
            h["origin"][b:b + 1].sub_(back[i:i + 1])
        if wbuf is None:
            return torch.view_as_complex(enh)[..., D:].contiguous(), (mag[..., D:].contiguous() if mag is not None else None)
        return torch.cat([torch.zeros((n, S, 128), **f32), wo], -1) if nocall else wo

    def _catch_up_clips(self, what: str, clips, given) -> list:
        idx = clip_indices(clips, self.B, what, duplicates="refuse", empty="refuse")
        if given != len(idx):
            raise RuntimeError(f"{what}: a backlog of {given} clips for {len(idx)} clip indices")
        return idx

    _MIXED_KINDS = ("{what}: clip {none} has made no call in its current utterance and clip {some} has: they get different frame counts "
                    "-- make one call per kind")

    def _call_kinds(self, idx):
        """The listed clips that have made no call in their utterance, and the ones that have (waveform sessions)."""
        calls = self.clip_calls()
        return [b for b in idx if calls[b] < 1], [b for b in idx if calls[b] >= 1]

    def catch_up(self, stft: torch.Tensor, clips=None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """Run a BACKLOG of ``N`` frames on clips of a running session at the speed of the offline kernels: ``stft`` complex64
        [len(clips), F, N] on the device, row i for ``clips[i]`` (``None``: every clip; any order).  Returns what ``N / hop`` calls
        of ``step`` would have returned for those clips -- ``(enh_stft [.., S, F, N], enh_mag`` or None when S > 1``)`` -- and leaves
        the session where those calls would have left it: last spikes, membranes, deep-filter history, spike counts
        (``count_spikes=True``), ``clip_frames()``.  The other clips are untouched.  A fresh clip (never stepped, or just
        ``reset(clips=[b])``) reads as zero state whatever memory holds, so ``reset(clips); catch_up(prefix, clips)`` is the warm
        start from a recorded prefix; repeated calls process a long recording in chunks.

        The new frames run through ``FullbandEngine._launch_frames`` behind ``D`` frames of the clips' history, from the carried
        state.  The one-launch tier reads the state out in one launch (``sfsn_fullband_hop_seed``) and takes the end state back in
        one (``sfsn_fullband_hop_advance``, csrc/sfsn_prime.hip), then moves the clips' origins back by ``N / hop`` launches; the
        per-kernel tier uses row copies, which the captured graph's next replay sees.  Bit for bit in both tiers, layer 0 included:
        the hop is bit-identical to the offline sequence (include/sfsn.h).

        ``N``: a positive multiple of ``hop``, the same for every listed clip (``ValueError``).  Ordered on torch's current stream,
        no synchronisation, like ``reset(clips=...)``."""
        if self.waveform:
            raise RuntimeError("this session was opened with waveform=True: use catch_up_wave(samples)")
        idx = self._catch_up_clips("catch_up", clips, stft.shape[0] if isinstance(stft, torch.Tensor) and stft.dim() == 3 else -1)
        N = check_frames("catch_up", stft, len(idx), self.F, self.dev, self.hop)
        out = self._catch_up_run(idx, stft=stft)
        self._clip_f0[idx] -= N
        return out

    def catch_up_wave(self, samples: torch.Tensor, clips=None) -> torch.Tensor:
        """``catch_up`` for waveform sessions (``host_io`` included; device tensors in and out): ``samples`` float32
        [len(clips), 128 c], ``c >= 1`` calls' worth.  Returns [.., S, 128 c], the concatenation of what ``c`` calls of ``step_wave``
        would have returned (zero blocks while the clip's frame index is below 2).  A clip that has made a call in its utterance
        continues: its frames come from the last 384 samples of its STFT state followed by the new samples (``spectral.stft``: the
        hop's transform, the same bits), ``c`` frames.  A clip that has made no call yet takes its first 128 samples into the STFT
        state, which makes no frame: ``c - 1`` frames (``c = 1`` writes only the STFT state).  The two kinds have different frame
        counts: all clips of one call must be of one kind (``ValueError`` naming the first clip of each).  The output blocks continue
        the clip's overlap-add accumulator in the hop's order and with its envelope; ``clip_calls()`` and ``clip_frames()`` advance
        by ``c`` calls.  Bit for bit, as ``catch_up``.  On a session with outer samples (``Model.streaming_outer``) ``samples`` is
        ``[len(clips), 128 * resample * c]`` of the session's dtype and the result ``[.., S, 128 * resample * c]`` of it
        (``_catch_up_wave_outer``: both filters are left where the ``c`` calls would have left them)."""
        if not self.waveform:
            raise RuntimeError("open the session with waveform=True")
        idx = self._catch_up_clips("catch_up_wave", clips, samples.shape[0] if isinstance(samples, torch.Tensor) and samples.dim() == 2 else -1)
        if self._io:
            return self._catch_up_wave_outer(samples, idx)
        Ls = check_samples("catch_up_wave", samples, len(idx), self.dev)
        none, some = self._call_kinds(idx)
        if none and some:
            raise ValueError(self._MIXED_KINDS.format(what="catch_up_wave", none=none[0], some=some[0]))
        res = self._catch_up_run(idx, samples=samples.contiguous(), nocall=bool(none))
        self._clip_c0[idx] -= Ls // 128
        return res

    def _catch_up_wave_outer(self, samples: torch.Tensor, idx) -> torch.Tensor:
        """``catch_up_wave`` of a session with outer samples (``resample=3`` / ``sample_format="s16"``): ``samples``
        [len(idx), 128 * resample * c] of the session's dtype -> [.., S, 128 * resample * c] of it, bit for bit the ``c`` calls of
        ``step_wave``, both filters left where those calls leave them.  No kernel of its own: the backlog goes through
        ``spectral.resample_down3`` from the clips' decimator rows (read as zero for clips without a call, as the hop reads them in a
        first call), the model-rate samples through ``_catch_up_run``, its blocks through ``spectral.resample_up3`` from the clips'
        interpolator rows -- read as zero for clips whose next call index is <= 2: the hop writes them as zero in every muted call,
        and the muted blocks of the inner result are zero, so the interpolator sees what the hop's sees."""
        n, S, r, dev, wv = len(idx), self.S, self.resample, self.dev, self._hop["wave"]
        if samples.device != dev or samples.dtype != self._fmt_dtype:
            raise RuntimeError(f"expected {self._sample_kind()} {(n, f'{self._outer} * c')} on {dev}, got {samples.dtype} {tuple(samples.shape)} "
                               f"on {samples.device}")
        Ls = samples.shape[1]
        if Ls < self._outer or Ls % self._outer != 0:
            raise ValueError(f"catch_up_wave: {Ls} samples is not a positive multiple of {self._outer} (resample={self.resample})")
        none, some = self._call_kinds(idx)
        if none and some:
            raise ValueError(self._MIXED_KINDS.format(what="catch_up_wave", none=none[0], some=some[0]))
        c, calls = Ls // self._outer, self.clip_calls()
        x = samples.contiguous()
        if r == 3:
            sel = self._clip_rows(idx)
            dec = wv["dec"].index_select(0, sel)
            if none:
                dec.zero_()
            y, dec = spectral.resample_down3(x, dec)
            wv["dec"].index_copy_(0, sel, dec)
        else:
            y = x.to(torch.float32) * (1.0 / 32768.0)  # (exact: sfsn_resample_dev.h's load of a 16-bit sample)
        res = self._catch_up_run(idx, samples=y.contiguous(), nocall=bool(none))
        self._clip_c0[idx] -= c
        if r == 3:
            pairs = self._clip_rows([b * S + s for b in idx for s in range(S)])
            ist = wv["int"].index_select(0, pairs)
            fresh = [i for i, b in enumerate(idx) if calls[b] <= 2]
            if len(fresh) == n:
                ist.zero_()
            elif fresh:
                ist.view(n, S * 32).index_fill_(0, self._clip_rows(fresh), 0.0)
            z, ist = spectral.resample_up3(res.reshape(n * S, 128 * c), ist, sample_format=self.sample_format)
            wv["int"].index_copy_(0, pairs, ist)
            return z.view(n, S, 3 * 128 * c)
        q = torch.round(res * 32768.0)  # (1, "s16"): sfsn_resample_dev.h's store -- rint, ties to even; NaN -> 0; clamped
        return torch.clamp(torch.where(torch.isnan(q), torch.zeros_like(q), q), -32768.0, 32767.0).to(torch.int16)

    def catch_up_ragged(self, stft: torch.Tensor, frames, clips=None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """``catch_up`` with a backlog of ITS OWN LENGTH per clip, in one call: ``stft`` complex64 [len(clips), F, Nmax] on the device,
        row i for ``clips[i]`` (``None``: every clip; any order of distinct indices); ``frames``: a sequence or CPU int tensor,
        ``frames[i]`` the frames row i really holds -- a positive multiple of ``hop``, at most ``Nmax`` (``ValueError`` naming the
        clip; a wrong count of lengths is a ``ValueError`` too).  Whatever row i holds at frames ``>= frames[i]`` is ignored, NaN
        included.

        The call returns, and leaves behind, exactly what the single-clip calls ``catch_up(stft[i:i+1, :, :frames[i]],
        clips=[clips[i]])`` would have: ``(enh_stft [.., S, F, Nmax], enh_mag`` or None``)`` equal over each clip's own frames and
        zero past them; ``clip_frames()``, the spike counts and every section of ``export_state`` equal bit for bit, in both tiers.
        Unlisted clips are untouched, a fresh clip reads as zero state.

        One seed launch, ONE padded forward from the carried state -- the per-layer scans with the per-frame membrane tap (the
        scans' own end state is the one after the last padded frame; ``sfsn_gsn_stack_scan`` has no tap) and the length-aware
        epilogue (``sfsn_fullband_proj_deepfilter_ragged``) -- and one hand-back launch (``sfsn_fullband_hop_advance_ragged``) that
        takes every clip's rows at its own last frame and moves its origin back by its own launches; the per-kernel tier gathers the
        same rows.  Where layer 0's input product depends on the row count (``F <= 192``), each clip's rows take the form its own
        call would have taken.  The lengths go to the device from pinned memory: ordered on torch's current stream, no
        synchronisation.  Equal lengths: the call IS ``catch_up``, plus padding of the result.  One call costs about three
        single-clip ``catch_up`` calls whatever the number of clips (profiles/cirm_catchup_ragged.md: 0.9 ms at the recipe), so it
        pays from FOUR distinct lengths on (1.14 x at four, 2.4 x at eight); up to three, loop over ``catch_up``."""
        if self.waveform:
            raise RuntimeError("this session was opened with waveform=True: use catch_up_wave_ragged(samples, lengths)")
        idx = self._catch_up_clips("catch_up_ragged", clips, stft.shape[0] if isinstance(stft, torch.Tensor) and stft.dim() == 3 else -1)
        Nmax = check_frames("catch_up_ragged", stft, len(idx), self.F, self.dev, 1)
        lens = clip_lengths("catch_up_ragged", frames, idx, self.hop, f"the session's hop ({self.hop})", Nmax, "frames")
        N = max(lens)

        def padded(t):  # zeros behind the longest clip, up to the caller's Nmax
            return t if t is None or N == Nmax else torch.nn.functional.pad(t, (0, Nmax - N))

        if min(lens) == N:
            enh, mag = self.catch_up(stft[..., :N], clips=clips)
        else:
            enh, mag = self._catch_up_run(idx, stft=stft[..., :N], lens=lens)
            self._clip_f0[idx] -= np.asarray(lens, dtype=self._clip_f0.dtype)
        return padded(enh), padded(mag)

    def catch_up_wave_ragged(self, samples: torch.Tensor, lengths, clips=None) -> torch.Tensor:
        """``catch_up_ragged`` for waveform sessions (``host_io`` included; device tensors in and out): ``samples`` float32
        [len(clips), 128 * cmax], ``lengths[i]`` the samples row i really holds, a positive multiple of 128 and at most
        ``128 * cmax``.  Returns [.., S, 128 * cmax]: over each clip's own samples what ``catch_up_wave(samples[i:i+1, :lengths[i]],
        clips=[clips[i]])`` returns, zeros behind; the session is left where those calls leave it (STFT state, overlap-add sums,
        ``clip_calls()`` and ``clip_frames()`` included).  Both kinds of clip are taken, one kind per call as in ``catch_up_wave``
        (the same ``ValueError`` for a mix): a clip that has made a call gets ``c_b = lengths[b] / 128`` frames; a clip that has made
        no call yet gets ``c_b - 1`` frames behind a block of zeros and an STFT state that ends ``128 c_b`` samples into its row --
        ``c_b = 1`` (no frame at all) is fine beside longer clips without a call."""
        if not self.waveform:
            raise RuntimeError("open the session with waveform=True")
        if self._io:
            raise NotImplementedError(f"catch_up_wave_ragged: not on a session with resample={self.resample!r}, sample_format="
                                      f"{self.sample_format!r} (a ragged backlog in outer samples is a follow-up: loop over catch_up_wave)")
        idx = self._catch_up_clips("catch_up_wave_ragged", clips,
                                   samples.shape[0] if isinstance(samples, torch.Tensor) and samples.dim() == 2 else -1)
        Lmax = check_samples("catch_up_wave_ragged", samples, len(idx), self.dev)
        lens = clip_lengths("catch_up_wave_ragged", lengths, idx, 128, "128", Lmax, "samples")
        Ls = max(lens)

        def padded(t):
            return t if Ls == Lmax else torch.nn.functional.pad(t, (0, Lmax - Ls))

        if min(lens) == Ls:
            return padded(self.catch_up_wave(samples[:, :Ls], clips=clips))
        none, some = self._call_kinds(idx)
        if none and some:
            raise ValueError(self._MIXED_KINDS.format(what="catch_up_wave", none=none[0], some=some[0]))
        res = self._catch_up_run(idx, samples=samples[:, :Ls].contiguous(), nocall=bool(none), lens=[v // 128 for v in lens])
        self._clip_c0[idx] -= np.asarray(lens, dtype=self._clip_c0.dtype) // 128
        return padded(res)

    # ---- moving a clip: its state out of its slot, and into a slot of this or another session ------------------------------------
    def _state_signature(self) -> tuple:
        """What two sessions must share for a clip to move between them (clip_state.py): tier, call geometry, model geometry."""
        cached = getattr(self, "_signature", None)
        if cached is not None:
            return cached
        sig = [("model", "cirm_gsn"), ("tier", "one_launch" if self._hop is not None else "per_kernel"), ("hop", self.hop),
               ("waveform", self.waveform), ("count_spikes", self.count_spikes), ("F", self.F), ("Hp", self.eng.Hp)]
        if self._io:  # (a plain session's signature is what it was: its states move to and from sessions made before these options)
            sig += [("resample", self.resample), ("sample_format", self.sample_format)]
        sig += [(k, v) for k, v in dataclasses.asdict(self.eng.spec).items() if k != "bn"]
        self._signature = tuple(sig)
        return self._signature

    def _state_parts(self) -> list:
        """The per-kernel sequence's carried state as (section, [B, n] view): what a later step reads before it writes."""
        parts = []
        for l in range(self.eng.spec.layers):
            parts += [(f"l{l}.h", self._flat[l, 0]), (f"l{l}.c", self._flat[l, 1])]
        parts.append(("hist", torch.view_as_real(self.hist).view(self.B, -1)))
        if self._rows is not None:
            parts.append(("rows", self._rows.t()))
        return parts

    def _make_state_layout(self):
        if self._hop is None:
            return layout_of([(name, t.shape[1] * t.element_size()) for name, t in self._state_parts()])
        layout, nbytes = fullband_sections(self.eng.spec.layers, self.eng.Hp, self.count_spikes, self.F, self.D, self.waveform, self.S)
        assert nbytes == self.eng.lib.sfsn_fullband_hop_state_bytes(self._hop["ref"], int(self.count_spikes), int(self.waveform)), \
            "clip_state.fullband_sections restates include/sfsn.h"
        self._launch_bytes = nbytes  # what sfsn_fullband_hop_state_export / _import move: the row's head
        if self.resample == 3:  # the two filters' carried samples behind it, moved by row copies beside the launch
            layout = layout + (("dec", nbytes, nbytes + 96 * 4), ("int", nbytes + 96 * 4, nbytes + 96 * 4 + self.S * 32 * 4))
            nbytes = layout[-1][2]
        return layout, nbytes

    def _filter_rows(self, name: str, idx, put=None):
        """The rows of clips ``idx`` (caller's order) of the carried filter samples ``name`` ("dec" / "int") as float32 [len(idx), n];
        ``put``: such rows, written into the session instead.  Stream-ordered row copies."""
        t, sel = self._hop["wave"][name].view(self.B, -1), self._clip_rows(idx)
        if put is None:
            return t.index_select(0, sel)
        t.index_copy_(0, sel, put)
        return None

    def _state_pointers(self):
        """(spike_slots, wave_state, ola_state) as the state launches take them (None: not part of this session)."""
        h = self._hop
        slots = ctypes.c_void_p(h["slots"].data_ptr()) if h["slots"] is not None else None
        if self.waveform:
            return slots, ctypes.c_void_p(h["wave"]["state"].data_ptr()), ctypes.c_void_p(h["wave"]["ola"].data_ptr())
        return slots, None, None

    def clip_calls(self) -> np.ndarray:
        """Waveform sessions: int64 [B], the step_wave / step_wave_host calls of each clip's utterance."""
        return self._calls - self._clip_c0

    def export_state(self, clips=None):
        """The carried state of ``clips`` (``None``: every clip) as a ``ClipState`` of ``len(clips)`` rows, row i = ``clips[i]``: what
        ``import_state`` needs to continue those clips, bit for bit, in other slots of this session or in another session of equal
        signature (``clip_state.py``).  (The warm start from a recorded prefix is ``reset(clips); catch_up(prefix, clips)``.)  The one-launch hop copies
        the state in one launch (``sfsn_fullband_hop_state_export``), the per-kernel sequence with stream-ordered row copies.  The
        session is not changed.  Ordered on torch's current stream, no synchronisation; may return before the copy has run."""
        idx = clip_list(clips, self.B, "export_state")
        layout, nbytes = self._state_layout()
        if self._hop is None:
            blob = self._export_rows(idx, nbytes, layout)
        else:
            head = self._launch_bytes
            blob = new_blob(len(idx), head, layout if head == nbytes else layout[:-2], self.dev)
            slots, wstate, ola = self._state_pointers()
            arr = (ctypes.c_int * len(idx))(*idx)  # (B <= 16: one launch)
            with torch.cuda.device(self.dev):
                rc = self.eng.lib.sfsn_fullband_hop_state_export(self._hop["ref"], slots, wstate, ola, arr, len(idx), ctypes.c_void_p(blob.data_ptr()),
                                                                 ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream))
            if rc:
                check(rc, "sfsn_fullband_hop_state_export")
            if head != nbytes:
                blob = torch.cat([blob] + [self._filter_rows(name, idx).contiguous().view(torch.uint8).view(len(idx), -1) for name in ("dec", "int")],
                                 dim=1)
        return ClipState(blob, self.clip_frames()[idx], self.clip_calls()[idx] if self.waveform else None, None, self._state_signature(),
                         layout)

    def import_state(self, state, clips=None) -> None:
        """Row i of ``state`` (an ``export_state`` result of a session of equal signature, on this session's device) becomes clip
        ``clips[i]`` (``None``: every clip); the next step continues it exactly where the export left it, bit for bit; all other
        clips go on untouched.  Ordered on torch's current stream, no synchronisation.  The weights are NOT compared: importing
        into a session of another model of the same geometry is the caller's decision.  Refusals as for
        ``StreamingSession.import_state``."""
        layout, nbytes = self._state_layout()
        idx = import_clips(state, clips, self.B, self.dev, self._state_signature(), layout, nbytes)
        blob = state.blob.contiguous()
        if self._hop is None:
            self._import_rows(idx, state, blob, layout)
            return
        h = self._hop
        if self._launch_bytes != nbytes:
            for name, a, b in layout[-2:]:
                self._filter_rows(name, idx, blob[:, a:b].contiguous().view(torch.float32))
            blob = blob[:, :self._launch_bytes].contiguous()
        slots, wstate, ola = self._state_pointers()
        arr = (ctypes.c_int * len(idx))(*idx)
        with torch.cuda.device(self.dev):
            rc = self.eng.lib.sfsn_fullband_hop_state_import(h["ref"], slots, wstate, ola, arr, len(idx), ctypes.c_void_p(blob.data_ptr()), 0,
                                                             ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream))
        if rc:
            check(rc, "sfsn_fullband_hop_state_import")
        self._fill_origins(h["origin"], h["desc"].launch_index, idx, state)  # (include/sfsn.h: the clips' origins)
        if self.waveform:
            self._clip_c0[idx] = self._calls - state.calls
        else:
            self._clip_f0[idx] = self.frames_done - state.frames

    def clip_frames(self) -> np.ndarray:
        """int64 [B]: the frames each clip has seen since its own utterance began (waveform sessions, as the kernel counts them: the
        calls since the clip's origin minus one, floored at zero -- a clip's first call has no frame yet)."""
        if self.waveform:
            return np.maximum(self._calls - self._clip_c0 - 1, 0)
        return self.frames_done - self._clip_f0

    def spike_summary(self, clips=None) -> list:
        """The model's layer list of the selected clips' current utterances (``clips=None``: every clip), shaped like the offline
        forward's ``want_counts`` list over ``clip_frames()`` frames: ``[x (T, nb, F)] + [SpikeSummary (T, nb, H) per layer] +
        [proj (T, nb, P)]``, input and projection entries shape-only (meta tensors), spike entries with the exact spike count of the
        selected clips.  ``H`` is the model's hidden size: the padded neurons never spike and do not enter the rate's denominator.
        Counts are summed on the device (nothing synchronises until they are read).  So
        ``metric.compute_synops(session.spike_summary([b]), [], shared_weights=...)`` is clip b's SynOPs.  The selected clips must
        have seen the same number of frames (``ValueError`` otherwise); the session must have been opened with ``count_spikes=True``
        (``RuntimeError``)."""
        idx, T = self._summary_clips(clips, self.clip_frames())
        nb = len(idx)
        eng, nl = self.eng, self.eng.spec.layers
        if self._hop is not None:  # (include/sfsn.h: layer by layer, [B][Hp / 4])
            counts = self._hop["slots"].view(nl, self.B, -1)[:, idx].sum((1, 2), dtype=torch.int64)
        else:
            counts = self._rows[:, idx].sum(1)

        def meta(*shape):
            return torch.empty(shape, dtype=torch.float32, device="meta")

        return [meta(T, nb, self.F)] + [SpikeSummary(counts[l], (T, nb, eng.H)) for l in range(nl)] + [meta(T, nb, eng.spec.P)]

    def check_errors(self) -> None:
        """Raise if a bounded hand-off wait expired inside an earlier launch (blocks until the steps enqueued so far have finished)."""
        torch.cuda.current_stream(self.dev).synchronize()
        if self._hop is not None:
            h = self._hop
            if int(h["scratch"][0].item()) != 0:
                h["scratch"][:1].zero_()  # sticky on the device: cleared when reported
                h["err"].zero_()
                h["err_pending"] = False
                torch.cuda.current_stream(self.dev).synchronize()
                raise RuntimeError("sfsn_fullband_stream_hop: a bounded hand-off wait expired inside a launch (results invalid)")
            return
        self.eng._errors.poll(block=True)
        sc = self._ws.get("scratch")
        if sc is not None and int(sc[0].item()) != 0:  # (graph replays are not watched launch by launch)
            self.eng._errors.clear([sc])
            raise RuntimeError("sfsn_gsn_stack_scan: a layer-to-layer hand-off wait expired inside a streaming step (results invalid)")

    def close(self) -> None:
        """Nothing keeps running between steps; kept for the shape of StreamingSession."""
