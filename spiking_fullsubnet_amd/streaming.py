"""Frame-by-frame (streaming) execution of the live model: BASELINE.json configs[4] / SURVEY.md section 8(d) "config 5".

The network is causal after the STFT: the features of frame t (compressed magnitude, sub-band unfold along frequency,
per-frame LayerNorm; modeling_spiking_fullsubnet.py:434-440, 239-258, 108-112) need frame t only, the recurrent cells carry
(h, c) (efficient_spiking_neuron.py:50-62 accepts and returns the states), and the deep filter reaches back ``df - 1``
frames of the *noisy* spectrum with zero padding before the first frame (modeling_spiking_fullsubnet.py:315-346).  A
session therefore keeps, on the device: the (h, c) state of every layer and ``max(df) - 1`` frames of input history, and
each ``step`` runs exactly the kernels of the offline forward on ``hop`` new frames.  Outputs are bit-identical to the
offline forward on the concatenated input (tested) -- for the one-launch hop with one reservation: its layer-0 input product sums
in another association than the offline kernels' (include/sfsn.h), so a layer-0 membrane closer to the threshold than that
product's rounding (a few 1e-7 of the sum's terms) can spike on one side only; everything is bit-identical from equal layer-0
spikes on.

Two ways to run a hop.  ``one_launch`` (default where the library covers the model: shared or separate gate weights, at most
3 layers / 4 groups): ``sfsn_stream_hop`` -- the whole frame in ONE launch of a few dozen small workgroups whose waves hand
the frame from stage to stage through L2 (csrc/sfsn_hop.hip); its state is its own (double-buffered int8 spikes, membranes,
history).  Otherwise the ~15 launches of the offline kernels, captured once into a HIP graph and replayed per hop: at
hop = 1 that step is launch-bound, not compute-bound.  Both are bit-identical to the offline forward (tested).

The frozen front-end (``model_low_freq.Separator``) with ``offline_laplace_norm`` / ``offline_gaussian_norm`` normalises with
utterance-level statistics (model_low_freq.py:147-169, 205-218), which are not causal -- everything else of it is.  A session on it
therefore takes the statistics from the caller (``norm_stats=``: an ``engine.NormStats`` from a calibration pass, an earlier utterance
of the same channel, or the clip itself) and raises ``NotImplementedError`` without them; fed a clip's own statistics it reproduces
the offline forward bit for bit, in both tiers.  The session owns device copies; ``set_norm_stats`` replaces them in stream order.
With ``cumulative_laplace_norm`` (every row by its own running mean) the front-end streams through the one-launch hop only.

Per-clip utterances: ``reset(clips=[...])`` starts a new utterance on some clips of a batched session while the others go on,
bit for bit.  The one-launch hop gives every clip its own origin (``sfsn_hop_desc.clip_start``: the launch at which its utterance
began) and reads a restarted clip's state as zero in that launch -- no synchronisation, and a resident launch keeps running.  The
per-kernel sequence zeroes the clips' rows of the states and the history with stream-ordered fills.

Priming: ``prime(stft, clips)`` / ``prime_wave(samples, clips)`` start the listed clips' utterances from a RECORDED prefix instead of
from silence (a clip joining mid-call, a seek, a reconnect, a backlog).  The prefix runs on the offline kernels
(``Engine.forward_stft(..., _end_state=True)``); the one-launch hop takes its end state in one launch (``sfsn_hop_prime``,
csrc/sfsn_prime.hip) and the clips' origins move back by the prefix's launches, so that the next hop continues at frame N; the
per-kernel sequence takes it as stream-ordered row copies into its states, history and counts.  Not for resident sessions.

A backlog: ``advance(stft, clips)`` / ``advance_wave(samples, clips)`` run many frames at once on clips that are ALREADY RUNNING (a
network stall that ends, a paused call that resumes, a file that goes live; chunked long-form processing) -- the offline kernels
started from the state the session carries (``Engine.forward_stft(..., _end_state=start)``: (h, c), running sums and ``frames_before``
in, D frames of history in front of the new ones) and their end state handed back.  The one-launch hop gives its state in one launch
(``sfsn_hop_seed``) and takes the end state in one (``sfsn_hop_advance``: counts added to, the overlap-add accumulator continued),
then the clips' origins move back by the backlog's launches; the per-kernel sequence uses row copies.  A fresh clip reads as zero:
``advance`` on it equals ``prime``.  Not for resident sessions.  ``advance_ragged(stft, frames, clips)`` /
``advance_wave_ragged(samples, lengths, clips)`` take a backlog of ITS OWN length per clip in one call and equal the single-clip
``advance`` calls bit for bit: one padded forward with per-clip lengths and the per-frame membranes, and a hand-back launch that takes
every clip's rows at its own last frame (``sfsn_hop_advance_ragged``).

Moving a clip: ``export_state(clips)`` copies the clips' carried state out of the session (a ``clip_state.ClipState``: one self-contained
blob per clip) and ``import_state(state, clips)`` puts it into slots of this or another session of the same geometry and tier, where
the clips continue bit for bit, layer 0 included -- compaction, rebalancing, pause / resume, rewind, fork.  One launch each way in the
one-launch tier (``sfsn_hop_state_export`` / ``sfsn_hop_state_import``, csrc/sfsn_state.hip; the clips' origins move with them), row
copies in the per-kernel tier; stream-ordered, no synchronisation.  Not for resident sessions.

Holding clips: live frames arrive with jitter, and at a tick some calls of a batched session have a frame and some do not.
``step(frames, clips=[...])`` / ``step_wave(samples, clips=[...])`` / ``step_wave_host(samples, clips=[...])`` advance only the listed
clips; every other clip is HELD: whatever its input row holds (NaN included) reaches nothing, its output rows are zero, and its carried
state, spike counts, ``clip_frames`` and ``clip_calls`` are afterwards what they were -- its next active call continues the utterance
with the next frame (waveform: with the next call's delay line), and ``reset`` / ``prime`` / ``advance`` / ``export_state`` /
``spike_summary`` see it as if the call had not happened for it.  The one-launch hop does it in the launch it makes anyway
(``sfsn_stream_hop_held``: the mask travels in the kernel arguments, held rows' state stores are suppressed, ``h`` and ``cum`` cross
the launch parity unchanged and the clip's origin moves on by one launch -- no fill, no copy, no second kernel); the per-kernel
sequence saves the held clips' rows of its states, history and counts before the graph replay and puts them back after it
(stream-ordered row copies).  ``clips=None`` is the call without the keyword: same code path, same launches.  An empty list holds
everybody: nothing is launched and zeros come back.  Not for resident sessions.

Spike counts: a session opened with ``count_spikes=True`` counts every layer's spikes per clip as it runs, and
``spike_summary(clips)`` returns them in the form of the offline forward's ``layer_outputs="counts"`` lists, so that
``metric.compute_synops`` / ``compute_neuronops`` give each clip's current utterance's SynOPs and NeuronOPs.  The one-launch hop
adds each launch's spikes into per-lane slots (``sfsn_hop_desc.spike_slots``; a restarted clip's slots read as zero); the
per-kernel sequence adds a per-clip count launch (``sfsn_spike_count_rows``) to its graph.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
import os
import time
import weakref
from typing import Optional, Tuple

import numpy as np
import torch

from ._lib import AdvanceRaggedSrc, AdvanceSrc, DfGroup, HopDesc, HopIo, HOP_MAX_GROUPS, HOP_MAX_LAYERS, NORM_CUMLAPLACE, PrimeSrc, SeedDst, check
from .clip_select import check_frames, check_samples, clip_indices, clip_lengths, held_masks, part_runs, runs, slot_order
from .clip_state import ClipState, clip_list, hop_sections, import_clips, layout_of, new_blob
from . import spectral
from .engine import Engine, NormStats, SpikeSummary, _ptr
from .session_common import SessionCommon, row_count_jobs


OFFLINE_NORM_MESSAGE = ("the frozen front-end's offline normalisation (model_low_freq.py:147-169, 205-218) divides by statistics of the "
                        "whole utterance, which a stream does not have: pass them as norm_stats= (an engine.NormStats, e.g. from "
                        "Separator.norm_stats(calibration_clip)); cumulative_laplace_norm and the live front-end stream without")


def _raw_stream(device_index: int) -> int:
    """The HIP stream handle of torch's current stream on a device (without building a torch.cuda.Stream object per call)."""
    try:
        return torch._C._cuda_getCurrentRawStream(device_index)
    except AttributeError:  # pragma: no cover - older / newer torch without the private accessor
        return torch.cuda.current_stream(device_index).cuda_stream


class StreamingSession(SessionCommon):
    """``step(frames [B, F, hop] complex64) -> (enh_stft [B, S, F, hop], enh_mag [B, S, F, hop])`` with state carried."""

    # the plain session's samples (the constructor replaces them for resample=3 / sample_format="s16")
    resample, sample_format, _io, _outer, _fmt_code, _fmt_dtype = 1, "f32", False, 128, 0, torch.float32

    def __init__(self, engine: Engine, batch: int = 1, hop: int = 1, graph: bool = True, rows_per_wg=None, owner=None,
                 one_launch="auto", waveform: bool = False, host_io: bool = False, resident: bool = False, idle_ms: int = 1000,
                 count_spikes: bool = False, norm_stats: Optional[NormStats] = None, resample: int = 1, sample_format: str = "f32"):
        spec = engine.spec
        # outer samples (waveform sessions): `resample` times the model's rate, as float32 or 16-bit PCM; (1, "f32") is the plain session
        if resample not in (1, 3):
            raise ValueError(f"resample must be 1 or 3 (the session's samples at the model's rate or at three times it), got {resample!r}")
        self._fmt_code, self._fmt_dtype = spectral.format_of(sample_format)
        self.resample, self.sample_format = int(resample), sample_format
        self._outer = 128 * self.resample  # samples per clip and call, each way
        self._io = self.resample != 1 or sample_format != "f32"
        if self._io and not waveform:
            raise ValueError("resample / sample_format go with waveform=True")
        if self._io and resident:
            raise NotImplementedError(f"resident=True with resample={resample!r}, sample_format={sample_format!r}: the resident launch takes "
                                      "float32 samples at the model's rate only")
        # the module the engine was packed from: reset() checks that its parameters have not changed since (the session's
        # captured graph holds pointers to THIS engine's packed weights)
        self._owner = weakref.ref(owner) if owner is not None else None
        if batch < 1 or hop < 1:
            raise ValueError("batch and hop must be positive")
        if norm_stats is not None:
            norm_stats.validate(spec, batch, engine.device)
        elif spec.laplace:
            raise NotImplementedError(OFFLINE_NORM_MESSAGE)
        # the session's own copies of the clips' statistics: the descriptors and the captured graph point at THESE
        self._stats = None if norm_stats is None else NormStats(*(None if t is None else t.clone().contiguous() for t in
                                                                  (norm_stats.mu_fb, norm_stats.mu_sb, norm_stats.sd_fb, norm_stats.sd_sb)))
        self.eng, self.B, self.hop = engine, batch, hop
        self.rows_per_wg = rows_per_wg  # (full-band, sub-band) rows per scan workgroup; None = the engine's setting
        self.use_stack = True           # layer-pipelined stack launches where the engine's rule picks them (few rows: always)
        dev = self.dev = engine.device
        self.F = spec.n_fft // 2 + 1
        self.D = D = max(spec.df) - 1  # frames of input history the deep filter reaches back
        self.Th = Th = D + hop
        f32 = dict(dtype=torch.float32, device=dev)
        B, F, S, ng = batch, self.F, spec.num_spks, spec.n_groups
        self.inp = torch.zeros((B, F, hop), dtype=torch.complex64, device=dev)
        self.hist = torch.zeros((B, F, Th), dtype=torch.complex64, device=dev)
        self._tmp = torch.zeros((B, F, max(D, 1)), dtype=torch.complex64, device=dev)
        self.x_fb = torch.empty((Th, B, spec.fb_in), **f32)
        self.xs = [torch.empty((Th, B * spec.units(g), spec.sb_input_size(g)), **f32) for g in range(ng)]
        self.enh = torch.zeros((B, S, F, Th), dtype=torch.complex64, device=dev)
        self.enh_mag = torch.zeros((B, S, F, Th), **f32)

        def stack(seqs, Rs):
            H, G, nl = seqs[0].H, seqs[0].cells[0].G, len(seqs[0].cells)
            HP = (H + 63) // 64 * 64
            nb = engine.lib.sfsn_stack_scratch_bytes(nl, len(Rs), sum(Rs))
            return dict(spk=[[None] * len(Rs) for _ in range(nl)], scratch=torch.zeros((nb // 4 + 1,), dtype=torch.int32, device=dev),
                        zin=[[torch.empty((hop, R, G * H), **f32) for R in Rs] for _ in range(nl)],
                        s8=[[torch.zeros((Th, R, HP), dtype=torch.int8, device=dev) for R in Rs] for _ in range(nl)],
                        states=engine._zero_states(Rs, H, nl),
                        proj=[torch.empty((Th, R, seq.P), **f32) for seq, R in zip(seqs, Rs)], nl=nl)
        self.fb = stack([engine.fb], [B])
        self.sb = stack(engine.sb, [x.shape[1] for x in self.xs])
        self.dfg = (DfGroup * ng)()
        for g in range(ng):
            self.dfg[g].proj, self.dfg[g].n_units = _ptr(self.sb["proj"][g]), spec.units(g)
            self.dfg[g].fc, self.dfg[g].df = spec.ctr[g], spec.df[g]
        # count_spikes: per-clip spike counts of every layer (spike_summary); the per-kernel sequence keeps them in `_rows`
        # [fb layers + groups x sb layers, B] int64, filled by one sfsn_spike_count_rows launch per step (captured with the rest)
        self.count_spikes = bool(count_spikes)
        self._rows = None
        ns = self._stats
        self.fg_fb = engine._feature_groups("fb", [self.x_fb], None if ns is None else ns.mu_fb, None if ns is None else ns.sd_fb)
        self.fg_sb = engine._feature_groups("sb", self.xs, None if ns is None else ns.mu_sb, None if ns is None else ns.sd_sb)
        self.frames_done = 0
        # per-clip utterances: the session's frame / call count at which each clip's utterance began (clip_frames = the difference)
        self._clip_f0 = np.zeros(batch, dtype=np.int64)
        self._clip_c0 = np.zeros(batch, dtype=np.int64)
        self._graph: Optional[torch.cuda.CUDAGraph] = None
        self._dev_index = self.dev.index if self.dev.index is not None else torch.cuda.current_device()
        self._hop = None
        self.waveform = bool(waveform)  # step_wave(): samples in, samples out (STFT and inverse STFT inside the launch)
        self._wave_calls = 0
        self._primed = False  # prime_wave() has run: the clips' own frame indices decide what a call returns (see step_wave)
        self.host_io = bool(host_io)  # waveform mode: samples come from and go to (pinned) host memory, no copy launches
        if self.host_io and not waveform:
            raise ValueError("host_io goes with waveform=True")
        # host_io only: ONE resident launch serves hop after hop (sfsn_stream_hop_resident), rung through a doorbell word in pinned
        # memory; it starts with the first hop that computes a frame and ends with reset(), close(), or idle_ms of silence
        self.resident = bool(resident)
        self.idle_ms = int(idle_ms)
        self._res = None
        if self.resident and not self.host_io:
            raise ValueError("resident goes with waveform=True, host_io=True")
        if spec.cum_laplace:
            one_launch = True  # the running means live in sfsn_stream_hop's state; the per-kernel sequence has no streaming form of it
        if self.waveform:
            if hop != 1 or spec.n_fft != 512:
                raise NotImplementedError("waveform streaming: one 128-sample hop per call, 512-point frames")
            one_launch = True
        if one_launch not in ("auto", True, False):
            raise ValueError("one_launch must be 'auto', True or False")
        if one_launch == "auto" and os.environ.get("SFSN_ONE_LAUNCH", "1") == "0":  # diagnostic: the per-kernel sequence everywhere
            one_launch = False
        if one_launch:
            self._hop = self._build_hop()
            if self._hop is None and one_launch is True:
                raise NotImplementedError("sfsn_stream_hop does not cover this model / batch (see include/sfsn.h)")
        if self._hop is None and self.count_spikes:
            self._rows = torch.zeros((spec.fb_layers + ng * spec.sb_layers, B), dtype=torch.int64, device=dev)
            tens = [(self.fb["s8"][l][0], 1) for l in range(spec.fb_layers)] + \
                   [(self.sb["s8"][l][g], spec.units(g)) for g in range(ng) for l in range(spec.sb_layers)]
            self._row_jobs = row_count_jobs(tens, self._rows)
        if self._hop is None and graph:
            self._capture()

    # -----------------------------------------------------------------------------------------------------------------
    def _build_hop(self):
        """Descriptors + state of the one-launch hop (sfsn_stream_hop); None when the library does not cover this session.

        A launch wants every workgroup resident at once (one per compute unit), which bounds the clips per launch (32 at
        baseline_m on an MI355X); a bigger batch is cut into equal parts, one launch each, back to back on the stream -- every part
        has its own state, all parts share the weights and write into the same output tensors."""
        eng, spec, L = self.eng, self.eng.spec, self.eng.lib
        B, F, S, hop, D, ng, dev = self.B, self.F, spec.num_spks, self.hop, self.D, spec.n_groups, self.dev
        if ng > HOP_MAX_GROUPS or max(spec.fb_layers, spec.sb_layers) > HOP_MAX_LAYERS or D + hop > 32:
            return None

        # Arenas instead of ~80 separately allocated tensors: the weights a launch reads (2.9 MB at baseline_m) and the state it
        # reads and writes sit in contiguous ranges -- a launch that starts cold on every compute unit then misses in the TLBs
        # for a handful of pages, not for one page per tensor.
        class Pool:
            def __init__(self):
                self.size, self.buf = 0, None

            def take(self, nbytes):
                off = self.size
                self.size += (nbytes + 255) // 256 * 256
                return None if self.buf is None else self.buf[off:off + nbytes]

            def put(self, t):  # a copy of tensor t inside the pool -> its address (None in the sizing pass)
                v = self.take(t.numel() * t.element_size())
                if v is None:
                    return None
                v.copy_(t.contiguous().view(-1).view(torch.uint8))
                return v.data_ptr()

            def zeros(self, shape, dtype):
                v = self.take(math.prod(shape) * torch.empty((), dtype=dtype).element_size())
                return None if v is None else v.view(dtype).view(shape)

            def allocate(self):
                self.buf = torch.zeros((max(self.size, 256),), dtype=torch.uint8, device=dev)
                self.size = 0

        def ptr(t):
            return None if t is None else t.data_ptr()

        # ---- weights, once (two passes: size, then copy)
        wpool = Pool()
        seqs = [eng.fb] + list(eng.sb)

        def put_weights():
            w = []
            for seq in seqs:
                d = dict(p=(wpool.put(seq.proj_q), wpool.put(seq.proj_dq), wpool.put(seq.proj_b)), layers=[],
                         ln=(wpool.put(seq.ln_w), wpool.put(seq.ln_b)) if seq.ln_w is not None else None)
                for l, cell in enumerate(seq.cells):
                    e = dict(hh=(wpool.put(cell.w_hh_q), wpool.put(cell.w_hh_dq)))
                    if l == 0:  # fp32 input weights in MFMA fragment order (include/sfsn.h): one coalesced request per 16 columns
                        w0 = cell.w_ih_f32
                        kc = (w0.shape[1] + 15) // 16
                        w0 = torch.nn.functional.pad(w0, (0, kc * 16 - w0.shape[1]))
                        # (separate gate weights: 2H rows, the forget gate's tiles first -- tile NT + j is the cell gate's tile j)
                        e["ih"] = (wpool.put(w0.view(w0.shape[0] // 16, 16, kc, 4, 4).permute(0, 2, 3, 1, 4).contiguous()),)
                    elif len(cell.w_ih_q) == 1:
                        e["ih"] = (wpool.put(cell.w_ih_q[0][0]), wpool.put(cell.w_ih_q[0][1]))
                    else:
                        # separate gate weights: the engine packs each gate's [H, H] on its own ([3][NT][KS] KiB images); the hop reads ONE
                        # image of 2H rows, [3][2 NT][KS] with the forget gate's tiles first, and one dq vector [2H]
                        nt_ = seq.H // 16
                        pk = torch.cat([q_[0].reshape(3, nt_, -1) for q_ in cell.w_ih_q], dim=1).contiguous()
                        dq = torch.cat([q_[1][:seq.H] for q_ in cell.w_ih_q]).contiguous()
                        e["ih"] = (wpool.put(pk.reshape(-1)), wpool.put(dq))
                    e["c"] = (wpool.put(cell.bias), wpool.put(cell.alpha), wpool.put(cell.beta))
                    d["layers"].append(e)
                w.append(d)
            win = wpool.put(torch.hann_window(512, device=dev, dtype=torch.float32)) if self.waveform else None
            return w, win

        put_weights()
        wpool.allocate()
        weights, window = put_weights()

        # ---- one part = the clips [b0, b0 + nb) of the batch: descriptor + state
        def make_desc(nb, spool, a=None, b0=0):
            """a: placeholder address for the sizing call (the plan never dereferences device pointers); b0: the part's first clip."""
            desc = HopDesc()
            fgs = [self.fg_fb[0]] + [self.fg_sb[g] for g in range(ng)]
            dsts = [desc.fb] + [desc.sb[g] for g in range(ng)]
            for i, (dst, seq, fg, w) in enumerate(zip(dsts, seqs, fgs, weights)):
                R = nb * (1 if i == 0 else spec.units(i - 1))
                HP = (seq.H + 63) // 64 * 64
                dst.n_layers, dst.H, dst.P = len(seq.cells), seq.H, seq.P
                dst.df, dst.fc = (0, 0) if i == 0 else (spec.df[i - 1], spec.ctr[i - 1])
                dst.feat = fg
                if w["ln"] is not None:
                    dst.feat.ln_w, dst.feat.ln_b = w["ln"]
                if self._stats is not None:  # given statistics: the part's clips of the session's copies ([B] / row i - 1 of [ng, B])
                    off = ((i - 1) * B if i else 0) + b0
                    dst.feat.mu = (self._stats.mu_fb if i == 0 else self._stats.mu_sb).data_ptr() + 4 * off
                    if spec.gaussian:
                        dst.feat.ln_w = (self._stats.sd_fb if i == 0 else self._stats.sd_sb).data_ptr() + 4 * off
                if spec.cum_laplace:  # the rows' running sums travel with the session
                    dst.feat.norm = NORM_CUMLAPLACE
                    c0, c1 = spool.zeros((R,), torch.float32), spool.zeros((R,), torch.float32)
                    dst.cum[0], dst.cum[1] = (a, a) if a else (ptr(c0), ptr(c1))
                dst.w_p, dst.w_p_dq, dst.b_p = w["p"]
                for l, e in enumerate(w["layers"]):
                    o = dst.layer[l]
                    o.w_hh, o.w_hh_dq = e["hh"]
                    if l == 0:
                        o.w_ih_frag = e["ih"][0]
                    else:
                        o.w_ih, o.w_ih_dq = e["ih"]
                    o.bias, o.bn_alpha, o.bn_beta = e["c"]
                    h0, h1 = spool.zeros((R, HP), torch.int8), spool.zeros((R, HP), torch.int8)
                    c, spk = spool.zeros((R, seq.H), torch.float32), spool.zeros((hop, R, HP), torch.int8)
                    o.h[0], o.h[1], o.c, o.spikes = (a, a, a, a) if a else (ptr(h0), ptr(h1), ptr(c), ptr(spk))
            desc.n_groups, desc.B, desc.F, desc.S, desc.hop, desc.D, desc.fdrc = ng, nb, F, S, hop, D, spec.fdrc
            desc.unshared = 0 if spec.shared else 1
            st = dict(hist=spool.zeros((nb, F, max(D, 1), 2), torch.float32))
            if self.waveform:
                st.update(state=spool.zeros((nb, 512), torch.float32), ola=spool.zeros((nb, S, 512), torch.float32),
                          spec_g=spool.zeros((nb, F, 4), torch.float32), enh_g=spool.zeros((nb, S, F, 4), torch.float32))
                if self.resample == 3:  # the two filters' carried samples (include/sfsn.h: sfsn_hop_io)
                    st.update(dec=spool.zeros((nb, 96), torch.float32), int=spool.zeros((nb, S, 32), torch.float32))
            if a:
                desc.inp_ri = desc.hist_ri = desc.enh_ri = desc.enh_mag = a
                if self.waveform:
                    desc.wave_in = desc.wave_state = desc.ola_state = desc.wave_out = desc.window = desc.spec_g = desc.enh_g = a
            else:
                desc.hist_ri = ptr(st["hist"])
                if self.waveform:
                    desc.wave_state, desc.ola_state, desc.window = ptr(st["state"]), ptr(st["ola"]), window
                    desc.spec_g, desc.enh_g = ptr(st["spec_g"]), ptr(st["enh_g"])
            return desc, st

        probe = torch.zeros((16,), dtype=torch.uint8, device=dev)
        n_parts, nbytes = 0, 0
        for n in range(1, 9):  # equal parts: the fewest launches whose workgroups fit the chip
            if n > B:
                break
            nbytes = L.sfsn_hop_scratch_bytes(ctypes.byref(make_desc(-(-B // n), Pool(), probe.data_ptr())[0]))
            if nbytes:
                n_parts = n
                break
        if not n_parts:
            return None
        per = -(-B // n_parts)
        enh = torch.zeros((B, S, F, hop, 2), dtype=torch.float32, device=dev)
        mag = torch.zeros((B, S, F, hop), dtype=torch.float32, device=dev)
        wave_out = torch.zeros((B, S, self._outer), dtype=self._fmt_dtype, device=dev) if self.waveform else None
        host = None
        if self.host_io:  # pinned host memory the kernel reads / writes directly (hipHostMalloc: device-reachable at the same address)
            host = dict(inp=torch.zeros((B, self._outer), dtype=self._fmt_dtype).pin_memory(),
                        out=torch.zeros((B, S, self._outer), dtype=self._fmt_dtype).pin_memory(),
                        done=torch.zeros((B * S,), dtype=torch.int32).pin_memory())
            host["done_np"] = host["done"].numpy()
            host["bell"] = torch.zeros((16,), dtype=torch.int32).pin_memory()  # the resident kernel's doorbell (word 0)
            host["bell_np"] = host["bell"].numpy().view("uint32")
            if self.resident:  # the clips' origins, read by the resident kernel after each doorbell (see reset(clips))
                host["origin"] = torch.zeros((B,), dtype=torch.int32).pin_memory()
                host["origin_np"] = host["origin"].numpy().view("uint32")
        parts = []
        for b0 in range(0, B, per):
            nb = min(per, B - b0)
            spool = Pool()
            make_desc(nb, spool, probe.data_ptr())
            spool.allocate()
            desc, st = make_desc(nb, spool, b0=b0)
            desc.inp_ri = _ptr(self.inp)
            desc.enh_ri, desc.enh_mag = ptr(enh[b0:]), ptr(mag[b0:])
            if self.waveform:
                desc.wave_in, desc.wave_out = probe.data_ptr(), ptr(wave_out[b0:])  # (wave_in: set per call)
                if host is not None:
                    desc.wave_out, desc.done = ptr(host["out"][b0:]), ptr(host["done"][b0 * S:])
            io = None
            if self._io:  # the launch goes through sfsn_stream_hop_io: the descriptor's own sample pointers are ignored
                io = HopIo()
                io.ratio, io.format, io.wave_out = self.resample, self._fmt_code, desc.wave_out
                if self.resample == 3:
                    taps, phase_taps = spectral.resample_taps(dev)
                    io.dec_state, io.int_state, io.taps, io.phase_taps = ptr(st["dec"]), ptr(st["int"]), ptr(taps), ptr(phase_taps)
            # the clips' origins (launch index of each clip's frame 0): written by stream-ordered fills, handed to the launches from
            # the first reset(clips) on (until then the session-wide counters serve); a resident session reads pinned host memory
            origin = torch.zeros((nb,), dtype=torch.int32, device=dev)
            if self.resident:
                desc.clip_start = ptr(host["origin"][b0:])
            nbytes = L.sfsn_hop_scratch_bytes(ctypes.byref(desc))
            assert nbytes, "the sizing call accepted this geometry"
            slots = None
            if self.count_spikes:  # running spike counts, one word per lane that writes 4 neurons of a row (include/sfsn.h)
                n = L.sfsn_hop_spike_slots(ctypes.byref(desc))
                # (resident: pinned host memory, read by the host while the launch runs; otherwise device memory, summed in stream order)
                slots = torch.zeros((n,), dtype=torch.int32).pin_memory() if self.resident else torch.zeros((n,), dtype=torch.int32, device=dev)
                desc.spike_slots = ptr(slots)
            scratch = torch.zeros((nbytes // 4 + 1,), dtype=torch.int32, device=dev)  # word 0: the error flag
            desc.scratch, desc.scratch_bytes = ptr(scratch), nbytes
            # the error word of a launch is looked at, without blocking, at a later step (pinned copy behind the launch)
            parts.append(dict(desc=desc, ref=ctypes.byref(desc), io=io, io_ref=None if io is None else ctypes.byref(io), b0=b0, nb=nb, st=st, spool=spool.buf, scratch=scratch, origin=origin, slots=slots,
                              err=torch.zeros((1,), dtype=torch.int32).pin_memory(), err_pending=False))
        return dict(parts=parts, desc=parts[0]["desc"], scratch=parts[0]["scratch"], wpool=wpool.buf, enh=torch.view_as_complex(enh),
                    mag=mag, wave_out=wave_out, host=host, bounds=[(part["b0"], part["nb"]) for part in parts], held_before=False)

    def _launch_hops(self, base_ptr: int, stride_bytes: int, field: str, frame_index=None, held=None) -> None:
        """One sfsn_stream_hop launch per part, back to back on torch's current stream; `field` of each descriptor is pointed at
        the part's slice of the caller's input (clips are the slowest axis: a part is a contiguous range).  `held`: per part the mask
        words of the clips that sit this hop out (clip_select.held_masks); a part with a held clip is launched through
        sfsn_stream_hop_held (still one launch; a part held as a whole is launched too: every part carries the same launch index),
        a part without one through sfsn_stream_hop."""
        idx, lib = self._dev_index, self.eng.lib
        st = ctypes.c_void_p(_raw_stream(idx))
        same = torch.cuda.current_device() == idx  # the C ABI launches on the calling thread's current device
        for pi, part in enumerate(self._hop["parts"]):
            if part["err_pending"] and int(part["err"][0]) != 0:  # written behind an earlier launch; no blocking here
                self.check_errors()  # (synchronises, clears the sticky words and raises)
            d = part["desc"]
            d.frames_before = self.frames_done
            setattr(d if part["io"] is None else part["io"], field, base_ptr + part["b0"] * stride_bytes)
            if frame_index is not None:
                d.frame_index = frame_index
            if part["io"] is not None:  # (outer samples: waveform sessions only, field is "wave_in")
                words = (ctypes.c_uint64 * len(held[pi]))(*held[pi]) if held is not None and any(held[pi]) else None
                name, fn, args = "sfsn_stream_hop_io", lib.sfsn_stream_hop_io, (part["ref"], part["io_ref"], words, st)
            elif held is not None and any(held[pi]):
                name, fn, args = "sfsn_stream_hop_held", lib.sfsn_stream_hop_held, (part["ref"], (ctypes.c_uint64 * len(held[pi]))(*held[pi]), st)
            else:
                name, fn, args = "sfsn_stream_hop", lib.sfsn_stream_hop, (part["ref"], st)
            if same:
                rc = fn(*args)
            else:
                with torch.cuda.device(self.dev):
                    rc = fn(*args)
            if rc:
                check(rc, name)
            d.launch_index += 1
        self.frames_done += self.hop
        if self.frames_done % 256 < self.hop:  # every ~256 frames the error words follow the launches into pinned memory
            self._error_words_follow(self._hop["parts"])

    # -----------------------------------------------------------------------------------------------------------------
    def reset(self, clips=None) -> None:
        """Back to the start of an utterance: zero (h, c) (modeling_spiking_fullsubnet.py:100-106) and zero history.

        ``clips`` (a sequence or 1-D tensor of clip indices; duplicates allowed, empty = nothing): only these clips start a new
        utterance, at their next call; the others go on as if nothing happened.  A restarted clip then behaves exactly like a fresh
        session fed the same input (waveform mode: zeros for its first three calls, then the samples of three calls earlier; the
        cumulative norm divides by its own frame count).  Ordered with the steps on torch's current stream: no synchronisation, and
        a resident launch keeps running.  ``clips=None``: every clip, the whole session (ends a resident launch; also checks that the
        module's parameters have not changed since the session packed them -- a walk over the state dict that a per-clip restart,
        issued between hops, does not pay)."""
        if clips is not None:
            self._reset_clips(clips)
            return
        self._check_owner()
        for d in (self.fb, self.sb):
            for layer in d["states"]:
                for h, c in layer:
                    h.zero_()
                    c.zero_()
        self.hist.zero_()
        self._stop_resident()
        if self._hop is not None:
            self.check_errors()
            for part in self._hop["parts"]:
                part["spool"].zero_()  # (h, c), tagged spike buffers, history, waveform state: one fill per part
                part["origin"].fill_(self._as_i32(part["desc"].launch_index))  # every clip's frame 0 is the next launch
                if part["slots"] is not None:
                    part["slots"].zero_()  # (pinned: the resident launch has ended)
            if self.resident:
                self._hop["host"]["origin_np"][:] = self._hop["parts"][0]["desc"].launch_index  # (the kernel has ended)
            self._wave_calls = 0
            self._primed = False
        if self._rows is not None:
            self._rows.zero_()
        self.frames_done = 0
        self._clip_f0[:] = 0
        self._clip_c0[:] = 0

    def set_norm_stats(self, stats: NormStats, clips=None) -> None:
        """Replace the statistics of every clip (``stats`` of the session's batch) or of ``clips`` (``stats`` of ``len(clips)`` clips,
        in that order; distinct indices).  Ordered with the steps on torch's current stream: hops already queued still read the old
        values.  A resident launch is ended first, as by ``reset()``.  Nothing of the statistics is state, so with
        ``reset(clips=[b])`` this starts a new utterance with its own statistics on clip b while the others go on."""
        if self._stats is None:
            raise ValueError("set_norm_stats: this session's model takes no utterance statistics")
        if clips is None:
            idx = None
            n = self.B
        else:
            idx = clip_indices(clips, self.B, "set_norm_stats", duplicates="refuse", empty="ok")
            if not idx:
                return
            n = len(idx)
        stats.validate(self.eng.spec, n, self.dev)
        self._stop_resident()
        sel = None if idx is None else torch.tensor(idx, dtype=torch.long).to(self.dev, non_blocking=True)
        for mine, new in ((self._stats.mu_fb, stats.mu_fb), (self._stats.mu_sb, stats.mu_sb), (self._stats.sd_fb, stats.sd_fb),
                          (self._stats.sd_sb, stats.sd_sb)):
            if mine is None:
                continue
            if sel is None:
                mine.copy_(new)
            else:
                mine.index_copy_(-1, sel, new)

    def _refuse_resident(self, what: str) -> None:
        if self.resident:
            raise NotImplementedError(f"{what}: not on a resident session (resident=True): its launch holds the state while it runs")

    def _refuse_outer(self, what: str) -> None:
        if self._io:
            raise NotImplementedError(f"{what}: not on a session with resample={self.resample!r}, sample_format={self.sample_format!r} "
                                      "(a recorded prefix or backlog in outer samples is a follow-up: open a plain session for it)")

    # ---- holding clips: a hop that advances only some clips of the batch ----------------------------------------------------------
    def _hold(self, clips, what: str):
        """``clips=`` (not None) of a step: None where every clip is listed; otherwise
        ``(active, held, per-part mask words)`` (clip_select.held_masks).  The one-launch tier's parts take the clips' own origins
        from now on, the way ``_reset_clips`` switches them at the first per-clip reset."""
        self._refuse_resident(f"{what}(clips=...)")
        h = self._hop
        active, held, words = held_masks(clips, self.B, [(0, self.B)] if h is None else h["bounds"], what)
        if not held:
            return None
        if h is not None and not h["held_before"]:  # (once: nothing ever takes a part back to the session-wide counters)
            h["held_before"] = True
            for part in h["parts"]:
                part["desc"].clip_start = part["origin"].data_ptr()
        # (waveform: no clip is older than the session's call count, so step_wave's zeros for the first three calls stay right, and
        #  from then on the launch mutes each clip by its own frame index)
        return active, held, words

    def _first_wave_call(self, src: torch.Tensor, hold) -> None:
        """A waveform session's first call launches nothing: the samples of the clips that make it enter the STFT state (``src``:
        [B, 128] on the device or pinned).  A held clip does not make it: its origin moves on by one launch (a stream-ordered add
        behind the queued launches), so that the next launch is ITS first call."""
        held = set() if hold is None else set(hold[1])
        for part in self._hop["parts"]:
            b0, nb = part["b0"], part["nb"]
            for i0, m in runs([b - b0 for b in range(b0, b0 + nb) if b not in held]):
                rows = src[b0 + i0:b0 + i0 + m]
                if self._io:  # outer samples: what the launch's first stage does to them, by the stand-alone kernels (same bits)
                    rows = rows.to(self.dev, non_blocking=True)
                    if self.resample == 3:
                        rows, _ = spectral.resample_down3(rows, state=part["st"]["dec"][i0:i0 + m])
                    else:
                        rows = rows.to(torch.float32) * (1.0 / 32768.0)
                part["st"]["state"][i0:i0 + m, 384:].copy_(rows)
            for i0, m in runs([b - b0 for b in range(b0, b0 + nb) if b in held]):
                part["origin"][i0:i0 + m].add_(1)
        if hold is not None:
            self._clip_c0[hold[1]] += 1

    def _reset_clips(self, clips) -> None:
        idx = clip_indices(clips, self.B, "reset", duplicates="merge_late", empty="ok")
        if not idx:
            return
        self._clip_f0[idx] = self.frames_done
        self._clip_c0[idx] = self._wave_calls
        if self._hop is None:  # the per-kernel sequence: zero the clips' rows of the states and their history, in stream order
            spec = self.eng.spec
            for d, units in ((self.fb, [1]), (self.sb, [spec.units(g) for g in range(spec.n_groups)])):
                for layer in d["states"]:
                    for (h, c), u in zip(layer, units):
                        for b in idx:
                            h[b * u:(b + 1) * u].zero_()
                            c[b * u:(b + 1) * u].zero_()
            for b in idx:
                self.hist[b].zero_()
                if self._rows is not None:
                    self._rows[:, b].zero_()
            return
        # the launch that will compute each clip's frame 0: the next one -- in waveform mode the one after (the next call is the
        # clip's first, which has no frame yet), unless the session itself is at its first call (which launches nothing)
        h = self._hop
        nxt = h["parts"][0]["desc"].launch_index + (self._res["k"] if self._res is not None else 0)
        org = nxt + (1 if self.waveform and self._wave_calls > 0 else 0)
        if self.resident:
            # pinned host memory: the previous hop's done words are in, and the next doorbell orders this write before the hop
            h["host"]["origin_np"][idx] = org & 0xFFFFFFFF
            return
        for part in h["parts"]:
            mine = [b - part["b0"] for b in idx if part["b0"] <= b < part["b0"] + part["nb"]]
            for i in mine:  # (a fill behind the queued launches: none of them sees the new origin)
                part["origin"][i:i + 1].fill_(self._as_i32(org))
            part["desc"].clip_start = part["origin"].data_ptr()  # from now on the launches take the clips' own origins

    # ---- priming: a recorded prefix through the offline kernels, its end state into the session ---------------------------------
    def _prime_clips(self, clips, n_given: int, what: str = "prime"):
        """(clip indices in the caller's order, the permutation that sorts them or None) of a prime / advance call."""
        idx = clip_indices(clips, self.B, what, duplicates="refuse", empty="refuse")
        if n_given != len(idx):
            raise RuntimeError(f"{what}: {'a prefix' if what.startswith('prime') else 'a backlog'} of {n_given} clips for {len(idx)} clip indices")
        return idx, slot_order(idx)[1]

    def _slot_ordered(self, rows, idx, order, run):
        """``run(rows, idx)`` -> a tuple of tensors with one row per clip, called with the rows and the clip indices in slot order
        (``order``: ``_prime_clips``'; None: they are) and its results put back into the caller's order."""
        if order is None:
            return run(rows, idx)
        perm = torch.tensor(order, dtype=torch.long).to(self.dev, non_blocking=True)
        res = run(rows.index_select(0, perm), [idx[j] for j in order])
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(len(order), device=self.dev)
        return tuple(t.index_select(0, inv) for t in res)

    def _put_states(self, es, idx) -> None:
        """The per-kernel sequence: rows of an offline forward's end state ``es`` into the (h, c) of the clips ``idx`` (ascending)."""
        spec = self.eng.spec
        units = [1] + [spec.units(g) for g in range(spec.n_groups)]
        for d, e, us in ((self.fb, es["fb"], units[:1]), (self.sb, es["sb"], units[1:])):
            for mine, theirs in zip(d["states"], e["states"]):
                for (h, c), (hs, cs), u in zip(mine, theirs, us):
                    j0 = 0  # (idx ascends: a run of consecutive clips is a run of consecutive rows on both sides)
                    for b0, m in runs(idx):
                        h[b0 * u:(b0 + m) * u].copy_(hs[j0 * u:(j0 + m) * u])
                        c[b0 * u:(b0 + m) * u].copy_(cs[j0 * u:(j0 + m) * u])
                        j0 += m

    def _part_chunks(self, idx) -> list:
        """``idx`` ascending: [(part, [(first position, local clip indices), ...])] for the parts that hold some of the clips, each
        part's clips in chunks of 256 at most (a launch takes 256 clip indices in its arguments)."""
        out = []
        for part, j0, local in self._part_runs(idx):
            if not out or out[-1][0] is not part:
                out.append((part, []))
            out[-1][1].append((j0, local))
        return out

    def _part_launch(self, name: str, part, local, arg, st) -> None:
        """One ``sfsn_hop_prime`` / ``_seed`` / ``_advance`` launch: clips ``local`` of ``part``, ``arg`` the launch's source / sink."""
        arr = (ctypes.c_int * len(local))(*local)
        with torch.cuda.device(self.dev):
            rc = getattr(self.eng.lib, name)(part["ref"], arr, len(local), ctypes.byref(arg), st)
        if rc:
            check(rc, name)

    def _chunk_launches(self, name: str, part, chunks, arg, st):
        """``_part_launch`` for every chunk of ``part`` (``_part_chunks``'); returns the runs of the part's clips launched for."""
        for j0, local in chunks:
            arg.b0 = j0
            self._part_launch(name, part, local, arg, st)
        return runs([b for _, local in chunks for b in local])

    def _end_state_ptrs(self, src, es) -> None:
        """The ``fb`` / ``sb[g]`` of a ``PrimeSrc`` / ``AdvanceSrc``: the spikes, membranes and running sums of an offline forward's
        end state ``es``."""
        ng = self.eng.spec.n_groups
        for o, e, gi in [(src.fb, es["fb"], 0)] + [(src.sb[g], es["sb"], g) for g in range(ng)]:
            for l in range(len(e["s8"])):
                o.layer[l].spikes_i8, o.layer[l].c = e["s8"][l][gi].data_ptr(), e["states"][l][gi][1].data_ptr()
        if es["cum"] is not None:
            src.fb.cum = es["cum"][0].data_ptr()
            for g in range(ng):
                src.sb[g].cum = es["cum"][1 + g].data_ptr()

    def _offline_forward(self, stft, idx, end_state, frames=None):
        """The offline forward of the clips ``idx``' frames ``stft`` with the session's statistics of those clips; ``end_state``:
        True (from zero) or the start buffers it continues from; ``frames``: the clips' own counts of new frames (a start made with
        ``per_clip_ends``)."""
        eng = self.eng
        ns = None if self._stats is None else (self._stats if len(idx) == self.B else self._stats.select(idx))
        # (the per-kernel sequence's layer-0 membranes are those of ITS input product, the form below 64 rows: these frames take it too)
        eng._l0_hop = self.hop if self._hop is None else None
        try:
            return eng.forward_stft(stft, want_layers=False, want_counts=self._rows is not None, norm_stats=ns, _end_state=end_state,
                                    frames=frames)
        finally:
            eng._l0_hop = None

    def _first_call_made(self, idx) -> None:
        """Waveform sessions, before clips ``idx`` take a state from outside: when nobody has called yet -- the session's first call
        launches nothing -- count that call as made, with every other clip's utterance beginning at the next call (origin = the
        launch after the next: that launch is their first call)."""
        if not self.waveform or self._wave_calls != 0:
            return
        self._wave_calls = 1
        self._clip_c0[:] = 1
        listed = set(idx)
        for part in self._hop["parts"]:
            others = [b - part["b0"] for b in range(part["b0"], part["b0"] + part["nb"]) if b not in listed]
            for b0, m in runs(others):
                part["origin"][b0:b0 + m].fill_(self._as_i32(part["desc"].launch_index + 1))
            part["desc"].clip_start = part["origin"].data_ptr()

    def _prime_sorted(self, stft, idx, tail=None):
        """The transplant.  ``stft``: complex64 [len(idx), F, N] contiguous, or None (waveform mode, no frame yet); ``idx`` ascending;
        ``tail``: waveform mode, float32 [len(idx), 512].  Returns the prefix's forward (None without frames).  Everything on torch's
        current stream."""
        n, N, hop = len(idx), (0 if stft is None else stft.shape[-1]), self.hop
        out = es = None
        if N:
            out = self._offline_forward(stft, idx, True)
            es = out["end_state"]
        if self._hop is None:
            # the per-kernel sequence: row copies into the states, the history and the counts the (captured) launches read and write
            self._put_states(es, idx)
            Th = self.Th
            for j, b in enumerate(idx):  # the last D + hop frames, zeros in front of a shorter prefix
                if N >= Th:
                    self.hist[b].copy_(stft[j, :, N - Th:])
                else:
                    self.hist[b, :, :Th - N].zero_()
                    self.hist[b, :, Th - N:].copy_(stft[j])
                if self._rows is not None:
                    self._rows[:, b].copy_(es["counts"][:, j])
            return out
        st = ctypes.c_void_p(_raw_stream(self._dev_index))
        src = PrimeSrc()
        src.Bp, src.N = n, N
        if N:
            src.stft_ri = torch.view_as_real(stft).data_ptr()
            src.enh_ri = torch.view_as_real(out["enh_stft"]).data_ptr()
            self._end_state_ptrs(src, es)
        if tail is not None:
            src.wave_tail = tail.data_ptr()
        for part, chunks in self._part_chunks(idx):
            d = part["desc"]
            # the clips' origin: launch_index is the next launch, which gives them frame index N / hop.  (N = 0, a waveform clip
            # whose first call has made no frame: the origin IS the next launch, which reads the state as zero -- as it must -- and
            # the samples from wave_state, which no origin makes it skip)
            org = self._as_i32(d.launch_index - N // hop)
            for b0, m in self._chunk_launches("sfsn_hop_prime", part, chunks, src, st):
                part["origin"][b0:b0 + m].fill_(org)  # (fills behind the queued launches, as in _reset_clips)
            d.clip_start = part["origin"].data_ptr()
        return out

    def prime(self, stft: torch.Tensor, clips=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Start a new utterance on ``clips`` (``None``: every clip) whose first ``N`` frames are the recorded prefix ``stft`` --
        complex64 [len(clips), F, N] on the device, row i for ``clips[i]`` -- at the speed of the offline forward instead of
        ``N / hop`` calls of ``step``.  Returns the prefix's ``(enh_stft [.., S, F, N], enh_mag)``; the next ``step`` continues as if
        the prefix had been streamed: bit for bit in the per-kernel tier, and in the one-launch tier with that tier's one
        reservation (layer 0's membranes are the offline forward's, which differ from the hop's in their low bits -- include/sfsn.h).
        Whatever state the clips held is replaced; the other clips go on untouched.  ``N`` is a multiple of ``hop``, at least
        ``hop`` (``ValueError``): a clip's origin is a launch index.  A frozen model with an offline norm runs the prefix with the
        session's current statistics of those clips.  Ordered on torch's current stream, no synchronisation, like
        ``reset(clips=...)``.  Not on resident sessions (``NotImplementedError``); every listed clip gets the same ``N``."""
        self._refuse_resident("prime")
        if self.waveform:
            raise RuntimeError("this session was opened with waveform=True: use prime_wave(samples)")
        idx, order = self._prime_clips(clips, stft.shape[0] if isinstance(stft, torch.Tensor) and stft.dim() == 3 else -1)
        N = check_frames("prime", stft, len(idx), self.F, self.dev, self.hop)

        def run(rows, slots):
            out = self._prime_sorted(rows.contiguous(), slots)
            return out["enh_stft"], out["enh_mag"]

        enh, mag = self._slot_ordered(stft, idx, order, run)
        if clips is None:  # the whole session: as after reset() and N frames of step()
            self.frames_done = N
            self._clip_f0[:] = 0
        else:
            self._clip_f0[idx] = self.frames_done - N
        return enh, mag

    def prime_wave(self, samples: torch.Tensor, clips=None) -> torch.Tensor:
        """``prime`` for waveform sessions (``host_io`` included; device tensors in and out): ``samples`` float32
        [len(clips), 128 * c], ``c >= 1`` calls' worth.  Returns [.., S, 128 * c], the concatenation of what ``c`` calls of
        ``step_wave`` would have returned (the first three blocks are zero).  The prefix has the frames ``0 .. c - 2``: the two
        further frames torch.stft(center=True) makes of these samples look into samples not yet heard and are not used; ``c = 1``
        has no frame, its samples only enter the STFT state."""
        self._refuse_resident("prime_wave")
        self._refuse_outer("prime_wave")
        if not self.waveform:
            raise RuntimeError("open the session with waveform=True")
        idx, order = self._prime_clips(clips, samples.shape[0] if isinstance(samples, torch.Tensor) and samples.dim() == 2 else -1)
        Ls = check_samples("prime_wave", samples, len(idx), self.dev)
        from . import spectral
        c, n, S = Ls // 128, len(idx), self.eng.spec.num_spks

        def run(rows, slots):
            rows = rows.contiguous()
            tail = rows[:, -512:].contiguous() if Ls >= 512 else torch.nn.functional.pad(rows, (512 - Ls, 0))
            stft = spectral.stft(rows, 512, 128)[:, :, :c - 1].contiguous() if c > 1 else None  # frames 0 .. c - 2 (see above)
            out = self._prime_sorted(stft, slots, tail=tail)
            res = torch.zeros((n, S, Ls), dtype=torch.float32, device=self.dev)
            if c > 3:  # calls 3 .. c - 1 return samples [0, 128 (c - 3)): complete with frame c - 2, the last one the prefix has
                res[:, :, 384:] = spectral.istft(out["enh_stft"].reshape(n * S, self.F, c - 1), 512, 128, length=128 * (c - 3)).view(n, S, -1)
            if clips is not None:
                self._first_call_made(slots)
            return (res,)

        res, = self._slot_ordered(samples, idx, order, run)
        if clips is None:  # the whole session: as after reset() and c calls of step_wave()
            self._wave_calls, self.frames_done = c, c - 1
            self._clip_c0[:] = 0
        else:
            self._clip_c0[idx] = self._wave_calls - c
        self._primed = True
        return res

    # ---- a backlog on running clips: the offline kernels from the carried state, their end state back into the session -----------
    def _advance_sorted(self, stft, idx, samples=None, lens=None):
        """``stft``: complex64 [len(idx), F, N], or None in waveform mode, where ``samples`` float32 [len(idx), 128 * N] contiguous
        give the frames; ``idx`` ascending.  Returns (the forward of the N new frames, the waveform blocks or None).  Everything on
        torch's current stream.  ``lens`` (``advance_ragged``): clip ``idx[i]`` has ``lens[i]`` of the N frames, the rest of its row is
        padding -- the same seed and forward, zeroed padding, and every clip's end taken at its own last frame
        (``_take_ragged``)."""
        eng, spec = self.eng, self.eng.spec
        n, hop, D, ng, dev = len(idx), self.hop, self.D, spec.n_groups, self.dev
        N = stft.shape[-1] if samples is None else samples.shape[1] // 128
        T = D + N
        start = eng._start_buffers(n, N, D, frames_before=int(self.clip_frames[idx[0]]), per_clip_ends=lens is not None)
        buf = start["stft"]
        units = [1] + [spec.units(g) for g in range(ng)]
        st = ctypes.c_void_p(_raw_stream(self._dev_index))
        wbuf = None
        if self._hop is None:
            # the per-kernel sequence: the clips' rows of its states and the last D frames of its history window
            sel = torch.tensor(idx, dtype=torch.long).to(dev, non_blocking=True)
            for d, e, us in ((self.fb, start["fb"], units[:1]), (self.sb, start["sb"], units[1:])):
                for mine, theirs in zip(d["states"], e):
                    for (h, c), (hs, cs), u in zip(mine, theirs, us):
                        hs.view(n, -1).copy_(h.view(self.B, -1).index_select(0, sel))
                        cs.view(n, -1).copy_(c.view(self.B, -1).index_select(0, sel))
            if D:
                buf[:, :, :D].copy_(self.hist.index_select(0, sel)[:, :, hop:])
        else:
            dst = SeedDst()
            dst.Bp, dst.T = n, T
            if D:
                dst.stft_ri = torch.view_as_real(buf).data_ptr()
            if samples is not None:  # [384 samples of context | the new samples]
                wbuf = torch.empty((n, 384 + 128 * N), dtype=torch.float32, device=dev)
                dst.wave_ctx, dst.wave_stride = wbuf.data_ptr(), wbuf.shape[1]
            for o, e, gi in [(dst.fb, start["fb"], 0)] + [(dst.sb[g], start["sb"], g) for g in range(ng)]:
                for l in range(len(e)):
                    o.layer[l].h, o.layer[l].c = e[l][gi][0].data_ptr(), e[l][gi][1].data_ptr()
            if start["cum"] is not None:
                dst.fb.cum = start["cum"][0].data_ptr()
                for g in range(ng):
                    dst.sb[g].cum = start["cum"][1 + g].data_ptr()
            for part, chunks in self._part_chunks(idx):
                part["desc"].clip_start = part["origin"].data_ptr()  # the clips' own origins from now on (they say which clip is fresh)
                self._chunk_launches("sfsn_hop_seed", part, chunks, dst, st)
        if samples is not None:
            from . import spectral
            wbuf[:, 384:].copy_(samples)
            # frame j of the backlog covers samples [128 j, 128 j + 512) of the buffer: the centred frame j + 2
            stft = spectral.stft(wbuf, 512, 128)[:, :, 2:2 + N]
        if lens is not None:
            from . import ragged
            fdev = ragged.upload(lens, dev)  # (pinned, on the current stream: no synchronisation)
            keep = torch.arange(N, device=dev).unsqueeze(0) < fdev.unsqueeze(1)
            # the padding reads as zero whatever the caller left there: the scans run over it, and nothing of it may be NaN
            buf[:, :, D:].copy_(torch.where(keep.unsqueeze(1), stft, torch.zeros((), dtype=stft.dtype, device=dev)))
            out = self._offline_forward(buf, idx, start, frames=lens)
            return out, self._take_ragged(out, buf, idx, lens, fdev, wbuf, st)
        buf[:, :, D:].copy_(stft)
        out = self._offline_forward(buf, idx, start)
        es = out["end_state"]
        if self._hop is None:
            self._put_states(es, idx)
            for j, b in enumerate(idx):  # the last D + hop frames of [history | new] (N >= hop: the buffer has them)
                self.hist[b].copy_(buf[j, :, T - self.Th:])
            if self._rows is not None:
                self._rows.index_add_(1, sel, es["counts"])
            return out, None
        src = AdvanceSrc()
        src.Bp, src.N, src.T = n, N, T
        src.stft_ri = torch.view_as_real(buf).data_ptr()
        self._end_state_ptrs(src, es)
        res = tail = None
        if samples is not None:
            enh = out["enh_stft"]  # (the new frames of the forward's [.., T] rows: the launch takes the rows)
            src.enh_ri = enh.data_ptr() - D * enh.element_size()
            tail = wbuf[:, -512:].contiguous()
            res = torch.empty((n, spec.num_spks, 128 * N), dtype=torch.float32, device=dev)
            src.wave_tail, src.wave_out = tail.data_ptr(), res.data_ptr()
        for part, chunks in self._part_chunks(idx):
            # the clips' origins move back by the backlog's launches (32-bit wrap-around, as the launch's unsigned difference), behind
            # the queued launches: the next launch continues N / hop frame indices further
            for b0, m in self._chunk_launches("sfsn_hop_advance", part, chunks, src, st):
                part["origin"][b0:b0 + m].sub_(N // hop)
        return out, res

    def _take_ragged(self, out, buf, idx, lens, fdev, wbuf, st):
        """The end of ``_advance_sorted`` with per-clip lengths: each clip ``idx[i]``'s state after ITS OWN last new frame
        ``lens[i] - 1`` into the session -- the spikes' row, the membrane tap's row (the scans' c_state is the one after the last
        padded frame), the history and the samples that end there, the counts over its own frames -- and its origin back by its own
        launches.  One-launch tier: ``sfsn_hop_advance_ragged``; per-kernel tier: row gathers.  Returns the waveform blocks or None."""
        spec = self.eng.spec
        n, hop, D, ng, dev = len(idx), self.hop, self.D, spec.n_groups, self.dev
        T = buf.shape[-1]
        N = T - D
        es = out["end_state"]
        if self._hop is None:
            last = (fdev - 1).long()
            rows = torch.arange(n, device=dev)
            units = [1] + [spec.units(g) for g in range(ng)]
            ends = {}
            for key, us in (("fb", units[:1]), ("sb", units[1:])):
                e = es[key]
                # (h as the scans take it: fp32 0 / 1 -- the int8 spikes of the clip's last frame, without the rows' padding columns)
                ends[key] = dict(states=[[(s8.view(N, n, u, -1)[last, rows][..., :m.shape[-1]].reshape(n * u, -1).float(),
                                           m.view(N, n, u, -1)[last, rows].reshape(n * u, -1))
                                          for s8, m, u in zip(s8s, ms, us)] for s8s, ms in zip(e["s8"], e["mem"])])
            self._put_states(ends, idx)
            for j, b in enumerate(idx):  # the D + hop frames that end with the clip's own last one (lens[j] >= hop: the row has them)
                self.hist[b].copy_(buf[j, :, D + lens[j] - self.Th:D + lens[j]])
            if self._rows is not None:
                self._rows.index_add_(1, torch.tensor(idx, dtype=torch.long).to(dev, non_blocking=True), es["counts"])
            return None
        src = AdvanceRaggedSrc()
        src.Bp, src.Nmax, src.T = n, N, T
        nd = es["frames_dev"]
        src.frames = nd.data_ptr()
        src.stft_ri = torch.view_as_real(buf).data_ptr()
        for o, e, gi in [(src.fb, es["fb"], 0)] + [(src.sb[g], es["sb"], g) for g in range(ng)]:
            for l in range(len(e["s8"])):
                o.layer[l].spikes_i8, o.layer[l].membrane = e["s8"][l][gi].data_ptr(), e["mem"][l][gi].data_ptr()
        res = None
        if wbuf is not None:
            enh = out["enh_stft"]  # (the new frames of the forward's [.., T] rows: the launch takes the rows)
            src.enh_ri = enh.data_ptr() - D * enh.element_size()
            res = torch.empty((n, spec.num_spks, 128 * N), dtype=torch.float32, device=dev)
            src.wave_ctx, src.wave_stride, src.wave_out = wbuf.data_ptr(), wbuf.shape[1], res.data_ptr()
        back = nd // hop if hop > 1 else nd  # each clip's own launches
        for part, chunks in self._part_chunks(idx):
            for j0, local in chunks:
                src.b0 = j0
                self._part_launch("sfsn_hop_advance_ragged", part, local, src, st)
            # the clips' origins move back by their own launches, behind the queued launches (32-bit wrap-around, as in _advance_sorted)
            for j0, local in chunks:
                for b0, m in runs(local):
                    part["origin"][b0:b0 + m].sub_(back[j0:j0 + m])
                    j0 += m
        return res

    def _advance_checks(self, what: str, idx) -> None:
        spec = self.eng.spec
        if spec.cum_laplace:
            ages = self.clip_frames[idx]
            if (ages != ages[0]).any():
                raise ValueError(f"{what}: with cumulative_laplace_norm the clips of one call must have seen the same number of frames, "
                                 f"clips {list(idx)} have seen {ages.tolist()}: make one call per age")

    def advance(self, stft: torch.Tensor, clips=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Run a BACKLOG of ``N`` frames on clips that are already running, at the speed of the offline forward: ``stft`` complex64
        [len(clips), F, N] on the device, row i for ``clips[i]`` (``None``: every clip).  The clips continue from whatever state
        they hold; the result ``(enh_stft [.., S, F, N], enh_mag)`` is what ``N / hop`` calls of ``step`` would have returned for
        them, and the session is left where those calls would have left them -- last spikes, membranes, cumulative-norm sums,
        deep-filter history, spike counts (``count_spikes=True``), ``clip_frames``.  The other clips are untouched.  A fresh clip
        (never stepped, or just ``reset``) reads as zero state whatever memory holds: ``advance`` on it equals ``prime``.  Repeated
        calls process a long recording in chunks.

        The offline kernels run on the new frames behind ``D`` frames of the clip's history, from the carried state
        (``Engine.forward_stft(..., _end_state=start)``).  The one-launch tier reads the state out in one launch
        (``sfsn_hop_seed``) and takes the end state back in one (``sfsn_hop_advance``, csrc/sfsn_prime.hip), then moves the clips'
        origins back by ``N / hop`` launches; the per-kernel tier uses row copies.  Exactness: bit for bit in the per-kernel tier;
        in the one-launch tier ``prime``'s one reservation and no other -- the layer-0 membranes written back are the offline
        kernels', which differ from the hop's in their low bits; where no layer-0 membrane lies within that rounding of the
        threshold, every spike, higher-layer membrane, output and count is that of the ``step`` sequence, bit for bit.

        ``N``: a positive multiple of ``hop``, the same for every listed clip (``ValueError``).  With the cumulative norm the listed
        clips must share their frame count so far (``ValueError`` naming them: one call per age).  A frozen model with given
        statistics uses the session's rows of those clips.  Ordered on torch's current stream, no synchronisation.  Not on resident
        sessions (``NotImplementedError``), not across tiers, not for cIRM-GSN sessions."""
        self._refuse_resident("advance")
        if self.waveform:
            raise RuntimeError("this session was opened with waveform=True: use advance_wave(samples)")
        idx, order = self._prime_clips(clips, stft.shape[0] if isinstance(stft, torch.Tensor) and stft.dim() == 3 else -1, "advance")
        N = check_frames("advance", stft, len(idx), self.F, self.dev, self.hop)
        self._advance_checks("advance", idx)

        def run(rows, slots):
            out, _ = self._advance_sorted(rows, slots)
            return out["enh_stft"], out["enh_mag"]

        enh, mag = self._slot_ordered(stft, idx, order, run)
        self._clip_f0[idx] -= N
        # (reordered results are copies already; otherwise the new frames of the forward's [.., T] rows are made contiguous here)
        return (enh, mag) if order is not None else (enh.contiguous(), mag.contiguous())

    def advance_wave(self, samples: torch.Tensor, clips=None) -> torch.Tensor:
        """``advance`` for waveform sessions (``host_io`` included; device tensors in and out): ``samples`` float32
        [len(clips), 128 * c], ``c >= 1`` calls' worth.  Returns [.., S, 128 * c], the concatenation of what ``c`` calls of
        ``step_wave`` would have returned.  The new frames come from the last 384 samples of the clip's STFT state followed by the
        new samples (``spectral.stft``: the hop's transform, the same bits); the output blocks continue the clip's overlap-add
        accumulator in the hop's order and with its envelope.  Every listed clip must have made at least one call in its current
        utterance (``ValueError`` naming the clip; start such a clip with ``prime_wave``).  Exactness as for ``advance``."""
        self._refuse_resident("advance_wave")
        self._refuse_outer("advance_wave")
        if not self.waveform:
            raise RuntimeError("open the session with waveform=True")
        idx, order = self._prime_clips(clips, samples.shape[0] if isinstance(samples, torch.Tensor) and samples.dim() == 2 else -1, "advance_wave")
        Ls = check_samples("advance_wave", samples, len(idx), self.dev)
        calls = self.clip_calls
        for b in idx:
            if calls[b] < 1:
                raise ValueError(f"advance_wave: clip {b} has made no call in its current utterance (no STFT state to continue from): "
                                 "start it with prime_wave")
        self._advance_checks("advance_wave", idx)
        res, = self._slot_ordered(samples, idx, order, lambda rows, slots: self._advance_sorted(None, slots, samples=rows.contiguous())[1:])
        self._clip_c0[idx] -= Ls // 128
        self._primed = True  # the launch mutes each clip by its own frame index (see step_wave)
        return res

    def _ragged_refusals(self, what: str, lens) -> None:
        if self.eng.spec.cum_laplace:
            raise NotImplementedError(f"{what}: with cumulative_laplace_norm the sub-band running sums after a clip's own last frame "
                                      f"are not available from a padded forward (lengths {list(lens)}): make one `advance` call per length")

    def advance_ragged(self, stft: torch.Tensor, frames, clips=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``advance`` with a backlog of ITS OWN LENGTH per clip, in one call: ``stft`` complex64 [len(clips), F, Nmax] on the device,
        row i for ``clips[i]`` (``None``: every clip); ``frames``: a sequence or CPU int tensor, ``frames[i]`` the frames row i really
        holds -- a positive multiple of ``hop``, at most ``Nmax`` (``ValueError`` naming the clip; a wrong count of lengths is a
        ``ValueError`` too).  Whatever row i holds at frames ``>= frames[i]`` is ignored.

        The call returns, and leaves behind, exactly what the single-clip calls ``advance(stft[i:i+1, :, :frames[i]],
        clips=[clips[i]])`` would have: ``(enh_stft [.., S, F, Nmax], enh_mag)`` equal over each clip's own frames and zero past
        them; ``clip_frames``, the spike counts and every section of ``export_state`` equal bit for bit, the layer-0 membranes
        included (both sides run the offline kernels), in both tiers.  Unlisted clips are untouched, a fresh clip reads as zero state.

        One seed launch, ONE padded forward from the carried state (``Engine.forward_stft(..., frames=, _end_state=start)`` with the
        per-frame membrane tap: the scans' own end state is the one after the last padded frame) and one hand-back launch
        (``sfsn_hop_advance_ragged``) that takes every clip's rows at its own last frame and moves its origin back by its own
        launches; the per-kernel tier gathers the same rows.  The lengths go to the device from pinned memory: ordered on torch's
        current stream, no synchronisation.  Equal lengths: the call IS ``advance``.  Refused: resident sessions and, where the
        lengths differ, ``cumulative_laplace_norm`` models (``NotImplementedError``: one ``advance`` call per length); waveform
        sessions (``RuntimeError``: ``advance_wave_ragged``).  cIRM-GSN sessions: ``FullbandStreamingSession.catch_up_ragged``."""
        self._refuse_resident("advance_ragged")
        if self.waveform:
            raise RuntimeError("this session was opened with waveform=True: use advance_wave_ragged(samples, lengths)")
        idx, order = self._prime_clips(clips, stft.shape[0] if isinstance(stft, torch.Tensor) and stft.dim() == 3 else -1, "advance_ragged")
        if stft.device != self.dev or stft.dtype != torch.complex64 or stft.shape[1] != self.F:
            raise RuntimeError(f"expected complex64 {(len(idx), self.F, 'Nmax')} on {self.dev}, got {stft.dtype} {tuple(stft.shape)} on {stft.device}")
        Nmax = stft.shape[2]
        lens = clip_lengths("advance_ragged", frames, idx, self.hop, f"the session's hop ({self.hop})", Nmax, "frames")
        N = max(lens)

        def padded(t):  # zeros behind the longest clip, up to the caller's Nmax
            return t.contiguous() if N == Nmax else torch.nn.functional.pad(t, (0, Nmax - N))

        if min(lens) == N:
            enh, mag = self.advance(stft[..., :N], clips=clips)
            return padded(enh), padded(mag)
        self._ragged_refusals("advance_ragged", lens)
        own = dict(zip(idx, lens))

        def run(rows, slots):
            out, _ = self._advance_sorted(rows, slots, lens=[own[b] for b in slots])
            return out["enh_stft"], out["enh_mag"]

        enh, mag = self._slot_ordered(stft[..., :N], idx, order, run)
        self._clip_f0[idx] -= np.asarray(lens, dtype=self._clip_f0.dtype)
        return padded(enh), padded(mag)

    def advance_wave_ragged(self, samples: torch.Tensor, lengths, clips=None) -> torch.Tensor:
        """``advance_ragged`` for waveform sessions (``host_io`` included; device tensors in and out): ``samples`` float32
        [len(clips), 128 * cmax], ``lengths[i]`` the samples row i really holds, a positive multiple of 128 and at most
        ``128 * cmax``.  Returns [.., S, 128 * cmax]: over each clip's own samples what ``advance_wave(samples[i:i+1, :lengths[i]],
        clips=[clips[i]])`` returns, zeros behind; the session is left where those calls leave it (STFT state, overlap-add sums,
        ``clip_calls`` included).  Every listed clip must have made at least one call in its current utterance (``ValueError``
        naming the clip, as ``advance_wave``)."""
        self._refuse_resident("advance_wave_ragged")
        self._refuse_outer("advance_wave_ragged")
        if not self.waveform:
            raise RuntimeError("open the session with waveform=True")
        idx, order = self._prime_clips(clips, samples.shape[0] if isinstance(samples, torch.Tensor) and samples.dim() == 2 else -1, "advance_wave_ragged")
        if samples.device != self.dev or samples.dtype != torch.float32:
            raise RuntimeError(f"expected float32 {(len(idx), '128 * cmax')} on {self.dev}, got {samples.dtype} {tuple(samples.shape)} on {samples.device}")
        Lmax = samples.shape[1]
        lens = clip_lengths("advance_wave_ragged", lengths, idx, 128, "128", Lmax, "samples")
        Ls = max(lens)

        def padded(t):
            return t if Ls == Lmax else torch.nn.functional.pad(t, (0, Lmax - Ls))

        if min(lens) == Ls:
            return padded(self.advance_wave(samples[:, :Ls], clips=clips))
        calls = self.clip_calls
        for b in idx:
            if calls[b] < 1:
                raise ValueError(f"advance_wave_ragged: clip {b} has made no call in its current utterance (no STFT state to continue "
                                 "from): start it with prime_wave")
        self._ragged_refusals("advance_wave_ragged", lens)
        own = dict(zip(idx, lens))
        res, = self._slot_ordered(samples[:, :Ls], idx, order, lambda rows, slots: self._advance_sorted(
            None, slots, samples=rows.contiguous(), lens=[own[b] // 128 for b in slots])[1:])
        self._clip_c0[idx] -= np.asarray(lens, dtype=self._clip_c0.dtype) // 128
        self._primed = True  # the launch mutes each clip by its own frame index (see step_wave)
        return padded(res)

    # ---- moving a clip: its state out of its slot, and into a slot of this or another session ------------------------------------
    def _state_signature(self) -> tuple:
        """What two sessions must share for a clip to move between them (clip_state.py): the tier, the call geometry and every
        number of the model's geometry -- not the weights."""
        cached = getattr(self, "_signature", None)
        if cached is not None:
            return cached
        sig = [("model", "spiking_fullsubnet"), ("tier", "one_launch" if self._hop is not None else "per_kernel"), ("hop", self.hop),
               ("waveform", self.waveform), ("count_spikes", self.count_spikes), ("given_stats", self._stats is not None)]
        if self._io:  # (a plain session's signature is what it was: its states move to and from sessions made before these options)
            sig += [("resample", self.resample), ("sample_format", self.sample_format)]
        sig += [(k, tuple(v) if isinstance(v, list) else v) for k, v in dataclasses.asdict(self.eng.spec).items()
                if k not in ("bn", "proj_name")]
        self._signature = tuple(sig)
        return self._signature

    def _state_parts(self) -> list:
        """The per-kernel sequence's carried state as (section, [B, n] view): what a later step reads before it writes."""
        B, ng = self.B, self.eng.spec.n_groups
        parts = []
        for d, names in ((self.fb, ["fb"]), (self.sb, [f"sb{g}" for g in range(ng)])):
            for gi, name in enumerate(names):
                for l, layer in enumerate(d["states"]):
                    h, c = layer[gi]
                    parts += [(f"{name}.l{l}.h", h.view(B, -1)), (f"{name}.l{l}.c", c.view(B, -1))]
        parts.append(("hist", torch.view_as_real(self.hist).view(B, -1)))
        if self._rows is not None:
            parts.append(("rows", self._rows.t()))
        return parts

    def _make_state_layout(self):
        if self._hop is None:
            return layout_of([(name, t.shape[1] * t.element_size()) for name, t in self._state_parts()])
        spec, eng, d = self.eng.spec, self.eng, self._hop["desc"]
        ng = spec.n_groups
        seqs = [("fb", 1, eng.fb.H, spec.fb_layers)] + [(f"sb{g}", spec.units(g), eng.sb[g].H, spec.sb_layers) for g in range(ng)]
        fcov = max(d.sb[g].feat.lo + d.sb[g].feat.n_units * d.sb[g].fc for g in range(ng))
        layout, nbytes = hop_sections(seqs, spec.cum_laplace, self.count_spikes, fcov, self.D, self.waveform, spec.num_spks)
        assert nbytes == eng.lib.sfsn_hop_state_bytes(self._hop["parts"][0]["ref"]), "clip_state.hop_sections restates include/sfsn.h"
        self._launch_bytes = nbytes  # what sfsn_hop_state_export / _import move: the row's head
        if self.resample == 3:  # the two filters' carried samples behind it, moved by row copies beside the launch
            layout = layout + (("dec", nbytes, nbytes + 96 * 4), ("int", nbytes + 96 * 4, nbytes + 96 * 4 + spec.num_spks * 32 * 4))
            nbytes = layout[-1][2]
        return layout, nbytes

    def _filter_rows(self, name: str, idx, put=None):
        """The rows of clips ``idx`` (caller's order) of the carried filter samples ``name`` ("dec" / "int") as float32 [len(idx), n];
        ``put``: such rows, written into the session instead.  Stream-ordered row copies, one per run of ``_part_runs``."""
        rows = []
        for part, j0, local in self._part_runs(idx):
            t, sel = part["st"][name].view(part["nb"], -1), self._clip_rows(local)
            if put is None:
                rows.append(t.index_select(0, sel))
            else:
                t.index_copy_(0, sel, put[j0:j0 + len(local)])
        return None if put is not None else torch.cat(rows, dim=0)

    def _part_runs(self, idx) -> list:
        """[part, first position, local clip indices] for runs of consecutive positions of ``idx`` that lie in one part, 256 at most
        (what one sfsn_hop_state_export / _import launch takes: consecutive blob rows, clip indices in its arguments)."""
        parts = self._hop["parts"]
        return [(parts[p], j0, local) for p, j0, local in part_runs(idx, [(part["b0"], part["nb"]) for part in parts])]

    def export_state(self, clips=None):
        """The carried state of ``clips`` (``None``: every clip) as a ``ClipState`` of ``len(clips)`` rows, row i = ``clips[i]``: what
        ``import_state`` needs to continue those clips, bit for bit, in other slots of this session or in another session of equal
        signature (same model geometry, tier, hop, waveform / counting mode; see ``clip_state.py``) -- to compact a half-empty
        session into a smaller one, rebalance, pause a call (``state.to("cpu")``), rewind or fork it.  The one-launch tier copies the
        state in one launch per part touched (``sfsn_hop_state_export``); the per-kernel sequence gathers the clips' rows with
        stream-ordered copies.  The session is not changed: the clips go on here as well unless the caller resets them.  Ordered on
        torch's current stream with no synchronisation, like ``reset(clips=...)``: the state is that behind every step queued so
        far, and the call may return before the copy has run.  Not on resident sessions (``NotImplementedError``)."""
        self._refuse_resident("export_state")
        idx = clip_list(clips, self.B, "export_state")
        layout, nbytes = self._state_layout()
        if self._hop is None:
            blob = self._export_rows(idx, nbytes, layout)
        else:
            head = self._launch_bytes
            blob = new_blob(len(idx), head, layout if head == nbytes else layout[:-2], self.dev)
            st = ctypes.c_void_p(_raw_stream(self._dev_index))
            for part, j0, local in self._part_runs(idx):
                arr = (ctypes.c_int * len(local))(*local)
                with torch.cuda.device(self.dev):
                    rc = self.eng.lib.sfsn_hop_state_export(part["ref"], arr, len(local), ctypes.c_void_p(blob.data_ptr() + j0 * head), st)
                if rc:
                    check(rc, "sfsn_hop_state_export")
            if head != nbytes:
                blob = torch.cat([blob] + [self._filter_rows(name, idx).view(torch.uint8).view(len(idx), -1) for name in ("dec", "int")], dim=1)
        stats = None
        if self._stats is not None:
            s = self._stats.select(idx)
            stats = (s.mu_fb, s.mu_sb, s.sd_fb, s.sd_sb)
        return ClipState(blob, self.clip_frames[idx], self.clip_calls[idx] if self.waveform else None, stats, self._state_signature(),
                         layout)

    def import_state(self, state, clips=None) -> None:
        """Row i of ``state`` (an ``export_state`` result of a session of equal signature, on this session's device) becomes clip
        ``clips[i]`` (``None``: every clip): whatever the slot held is replaced, ``clip_frames`` / ``clip_calls`` and, for a frozen
        model with given statistics, the clip's statistics follow, and the next ``step`` continues the clip exactly where the
        export left it -- bit for bit in both tiers, layer 0 included (the state is copied, not recomputed as by ``prime``).  All
        other clips go on untouched.  Ordered on torch's current stream, no synchronisation: every step queued after it sees it.
        The weights are NOT compared: importing into a session of another model of the same geometry is the caller's decision.
        ``ValueError``: a signature mismatch (named), duplicate indices; ``IndexError``: an index out of range; ``TypeError``: wrong
        types; ``RuntimeError``: a state on another device (``state.to(...)`` first), a row count other than ``len(clips)``;
        ``NotImplementedError``: a resident session."""
        self._refuse_resident("import_state")
        layout, nbytes = self._state_layout()
        idx = import_clips(state, clips, self.B, self.dev, self._state_signature(), layout, nbytes)
        blob = state.blob.contiguous()
        if self._stats is not None:
            self.set_norm_stats(NormStats(*state.stats), clips=idx)
        if self._hop is None:
            self._import_rows(idx, state, blob, layout)
            return
        self._first_call_made(idx)
        if self._launch_bytes != nbytes:
            head = self._launch_bytes
            for name, a, b in layout[-2:]:
                self._filter_rows(name, idx, blob[:, a:b].contiguous().view(torch.float32))
            blob = blob[:, :head].contiguous()
        st = ctypes.c_void_p(_raw_stream(self._dev_index))
        for part, j0, local in self._part_runs(idx):
            arr = (ctypes.c_int * len(local))(*local)
            with torch.cuda.device(self.dev):
                rc = self.eng.lib.sfsn_hop_state_import(part["ref"], arr, len(local), ctypes.c_void_p(blob.data_ptr()), j0, st)
            if rc:
                check(rc, "sfsn_hop_state_import")
            self._fill_origins(part["origin"], part["desc"].launch_index, local, state, j0)  # (include/sfsn.h: the clips' origins)
            part["desc"].clip_start = part["origin"].data_ptr()
        if self.waveform:
            self._clip_c0[idx] = self._wave_calls - state.calls
            self._primed = True  # the launch mutes each clip by its own frame index (see step_wave)
        else:
            self._clip_f0[idx] = self.frames_done - state.frames

    @property
    def clip_frames(self) -> np.ndarray:
        """int64 [B] (read-only copy): the frames each clip has seen since its own utterance began."""
        if self.waveform:
            out = np.maximum(self.clip_calls - 1, 0)
        else:
            out = self.frames_done - self._clip_f0
        out.flags.writeable = False
        return out

    @property
    def clip_calls(self) -> np.ndarray:
        """Waveform sessions: int64 [B] (read-only copy), the step_wave / step_wave_host calls of each clip's utterance."""
        out = self._wave_calls - self._clip_c0
        out.flags.writeable = False
        return out

    def spike_summary(self, clips=None):
        """``(fb_all, sb_all)`` of the selected clips' current utterances (``clips=None``: every clip), shaped like the offline
        forward's ``layer_outputs="counts"`` lists over ``clip_frames`` frames: input and projection entries are shape-only (meta
        tensors), spike entries ``SpikeSummary`` objects with the exact spike count of the selected clips.  Counts are summed on
        the device (nothing synchronises until they are read); a resident session reads them from pinned host memory.  So
        ``metric.compute_synops(*session.spike_summary([b]), shared_weights=...)`` is clip b's SynOPs.  The selected clips must
        have seen the same number of frames (``ValueError`` otherwise); the session must have been opened with
        ``count_spikes=True`` (``RuntimeError``)."""
        idx, T = self._summary_clips(clips, self.clip_frames)
        nb = len(idx)
        spec, eng = self.eng.spec, self.eng
        ng, nl_fb, nl_sb = spec.n_groups, spec.fb_layers, spec.sb_layers
        if self._hop is None:
            counts = self._rows[:, idx].sum(1)
        else:
            counts = None
            seqs = [eng.fb] + list(eng.sb)
            units = [1] + [spec.units(g) for g in range(ng)]
            for part in self._hop["parts"]:
                mine = [b - part["b0"] for b in idx if part["b0"] <= b < part["b0"] + part["nb"]]
                if not mine:
                    continue
                slots = part["slots"]
                if self.resident:
                    slots = torch.from_numpy(slots.numpy().copy())  # (a snapshot: the launch may be serving the next hop)
                per, off = [], 0
                for seq, u in zip(seqs, units):  # (include/sfsn.h: sequences, layers, rows = clip * units + unit, column groups)
                    n = part["nb"] * u * (seq.H // 4)
                    for _ in seq.cells:
                        per.append(slots[off:off + n].view(part["nb"], -1)[mine].sum(dtype=torch.int64))
                        off += n
                c = torch.stack(per)
                counts = c if counts is None else counts + c
        fb_sh = [(T, nb, eng.fb.H)] * nl_fb
        sb_sh = [(T, nb * spec.units(g), eng.sb[g].H) for g in range(ng) for _ in range(nl_sb)]
        summ = [SpikeSummary(counts[i], shp) for i, shp in enumerate(fb_sh + sb_sh)]

        def meta(*shape):
            return torch.empty(shape, dtype=torch.float32, device="meta")

        fb_all = [meta(T, nb, spec.fb_in)] + summ[:nl_fb] + [meta(T, nb, eng.fb.P)]
        sb_all = [[meta(T, nb * spec.units(g), spec.sb_input_size(g))] + summ[nl_fb + g * nl_sb:nl_fb + (g + 1) * nl_sb] +
                  [meta(T, nb * spec.units(g), eng.sb[g].P)] for g in range(ng)]
        return fb_all, sb_all

    def check_errors(self) -> None:
        """Raise if a hand-off wait of an earlier one-launch hop expired (blocks until the hops enqueued so far have finished)."""
        if self._hop is None:
            return
        torch.cuda.current_stream(self.dev).synchronize()
        bad = False
        for part in self._hop["parts"]:
            if int(part["scratch"][0].item()) != 0:
                # the word is sticky on the device: clear it (and the pinned copy) when reporting, or every later check --
                # reset() included -- would report this failure again (round-2 advisor finding)
                part["scratch"][:1].zero_()
                part["err"].zero_()
                part["err_pending"] = False
                bad = True
        if bad:
            torch.cuda.current_stream(self.dev).synchronize()
            raise RuntimeError("sfsn_stream_hop: a bounded hand-off wait expired inside a launch (results invalid)")

    def _enqueue(self) -> None:
        """One hop on torch's current stream: history shift, then the offline forward's kernels on frames [D, D+hop)."""
        with torch.cuda.device(self.dev):  # the C ABI launches on the calling thread's current device
            self._enqueue_on_device()

    def _enqueue_on_device(self) -> None:
        eng, spec, L = self.eng, self.eng.spec, self.eng.lib
        B, F, D, hop, Th, S, ng = self.B, self.F, self.D, self.hop, self.Th, spec.num_spks, spec.n_groups
        st = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        ri = torch.view_as_real(self.hist)
        self._shift_history(ri, st)
        # default: the engine's full-band setting, 16 rows per workgroup for the sub-band stack -- few rows per hop anyway, and
        # that geometry lets layers >= 1 take their input product inside the scan (three launches less per hop)
        rpw_fb, rpw_sb = (eng.rows_per_wg[0], 16) if self.rows_per_wg is None else self.rows_per_wg

        def model(seqs, d, xs, tag, rpw):
            use_stack, wide, rpw_stack = eng._stack_choice(seqs, [x.shape[1] for x in xs], False)
            if use_stack and self.use_stack:
                # every layer of the stack in one launch (their prologues -- weights into registers / LDS -- run side by side
                # instead of one launch after the other; the layers hand each frame over inside the launch)
                eng._stage_input(seqs, 0, xs, d["zin"][0], D, hop, st, tag)
                eng._stage_stack(seqs, d, D, hop, st, tag, wide, rpw_stack, lag=0, scratch=d["scratch"])
                eng._stage_proj(seqs, d["s8"][-1], d["proj"], D, hop, st, tag)
                return
            fused = eng._fusable(seqs, rpw, False)  # layers >= 1: input product inside the scan (three launches less per hop)
            for l in range(d["nl"]):
                if l > 0 and fused:
                    eng._stage_scan_fused(seqs, l, d["states"][l], [None] * len(seqs), d["s8"], D, hop, st, tag)
                    continue
                # chunk-local zin holds frames [D, D+hop) at rows [0, hop): sources are offset by D inside _stage_input
                eng._stage_input(seqs, l, xs if l == 0 else d["s8"][l - 1], d["zin"][l], D, hop, st, tag)
                eng._stage_scan(seqs, l, d["zin"][l], d["states"][l], [None] * len(seqs), d["s8"][l], [None] * len(seqs), D, hop, st, tag, rpw)
            eng._stage_proj(seqs, d["s8"][-1], d["proj"], D, hop, st, tag)

        check(L.sfsn_features(_ptr(ri), None, B, F, Th, 0, spec.fdrc, self.fg_fb, 1, D, hop, st), "sfsn_features(fb)")
        model([eng.fb], self.fb, [self.x_fb], "fb", rpw_fb)
        check(L.sfsn_features(_ptr(ri), _ptr(self.fb["proj"][0]), B, F, Th, spec.fb_proj, spec.fdrc, self.fg_sb, ng, D, hop, st),
              "sfsn_features(sb)")
        model(eng.sb, self.sb, self.xs, "sb", rpw_sb)
        check(L.sfsn_deepfilter(_ptr(ri), B, F, Th, S, self.dfg, ng, _ptr(torch.view_as_real(self.enh)), _ptr(self.enh_mag), D, hop, st),
              "sfsn_deepfilter")
        if self._rows is not None:  # every layer's spikes of frames [D, D + hop), per clip
            for arr in self._row_jobs:
                check(L.sfsn_spike_count_rows(arr, len(arr), D, hop, st), "sfsn_spike_count_rows")

    def step(self, frames: torch.Tensor, copy: bool = True, clips=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``frames``: complex64 [B, F, hop] on the device.  Returns the enhanced frames and their magnitudes; with
        ``copy=False`` the returned tensors are views of the session's buffers, valid until the next ``step``.

        ``clips`` (a sequence or 1-D tensor of clip indices, checked like ``reset(clips)``'s; duplicates merged): only these clips
        take the hop, every other clip is HELD -- its rows of ``frames`` may hold anything (NaN included), its output rows are
        zero, and its state, counts and ``clip_frames`` are what they were: its next active call continues its utterance with the
        next frame.  Shapes do not change and the call stays zero-copy.  The one-launch tier holds clips inside the one launch per
        part it makes anyway (``sfsn_stream_hop_held``); the per-kernel tier saves and restores the held clips' rows around the
        replay.  An empty list advances nobody: nothing is launched, zeros are returned.  ``clips=None``: today's call.
        ``ValueError``: an index out of range (named); ``TypeError``: wrong types; ``NotImplementedError``: a resident session."""
        if frames.device != self.dev or frames.dtype != torch.complex64 or tuple(frames.shape) != (self.B, self.F, self.hop):
            raise RuntimeError(f"expected complex64 {(self.B, self.F, self.hop)} on {self.dev}, got {frames.dtype} {tuple(frames.shape)} "
                               f"on {frames.device}")
        if self.waveform:
            raise RuntimeError("this session was opened with waveform=True: use step_wave(samples)")
        hold = None if clips is None else self._hold(clips, "step")
        if self._hop is not None:
            h = self._hop
            if hold is not None and not hold[0]:  # nobody advances
                return torch.zeros_like(h["enh"]), torch.zeros_like(h["mag"])
            if not (frames.is_contiguous() and frames.data_ptr() % 8 == 0):
                self.inp.copy_(frames)
                frames = self.inp
            # read in place: no staging copy in front
            self._launch_hops(frames.data_ptr(), self.F * self.hop * 8, "inp_ri", held=None if hold is None else hold[2])
            if hold is not None:
                self._held_bookkeeping(hold[1])
            return (h["enh"].clone(), h["mag"].clone()) if copy else (h["enh"], h["mag"])
        e, m = self.enh[..., self.D:], self.enh_mag[..., self.D:]
        if hold is not None and not hold[0]:
            return torch.zeros_like(e), torch.zeros_like(m)
        saved = None if hold is None else self._save_held(hold[1])  # (put back behind the replay)
        self.inp.copy_(frames)
        if self._graph is not None:
            self._graph.replay()
        else:
            self._enqueue()
        self.frames_done += self.hop
        if saved is not None:
            self._restore_held(saved, (e, m))
            self._held_bookkeeping(hold[1])
        return (e.clone(), m.clone()) if copy else (e, m)

    def step_wave(self, samples: torch.Tensor, copy: bool = True, clips=None) -> torch.Tensor:
        """Waveform streaming (``waveform=True``): ``samples`` float32 [B, 128] on the device -- the next 8 ms of every clip.
        Returns enhanced samples [B, S, 128]: call c returns the samples that entered with call c - 3 (the framing of
        torch.stft(center=True) needs 256 samples of look-ahead, the overlap-add another hop: 24 ms of algorithmic delay, as for
        any causal use of the reference's 32 ms / 8 ms analysis); the first three calls of an utterance return zeros.
        One launch per call: the frame's STFT, the whole model, the inverse STFT with its overlap-add state.

        ``clips``: as for ``step`` -- only the listed clips make this call; a held clip's row of ``samples`` is ignored, it gets
        zeros, its ``clip_calls`` stays, and its next active call returns what that call would have returned (the three-call delay
        line of its OWN calls).  A clip may be held at the session's first call, and before it has ever run.

        Outer samples (``resample=3`` and / or ``sample_format="s16"`` at ``model.streaming``): ``samples`` is ``[B, 128 * resample]`` of
        float32 or int16 and the result ``[B, S, 128 * resample]`` of the same format -- 48 kHz and 16-bit PCM as a decoder or a sound
        card delivers them, converted inside the same one launch (``sfsn_stream_hop_io``): int16 -> ``s * 2**-15``, a 96-tap low-pass
        and decimation by 3 with carried samples (``D3``), the hop, interpolation by 3 with carried samples (``U3``), and
        ``Q(v) = clamp(rint(v * 32768), -32768, 32767)`` (ties to even, NaN -> 0).  Call by call the result is
        ``Q(U3(control(D3(x * 2**-15))))`` with ``control`` a plain float32 session of the same model on the same calls: bit for bit
        what ``spectral.resample_down3``, that session and ``spectral.resample_up3`` give with their states carried.  The delay is
        the three calls above plus 95 outer samples (47.5 each way through the linear-phase filter): 3 * 384 + 95 = 1247 samples at
        48 kHz, 26 ms.  ``reset(clips)``, ``clips=`` holding and ``export_state`` / ``import_state`` (sections ``"dec"`` / ``"int"``)
        carry the filters with the clip; ``prime_wave`` / ``advance_wave`` / ``advance_wave_ragged`` and ``resident=True`` are not
        built for such sessions (``NotImplementedError``)."""
        if not self.waveform:
            raise RuntimeError("open the session with waveform=True")
        if samples.device != self.dev or samples.dtype != self._fmt_dtype or tuple(samples.shape) != (self.B, self._outer) or not samples.is_contiguous():
            what = "float32" if not self._io else f"{self._fmt_dtype} (resample={self.resample}, sample_format={self.sample_format!r})".replace("torch.", "")
            raise RuntimeError(f"expected contiguous {what} {(self.B, self._outer)} on {self.dev}, got {samples.dtype} {tuple(samples.shape)}")
        h = self._hop
        out = h["wave_out"]
        hold = None if clips is None else self._hold(clips, "step_wave")
        if hold is not None and not hold[0]:  # nobody makes this call
            return torch.zeros_like(out)
        c = self._wave_calls
        self._wave_calls += 1
        if c == 0:  # no frame ends here yet (frame 0 covers samples [-256, 256)): the samples only enter the state
            self._first_wave_call(samples, hold)
            return torch.zeros_like(out)
        self._launch_hops(samples.data_ptr(), self._outer * samples.element_size(), "wave_in", frame_index=c - 1, held=None if hold is None else hold[2])
        if hold is not None:
            self._held_bookkeeping(hold[1])
        if c < 3 and not self._primed:  # padded positions torch.istft trims (primed clips: the launch mutes each clip by its own index)
            return torch.zeros_like(out)
        return out.clone() if copy else out


    # ---- the resident launch (host_io, resident=True) ---------------------------------------------------------------------------
    def _start_resident(self, c: int) -> None:
        h = self._hop
        if len(h["parts"]) != 1:
            raise NotImplementedError("resident streaming: batches one launch covers (one part)")
        part, host = h["parts"][0], h["host"]
        d = part["desc"]
        d.frames_before, d.frame_index, d.wave_in = self.frames_done, c - 1, host["inp"].data_ptr()
        host["bell_np"][:2] = 0  # word 0: the doorbell; word 1: set by the kernel when it leaves
        with torch.cuda.device(self.dev):
            side = torch.cuda.Stream(self.dev)  # non-blocking: the kernel stays resident behind everything else the caller does
            side.wait_stream(torch.cuda.current_stream(self.dev))  # (state fills / the first call's copy come first)
            rc = self.eng.lib.sfsn_stream_hop_resident(part["ref"], ctypes.c_void_p(host["bell"].data_ptr()), self.idle_ms,
                                                       ctypes.c_void_p(side.cuda_stream))
        if rc:
            check(rc, "sfsn_stream_hop_resident")
        self._res = dict(k=0, stream=side)

    def _stop_resident(self) -> None:
        """End the resident launch (no-op without one) and fold the hops it served into the descriptor's launch counter."""
        r = self._res
        if r is None:
            return
        self._res = None
        self._hop["host"]["bell_np"][0] = 0xFFFFFFFF
        r["stream"].synchronize()
        self._hop["parts"][0]["desc"].launch_index += r["k"]

    def _ring_resident(self, c: int) -> int:
        r = self._res
        if r is not None and self._hop["host"]["bell_np"][1] != 0:
            self._stop_resident()  # the doorbell stayed silent long enough for the kernel to leave: start another
            r = None
        if r is None:
            self._start_resident(c)
            r = self._res
        r["k"] += 1
        self._hop["host"]["bell_np"][0] = r["k"]
        self.frames_done += self.hop
        return self._hop["parts"][0]["desc"].launch_index + r["k"]

    def close(self) -> None:
        """End a resident launch, if one is running (reset() does the same)."""
        self._stop_resident()

    def __del__(self):
        try:
            self._stop_resident()
        except Exception:
            pass

    def step_wave_host(self, samples, timeout_s: float = 2.0, clips=None) -> torch.Tensor:
        """Waveform streaming with the samples on the HOST (``waveform=True, host_io=True``): ``samples`` = float32 [B, 128] CPU
        tensor (or anything ``torch.as_tensor`` takes).  The launch reads them from pinned host memory and writes the enhanced
        samples and a completion word per (clip, speaker) back into pinned host memory; the caller's thread spins on the words --
        no copy launch, no stream synchronisation.  Returns a CPU tensor [B, S, 128] (a view of the session's pinned buffer, valid
        until the next call); same three-hop delay as ``step_wave``.  ``clips``: as for ``step_wave`` (non-resident sessions); the
        held clips' completion words are written too, so the wait ends as it always does."""
        h = self._hop
        if not self.host_io or h is None:
            raise RuntimeError("open the session with waveform=True, host_io=True")
        host = h["host"]
        hold = None if clips is None else self._hold(clips, "step_wave_host")
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
        c = self._wave_calls
        self._wave_calls += 1
        if c == 0:
            self._first_wave_call(host["inp"], hold)  # (blocking: the next call overwrites the pinned buffer right away)
            torch.cuda.current_stream(self.dev).synchronize()
            return torch.zeros_like(host["out"])
        if self.resident:
            target = self._ring_resident(c)
        else:
            target = h["parts"][0]["desc"].launch_index + 1
            self._launch_hops(host["inp"].data_ptr(), self._outer * host["inp"].element_size(), "wave_in", frame_index=c - 1,
                              held=None if hold is None else hold[2])
            if hold is not None:
                self._held_bookkeeping(hold[1])
        done, t_end, t_soft = host["done_np"], None, None
        target &= 0xFFFFFFFF
        while (int(done.min()) & 0xFFFFFFFF) != target or (int(done.max()) & 0xFFFFFFFF) != target:  # (all parts carry the same launch index; uint32 compare: the index wraps)
            if t_end is None:
                t_end = time.perf_counter() + timeout_s
                t_soft = t_end - timeout_s + 0.02
            elif t_soft is not None and not self.resident and time.perf_counter() > t_soft:
                # 20 ms without the words (a hop takes tens of microseconds): a hand-off wait inside the launch has probably
                # expired -- the launch has ended by now, its error word says so, and check_errors() raises it (round-2 advisor:
                # a failed launch used to show up only as the 2 s timeout)
                t_soft = None
                self.check_errors()
            elif time.perf_counter() > t_end:
                if self.resident:
                    self._stop_resident()
                raise RuntimeError("sfsn_stream_hop: no completion word from the launch (see check_errors())")
            if self._res is not None and host["bell_np"][1] != 0 and (int(done.min()) & 0xFFFFFFFF) != target:
                # the resident kernel's watchdog fired just as this hop was rung: the hop was not served -- start another kernel on it
                self.frames_done -= self.hop
                self._res["k"] -= 1
                self._stop_resident()
                self.check_errors()
                target = self._ring_resident(c) & 0xFFFFFFFF
        return torch.zeros_like(host["out"]) if c < 3 and not self._primed else host["out"]
