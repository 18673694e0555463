"""Host-side driver of the hot path: packs a model's weights for the gfx950 kernels and enqueues the
launch sequence of one forward (complex STFT in HBM -> enhanced STFT / magnitude + the per-layer
tensors the reference's modules return) on torch's current HIP stream, through the C ABI only.

PyTorch is used here for device memory and streams; every arithmetic step of the path runs in
``libsfsn_hip.so``.  There is no CPU / eager fallback: CPU tensors raise.

Reference call stack replaced: ``SpikingFullSubNet.forward`` modeling_spiking_fullsubnet.py:434-472
(frozen twin ``Separator.forward`` model_low_freq.py:574-607) and everything below it.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import (CountTensor, DfGroup, FeatProjJob, FeatureGroup, FusedInput, FusedX, InProjJob, ProjDfGroup, ProjJob, RowCount, ScanSegment,
                   check)


@dataclass
class PathSpec:
    """Geometry of one model, normalised over the live and frozen front-ends."""
    front: str                    # "live" (LayerNorm inputs, `proj`) | "frozen" (offline Laplace norm, `fc_output_layer`)
    n_fft: int
    fdrc: float
    fb_in: int
    fb_hidden: int
    fb_layers: int
    fb_proj: int
    sb_hidden: int
    sb_layers: int
    cutoffs: List[int]
    ctr: List[int]
    nbr: List[int]
    ctr_fb: List[int]
    nbr_fb: List[int]
    df: List[int]
    num_spks: int = 1
    shared: bool = False
    bn: bool = False
    ln_fb: bool = True
    ln_sb: bool = True
    laplace: bool = False         # frozen front-end with an utterance-level (offline, non-causal) norm: offline_laplace_norm, or ...
    gaussian: bool = False        # ... offline_gaussian_norm (set together with `laplace`: same schedule, other statistics)
    cum_laplace: bool = False     # frozen front-end with cumulative_laplace_norm (causal: every row by its own running mean)
    proj_name: str = "proj"

    @property
    def n_groups(self) -> int:
        return len(self.ctr)

    @property
    def num_freqs(self) -> int:  # bins the network processes (Nyquist excluded)
        return self.n_fft // 2

    def units(self, g: int) -> int:
        return (self.cutoffs[g + 1] - self.cutoffs[g]) // self.ctr[g]

    def sb_input_size(self, g: int) -> int:
        return (self.ctr[g] + 2 * self.nbr[g]) + (self.ctr_fb[g] + 2 * self.nbr_fb[g])

    def sb_proj_size(self, g: int) -> int:
        return 2 * self.ctr[g] * self.df[g] * self.num_spks


def _dev(a: np.ndarray, device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def pack_w3(w: np.ndarray, bits: int = 24):
    """fp32 [N, K] -> (int8 digits in MFMA fragment order, dq [pad16(N)]) as numpy arrays (host packing).  bits = 16: the
    16-bit-weight mode (weights rounded to 16 significant bits of the row grid, least-significant digit plane zero)."""
    L = _lib.lib()
    w = np.ascontiguousarray(w, dtype=np.float32)
    n, k = w.shape
    packed = np.empty(L.sfsn_w3_packed_bytes(n, k), np.int8)
    dq = np.empty(L.sfsn_w3_padded_rows(n), np.float32)
    check(L.sfsn_w3_pack_bits(w.ctypes.data, n, k, bits, packed.ctypes.data, dq.ctypes.data), "sfsn_w3_pack_bits")
    return packed, dq


def unpack_w3(packed: np.ndarray, dq: np.ndarray, n: int, k: int) -> np.ndarray:
    L = _lib.lib()
    w = np.empty((n, k), np.float32)
    check(L.sfsn_w3_unpack(packed.ctypes.data, dq.ctypes.data, n, k, w.ctypes.data), "sfsn_w3_unpack")
    return w


def fold_batchnorm(weight, bias, mean, var, eps=1e-5):
    """Eval-mode BatchNorm1d as ATen's CPU kernel evaluates it (probed bit-exact, see oracle/sfsn_oracle.c):
    alpha = gamma / sqrt(var + eps), beta = fma(-mean, alpha, bias), y = fma(x, alpha, beta)."""
    f32 = np.float32
    invstd = (f32(1) / np.sqrt(var.astype(f32) + f32(eps))).astype(f32)
    alpha = (invstd * weight.astype(f32)).astype(f32)
    beta = (bias.astype(np.float64) - mean.astype(np.float64) * alpha.astype(np.float64)).astype(f32)
    return alpha, beta


@dataclass
class _Cell:
    H: int
    G: int
    w_ih_f32: Optional[torch.Tensor] = None                 # layer 0: [G*H, I] fp32
    w_ih_q: List[tuple] = field(default_factory=list)        # layer >= 1: per gate (packed, dq) of [H, H]
    w_hh_q: Optional[torch.Tensor] = None                    # packed [G*H, H]
    w_hh_dq: Optional[torch.Tensor] = None
    bias: Optional[torch.Tensor] = None
    alpha: Optional[torch.Tensor] = None
    beta: Optional[torch.Tensor] = None


@dataclass
class _Seq:
    I: int
    H: int
    P: int
    cells: List[_Cell]
    proj_q: torch.Tensor
    proj_dq: torch.Tensor
    proj_b: torch.Tensor
    ln_w: Optional[torch.Tensor] = None
    ln_b: Optional[torch.Tensor] = None


def _pack_seq(sd: Dict[str, np.ndarray], prefix: str, spec: PathSpec, I: int, H: int, L: int, P: int, use_ln: bool, device, bits: int = 24) -> _Seq:
    G = 1 if spec.shared else 2
    cells = []
    for l in range(L):
        p = f"{prefix}sequence_model.layers.{l}.cell."
        w_ih, w_hh, b = sd[p + "weight_ih"], sd[p + "weight_hh"], sd[p + "bias_ih"]
        Il = I if l == 0 else H
        assert w_ih.shape == (G * H, Il) and w_hh.shape == (G * H, H) and b.shape == (2 * H,), (p, w_ih.shape, w_hh.shape)
        cell = _Cell(H=H, G=G)
        if l == 0:
            cell.w_ih_f32 = _dev(w_ih.astype(np.float32), device)
        else:
            for g in range(G):
                pk, dq = pack_w3(w_ih[g * H:(g + 1) * H], bits)
                cell.w_ih_q.append((_dev(pk, device), _dev(dq, device)))
        pk, dq = pack_w3(w_hh, bits)
        cell.w_hh_q, cell.w_hh_dq = _dev(pk, device), _dev(dq, device)
        cell.bias = _dev(b.astype(np.float32), device)
        if spec.bn:
            a, be = fold_batchnorm(sd[p + "batchnorm.weight"], sd[p + "batchnorm.bias"], sd[p + "batchnorm.running_mean"],
                                   sd[p + "batchnorm.running_var"])
        else:
            a, be = np.ones(H, np.float32), np.zeros(H, np.float32)
        cell.alpha, cell.beta = _dev(a, device), _dev(be, device)
        cells.append(cell)
    pn = prefix + spec.proj_name
    pw, pb = sd[pn + ".weight"], sd[pn + ".bias"]
    assert pw.shape == (P, H), (pn, pw.shape, (P, H))
    pk, dq = pack_w3(pw, bits)
    seq = _Seq(I=I, H=H, P=P, cells=cells, proj_q=_dev(pk, device), proj_dq=_dev(dq, device), proj_b=_dev(pb.astype(np.float32), device))
    if use_ln:
        seq.ln_w = _dev(sd[prefix + "pre_layer_norm.weight"].astype(np.float32), device)
        seq.ln_b = _dev(sd[prefix + "pre_layer_norm.bias"].astype(np.float32), device)
    return seq


class SpikeSummary:
    """Stand-in for one fp32 spike tensor of ``all_layer_outputs`` when only its statistics are wanted
    (``layer_outputs="counts"``): the exact number of spikes, counted on the device from the int8 spikes the scan writes,
    plus the shape the tensor would have had.  ``metric.compute_synops`` / ``compute_neuronops`` accept it in place of
    the tensor (audiozen/metric.py:303-340 read only ``gt(x, 0).float().mean()`` and ``size(-1)``)."""

    def __init__(self, count: torch.Tensor, shape):
        self.count, self.shape = count, torch.Size(shape)

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def numel(self) -> int:
        return self.shape.numel()

    def rate(self) -> torch.Tensor:
        """fp32 firing rate = what ``torch.gt(x, 0).float().mean()`` estimates (here exact count / numel, rounded once)."""
        return (self.count.to(torch.float64) / self.numel()).to(torch.float32)

    def __repr__(self):
        return f"SpikeSummary(shape={tuple(self.shape)})"


SOAKED_HW_QUEUES = (4, 24)  # GPU_MAX_HW_QUEUES values the two-stream schedule has been soaked under (unset = HIP's default of 4)
_hw_queues_warned = False


@dataclass
class NormStats:
    """The utterance-level statistics of the frozen front-end's offline norms (model_low_freq.py:147-169, 205-218), one set per
    clip: ``mu_fb`` [B] divides (Gaussian: is subtracted from) the full-band input, ``mu_sb`` [n_groups, B] each sub-band group's;
    ``sd_fb`` / ``sd_sb`` (same shapes) are the standard deviations of ``offline_gaussian_norm`` and ``None`` otherwise.  float32, on
    the model's device.  An offline forward computes them from the whole clip (``forward_stft(..., return_norm_stats=True)``,
    ``Separator.norm_stats``); given to ``forward_stft(..., norm_stats=...)`` or to a streaming session they replace that pass."""
    mu_fb: torch.Tensor
    mu_sb: torch.Tensor
    sd_fb: Optional[torch.Tensor] = None
    sd_sb: Optional[torch.Tensor] = None

    def _map(self, fn) -> "NormStats":
        return NormStats(*(None if t is None else fn(t) for t in (self.mu_fb, self.mu_sb, self.sd_fb, self.sd_sb)))

    def select(self, clips) -> "NormStats":
        """The statistics of the given clips (a sequence or 1-D tensor of clip indices), in that order."""
        idx = torch.as_tensor(clips, dtype=torch.long, device=self.mu_fb.device).reshape(-1)
        return self._map(lambda t: t.index_select(-1, idx))

    def to(self, device) -> "NormStats":
        return self._map(lambda t: t.to(device))

    def clone(self) -> "NormStats":
        return self._map(lambda t: t.clone())

    def validate(self, spec: PathSpec, batch: int, device) -> None:
        """``ValueError`` naming what is wrong: a model that takes no statistics, a missing / surplus ``sd``, shape, dtype, device."""
        if not spec.laplace:
            kind = "cumulative_laplace_norm computes its running means itself" if spec.cum_laplace else \
                "the live front-end normalises every frame by LayerNorm"
            raise ValueError(f"norm_stats: this model takes no utterance statistics ({kind})")
        want = [("mu_fb", self.mu_fb, (batch,)), ("mu_sb", self.mu_sb, (spec.n_groups, batch))]
        if spec.gaussian:
            want += [("sd_fb", self.sd_fb, (batch,)), ("sd_sb", self.sd_sb, (spec.n_groups, batch))]
        elif self.sd_fb is not None or self.sd_sb is not None:
            raise ValueError("norm_stats: sd_fb / sd_sb belong to offline_gaussian_norm; this model uses offline_laplace_norm")
        device = torch.device(device)
        for name, t, shape in want:
            if t is None:
                raise ValueError(f"norm_stats.{name} is missing: offline_gaussian_norm needs the clips' standard deviations")
            if not torch.is_tensor(t):
                raise ValueError(f"norm_stats.{name}: expected a tensor, got {type(t).__name__}")
            if tuple(t.shape) != shape:
                raise ValueError(f"norm_stats.{name}: expected shape {shape}, got {tuple(t.shape)}")
            if t.dtype != torch.float32:
                raise ValueError(f"norm_stats.{name}: expected float32, got {t.dtype}")
            if t.device != device:
                raise ValueError(f"norm_stats.{name}: expected a tensor on {device}, got one on {t.device}")


def _check_hw_queues() -> int:
    """The overlapped schedule of a forward alone runs two launches of resident workgroups with in-launch waits on two HIP streams
    (the sub-band pair launch and the full-band stack), and bench.py's timed region a dozen forwards on as many streams.  How the
    runtime maps streams onto hardware queues is `GPU_MAX_HW_QUEUES` (read by HIP once, at its initialisation).  Three such launches
    on three streams stopped being dispatched within 3-120 iterations at 4 and 8 queues and never at 2 (the training path's layer
    calls, scripts/dbg_train_hang.py, profiles/EXPERIMENTS.md; root cause unknown -- training was moved to one grid).  The inference
    schedules were soaked at the default (4: the -m gpu suite, scripts/soak_r04.py, 3000 forwards) and at 24 (bench.py): every
    in-launch wait is bounded and reported, so another value can cost a loud failure, never wrong results -- warn once."""
    global _hw_queues_warned
    raw = os.environ.get("GPU_MAX_HW_QUEUES", "")
    try:
        n = int(raw) if raw else 4
    except ValueError:
        n = 4
    if n not in SOAKED_HW_QUEUES and not _hw_queues_warned:
        _hw_queues_warned = True
        import warnings
        warnings.warn(f"GPU_MAX_HW_QUEUES={raw}: the two-stream schedule of spiking_fullsubnet_amd was soaked at {SOAKED_HW_QUEUES} "
                      "hardware queues only (see README.md, limits); in-launch waits are bounded and raise, results are never silently wrong",
                      RuntimeWarning, stacklevel=3)
    return n


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def fill_segment(sg: ScanSegment, cell, R: int, H: int, t0: int, zin, state, spikes_i8, spikes_f32=None, membrane=None, count=None) -> None:
    """One sfsn_scan_segment of a launch over the frames from `t0` on.  `cell`: anything with w_hh_q, w_hh_dq, bias, alpha, beta
    (_Cell, fullband_engine._Layer).  zin is chunk-local (or None: the launch forms the input term itself), state = (h, c); the output
    tensors are whole-sequence [T, R, .] buffers and start at frame t0: fp32 spikes / membranes at t0 * R * H * 4 bytes, the int8
    spikes (rows padded to 64 bytes) at t0 * R * ceil64(H)."""
    f32_at, i8_at = t0 * R * H * 4, t0 * R * ((H + 63) // 64 * 64)
    sg.zin, sg.w_hh, sg.w_dq, sg.bias = _ptr(zin), _ptr(cell.w_hh_q), _ptr(cell.w_hh_dq), _ptr(cell.bias)
    sg.bn_alpha, sg.bn_beta, sg.h_state, sg.c_state = _ptr(cell.alpha), _ptr(cell.beta), _ptr(state[0]), _ptr(state[1])
    sg.spikes_f32 = None if spikes_f32 is None else ctypes.c_void_p(spikes_f32.data_ptr() + f32_at)
    sg.membrane = None if membrane is None else ctypes.c_void_p(membrane.data_ptr() + f32_at)
    sg.spikes_i8 = ctypes.c_void_p(spikes_i8.data_ptr() + i8_at)
    sg.R = R
    sg.spike_count = _ptr(count)


STACK_ROWS_PER_WG = {"fb": 4, "sb": 8}  # Engine.stack_rows_per_wg of a fresh engine


def stack_rule(shared, nl, H, n_groups, Rs, want_membrane, stack_scan, stack_wide, stack_rows_fb_auto, pair_scan, rows_per_wg, alone, n_cu):
    """(use the stack launch?, wide flavour?, rows per workgroup) for one stack of `n_groups` sequence models of `nl` layers and hidden
    size `H` with `Rs` rows each, on a chip of `n_cu` compute units; `alone`: no other forward of the engine is in flight.  Pure:
    no device, no engine (Engine._stack_choice supplies `alone` and `n_cu`).

    sfsn_gsn_stack_scan runs all layers of a stack in one launch, layer l+1 trailing layer l.  It wins where one layer's
    workgroups leave most of the chip idle; where a single layer already fills the chip at 4 rows per workgroup the layers
    side by side get half the CUs each and the input terms' traffic through L2 / HBM doubles up, and full-chip launches
    in a row are faster.  Measured on MI355X, T=1000, baseline_m sizes (scripts/exp_stack.py), sub-band stack
    (per-layer scans + input products / narrow stack / wide stack, ms): B=4 1.9 / 1.7 / 1.2, B=16 1.9 / 1.7 / 1.2,
    B=32 2.0 / 1.7 / 1.95, B=64 1.66 / 1.83 / 2.33; full-band stack (H=320, B rows) 2.26 -> 1.25 at every B.
    `stack_scan`: "auto" (the rule below), True (always, `stack_rows_per_wg` / `stack_wide` as set), False (never)."""
    ok = bool(stack_scan and shared and not want_membrane and nl >= 2 and n_groups * (1 + (nl - 1) * 2) <= 24)
    if not ok:
        return False, False, 0
    if stack_scan != "auto":
        return True, stack_wide, None
    rows = sum(Rs)
    if H > 256:  # the full-band model: few rows, PROJ + gated scan roles
        rp = stack_rows_fb_auto
        return (rows + rp - 1) // rp * nl + (rows + 15) // 16 <= n_cu, False, rp
    # round 4: H <= 224 stacks without input-term buffers run their layers >= 1 as FUSED3 roles (the input product inside the
    # 8-row IO-wave scan): all layers side by side in one launch, no fp32 input term for the layers >= 1.  Every workgroup of
    # the launch has to be resident beside the full-band stack of the same forward (<= 40 workgroups), and the forward has
    # to be alone on the chip -- `rows_per_wg` (0 or 8 for the sub-band models) says so: bench.py's timed region, with a
    # dozen forwards in flight, sets 16 and keeps its per-layer launches.  Measured at B = 64, T = 1000 (scripts/exp_pair.py):
    # 1.03 ms against 1.43 (scan3 at 4 rows + sfsn_spike_proj), 1.72 (8-wave FUSED roles), 2.4 (PROJ roles).
    wgs8 = nl * sum((R + 7) // 8 for R in Rs)
    if pair_scan and alone and H <= 224 and rows_per_wg[1] in (0, 8) and wgs8 <= n_cu - 40:
        return True, False, 8
    if rows <= n_cu:       # every layer's workgroups at 8 rows + the PROJ workgroups fit several times over
        return True, True, 8
    if rows <= 2 * n_cu:   # 8 rows per workgroup: both layers side by side still fit
        return True, False, 8
    return False, False, 0


class ForwardPlan(NamedTuple):
    """The schedule of one forward (plan_forward)."""
    pipeline: bool   # the time-pipelined schedule: a stream pair per layer, chunks of `pipeline_chunk` frames
    overlap: bool    # the overlapped schedule: full-band model on one stream, sub-band models one chunk behind on a second
    bounds: tuple    # ((t0, nt), ...): the chunks of the sequence
    nt_max: int      # frames of the longest chunk (the chunk-local buffers' size)
    rpw_fb: int      # rows per workgroup of the per-layer scans, full-band / ...
    rpw_sb: int      # ... sub-band (0: the library spreads the rows over all CUs)
    staged: bool     # several streams chained by events


def _overlap_bounds(T, sb_rows, overlap_chunks, overlap_fracs, overlap_first):
    """The chunks of the overlapped schedule."""
    # a short first chunk: the sub-band models can only start once the full-band model has finished a chunk, so the first
    # one is the lead-in of the whole forward; the rest is cut evenly (the full-band model is ~2x faster per frame and
    # stays ahead)
    first = overlap_first if overlap_first >= 0 else int(round(0.24 * T / 8.0)) * 8
    first = min(max(int(first), 0), T // 2)
    fracs = overlap_fracs
    if not fracs and overlap_first < 0 and overlap_chunks == 3 and T >= 256 and sb_rows < 600:
        # round 5 (scripts/exp_chunks_ab*_r05.sh, interleaved A/B on two boxes): below ~600 sub-band rows (B <= 32 of
        # baseline_m) a LONGER lead-in chunk wins -- (.36,.32,.32) T: 2.03-2.06 / 2.13 / 2.34 ms at B = 4 / 16 / 32 against
        # 2.08-2.10 / 2.19 / 2.39-2.42 with 0.24 T.  At B = 64 the balance sits on a knife edge (full-band chunk c+1 must fit
        # beside sub-band chunk c): (.32,.33,.35) measured 2.65-2.69 on one box and 2.80-2.82 on the next against 2.70-2.76
        # for 0.24 T on both, so 0.24 T stays there.
        fracs = (0.36, 0.32, 0.32)
    if fracs:  # explicit chunk lengths as fractions of T (experiments: scripts/exp_forward_r04.py)
        cuts = [int(round(f * T / 8.0)) * 8 for f in fracs]
        lens = [c for c in cuts if c > 0]
        lens = lens[:-1] + [T - sum(lens[:-1])] if sum(lens[:-1]) < T else [T]
        bounds, t0 = [], 0
        for n_ in lens:
            bounds.append((t0, n_))
            t0 += n_
        return bounds
    if first:
        rest = -(-(T - first) // (overlap_chunks - 1))
        return [(0, first)] + [(t0, min(rest, T - t0)) for t0 in range(first, T, rest)]
    nt = -(-T // overlap_chunks)
    return [(t0, min(nt, T - t0)) for t0 in range(0, T, nt)]


def plan_forward(spec: PathSpec, B: int, T: int, pipeline: Optional[bool], n_cu: int, want_membrane: bool = False, pipeline_default: bool = False,
                 pipeline_chunk: int = 128, seq_chunk: int = 0, overlap_chunks: int = 3, overlap_fracs=None, overlap_first: int = -1,
                 rows_per_wg=(0, 0), fuse_input: bool = True, stack_scan="auto", stack_rows_per_wg=None, stack_wide: bool = True,
                 stack_rows_fb_auto: int = 4, pair_scan: bool = True) -> ForwardPlan:
    """Which of the three schedules (sequential, overlapped, pipelined) a forward of B clips of T frames runs, its chunks and its rows
    per scan workgroup.  `pipeline`: the caller's argument (None: the engine's default); the other keywords are the Engine attributes
    of the same names (defaults: a fresh engine's), `n_cu` the chip's compute units.  Pure: no device, no engine, no environment."""
    chunk = pipeline_chunk
    if pipeline is None:
        pipeline = pipeline_default and chunk > 0 and T >= 2 * chunk
    if spec.cum_laplace:
        pipeline = False  # (the running-mean state and its scratch are per forward, not per stage: single-stream order only)
    Rs_sb = [B * spec.units(g) for g in range(spec.n_groups)]
    # sequential schedule: optionally still cut the sequence into chunks (single stream): the chunk-sized input-term
    # buffer is then produced and consumed while it is still in the 256 MB Infinity Cache instead of making a round
    # trip through HBM (745 MB per sub-band layer at B=64, T=1000)
    overlap = bool(not pipeline and overlap_chunks > 1 and not spec.laplace and not spec.cum_laplace and not (0 < seq_chunk < T)
                   and T >= 96 * overlap_chunks)
    if overlap and stack_scan is True:
        # forced stack launches for both models: side by side on two streams they must not ask for more workgroups than the
        # chip has compute units -- in-launch hand-offs rely on producers being resident (the "auto" rule never gets here)
        def blocks(nl, H, n_groups, Rs, tag):
            use, wide, rp = stack_rule(spec.shared, nl, H, n_groups, Rs, want_membrane, stack_scan, stack_wide, stack_rows_fb_auto,
                                       pair_scan, rows_per_wg, True, n_cu)
            rp = rp or (stack_rows_per_wg or STACK_ROWS_PER_WG)[tag]
            scan = sum(-(-R // rp) for R in Rs)
            proj = sum(-(-R // 16) for R in Rs) if (wide or H > 256) else 0
            return (nl * (scan + 7) // 8 * 8 + (nl - 1) * (proj + 7) // 8 * 8) if use else 0
        b_fb = blocks(spec.fb_layers, spec.fb_hidden, 1, [B], "fb")
        b_sb = blocks(spec.sb_layers, spec.sb_hidden, spec.n_groups, Rs_sb, "sb")
        if b_fb and b_sb and b_fb + b_sb > n_cu:
            overlap = False
    if overlap:
        bounds = _overlap_bounds(T, sum(Rs_sb), overlap_chunks, overlap_fracs, overlap_first)
        nt_max = max(n for _, n in bounds)
    else:
        nt_max = chunk if pipeline else (seq_chunk if 0 < seq_chunk < T else T)
        bounds = [(t0, min(nt_max, T - t0)) for t0 in range(0, T, nt_max)]
    rpw_fb, rpw_sb = (16, 16) if pipeline else rows_per_wg
    if rpw_sb == 0 and fuse_input and spec.shared and 128 < spec.sb_hidden <= 256 and (sum(Rs_sb) + 7) // 8 > n_cu:
        # Many sub-band rows (baseline_l: 43 units per clip = 2752 rows at B = 64): left to itself the library spreads them at 8
        # rows per workgroup (344 workgroups: two rounds on 256 compute units, round 2's body for 16 tiles) behind a separate
        # layer-0 input product and a layer-2 spike product (5.6 GB of fp32 input terms written and read).  At 16 rows per workgroup
        # the launch is one round and the fused-input kernels apply (input products inside the scan, defined at 16 rows): said
        # explicitly here whenever 8 rows would not fit the chip in one round.
        rpw_sb = 16
    return ForwardPlan(bool(pipeline), overlap, tuple(bounds), nt_max, rpw_fb, rpw_sb, bool(pipeline or overlap))


class ErrorWords:
    """The error words of launches with bounded in-launch waits (first word of a launch's scratch buffer, sticky: non-zero = a
    hand-off wait expired, the results are invalid).  A word travels to pinned host memory behind its launch and is looked at
    without blocking at the next forward (and by check()): a failed launch cannot go unnoticed for long."""

    def __init__(self, engine):
        self.engine = engine  # its `device`, and its `_err_stream` for words collected off the launch's chain
        self.pending: List[tuple] = []  # (event, pinned copy, what, scratch buffers)

    def watch(self, stream, scratch, what: str) -> None:
        """Copy the word of `scratch` (a list: the maximum of their words) behind what `stream` holds so far.  stream None: on the
        engine's `_err_stream`, behind what the current stream holds so far -- nothing on the current stream waits for the copy."""
        eng = self.engine
        scratch = list(scratch) if isinstance(scratch, (list, tuple)) else [scratch]
        if stream is None:
            if eng._err_stream is None:
                eng._err_stream = torch.cuda.Stream(device=eng.device)
            stream = eng._err_stream
            ev0 = torch.cuda.Event()
            ev0.record(torch.cuda.current_stream(eng.device))
            stream.wait_event(ev0)
            for sc in scratch:
                sc.record_stream(stream)
        with torch.cuda.stream(stream):
            word = scratch[0][:1] if len(scratch) == 1 else torch.stack([sc[0] for sc in scratch]).max().reshape(1)
            pin = torch.empty((1,), dtype=torch.int32, pin_memory=True)
            pin.copy_(word, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
        self.pending.append((ev, pin, what, scratch))

    def poll(self, block: bool = False) -> None:
        keep = []
        for item in self.pending:
            ev, pin, what, scratch = item
            if block:
                ev.synchronize()
            if not ev.query():
                keep.append(item)
            elif int(pin[0]) != 0:
                self.pending = []
                self.clear(scratch)
                raise RuntimeError("sfsn_gsn_stack_scan: a layer-to-layer hand-off wait expired in an earlier launch "
                                   f"(that forward's results are invalid): {what}")
        self.pending = keep

    def clear(self, scratch) -> None:
        """After a failed launch: the error word is sticky by design (nobody clears it on the device) and the progress counters
        of a launch that gave up are not all zeroed by its last workgroup -- reset both, or every later launch on this scratch
        buffer would report the old failure.  Synchronised on both sides: no launch may still poll the counters, and none may
        start before they are zero."""
        torch.cuda.synchronize(self.engine.device)
        for sc in scratch:
            sc.zero_()
        torch.cuda.synchronize(self.engine.device)

    def check(self) -> None:
        """Raise if a watched launch failed (synchronises the device)."""
        torch.cuda.synchronize(self.engine.device)
        self.poll(block=True)


@dataclass
class _ModelRun:
    """One of the two models of a forward (full-band, sub-band) as the launch loop sees it."""
    tag: str                 # "fb" | "sb"
    seqs: list               # its sequence models (_Seq): one, or one per sub-band group
    d: dict                  # their per-forward tensors (_alloc_stack)
    xs: list                 # feature rows per sequence model, [T, R, I]
    first: int               # index of its layer 0 among the forward's stages (streams)
    rpw: int                 # rows per workgroup of its per-layer scans
    fg: object               # FeatureGroup array of its feature launch
    fb_proj: Optional[torch.Tensor]  # sub-band: the full-band model's output, read by the features and the statistics
    dims: tuple              # (B, F, T, width of fb_proj, fdrc) of the feature launches
    mu: Optional[torch.Tensor]       # offline norms: the clips' statistics of its input ...
    sd: Optional[torch.Tensor]       # ... (offline_gaussian_norm only)
    cum0: int                # cumulative_laplace_norm: index of its first running-mean state


@dataclass
class _Forward:
    """What one forward's steps share: its plan, tensors and streams, and what a step reports to a later one."""
    plan: ForwardPlan
    ri: torch.Tensor         # the input as [B, F, T, 2] float32
    want_layers: bool
    want_membrane: bool
    frames: Optional[list]   # ragged batch: the clips' lengths, on the host / ...
    frames_dev: Optional[torch.Tensor]  # ... on the device
    fbm: _ModelRun
    sbm: _ModelRun
    enh: torch.Tensor
    enh_ri: torch.Tensor
    enh_mag: torch.Tensor
    dfg: object              # DfGroup array of the deep filter
    stats_scratch: Optional[torch.Tensor]
    cum: Optional[dict]      # cumulative_laplace_norm: running-mean states and scratch
    zero: Optional[torch.Tensor]  # the scans' state buffer while it waits for the feature launch that zeroes it (then None)
    in_scan: bool            # the scans count their spikes
    write_proj: bool         # the coefficient rows are wanted
    main: Optional[torch.cuda.Stream] = None  # the calling stream; per stage: the streams of the scans / of the time-parallel kernels ...
    sstreams: list = field(default_factory=list)
    gstreams: list = field(default_factory=list)
    hS: list = field(default_factory=list)    # ... and their handles for the C ABI
    hG: list = field(default_factory=list)
    x_skipped: dict = field(default_factory=lambda: dict(fb=set(), sb=set()))  # feature rows a fused feature launch did not write
    proj_skipped: bool = False  # the fused epilogue ran and left the coefficient rows unwritten
    epi_chunk: Optional[tuple] = None  # (t0, nt) of the sub-band chunk whose epilogue ran inside its scan launch (_stage_scan_l01)
    lead: int = 0            # a forward with a start (_start_buffers): history frames in front of the new ones; the stages run behind them
    frames_before: int = 0   # ... and the frames the clips had seen before (cumulative_laplace_norm's denominator)
    l0_alone: Optional[dict] = None  # per-clip ends: {tag: [(sequence model, rows of x as [T * R] indices, ascending)]} -- _l0_as_alone

    def link(self, src, dst) -> None:
        """dst waits for everything enqueued on src so far (no-op on the sequential path)."""
        if self.plan.staged and src is not dst:
            dst.wait_event(_record(src))


def _record(stream) -> torch.cuda.Event:
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev


def _pick(lst, idx):
    return [lst[i] for i in idx]


class Engine:
    """Packed weights + launch sequence for one model on one device."""

    def __init__(self, spec: PathSpec, state_dict: Dict[str, np.ndarray], device, weight_bits: int = 24):
        """weight_bits = 24: the exact fp32-parity mode.  16: the 16-bit-weight fast mode -- the recurrent, spike-input and
        projection weights rounded to 16 significant bits of their row grid (the real-valued layer-0 input product stays
        exact); reported against the fp32 oracle by tests/test_hip_parity.py::test_sixteen_bit_weight_mode_report."""
        if weight_bits not in (24, 16):
            raise ValueError("weight_bits must be 24 (exact) or 16")
        self.weight_bits = weight_bits
        self.w16_fast = os.environ.get("SFSN_W16_FAST", "1") != "0"  # 16-bit mode: skip the zero digit plane in the scans that can
        self.spec = spec
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("spiking_fullsubnet_amd runs on a HIP device only (no CPU path); move the module to 'cuda'")
        self.lib = _lib.lib()
        self.n_cu = torch.cuda.get_device_properties(self.device).multi_processor_count  # asked once: the schedule rules read it per forward
        for H in (spec.fb_hidden, spec.sb_hidden):
            if H % 16 != 0 or H > _lib.MAX_HIDDEN:
                raise NotImplementedError(f"hidden size {H}: the gfx950 scan holds W_hh register-resident for H % 16 == 0, H <= {_lib.MAX_HIDDEN}")
        if spec.n_groups > _lib.MAX_SEGMENTS:
            raise NotImplementedError(f"more than {_lib.MAX_SEGMENTS} sub-band groups")
        if len(spec.cutoffs) == 2:
            raise NotImplementedError("single-group models hit a latent reflect-pad quirk of the reference (SubbandModel._freq_unfold)")
        sd = {k: np.asarray(v) for k, v in state_dict.items()}
        self.fb = _pack_seq(sd, "fb_model.", spec, spec.fb_in, spec.fb_hidden, spec.fb_layers, spec.fb_proj, spec.ln_fb, self.device, weight_bits)
        self.sb = [_pack_seq(sd, f"sb_model.sb_models.{g}.", spec, spec.sb_input_size(g), spec.sb_hidden, spec.sb_layers,
                             spec.sb_proj_size(g), spec.ln_sb, self.device, weight_bits) for g in range(spec.n_groups)]
        self._ws: Dict[tuple, dict] = {}
        self.ws_budget_bytes = int(float(os.environ.get("SFSN_WS_BUDGET_GB", "96")) * 2**30)  # scratch cache budget (of 288 GB HBM)
        self.timers: Optional[dict] = None  # set to {} to record HIP events around each launch group (bench.py)
        self.seq_chunk = 0  # frames per chunk of the single-stream schedule (0 = whole sequence per launch)
        self.rows_per_wg = (0, 0)  # (full-band, sub-band) rows per scan workgroup; 0 = let the library spread over all CUs
        self.fuse_input = True  # input term inside the scan where the geometry allows it (see _fusable / _fusable_x)
        self.launches: Dict[str, int] = {}  # launches per C-ABI scan entry point (tests assert which path ran)
        self.timer_tags = None  # optional set of tags to time (each timed group costs ~10 us of launch gap)
        self._stream_objs: Dict[int, torch.cuda.Stream] = {}
        self._side: List[torch.cuda.Stream] = []
        self.pipeline_chunk = 128  # frames per chunk of the time-pipelined schedule
        self.pipeline_default = False  # opt-in until the stages own disjoint CU sets
        self.pipeline_two_phase = bool(int(os.environ.get('SFSN_TWO_PHASE', '1')))
        # layer-pipelined stack scan (sfsn_gsn_stack_scan): all layers of a stack in one launch, layer l+1 trailing layer l
        # by a few frames.  Shared gate weights only; membrane outputs (a test tap of the per-layer kernel) use the per-layer path.
        _ss = os.environ.get('SFSN_STACK_SCAN', 'auto')
        self.stack_scan = "auto" if _ss == "auto" else bool(int(_ss))
        self.stack_rows_fb_auto = int(os.environ.get("SFSN_FB_STACK_ROWS", "4"))  # rows per workgroup of the full-band stack under "auto"
        self.split_scan = os.environ.get("SFSN_SPLIT_SCAN", "1") != "0"  # large separate gate weights: sfsn_gsn_layer_scan_split (see _stage_scan)
        self.merge_products = os.environ.get("SFSN_MERGE_PRODUCTS", "1") != "0"  # the independent products of a stage in one launch
        # features + layer-0 input products of a chunk in ONE launch (sfsn_features_proj): the rows never make the round trip through
        # HBM between the two, and are not written at all when nobody reads them (layer_outputs "counts" / "none").  OFF by default:
        # bit-identical and 0.34 GB less traffic per forward, but slower -- the row arithmetic is bound by VALU issue (~110 wave
        # instructions per row) and the product's W pieces (120 registers per wave) leave two waves per SIMD where the feature kernel
        # has three: 316 us per sub-band chunk against 67 + 72 (profiles/EXPERIMENTS.md).  SFSN_FEATPROJ=1 switches it on.
        self.fuse_featproj = os.environ.get("SFSN_FEATPROJ", "0") == "1"
        # round 6: the sub-band projection, the output re-index, the deep filter and |.| in ONE launch (sfsn_proj_deepfilter): the
        # coefficient rows are written once and never re-read (0.3 GB per forward at B = 64, T = 1000).  SFSN_PROJDF=0: the two launches.
        self.fuse_projdf = os.environ.get("SFSN_PROJDF", "1") != "0"
        # opt-in for the lean modes (want_layers False): the coefficient rows (`all_layer_outputs[-1]`) are not written either -- the live
        # recipe discards the lists (trainer.py:31,52) and metric.compute_neuronops reads size(-1) only; the entry keeps its shape as a
        # meta tensor, like the feature rows a fused feature launch skips.  Off by default: `layer_outputs = "counts"` promises the
        # projection tensor (tests).  bench.py's no-layer-outputs leg switches it on and says so.
        self.lean_skips_proj = os.environ.get("SFSN_LEAN_SKIP_PROJ", "0") == "1"
        self._l0_hop = None  # set around a forward by StreamingSession.prime (per-kernel tier): see _stage_input
        self.count_in_scan = os.environ.get("SFSN_COUNT_IN_SCAN", "1") != "0"  # layer_outputs="counts": counted by the scans themselves
        self.pair_scan = os.environ.get("SFSN_PAIR_SCAN", "1") != "0"  # H <= 224 stacks as one launch of FUSED3 roles (see _stack_choice)
        # layer 0 of the per-layer path at 16 rows per workgroup: the fused-x groups and the groups with an input term in ONE launch
        # (sfsn_gsn_layer_scan_l0: same results; with few hardware queues a forward is as long as its chain of launches)
        self.merge_layer0 = os.environ.get("SFSN_L0_MERGE", "1") != "0"
        self._l0_refused = set()  # geometries the library answered SFSN_EUNSUPPORTED for (the two calls then, without asking again)
        # layers 0 AND 1 of a two-layer stack of the per-layer path at 16 rows per workgroup in ONE launch (sfsn_gsn_layer_scan_l01: same
        # results, layer 1 trailing layer 0 by a few frames; the next link cut from the chain).  Not under graph capture and
        # not on the staged schedules, which keep their per-layer launches.  SFSN_L01_PAIR=0 / 1 overrides the default.
        self.pair16 = os.environ.get("SFSN_L01_PAIR", "1") != "0"
        self._l01_refused = set()
        # ... and the sub-band epilogue (sfsn_proj_deepfilter's work) as a third tier of workgroups of that launch
        # (sfsn_gsn_layer_scan_l01_projdf: same results; the epilogue follows layer 1 a 16-frame tile or two behind and its launch leaves
        # the forward's chain).  Taken only where the pair launch AND the one-launch epilogue would be taken.  ON by default: +2.1 % / +3.75 %
        # on bench.py's timed region at four hardware queues, 16 of 16 pairs (profiles/l01_epilogue_one_launch.md).  SFSN_L01_PROJDF=0 / 1
        # overrides the default.
        self.pair16_epilogue = os.environ.get("SFSN_L01_PROJDF", "1") != "0"
        self._l01e_refused = set()
        self.stack_rows_per_wg = dict(STACK_ROWS_PER_WG)  # rows per workgroup of every layer of a stack: sum of workgroups <= CUs
        # frames a consumer role that had to wait lets its producers run ahead before it resumes (the hand-offs' hysteresis).  Round 2: 16
        # (every wave of a workgroup stood in the poll); since the IO-wave roles one lane polls, and a launch ends lag + ring frames after
        # its first layer does: 16 / 8 / 4 / 2 / 1 -> strict forward 2.74-2.76 / 2.65-2.70 / 2.62 / 2.63 / 2.63 ms (scripts/exp_lag_r05.sh)
        self.stack_lag = int(os.environ.get("SFSN_STACK_LAG", "4"))
        # full-band / sub-band overlap of ONE forward: the sequence is cut into this many chunks, the full-band model runs them
        # on one stream, the sub-band models follow one chunk behind on a second stream (they need the full-band output of the
        # SAME frames only, MODEL:441-447; states are carried by the ABI's h_state / c_state).  The full-band chain (few
        # workgroups, long) then hides behind the sub-band work of the previous chunk.  0 / 1 = off.
        # Measured (B=64, T=1000, scripts/exp_overlap.py): 3.93 ms without, 3.67 / 3.60 / 3.62 / 3.87 / 4.38 ms with 2 / 3 / 4 / 5 / 8
        # chunks -- every chunk costs ~0.15 ms of launch boundaries, scan prologues and hand-off lag.  Off when several forwards
        # are in flight anyway (bench.py's timed region sets 0).
        self.overlap_chunks = int(os.environ.get("SFSN_OVERLAP_CHUNKS", "3"))
        self.overlap_fracs = None  # optional explicit chunk lengths (fractions of T) of the overlapped schedule
        if os.environ.get("SFSN_OVERLAP_FRACS"):
            self.overlap_fracs = [float(v) for v in os.environ["SFSN_OVERLAP_FRACS"].split(",")]
        # frames of the first chunk: -1 = 0.24 T (measured, scripts/exp_overlap.py: 3.55 -> 3.40 ms at B=64, the same 3-4 % at B=4..32 and
        # T=500; 64..128 frames and 0.32 T gain nothing), 0 = equal chunks
        self.overlap_first = int(os.environ.get("SFSN_OVERLAP_FIRST", "-1"))
        # True: forward_stft() returns only after the error words of its stack launches have been read (a launch whose bounded
        # hand-off wait expired raises HERE instead of at the next forward); False: non-blocking, see check_stack_errors()
        self.strict_errors = os.environ.get("SFSN_STRICT_ERRORS", "0") == "1"
        self._ov_streams = None
        self.stack_wide = True
        self._stack_scratch: List[torch.Tensor] = []
        self._errors = ErrorWords(self)  # the launches' error words: polled at the next forward
        self._defer_err = None  # overlapped schedule: [(what, scratch)] of the running forward's stack launches (one copy per forward)
        self._err_stream = None  # ErrorWords' stream for the once-per-forward collection
        self.hw_queues = _check_hw_queues()
        self._last_forward: Dict[int, torch.cuda.Event] = {}  # per calling stream: recorded behind its most recent forward

    # ---------------------------------------------------------------------------------------------
    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _count(self, what: str) -> None:
        self.launches[what] = self.launches.get(what, 0) + 1

    class _Timed:
        """HIP events on the launch stream around a group of launches; no-op unless ``engine.timers`` is a dict."""

        def __init__(self, eng, tag, stream):
            self.eng, self.tag, self.stream = eng, tag, stream

        def __enter__(self):
            self.on = self.eng.timers is not None and (self.eng.timer_tags is None or self.tag in self.eng.timer_tags)
            if self.on:
                self.e0 = torch.cuda.Event(enable_timing=True)
                self.e1 = torch.cuda.Event(enable_timing=True)
                self.e0.record(self.eng._tstream(self.stream))
            return self

        def __exit__(self, *exc):
            if self.on:
                self.e1.record(self.eng._tstream(self.stream))
                self.eng.timers.setdefault(self.tag, []).append((self.e0, self.e1))
            return False

    def timed(self, tag, st=None):
        return Engine._Timed(self, tag, st)

    def _tstream(self, st):
        """torch stream object for a raw stream handle handed to the C ABI (None = current stream)."""
        if st is None:
            return torch.cuda.current_stream(self.device)
        return self._stream_objs.get(st.value, torch.cuda.current_stream(self.device))

    def timer_summary(self) -> dict:
        """{tag: {mean_ms, n}} per launch group (one group = the launches of one call site in one forward)."""
        if not self.timers:
            return {}
        torch.cuda.synchronize(self.device)
        out = {}
        for tag, evs in self.timers.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            out[tag] = dict(mean_ms=float(np.mean(ms)), min_ms=float(np.min(ms)), n=len(ms))
        return out

    @staticmethod
    def _nbytes(obj) -> int:
        if torch.is_tensor(obj):
            return obj.numel() * obj.element_size()
        if isinstance(obj, dict):
            return sum(Engine._nbytes(v) for v in obj.values())
        if isinstance(obj, (list, tuple)):
            return sum(Engine._nbytes(v) for v in obj)
        return 0

    def _workspace(self, key, make):
        """Scratch cache: least-recently-used entries are dropped once the total exceeds `ws_budget_bytes` (the entry being
        asked for is never dropped).  Entries are keyed on (tag, rows, stream) and sized by CAPACITY (see _alloc_stack): a
        stream that sees clips of many lengths keeps one buffer set, grown to the longest."""
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = make()
            total = sum(self._nbytes(v) for v in self._ws.values())
            for k in list(self._ws.keys()):
                if total <= self.ws_budget_bytes or k == key:
                    continue
                total -= self._nbytes(self._ws.pop(k))
        else:
            self._ws[key] = self._ws.pop(key)  # most recently used last (dicts keep insertion order)
        return ws

    # ---- per-stage launch helpers: every one works on the frame range [t0, t0+nt) and on an explicit stream, so
    #      that the same code serves the sequential path (one chunk, current stream) and the time-pipelined path ----
    def _stage_input(self, seqs, l, srcs, zins, t0, nt, st, tag):
        """zin (chunk-local, [nt, R, G*H]) = layer input . W_ih^T + bias_ih.  srcs: x (l = 0, full [T,R,I] fp32) or the
        previous layer's int8 spikes (l >= 1, full [T,R,HP])."""
        L = self.lib
        with self.timed(("inproj:" if l == 0 else "spikeproj_in:") + tag, st):
            jobs = []  # (x or s, w, dq, bias, z, M, K, N, ld) per (sequence model, gate)
            for seq, src, z in zip(seqs, srcs, zins):
                cell, H, G, R = seq.cells[l], seq.H, seq.cells[l].G, src.shape[1]
                M = nt * R
                for g in range(G):
                    zp = z.data_ptr() + g * H * 4
                    bp = cell.bias.data_ptr() + g * H * 4
                    if l == 0:
                        jobs.append((src.data_ptr() + t0 * R * seq.I * 4, cell.w_ih_f32.data_ptr() + g * H * seq.I * 4, None, bp, zp, M, seq.I, H, G * H))
                    else:
                        pk, dq = cell.w_ih_q[g]
                        jobs.append((src.data_ptr() + t0 * R * src.shape[2], pk.data_ptr(), dq.data_ptr(), bp, zp, M, H, H, G * H))
            if l == 0 and self._l0_hop is not None:
                # (StreamingSession.prime, per-kernel tier) the real-valued product in the form a streaming step takes: below 64 rows
                # sfsn_input_proj_f32 adds the chunks into one accumulator, from 64 rows on it takes the bf16 split -- another rounding
                # (include/sfsn.h).  Whole frames per call, fewer than 64 rows each: the step's bits at a fraction of its launches.
                P = ctypes.c_void_p
                for (a_, w_, _, b_, z_, M, K, N, ld), src in zip(jobs, [s_ for s_ in srcs for _ in range(seqs[0].cells[0].G)]):
                    R = src.shape[1]
                    step = self._l0_hop * R if self._l0_hop * R >= 64 else 63 // R * R  # (64 rows and more: the step's own call)
                    for r0 in range(0, M, step):
                        check(L.sfsn_input_proj_f32(P(a_ + r0 * K * 4), P(w_), P(b_), P(z_ + r0 * ld * 4), min(step, M - r0), K, N, ld, st),
                              "sfsn_input_proj_f32")
                return
            if self.merge_products and 1 < len(jobs) <= _lib.MAX_SEGMENTS:
                # the products of a stage in ONE launch (a block range per job, every job its own tiling: the same results)
                if l == 0:
                    arr = (InProjJob * len(jobs))()
                    for a, (x_, w_, _, b_, z_, M, K, N, ld) in zip(arr, jobs):
                        a.x, a.w, a.bias, a.z, a.M, a.K, a.N, a.ldz = x_, w_, b_, z_, M, K, N, ld
                    rc = L.sfsn_input_proj_f32_multi(arr, len(jobs), st)
                else:
                    arr = (ProjJob * len(jobs))()
                    for a, (s_, w_, dq_, b_, z_, M, K, N, ld) in zip(arr, jobs):
                        a.s, a.w_packed, a.w_dq, a.bias, a.y, a.M, a.K, a.N, a.ldy = s_, w_, dq_, b_, z_, M, K, N, ld
                    rc = L.sfsn_spike_proj_multi(arr, len(jobs), st)
                if rc == 0:
                    self._count("merged_products")
                    return
                if rc != _lib.SFSN_EUNSUPPORTED:
                    check(rc, "sfsn_input_proj_f32_multi" if l == 0 else "sfsn_spike_proj_multi")
            P = ctypes.c_void_p
            for a_, w_, dq_, b_, z_, M, K, N, ld in jobs:
                if l == 0:
                    check(L.sfsn_input_proj_f32(P(a_), P(w_), P(b_), P(z_), M, K, N, ld, st), "sfsn_input_proj_f32")
                else:
                    check(L.sfsn_spike_proj(P(a_), P(w_), P(dq_), P(b_), P(z_), M, K, N, ld, st), "sfsn_spike_proj")

    def _stage_featproj(self, fg, seqs, idx, zins, stft_ri, fb_proj, dims, t0, nt, zero, need_x, st, tag) -> bool:
        """Features of every group of `fg` AND the layer-0 input term of the groups `idx` (zins: their chunk-local buffers) in one
        launch.  False (nothing launched) when the library would not run the pair bit-identically (sfsn_features_proj's
        SFSN_EUNSUPPORTED, separate gate weights): the caller issues the two calls then.  need_x False: the rows of the groups in
        `idx` are not written."""
        B, F, T, FB, fdrc = dims
        n = len(seqs)
        if not self.fuse_featproj or not idx or n > _lib.MAX_GROUPS or any(seqs[i].cells[0].G != 1 for i in idx):
            return False
        jobs = (FeatProjJob * n)()
        for i in range(n):
            jobs[i].feat = fg[i]
            if i in idx:
                seq, z = seqs[i], zins[idx.index(i)]
                cell = seq.cells[0]
                jobs[i].w, jobs[i].bias, jobs[i].z = cell.w_ih_f32.data_ptr(), cell.bias.data_ptr(), z.data_ptr()
                jobs[i].H, jobs[i].ldz = seq.H, seq.H
                if not need_x:
                    jobs[i].feat.x = None
        with self.timed("featproj:" + tag, st):
            rc = self.lib.sfsn_features_proj(_ptr(stft_ri), None if fb_proj is None else _ptr(fb_proj), B, F, T, FB, fdrc, jobs, n, t0, nt,
                                             None if zero is None else _ptr(zero), 0 if zero is None else zero.numel() * 4, st)
        if rc == _lib.SFSN_EUNSUPPORTED:
            return False
        check(rc, "sfsn_features_proj")
        self._count("featproj")
        return True

    def _stage_scan(self, seqs, l, zins, states, spks, s8s, mems, t0, nt, st, tag, rpw, cnts=None):
        L, spec = self.lib, self.spec
        H = seqs[0].H
        segs = (ScanSegment * len(seqs))()
        for i, seq in enumerate(seqs):
            fill_segment(segs[i], seq.cells[l], s8s[i].shape[1], H, t0, zins[i], states[i], s8s[i], spks[i], mems[i],
                         None if cnts is None else cnts[i])
        with self.timed("scan:" + tag, st):
            rc = _lib.SFSN_EUNSUPPORTED
            if (self.split_scan and not spec.shared and H > 256 and len(seqs) == 1 and nt >= 16
                    and not torch.cuda.is_current_stream_capturing()):
                # separate gate weights too large for one compute unit (baseline_xl's full-band model): the tiles of a row block split
                # over workgroups with resident weights and a spike exchange per step, instead of streaming all of W_hh every step
                # (10 us per step): same results; its scratch (tagged exchange words, error word first) is zeroed per call.  Not for a
                # few frames (a streaming hop: the workgroups' weights are loaded per call) and not under graph capture (the scratch
                # buffer is this call's)
                R0 = s8s[0].shape[1]
                stream = self._tstream(st)
                with torch.cuda.stream(stream):
                    # allocated AND zeroed under the launch's stream: the block then comes from that stream's pool, so its previous use
                    # is ordered before the fill (round-5 advisor finding: a block freed on the caller's stream could still be in use
                    # there when the stage stream zeroed it -- a corrupted epoch tag ends in a bounded-spin error)
                    scr = torch.zeros((L.sfsn_scan_split_scratch_bytes(R0, H) // 4,), dtype=torch.int32, device=self.device)
                rc = L.sfsn_gsn_layer_scan_split(segs, 1, nt, H, 0, _ptr(scr), scr.numel() * 4, st)
                if rc == 0:
                    self._errors.watch(stream, scr, f"split scan {tag} H={H}")
                    self._count("split_scan")
                    return
                if rc != _lib.SFSN_EUNSUPPORTED:
                    check(rc, "sfsn_gsn_layer_scan_split")
            if self.weight_bits == 16 and self.w16_fast:  # the two-plane scan where the library has it (same results)
                rc = L.sfsn_gsn_layer_scan_w16(segs, len(seqs), nt, H, int(spec.shared), rpw, st)
                if rc not in (0, _lib.SFSN_EUNSUPPORTED):
                    check(rc, "sfsn_gsn_layer_scan_w16")
            if rc != 0:
                check(L.sfsn_gsn_layer_scan(segs, len(seqs), nt, H, int(spec.shared), rpw, st), "sfsn_gsn_layer_scan")

    def _fusable(self, seqs, rpw, want_membrane) -> bool:
        """Layers >= 1 can take their input term inside the scan (sfsn_gsn_layer_scan_fused): shared gates, 128 < H <= 256,
        16 rows per workgroup -- the launch geometry of a full chip, where the scan is HBM-bound and the saved round trip of
        the fp32 input term is pure gain; with 4 rows per workgroup (one forward alone) the doubled MFMA work would cost more."""
        return bool(self.fuse_input and self.spec.shared and 128 < seqs[0].H <= 256 and rpw == 16 and not want_membrane)

    def _fusable_x(self, seq, x, rpw, want_membrane) -> bool:
        """Layer 0 of a group can take its real-valued input product inside the scan (sfsn_gsn_layer_scan_fused_x) when, on
        top of _fusable's conditions, the feature rows are narrow (even I <= 64: W_ih pieces fit in registers) and the row
        count is a multiple of 16 (a step's rows are copied as one flat block)."""
        return bool(self.fuse_input and self.spec.shared and 128 < seq.H <= 256 and rpw == 16 and not want_membrane
                    and seq.I % 2 == 0 and seq.I <= 64 and x.shape[1] % 16 == 0)

    # ---- the argument arrays of the 16-row scan entry points, for the groups `idx` of `seqs` (an empty list gives arrays of one unused
    #      entry: ctypes has no empty array to pass).  states / spks / s8s / cnts: the layer's, indexed by group.
    @staticmethod
    def _segs_fused_x(seqs, idx, xs_, states, spks, s8s, H, t0, cnts=None):
        """Layer 0 with the input product inside the scan: (ScanSegment array, FusedX array)."""
        segs, fin = (ScanSegment * max(len(idx), 1))(), (FusedX * max(len(idx), 1))()
        for k, i in enumerate(idx):
            cell, R = seqs[i].cells[0], xs_[i].shape[1]
            fill_segment(segs[k], cell, R, H, t0, None, states[i], s8s[i], spks[i], count=None if cnts is None else cnts[i])
            fin[k].x = xs_[i].data_ptr() + t0 * R * seqs[i].I * 4
            fin[k].w_ih, fin[k].I = cell.w_ih_f32.data_ptr(), seqs[i].I
        return segs, fin

    @staticmethod
    def _segs_zin(seqs, idx, zins, states, spks, s8s, H, t0, cnts=None):
        """Layer 0 with its input term in `zins`: ScanSegment array."""
        segs = (ScanSegment * max(len(idx), 1))()
        for k, i in enumerate(idx):
            fill_segment(segs[k], seqs[i].cells[0], s8s[i].shape[1], H, t0, zins[i], states[i], s8s[i], spks[i],
                         count=None if cnts is None else cnts[i])
        return segs

    @staticmethod
    def _segs_fused(seqs, idx, l, states, spks, s8_in, s8s, H, t0, cnts=None):
        """Layer l >= 1 with the input product of the int8 spikes `s8_in` inside the scan: (ScanSegment array, FusedInput array)."""
        HP = (H + 63) // 64 * 64
        segs, fin = (ScanSegment * max(len(idx), 1))(), (FusedInput * max(len(idx), 1))()
        for k, i in enumerate(idx):
            cell, R = seqs[i].cells[l], s8s[i].shape[1]
            pk, dq = cell.w_ih_q[0]
            fill_segment(segs[k], cell, R, H, t0, None, states[i], s8s[i], spks[i], count=None if cnts is None else cnts[i])
            fin[k].spikes_in = s8_in[i].data_ptr() + t0 * R * HP
            fin[k].w_ih, fin[k].w_ih_dq = pk.data_ptr(), dq.data_ptr()
        return segs, fin

    def _projdf_groups(self, seqs, s8s, projs, write_proj):
        """The groups of the sub-band epilogue (last-layer spikes `s8s`, coefficient rows `projs`): ProjDfGroup array."""
        spec = self.spec
        arr = (ProjDfGroup * len(seqs))()
        for g, (a, seq, s8, y) in enumerate(zip(arr, seqs, s8s, projs)):
            a.spikes_i8, a.w_packed, a.w_dq, a.bias = s8.data_ptr(), seq.proj_q.data_ptr(), seq.proj_dq.data_ptr(), seq.proj_b.data_ptr()
            a.proj = y.data_ptr() if write_proj else None
            a.n_units, a.fc, a.df = spec.units(g), spec.ctr[g], spec.df[g]
        return arr

    def _stage_scan_fused_x(self, seqs, xs_, states, spks, s8s, t0, nt, st, tag, cnts=None):
        """Layer 0 of the given sequence models, input product inside the scan."""
        L = self.lib
        H = seqs[0].H
        segs, fin = self._segs_fused_x(seqs, range(len(seqs)), xs_, states, spks, s8s, H, t0, cnts)
        self._count("fused_x")
        with self.timed("scanx:" + tag, st):
            check(L.sfsn_gsn_layer_scan_fused_x(segs, fin, len(seqs), nt, H, st), "sfsn_gsn_layer_scan_fused_x")

    def _stage_scan_l0(self, seqs, fx, rest, xs_, zins, states, spks, s8s, t0, nt, st, tag, cnts=None) -> bool:
        """Layer 0 of the groups `fx` (input product inside the scan) and `rest` (input term in `zins`) in ONE launch at 16 rows per
        workgroup (sfsn_gsn_layer_scan_l0): the same results as _stage_scan_fused_x + _stage_scan, one link shorter in the forward's
        chain of launches.  False (nothing launched) where the library refuses the pair; the refusal is remembered per geometry."""
        H = seqs[0].H
        key = (H, tuple((xs_[i].shape[1], seqs[i].I) for i in fx), tuple(xs_[i].shape[1] for i in rest), spks[fx[0]] is None)
        if key in self._l0_refused:
            return False
        sx, fin = self._segs_fused_x(seqs, fx, xs_, states, spks, s8s, H, t0, cnts)
        sz = self._segs_zin(seqs, rest, zins, states, spks, s8s, H, t0, cnts)
        with self.timed("scanx:" + tag, st):
            rc = self.lib.sfsn_gsn_layer_scan_l0(sx, fin, len(fx), sz, len(rest), nt, H, int(self.spec.shared), st)
        if rc == _lib.SFSN_EUNSUPPORTED:
            self._l0_refused.add(key)
            return False
        check(rc, "sfsn_gsn_layer_scan_l0")
        self._count("fused_x")  # (the fused-x scan ran, as after _stage_scan_fused_x) ...
        self._count("l0_merged")  # ... inside the one launch: fused_x - l0_merged = the separate fused-x calls
        return True

    def _stage_scan_l01(self, seqs, fx, rest, xs_, d, t0, nt, st, tag, cn=None, epi=None) -> bool:
        """Layers 0 and 1 of a two-layer stack in ONE launch at 16 rows per workgroup (sfsn_gsn_layer_scan_l01): the layer-0 launch of
        _stage_scan_l0 (or the single call where `fx` or `rest` is empty) and _stage_scan_fused of layer 1 side by side, layer 1 trailing
        layer 0 by a few frames.  Scratch and error word as in _stage_stack.  False (nothing launched) where the library refuses; the
        refusal is remembered per geometry.  `epi` (the forward and its sub-band model, where the chunk's epilogue may join the launch):
        sfsn_gsn_layer_scan_l01_projdf with _stage_projdf's arguments; it notes the chunk in f.epi_chunk, and a refusal (remembered per
        geometry) leaves today's launch."""
        L = self.lib
        H = seqs[0].H
        order = list(fx) + list(rest)
        key = (H, tuple((xs_[i].shape[1], seqs[i].I) for i in fx), tuple(xs_[i].shape[1] for i in rest), d["spk"][0][order[0]] is None)
        if key in self._l01_refused:
            return False
        states, spks, s8s, zins = d["states"], d["spk"], d["s8"], d["zin"][0]
        cn0, cn1 = (None, None) if cn is None else (cn[0], cn[1])
        sx, fin = self._segs_fused_x(seqs, fx, xs_, states[0], spks[0], s8s[0], H, t0, cn0)
        sz = self._segs_zin(seqs, rest, zins, states[0], spks[0], s8s[0], H, t0, cn0)
        s1, fin1 = self._segs_fused(seqs, order, 1, states[1], spks[1], s8s[0], s8s[1], H, t0, cn1)
        rows = sum(s8s[1][i].shape[1] for i in order)
        nbytes = L.sfsn_stack_scratch_bytes(2, len(order), rows)

        def make():  # zero-filled once, on the stream the kernel is launched on (see _stage_stack)
            with torch.cuda.stream(self._tstream(st)):
                return dict(t=torch.zeros((nbytes // 4,), dtype=torch.int32, device=self.device))
        scratch = self._workspace(("l01_scratch", tag, len(order), rows, torch.cuda.current_stream(self.device).cuda_stream,
                                   self._tstream(st).cuda_stream), make)["t"]
        assert scratch.numel() * 4 >= nbytes
        rc = _lib.SFSN_EUNSUPPORTED
        ekey = key + (None if epi is None else (epi[0].write_proj, epi[1].dims[:3]),)
        if epi is not None and ekey not in self._l01e_refused:
            f, m = epi
            B, F, T = m.dims[:3]
            spec = self.spec
            arr = self._projdf_groups(seqs, s8s[1], d["proj"], f.write_proj)
            with self.timed("stack:" + tag, st):
                rc = L.sfsn_gsn_layer_scan_l01_projdf(sx if fx else None, fin if fx else None, len(fx), sz if rest else None, len(rest), s1, fin1,
                                                      H, int(self.spec.shared), self.stack_lag, _ptr(scratch), nbytes, _ptr(f.ri), B, F, T,
                                                      spec.num_spks, arr, len(seqs), _ptr(f.enh_ri), _ptr(f.enh_mag), t0, nt, st)
            if rc == _lib.SFSN_EUNSUPPORTED:
                self._l01e_refused.add(ekey)
            else:
                check(rc, "sfsn_gsn_layer_scan_l01_projdf")
                f.epi_chunk = (t0, nt)
                self._count("projdf")  # (the one-launch epilogue ran, as after _stage_projdf) ...
                self._count("l01_projdf")  # ... inside the scan launch
        if rc == _lib.SFSN_EUNSUPPORTED:
            with self.timed("stack:" + tag, st):
                rc = L.sfsn_gsn_layer_scan_l01(sx if fx else None, fin if fx else None, len(fx), sz if rest else None, len(rest), s1, fin1,
                                               nt, H, int(self.spec.shared), self.stack_lag, _ptr(scratch), nbytes, st)
        if rc == _lib.SFSN_EUNSUPPORTED:
            self._l01_refused.add(key)
            return False
        check(rc, "sfsn_gsn_layer_scan_l01")
        if not any(scratch is t for t in self._stack_scratch):
            self._stack_scratch.append(scratch)
        if fx:
            self._count("fused_x")  # (where the layer-0 launch this one replaces would have counted: _stage_scan_l0 / _stage_scan_fused_x)
            if rest:
                self._count("l0_merged")
        self._count("fused")  # layer 1's fused scan ran
        self._count("l01_pair")
        self._errors.watch(self._tstream(st), scratch, f"{tag} layers 0+1 rows={rows} frames={nt} lag={self.stack_lag}")
        return True

    def _stage_scan_fused(self, seqs, l, states, spks, s8s, t0, nt, st, tag, cnts=None):
        L = self.lib
        H = seqs[0].H
        segs, fin = self._segs_fused(seqs, range(len(seqs)), l, states, spks, s8s[l - 1], s8s[l], H, t0, cnts)
        self._count("fused")
        with self.timed("scanf:" + tag, st):
            check(L.sfsn_gsn_layer_scan_fused(segs, fin, len(seqs), nt, H, st), "sfsn_gsn_layer_scan_fused")

    def _stack_choice(self, seqs, Rs, want_membrane):
        """(use the stack launch?, wide flavour?, rows per workgroup) for one stack of sequence models: `stack_rule` with what only the
        engine knows -- the chip's compute units and whether the forward has the chip to itself."""
        H = seqs[0].H
        # (the launch assumes the forward has the chip to itself: its 2 x 104 workgroups wait for each other inside the launch.  A second
        #  forward of this engine still in flight on another stream (its end-of-forward event has not fired) takes the per-layer
        #  launches instead: round-4 advisor finding.  Work of OTHER processes or libraries cannot be seen from here; the waits
        #  are bounded and reported.)  Asked only where the rule reads it: the "auto" rule of an H <= 256 stack.
        alone = True
        if self.stack_scan == "auto" and H <= 256:
            me = torch.cuda.current_stream(self.device).cuda_stream
            alone = all(ev.query() for k, ev in self._last_forward.items() if k != me)
        return stack_rule(self.spec.shared, len(seqs[0].cells), H, len(seqs), Rs, want_membrane, self.stack_scan, self.stack_wide,
                          self.stack_rows_fb_auto, self.pair_scan, self.rows_per_wg, alone, self.n_cu)

    def _stack_x_groups(self, seqs, xs_, nt, wide, rpw_stack, want_membrane=False):
        """Groups whose LAYER 0 takes its real-valued input product inside the stack launch (FUSEDX3 role, sfsn_gsn_stack_scan_x):
        the layout H <= 224 stacks without input-term buffers get (8 rows per workgroup), even I <= 64, whole 8-row blocks, and at
        least 64 row-frames (below that sfsn_input_proj_f32 itself takes its fp32-MFMA form: the schedules would differ in the last bit)."""
        if not (self.fuse_input and self.pair_scan and self.spec.shared and not wide and rpw_stack == 8 and not want_membrane
                and seqs[0].H <= 224 and len(seqs[0].cells) >= 2 and not os.environ.get("SFSN_STACK_FUSED8")
                and not os.environ.get("SFSN_SCAN_V2")):  # (the library refuses the FUSEDX3 role under either switch)
            return []
        return [i for i, (seq, x) in enumerate(zip(seqs, xs_))
                if seq.I % 2 == 0 and seq.I <= 64 and x.shape[1] % 8 == 0 and nt * x.shape[1] >= 64]

    def _stage_stack(self, seqs, d, t0, nt, st, tag, wide, rpw_stack, lag=None, scratch=None, xs_=None, xg=()):
        """Every layer of the given sequence models in one launch (layer 0's input term is already in d["zin"][0]; for the groups
        in `xg` the launch forms it itself from the feature rows xs_[i])."""
        L = self.lib
        H, nl, ns = seqs[0].H, len(seqs[0].cells), len(seqs)
        HP = (H + 63) // 64 * 64
        segs = (ScanSegment * (nl * ns))()
        fin = (FusedInput * (nl * ns))()
        fx = (FusedX * ns)() if xg else None
        for i in xg:
            x, cell = xs_[i], seqs[i].cells[0]
            fx[i].x, fx[i].w_ih, fx[i].I = x.data_ptr() + t0 * x.shape[1] * seqs[i].I * 4, cell.w_ih_f32.data_ptr(), seqs[i].I
        rows = 0
        for l in range(nl):
            for i, seq in enumerate(seqs):
                cell, R = seq.cells[l], d["s8"][l][i].shape[1]
                rows += R if l == 0 else 0
                # layers >= 1: an input-term buffer selects the wide flavour for H <= 256 (16-wave scans fed by PROJ workgroups
                # of the same launch); without it the 8-wave fused-input roles run
                zin = d["zin"][l][i] if ((l == 0 and i not in xg) or (l > 0 and (H > 256 or wide))) else None
                fill_segment(segs[l * ns + i], cell, R, H, t0, zin, d["states"][l][i], d["s8"][l][i], d["spk"][l][i],
                             count=d["cnt"][l][i] if d.get("cnt") is not None else None)
                if l > 0:
                    pk, dq = cell.w_ih_q[0]
                    fin[l * ns + i].spikes_in = d["s8"][l - 1][i].data_ptr() + t0 * R * HP
                    fin[l * ns + i].w_ih, fin[l * ns + i].w_ih_dq = pk.data_ptr(), dq.data_ptr()
        nbytes = L.sfsn_stack_scratch_bytes(nl, ns, rows)
        own_scratch = scratch is None
        if scratch is None:  # (a streaming session owns its own: its captured graph must not outlive a cache entry)
            def make():
                # zero-filled on the stream the kernel is launched on: on the overlapped schedule that is a side stream which
                # only waits for the fork event, and a fill enqueued on the caller's stream after that event would not be
                # ordered before the kernel that polls these counters (round-2 advisor finding)
                with torch.cuda.stream(self._tstream(st)):
                    return dict(t=torch.zeros((nbytes // 4,), dtype=torch.int32, device=self.device))
            scratch = self._workspace(("stack_scratch", tag, nl, ns, rows, torch.cuda.current_stream(self.device).cuda_stream,
                                       self._tstream(st).cuda_stream), make)["t"]
        assert scratch.numel() * 4 >= nbytes
        if not any(scratch is t for t in self._stack_scratch):
            self._stack_scratch.append(scratch)
        rp = rpw_stack if rpw_stack else self.stack_rows_per_wg[tag]
        rpw = (ctypes.c_int * nl)(*([rp] * nl))
        lag = self.stack_lag if lag is None else lag
        self._count("stack")
        with self.timed("stack:" + tag, st):
            rc16 = _lib.SFSN_EUNSUPPORTED
            if self.weight_bits == 16 and self.w16_fast:  # the two-plane roles where the library has them (the pair layout): same results
                rc16 = L.sfsn_gsn_stack_scan_x_w16(segs, fin, fx, nl, ns, nt, H, rpw, lag, _ptr(scratch), nbytes, st)
                if rc16 not in (0, _lib.SFSN_EUNSUPPORTED):
                    check(rc16, "sfsn_gsn_stack_scan_x_w16")
                if rc16 == 0:
                    self._count("stack_w16")
            if rc16 == 0:
                pass
            elif xg:
                check(L.sfsn_gsn_stack_scan_x(segs, fin, fx, nl, ns, nt, H, rpw, lag, _ptr(scratch), nbytes, st),
                      "sfsn_gsn_stack_scan_x")
            else:
                check(L.sfsn_gsn_stack_scan(segs, fin, nl, ns, nt, H, rpw, lag, _ptr(scratch), nbytes, st),
                      "sfsn_gsn_stack_scan")
        if not torch.cuda.is_current_stream_capturing():  # the launch's error word (ErrorWords)
            what = f"{tag} rows={rows} frames={nt} wide={wide} rows_per_wg={rp} lag={lag}"
            if self._defer_err is not None and own_scratch:
                # the overlapped schedule of a forward alone: the copy (a 4-byte blit + its completion) would sit between this launch
                # and the projection that follows it on the same stream, ~10 us on the forward's chain per launch -- the forward
                # collects its launches' words once, off the chain, when its streams have joined (_forward_stft)
                self._defer_err.append((what, scratch))
                return
            self._errors.watch(self._tstream(st), scratch, what)

    def check_stack_errors(self) -> None:
        """Raise if a hand-off wait of a stack launch expired (synchronises; tests and bench call it after a forward)."""
        self._errors.check()
        for t in self._stack_scratch:
            if int(t[0].item()) != 0:
                self._errors.clear([t])
                raise RuntimeError("sfsn_gsn_stack_scan: a layer-to-layer hand-off wait expired (results invalid)")

    def _stage_proj(self, seqs, s8s, projs, t0, nt, st, tag):
        L = self.lib
        with self.timed("proj:" + tag, st):
            if self.merge_products and 1 < len(seqs) <= _lib.MAX_SEGMENTS:  # the groups' projections in ONE launch
                arr = (ProjJob * len(seqs))()
                for a, seq, s8, y in zip(arr, seqs, s8s, projs):
                    R = s8.shape[1]
                    a.s, a.w_packed, a.w_dq, a.bias = s8.data_ptr() + t0 * R * s8.shape[2], seq.proj_q.data_ptr(), seq.proj_dq.data_ptr(), seq.proj_b.data_ptr()
                    a.y, a.M, a.K, a.N, a.ldy = y.data_ptr() + t0 * R * seq.P * 4, nt * R, seq.H, seq.P, seq.P
                rc = L.sfsn_spike_proj_multi(arr, len(seqs), st)
                if rc == 0:
                    self._count("merged_products")
                    return
                if rc != _lib.SFSN_EUNSUPPORTED:
                    check(rc, "sfsn_spike_proj_multi(proj)")
            for seq, s8, y in zip(seqs, s8s, projs):
                R = s8.shape[1]
                check(L.sfsn_spike_proj(ctypes.c_void_p(s8.data_ptr() + t0 * R * s8.shape[2]), _ptr(seq.proj_q), _ptr(seq.proj_dq),
                                        _ptr(seq.proj_b), ctypes.c_void_p(y.data_ptr() + t0 * R * seq.P * 4), nt * R, seq.H, seq.P, seq.P,
                                        st), "sfsn_spike_proj(proj)")

    def _stage_projdf(self, seqs, s8s, projs, ri, enh_ri, enh_mag, dims, t0, nt, st, write_proj=True) -> bool:
        """Projection of every group's last-layer spikes + deep filter + pass-through + |.| in one launch (sfsn_proj_deepfilter).
        False (nothing launched): the library does not cover the shapes, the caller issues _stage_proj and sfsn_deepfilter."""
        if not self.fuse_projdf:
            return False
        B, F, T, S = dims
        arr = self._projdf_groups(seqs, s8s, projs, write_proj)
        with self.timed("projdf", st):
            rc = self.lib.sfsn_proj_deepfilter(_ptr(ri), B, F, T, S, seqs[0].H, arr, len(seqs), _ptr(enh_ri), _ptr(enh_mag), t0, nt, st)
        if rc == _lib.SFSN_EUNSUPPORTED:
            return False
        check(rc, "sfsn_proj_deepfilter")
        self._count("projdf")
        return True

    def _zero_states(self, Rs, H, nl, flat=None):
        """(h, c) state pairs of a stack as views of one flat buffer; ``flat`` given = a slice of the forward's state buffer, which the
        forward's first feature launch zeroes (sfsn_features_z) -- otherwise a fill of its own."""
        if flat is None:
            flat = torch.zeros((2 * nl * sum(Rs) * H,), dtype=torch.float32, device=self.device)
        out, pos = [], 0
        for _ in range(nl):
            row = []
            for R in Rs:
                h = flat[pos:pos + R * H].view(R, H)
                c = flat[pos + R * H:pos + 2 * R * H].view(R, H)
                pos += 2 * R * H
                row.append((h, c))
            out.append(row)
        return out

    def _start_buffers(self, n: int, N: int, lead: int, frames_before: int = 0, per_clip_ends: bool = False) -> dict:
        """The start of a forward that continues ``n`` running clips by ``N`` frames (``forward_stft(start["stft"], _end_state=start)``),
        for the caller to fill: ``fb`` / ``sb``: ``[l][i] = (h, c)`` of layer l, sequence model i as the scans take them (fp32 0 / 1
        spikes, membranes; views of ``state_flat``, the forward's state buffer); ``cum``: the running sums per sequence model
        (cumulative_laplace_norm, else None); ``stft``: complex64 [n, F, lead + N], ``lead`` frames of history and the new frames.
        ``per_clip_ends``: the forward will run with ``frames`` -- N is the longest clip's count (``forward_stft``)."""
        spec, dev = self.spec, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        Rs = [n * spec.units(g) for g in range(spec.n_groups)]
        n_fb = 2 * spec.fb_layers * n * self.fb.H
        n_sb = 2 * spec.sb_layers * sum(Rs) * self.sb[0].H
        flat = torch.empty((n_fb + n_sb,), **f32)
        return dict(state_flat=flat, fb=self._zero_states([n], self.fb.H, spec.fb_layers, flat[:n_fb]),
                    sb=self._zero_states(Rs, self.sb[0].H, spec.sb_layers, flat[n_fb:]),
                    cum=[torch.empty((R,), **f32) for R in [n] + Rs] if spec.cum_laplace else None,
                    stft=torch.empty((n, spec.n_fft // 2 + 1, lead + N), dtype=torch.complex64, device=dev),
                    lead=lead, frames_before=frames_before, per_clip_ends=per_clip_ends)

    def _alloc_stack(self, seqs, Rs, T, nt_max, want_layers, want_membrane, tag, state_flat=None, counts=None):
        """Per-forward tensors of a stack of sequence models sharing (H, L): API outputs are fresh, scratch is cached."""
        dev, H, G, nl = self.device, seqs[0].H, seqs[0].cells[0].G, len(seqs[0].cells)
        HP = (H + 63) // 64 * 64
        key = (tag, tuple(Rs), torch.cuda.current_stream(dev).cuda_stream)
        old = self._ws.get(key)
        if old is not None and (old["T"] < T or old["nt"] < nt_max):  # grow: one buffer set per (tag, rows, stream), sized for the
            T_cap, nt_cap = max(T, old["T"]), max(nt_max, old["nt"])  # longest clip seen -- not one set per clip length
            del self._ws[key], old
        else:
            T_cap, nt_cap = T, nt_max
        ws = self._workspace(key, lambda: dict(
            T=T_cap, nt=nt_cap,
            zin=[[torch.empty((nt_cap, R, G * H), dtype=torch.float32, device=dev) for R in Rs] for _ in range(nl)],
            s8=[[torch.zeros((T_cap, R, HP), dtype=torch.int8, device=dev) for R in Rs] for _ in range(nl)]))  # (pad columns stay 0)
        f32 = dict(dtype=torch.float32, device=dev)
        return dict(
            zin=[[z[:nt_max] for z in zl] for zl in ws["zin"]], s8=[[b[:T] for b in bl] for bl in ws["s8"]],
            states=self._zero_states(Rs, H, nl, state_flat),  # zero init, modeling:100-106
            spk=[[torch.empty((T, R, H), **f32) if want_layers else None for R in Rs] for _ in range(nl)],
            mem=[[torch.empty((T, R, H), **f32) if want_membrane else None for R in Rs] for _ in range(nl)],
            proj=[torch.empty((T, R, seq.P), **f32) for seq, R in zip(seqs, Rs)],
            # in-scan spike counters (layer_outputs="counts"): one zeroed int64 per (layer, sequence model), or None
            cnt=None if counts is None else [[counts[l * len(Rs) + i] for i in range(len(Rs))] for l in range(nl)])

    def _feature_groups(self, which: str, xs, mu, sd=None):
        spec = self.spec
        if which == "fb":
            g = FeatureGroup()
            g.x, g.lo, g.n_units, g.ctr, g.nbr, g.ctr_fb, g.nbr_fb = _ptr(xs[0]), 0, 1, spec.fb_in, 0, 0, 0
            g.ln_eps = 1e-5
            if spec.laplace and spec.gaussian:
                g.norm, g.mu, g.ln_w = _lib.NORM_GAUSSIAN, _ptr(mu), _ptr(sd)  # (the clips' standard deviations travel in ln_w)
            elif spec.laplace:
                g.norm, g.mu = _lib.NORM_LAPLACE, _ptr(mu)
            elif spec.ln_fb:
                g.norm, g.ln_w, g.ln_b = _lib.NORM_LAYERNORM, _ptr(self.fb.ln_w), _ptr(self.fb.ln_b)
            else:
                g.norm = _lib.NORM_NONE
            arr = (FeatureGroup * 1)()
            arr[0] = g
            return arr
        arr = (FeatureGroup * spec.n_groups)()
        for i in range(spec.n_groups):
            g = arr[i]
            g.x = _ptr(xs[i]) if xs is not None else None
            g.lo, g.n_units, g.ctr, g.nbr = spec.cutoffs[i], spec.units(i), spec.ctr[i], spec.nbr[i]
            g.ctr_fb, g.nbr_fb, g.ln_eps = spec.ctr_fb[i], spec.nbr_fb[i], 1e-5
            if spec.laplace:
                g.norm = _lib.NORM_GAUSSIAN if spec.gaussian else _lib.NORM_LAPLACE
                g.mu = ctypes.c_void_p(mu.data_ptr() + i * mu.shape[1] * 4) if mu is not None else None
                if spec.gaussian:
                    g.ln_w = ctypes.c_void_p(sd.data_ptr() + i * sd.shape[1] * 4) if sd is not None else None
            elif spec.ln_sb:
                g.norm, g.ln_w, g.ln_b = _lib.NORM_LAYERNORM, _ptr(self.sb[i].ln_w), _ptr(self.sb[i].ln_b)
            else:
                g.norm = _lib.NORM_NONE
        return arr

    _hip = None

    def _masked_stream(self, cus: List[int]) -> torch.cuda.Stream:
        """A HIP stream restricted to the given compute units (hipExtStreamCreateWithCUMask), wrapped for torch.  The
        four recurrent scans of the pipelined schedule each get their own CUs and the time-parallel kernels the rest, so
        that a 2000-block GEMM cannot flood the chip and starve a 52-workgroup scan (or vice versa)."""
        if Engine._hip is None:
            Engine._hip = ctypes.CDLL("libamdhip64.so")
            Engine._hip.hipExtStreamCreateWithCUMask.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
            Engine._hip.hipExtStreamCreateWithCUMask.restype = ctypes.c_int
        words = (self.n_cu + 31) // 32
        mask = (ctypes.c_uint32 * words)()
        for c in cus:
            mask[c // 32] |= (1 << (c % 32))
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            rc = Engine._hip.hipExtStreamCreateWithCUMask(ctypes.byref(h), words, mask)
        if rc != 0 or not h.value:
            raise RuntimeError(f"hipExtStreamCreateWithCUMask failed ({rc})")
        return torch.cuda.ExternalStream(h.value, device=self.device)

    def _pipeline_streams(self, n_fb: int, n_sb: int, fb_tiles: int, sb_tiles: int):
        """(scan streams per stage, G streams per stage): disjoint CU sets, created once per geometry."""
        key = (n_fb, n_sb, fb_tiles, sb_tiles)
        if getattr(self, "_pipe_key", None) != key:
            # CU ids are (32-bit mask word w, bit b) = w*32 + b; measured on MI355X (scripts/exp_cumask.py): a mask word
            # is one XCD, and masks are honoured when every word enables a contiguous bit range.  Pools are therefore bit
            # COLUMNS: the same range of CUs in every XCD -- each pool spans all eight L2s.
            words = self.n_cu // 32
            def columns(b0, b1, w0=0, w1=None):
                return [w * 32 + b for w in range(w0, words if w1 is None else w1) for b in range(b0, b1)]
            pools, col = [], 0
            for tiles in [fb_tiles] * n_fb + [sb_tiles] * n_sb:
                ncol = -(-tiles // words)  # bit columns needed: ceil(tiles / XCDs)
                pools.append(columns(col, col + ncol))
                col += ncol
            if col > 24:
                raise NotImplementedError("pipelined schedule: the scans would leave fewer than a quarter of the CUs to the other kernels")
            g_pool = columns(col, 32)
            self._pipe_scan = [self._masked_stream(p) for p in pools]
            self._pipe_g = [self._masked_stream(g_pool) for _ in pools]  # same CU pool, one queue per stage (a stage's
            # time-parallel kernels wait for its own scan; a shared queue would serialise all four stages)
            self._pipe_key = key
        return self._pipe_scan, self._pipe_g

    def _handle(self, stream: torch.cuda.Stream):
        self._stream_objs[stream.cuda_stream] = stream
        return ctypes.c_void_p(stream.cuda_stream)

    def _count_spikes(self, s8_lists, shapes, st):
        """One launch of sfsn_spike_count over every layer's int8 spike tensor -> list of SpikeSummary."""
        n = len(s8_lists)
        if n > _lib.MAX_COUNT_TENSORS:
            raise NotImplementedError(f"more than {_lib.MAX_COUNT_TENSORS} spike tensors to count")
        counts = torch.zeros((n,), dtype=torch.int64, device=self.device)
        arr = (CountTensor * n)()
        for i, t in enumerate(s8_lists):
            arr[i].spikes_i8, arr[i].n_bytes, arr[i].count = t.data_ptr(), t.numel(), counts.data_ptr() + 8 * i
        with self.timed("spike_count", st):
            check(self.lib.sfsn_spike_count(arr, n, st), "sfsn_spike_count")
        return [SpikeSummary(counts[i], shp) for i, shp in enumerate(shapes)]

    def _count_spikes_ragged(self, s8_lists, shapes, rpcs, frames, frames_dev, st):
        """One launch of sfsn_spike_count_rows_ragged over every layer's int8 spike tensor -> list of ragged.ClipSpikeSummary
        (per-clip counts over each clip's own frames)."""
        from .ragged import ClipSpikeSummary
        n, B = len(s8_lists), len(frames)
        if n > _lib.MAX_COUNT_TENSORS:
            raise NotImplementedError(f"more than {_lib.MAX_COUNT_TENSORS} spike tensors to count")
        counts = torch.zeros((n, B), dtype=torch.int64, device=self.device)
        arr = (RowCount * n)()
        T = s8_lists[0].shape[0]
        for i, t in enumerate(s8_lists):
            arr[i].spikes_i8, arr[i].T, arr[i].R, arr[i].HP, arr[i].rows_per_clip = t.data_ptr(), t.shape[0], t.shape[1], t.shape[2], rpcs[i]
            arr[i].counts = counts.data_ptr() + 8 * i * B
        with self.timed("spike_count", st):
            check(self.lib.sfsn_spike_count_rows_ragged(arr, n, 0, T, _ptr(frames_dev), B, st), "sfsn_spike_count_rows_ragged")
        return [ClipSpikeSummary(counts[i], shp, frames) for i, shp in enumerate(shapes)]

    def forward_stft(self, stft: torch.Tensor, want_layers: bool = True, want_membrane: bool = False, pipeline: Optional[bool] = None,
                     want_counts: bool = False, norm_stats: Optional[NormStats] = None, return_norm_stats: bool = False,
                     frames=None, frames_dev: Optional[torch.Tensor] = None, _end_state=False) -> dict:
        """See ``_forward_stft``; runs with this engine's device current (the C ABI launches on the calling thread's device).

        ``_end_state`` (internal: ``StreamingSession.prime``) -- the result also carries ``"end_state"``, what the forward leaves behind
        its last frame (``_end_state_of``); not with ``frames``.  A START instead of ``True`` (internal: ``StreamingSession.advance``;
        the dict ``_start_buffers`` made, filled by the caller): the forward continues clips that are already running.  ``stft`` is
        then the start's ``[lead + N]``-frame buffer -- ``lead`` frames of history in front of the N new ones -- and the stages run
        on frames ``[lead, lead + N)`` of it from the start's (h, c) per layer and sequence model, its cumulative sums and
        ``frames_before``, so that the deep filter reaches back into real history; the first feature launch does not zero the state
        buffer; the results are those of the N new frames.  Without a start the launches are exactly the same as ever.
        A start made with ``per_clip_ends=True`` (internal: ``StreamingSession.advance_ragged``) runs WITH ``frames``: clip b has
        ``frames[b]`` of the N new frames (``1 <= frames[b] <= N``), the forward runs with the membrane tap whatever
        ``want_membrane`` says, and ``"end_state"`` carries the per-frame membranes (``mem``) from which the caller takes each clip's
        own end (``_end_state_of``); not for the cumulative norm, whose running sums after a clip's own last frame exist nowhere.

        ``frames`` -- a ragged batch (``ragged.py``): a length-B sequence of ints, clip b has ``frames[b]`` frames
        (``1 <= frames[b] <= T``; ``ValueError`` otherwise) and the rest of its row is padding.  The launches of the model are the
        same; the offline norms' statistics run over each clip's own frames, ``want_counts`` gives per-clip counts over each clip's
        own frames (``ragged.ClipSpikeSummary``) and ``enh_stft`` / ``enh_mag`` are zero at frames ``>= frames[b]``.  The lengths go to
        the device once, without a host synchronisation (``frames_dev``: they are there already, as int32 [B]).

        Frozen front-end with an offline norm only (``ValueError`` otherwise): ``norm_stats`` -- the clips' statistics are taken as
        given instead of being computed from ``stft`` (the two statistics launches are skipped, the schedule is otherwise the same);
        ``return_norm_stats=True`` -- the result also carries ``"norm_stats"``, the statistics this forward used, as clones."""
        if norm_stats is not None:
            norm_stats.validate(self.spec, stft.shape[0] if stft.dim() == 3 else -1, self.device)
        elif return_norm_stats and not self.spec.laplace:
            raise ValueError("return_norm_stats: this model computes no utterance statistics")
        if frames is not None:
            from . import ragged
            per_clip = isinstance(_end_state, dict) and bool(_end_state.get("per_clip_ends"))
            if _end_state and not per_clip:
                raise ValueError("_end_state: not with a ragged batch (the clips end at different frames)")
            if per_clip and self.spec.cum_laplace:
                raise NotImplementedError("_end_state with per-clip ends: not with cumulative_laplace_norm (no running sums after a "
                                          "clip's own last frame)")
            lead = int(_end_state["lead"]) if per_clip else 0
            frames = ragged.check_frames(frames, stft.shape[0] if stft.dim() == 3 else -1, stft.shape[-1] - lead,
                                         gaussian=self.spec.gaussian and norm_stats is None)
            if per_clip:  # (lengths within the [history | new] rows from here on; the membrane tap: every frame's c is kept)
                frames, frames_dev, want_membrane = [lead + n for n in frames], None, True
        elif isinstance(_end_state, dict) and _end_state.get("per_clip_ends"):
            raise ValueError("_end_state: a start with per-clip ends needs frames")
        with torch.cuda.device(self.device):
            self._errors.poll()
            if frames is not None and frames_dev is None:
                frames_dev = ragged.upload(frames, self.device)
            out = self._forward_stft(stft, want_layers, want_membrane, pipeline, want_counts, norm_stats, frames, frames_dev, _end_state)
            if return_norm_stats:
                out["norm_stats"] = NormStats(out["mu_fb"][0], out["mu_sb"], None if out["sd_fb"] is None else out["sd_fb"][0],
                                              out["sd_sb"]).clone()
            if not torch.cuda.is_current_stream_capturing():
                cur = torch.cuda.current_stream(self.device)
                ev = self._last_forward.get(cur.cuda_stream)
                if ev is None:
                    ev = self._last_forward[cur.cuda_stream] = torch.cuda.Event()
                ev.record(cur)  # (what _stack_choice asks: is another stream's forward still running?)
            if self.strict_errors:
                # results are only handed out once every stack launch of THIS forward is known to have completed its hand-offs
                # (one stream synchronisation per forward: for callers that keep several forwards in flight leave it off and
                # call check_stack_errors() at their own synchronisation points)
                self._errors.poll(block=True)
            return out

    def _forward_stft(self, stft: torch.Tensor, want_layers: bool = True, want_membrane: bool = False, pipeline: Optional[bool] = None,
                      want_counts: bool = False, norm_stats: Optional[NormStats] = None, frames=None, frames_dev=None,
                      end_state=False) -> dict:
        """complex64 [B, n_fft/2+1, T] on the device -> dict(enh_stft [B,S,F,T] complex64, enh_mag [B,S,F,T],
        fb_all, sb_all (the reference's all_layer_outputs lists; spike entries are None when want_layers=False)).

        Schedule (plan_forward).  The four recurrent scans of a model (full-band layer 1/2, sub-band layer 1/2) are each a chain of T
        dependent steps that occupies only a fraction of the chip, and layer l+1 / the sub-band model need frame t of
        their producer only at frame t.  With ``pipeline`` (default: live front-end and T >= 2 chunks) the sequence is
        cut into chunks of ``pipeline_chunk`` frames and the stages run as a software pipeline on separate HIP streams
        chained by events -- stage s works on chunk c while stage s+1 works on chunk c-1 -- with the scan state carried in
        the ABI's h_state / c_state buffers.  Results are bit-identical to the sequential schedule (same kernels, same
        arithmetic; tested).  The frozen front-end's utterance-level Laplace mean needs the whole full-band output, so
        only its two layer pairs overlap.
        """
        spec = self.spec
        self._defer_err = None  # (a forward that raised half way must not leave the next one's error words uncollected)
        want_layers = want_layers or want_membrane  # membranes are a test output of the fp32-spike kernel variant
        B, F, T = self._validate(stft)
        start = end_state if isinstance(end_state, dict) else None
        lead = 0 if start is None else int(start["lead"])
        if start is not None and (stft.data_ptr() != start["stft"].data_ptr() or tuple(stft.shape) != tuple(start["stft"].shape) or T <= lead):
            raise ValueError("_end_state: a start runs on its own [history | new] buffer (Engine._start_buffers)")
        plan = self._plan(B, T - lead, pipeline, want_membrane)
        if lead:  # the chunks of the N new frames, behind the history
            plan = plan._replace(bounds=tuple((t0 + lead, nt) for t0, nt in plan.bounds))
        f = self._alloc_forward(stft, plan, want_layers, want_membrane, want_counts, norm_stats, frames, frames_dev, start)
        if start is not None and frames is not None and self._l0_hop is None:
            f.l0_alone = self._l0_alone_rows(f)
        self._open_streams(f)
        fbm, sbm, gs_sb = f.fbm, f.sbm, f.gstreams[spec.fb_layers]
        if spec.laplace and norm_stats is None:
            if start is not None:
                raise ValueError("_end_state: a start of a model with an offline norm needs norm_stats (the clips' statistics so far)")
            self._stats(f, fbm)
        fb_done = self._run_model(f, fbm, None)
        if spec.laplace:
            # the utterance-level Laplace mean of the sub-band input needs the whole full-band output: no chunk overlap fb -> sb
            if plan.pipeline:
                gs_sb.wait_event(fb_done[-1])
            if norm_stats is None:
                self._stats(f, sbm)
            self._run_model(f, sbm, None)
        elif plan.pipeline and self.pipeline_two_phase:
            # full-band model first (its two layers overlapped), then the sub-band models (their two layers overlapped)
            gs_sb.wait_event(fb_done[-1])
            self._run_model(f, sbm, None)
        else:
            self._run_model(f, sbm, fb_done if plan.staged else None)
        self._join(f)
        if frames is not None:
            self._zero_tail(f)
        if want_counts and not want_layers and start is None:  # (a start's caller takes the per-clip counts of the end state)
            self._summaries(f)
        out = self._result(f)
        if end_state:
            out["end_state"] = self._end_state_of(f, want_counts)
        return out

    def _plan(self, B: int, T: int, pipeline: Optional[bool], want_membrane: bool) -> ForwardPlan:
        """``plan_forward`` with this engine's attributes."""
        return plan_forward(self.spec, B, T, pipeline, self.n_cu, want_membrane, pipeline_default=self.pipeline_default,
                            pipeline_chunk=self.pipeline_chunk, seq_chunk=self.seq_chunk, overlap_chunks=self.overlap_chunks,
                            overlap_fracs=self.overlap_fracs, overlap_first=self.overlap_first, rows_per_wg=self.rows_per_wg,
                            fuse_input=self.fuse_input, stack_scan=self.stack_scan, stack_rows_per_wg=self.stack_rows_per_wg,
                            stack_wide=self.stack_wide, stack_rows_fb_auto=self.stack_rows_fb_auto, pair_scan=self.pair_scan)

    def _l0_alone_rows(self, f: _Forward) -> dict:
        """A ragged batch behind a start promises each clip the bits of ITS OWN forward (``StreamingSession.advance_ragged``: the
        single-clip ``advance`` call).  One arithmetic of the forward depends on how many rows a launch has: the layer-0 input product
        takes its bf16-split form from 64 row-frames per chunk on and the fp32 form below (include/sfsn.h, sfsn_input_proj_f32; every
        schedule keeps to that rule: _stack_x_groups, sfsn_features_proj).  The batch has more row-frames than any clip alone, so
        where a clip's own forward -- ``_plan(1, N_b)``'s chunks, ``units`` rows per frame -- stays below 64 the batch's product
        is redone for those rows in the fp32 form (``_l0_as_alone``).  Returns the rows per model and sequence model."""
        lead = f.lead
        alone = [self._plan(1, end - lead, None, False).bounds for end in f.frames]  # the chunks of each clip's own forward
        out = {}
        for m in (f.fbm, f.sbm):
            per_seq = []
            for i, x in enumerate(m.xs):
                R = x.shape[1]
                u = R // len(f.frames)
                rows = []
                for b, bounds in enumerate(alone):
                    for t0, nt in bounds:
                        if nt * u < 64:
                            rows.append(((lead + np.arange(t0, t0 + nt))[:, None] * R + (b * u + np.arange(u))[None, :]).ravel())
                if rows:
                    per_seq.append((i, np.sort(np.concatenate(rows))))
            out[m.tag] = per_seq
        return out

    def _l0_as_alone(self, f: _Forward, m: _ModelRun, t0: int, nt: int, stream, st) -> None:
        """Behind a chunk's layer-0 input product: the rows of ``f.l0_alone`` inside the chunk again, in calls below 64 rows (the fp32
        form; a row's result depends on nothing but the row), into the chunk-local input term."""
        for i, rows in f.l0_alone.get(m.tag, ()):
            x, z, seq = m.xs[i], m.d["zin"][0][i], m.seqs[i]
            R, I, cell = x.shape[1], seq.I, seq.cells[0]
            mine = rows[(rows >= t0 * R) & (rows < (t0 + nt) * R)]
            if not len(mine):
                continue
            G, H = cell.G, seq.H
            P = ctypes.c_void_p
            with torch.cuda.stream(stream):
                idx = torch.from_numpy(mine.astype(np.int64)).pin_memory().to(self.device, non_blocking=True)
                xr = x.view(-1, I).index_select(0, idx)
                zr = torch.empty((len(mine), G * H), dtype=torch.float32, device=self.device)
                for r0 in range(0, len(mine), 63):
                    for g in range(G):
                        check(self.lib.sfsn_input_proj_f32(P(xr.data_ptr() + r0 * I * 4), P(cell.w_ih_f32.data_ptr() + g * H * I * 4),
                                                           P(cell.bias.data_ptr() + g * H * 4), P(zr.data_ptr() + (r0 * G + g) * H * 4),
                                                           min(63, len(mine) - r0), I, H, G * H, st), "sfsn_input_proj_f32")
                z.view(-1, G * H).index_copy_(0, idx - t0 * R, zr)

    def _end_state_of(self, f: _Forward, want_counts: bool) -> dict:
        """What a forward leaves behind its last frame, for a streaming session that goes on from there (``StreamingSession.prime``):
        ``fb`` / ``sb``: ``states[l][i] = (h, c)`` of layer l, sequence model i after the last frame (the ABI's h_state / c_state) and
        ``s8[l][i]`` the int8 spikes of every frame [T, R, pad64(H)] (row T - 1: the last frame's); ``cum``: the running sums of
        cumulative_laplace_norm per sequence model (full-band first), else None; ``counts``: with ``want_counts`` the spikes per
        (layer, clip), int64 [fb layers + groups x sb layers, B] in ``spike_summary``'s order, else None.  The states and the spikes
        are the forward's own buffers, in stream order: the spikes are valid until the next forward on this stream.
        A start with per-clip ends (a ragged batch behind a start): ``states`` are those after the last PADDED frame and of no use;
        ``fb`` / ``sb`` also carry ``mem[l][i]``, the new frames' post-BatchNorm membranes [N, R, H] (row ``frames[b] - 1``: what c_state
        would be had the scan stopped at clip b's own last frame), ``counts`` run over each clip's own frames and ``frames_dev`` holds
        the clips' counts of NEW frames, int32 on the device."""
        spec, fb, sb = self.spec, f.fbm.d, f.sbm.d
        ng, nl_fb, nl_sb = spec.n_groups, spec.fb_layers, spec.sb_layers
        counts = None
        if want_counts:
            T, B = f.fbm.xs[0].shape[:2]
            t0 = f.lead  # (a forward with a start: the new frames only)
            tens = [(fb["s8"][l][0], 1) for l in range(nl_fb)] + [(sb["s8"][l][g], spec.units(g)) for g in range(ng) for l in range(nl_sb)]
            counts = torch.zeros((len(tens), B), dtype=torch.int64, device=self.device)
            hm = self._handle(f.main)
            for i0 in range(0, len(tens), _lib.MAX_COUNT_TENSORS):
                part = tens[i0:i0 + _lib.MAX_COUNT_TENSORS]
                arr = (RowCount * len(part))()
                for j, (t, rpc) in enumerate(part):
                    arr[j].spikes_i8, arr[j].T, arr[j].R, arr[j].HP, arr[j].rows_per_clip = t.data_ptr(), t.shape[0], t.shape[1], t.shape[2], rpc
                    arr[j].counts = counts.data_ptr() + 8 * (i0 + j) * B
                if f.frames is not None:  # (per-clip ends: frames_dev counts from the row's first frame, history included)
                    check(self.lib.sfsn_spike_count_rows_ragged(arr, len(part), t0, T - t0, _ptr(f.frames_dev), B, hm), "sfsn_spike_count_rows_ragged")
                else:
                    check(self.lib.sfsn_spike_count_rows(arr, len(part), t0, T - t0, hm), "sfsn_spike_count_rows")

        def s8(d):  # (a forward with a start: the new frames' rows)
            return [[t[f.lead:] for t in row] for row in d["s8"]] if f.lead else d["s8"]
        es = dict(fb=dict(states=fb["states"], s8=s8(fb)), sb=dict(states=sb["states"], s8=s8(sb)),
                  cum=None if f.cum is None else f.cum["state"], counts=counts)
        if f.frames is not None:
            for d, e in ((fb, es["fb"]), (sb, es["sb"])):
                e["mem"] = [[t[f.lead:] for t in row] for row in d["mem"]]
            es["frames_dev"] = f.frames_dev - f.lead
        return es

    def _validate(self, stft):
        """(B, F, T) of a forward's input, or the error that says what is wrong with it."""
        spec = self.spec
        if stft.device != self.device or stft.dtype != torch.complex64 or stft.dim() != 3:
            raise RuntimeError(f"expected a complex64 [B, F, T] tensor on {self.device}, got {stft.dtype} {tuple(stft.shape)} on {stft.device}")
        B, F, T = stft.shape
        if F != spec.n_fft // 2 + 1:
            raise ValueError(f"expected {spec.n_fft // 2 + 1} frequency bins, got {F}")
        for g in range(spec.n_groups):  # the reference's ValueError, modeling_spiking_fullsubnet.py:283-287
            lo, hi, c = spec.cutoffs[g], spec.cutoffs[g + 1], spec.ctr[g]
            if (hi - lo) % c != 0:
                raise ValueError(f"Number of frequency bins must be divisible by the center frequency.GOT: ctr_freq={c}, "
                                 f"upper_cutoff_freq={hi}, lower_cutoff_freq={lo}")
        return B, F, T

    def _alloc_forward(self, stft, plan, want_layers, want_membrane, want_counts, norm_stats, frames, frames_dev, start=None) -> _Forward:
        """Every tensor of one forward (API outputs fresh, scratch cached: _alloc_stack) and the two models' launch arguments."""
        spec, dev = self.spec, self.device
        B, F, T = stft.shape
        S, ng, nl_fb, nl_sb = spec.num_spks, spec.n_groups, spec.fb_layers, spec.sb_layers
        f32 = dict(dtype=torch.float32, device=dev)
        ri = torch.view_as_real(stft.contiguous())  # [B, F, T, 2] float32 view, no copy
        if start is not None:
            assert stft.is_contiguous()
        x_fb = torch.empty((T, B, spec.fb_in), **f32)
        xs = [torch.empty((T, B * spec.units(g), spec.sb_input_size(g)), **f32) for g in range(ng)]
        # the zero initial state of every scan of the forward: ONE buffer, zeroed by the forward's first feature launch (every scan
        # depends on that launch through its input) -- no fill launch on the forward's chain
        n_fb = 2 * nl_fb * B * self.fb.H
        n_sb = 2 * nl_sb * sum(x.shape[1] for x in xs) * self.sb[0].H
        fold = os.environ.get("SFSN_ZERO_FOLD", "1") != "0"  # (0: a fill launch of its own, for comparison)
        # layer_outputs="counts": the scans count the spikes they write (sfsn_scan_segment.spike_count) -- the int64 counters sit behind
        # the states in the same zeroed buffer (two floats each; the buffer's length stays a multiple of 16 bytes)
        # (a ragged batch counts each clip's own frames after the forward: the in-scan counter is per tensor, not per clip)
        in_scan = bool(want_counts and not want_layers and self.count_in_scan and frames is None and start is None)
        n_cnt = (nl_fb + ng * nl_sb) if in_scan else 0
        n_cnt_f = (2 * n_cnt + 3) // 4 * 4
        if start is not None:  # the scans go on from the caller's states: nothing zeroes them
            state_flat, fold = start["state_flat"], False
            assert state_flat.numel() == n_fb + n_sb and state_flat.dtype == torch.float32 and state_flat.device == dev
        else:
            state_flat = torch.empty((n_fb + n_sb + n_cnt_f,), **f32) if fold else torch.zeros((n_fb + n_sb + n_cnt_f,), **f32)
        cnt_all = state_flat[n_fb + n_sb:n_fb + n_sb + 2 * n_cnt].view(torch.int64) if in_scan else None
        fb = self._alloc_stack([self.fb], [B], T, plan.nt_max, want_layers, want_membrane, "fb", state_flat[:n_fb],
                               None if cnt_all is None else cnt_all[:nl_fb])
        sb = self._alloc_stack(self.sb, [x.shape[1] for x in xs], T, plan.nt_max, want_layers, want_membrane, "sb",
                               state_flat[n_fb:n_fb + n_sb], None if cnt_all is None else cnt_all[nl_fb:])
        enh = torch.empty((B, S, F, T), dtype=torch.complex64, device=dev)
        dfg = (DfGroup * ng)()
        for g in range(ng):
            dfg[g].proj, dfg[g].n_units, dfg[g].fc, dfg[g].df = _ptr(sb["proj"][g]), spec.units(g), spec.ctr[g], spec.df[g]
        mu_fb = mu_sb = sd_fb = sd_sb = scratch = None
        if norm_stats is not None:  # (validated by forward_stft) the clips' statistics as given: no statistics launches
            mu_fb, mu_sb = norm_stats.mu_fb.contiguous().view(1, B), norm_stats.mu_sb.contiguous()
            if spec.gaussian:
                sd_fb, sd_sb = norm_stats.sd_fb.contiguous().view(1, B), norm_stats.sd_sb.contiguous()
        elif spec.laplace:
            mu_fb, mu_sb = torch.empty((1, B), **f32), torch.empty((ng, B), **f32)
            if spec.gaussian:
                sd_fb, sd_sb = torch.empty((1, B), **f32), torch.empty((ng, B), **f32)
            scratch = torch.empty(((5 if spec.gaussian else 1) * B * (F - 1 + spec.fb_proj) + 2,), **f32)
        cum = None
        if spec.cum_laplace:
            # cumulative_laplace_norm: the rows leave sfsn_features unnormalised and are divided by their running means (state per
            # row, so a sequence fed in pieces continues where it stopped)
            rows = [B] + [x.shape[1] for x in xs]
            cum = dict(state=[torch.zeros((R,), **f32) for R in rows] if start is None else start["cum"],
                       scratch=torch.empty((plan.nt_max * max(rows),), **f32))
        fb_proj = fb["proj"][0]
        fbm = _ModelRun("fb", [self.fb], fb, [x_fb], 0, plan.rpw_fb, self._feature_groups("fb", [x_fb], mu_fb, sd_fb), None,
                        (B, F, T, 0, spec.fdrc), mu_fb, sd_fb, 0)
        sbm = _ModelRun("sb", self.sb, sb, xs, nl_fb, plan.rpw_sb, self._feature_groups("sb", xs, mu_sb, sd_sb), fb_proj,
                        (B, F, T, spec.fb_proj, spec.fdrc), mu_sb, sd_sb, 1)
        return _Forward(plan=plan, ri=ri, want_layers=want_layers, want_membrane=want_membrane, frames=frames, frames_dev=frames_dev,
                        fbm=fbm, sbm=sbm, enh=enh, enh_ri=torch.view_as_real(enh), enh_mag=torch.empty((B, S, F, T), **f32), dfg=dfg,
                        stats_scratch=scratch, cum=cum, zero=state_flat if fold else None, in_scan=in_scan,
                        # round 6: projection + deep filter of a chunk in one launch; in the lean modes the coefficient rows are not written
                        write_proj=bool(want_layers or want_membrane or not self.lean_skips_proj),
                        lead=0 if start is None else int(start["lead"]), frames_before=0 if start is None else int(start["frames_before"]))

    def _open_streams(self, f: _Forward) -> None:
        """The streams of the forward's stages: sequential = the current stream; pipelined = per stage one scan stream (own CUs) and one
        stream for its time-parallel kernels (shared CU pool), chained by events; overlapped = one stream per model."""
        spec, plan, dev = self.spec, f.plan, self.device
        nl_fb, nl_sb = spec.fb_layers, spec.sb_layers
        main = f.main = torch.cuda.current_stream(dev)
        if plan.pipeline:
            fb_tiles = (f.fbm.xs[0].shape[1] + plan.rpw_fb - 1) // plan.rpw_fb
            sb_tiles = sum((x.shape[1] + plan.rpw_sb - 1) // plan.rpw_sb for x in f.sbm.xs)
            f.sstreams, f.gstreams = self._pipeline_streams(nl_fb, nl_sb, fb_tiles, sb_tiles)
            forked = f.sstreams + f.gstreams
        elif plan.overlap:
            if self._ov_streams is None:
                self._ov_streams = {}
            if main.cuda_stream not in self._ov_streams:  # a pair per calling stream: forwards in flight stay independent
                self._ov_streams[main.cuda_stream] = (torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev))
            sa, sb_ = forked = self._ov_streams[main.cuda_stream]
            self._defer_err = []
            f.sstreams = f.gstreams = [sa] * nl_fb + [sb_] * nl_sb
        else:
            f.sstreams = f.gstreams = [main] * (nl_fb + nl_sb)
            forked = ()
        if forked:
            fork = torch.cuda.Event()
            fork.record(main)
            for s_ in forked:
                s_.wait_event(fork)
        f.hS = [self._handle(s_) for s_ in f.sstreams]
        f.hG = [self._handle(s_) for s_ in f.gstreams]

    def _stats(self, f: _Forward, m: _ModelRun) -> None:
        """The clips' utterance statistics of one model's input; a ragged batch: over each clip's own frames."""
        spec, L = self.spec, self.lib
        B, F, T, FB, fdrc = m.dims
        ri, fb_tbf, n, mu, sd, scratch = _ptr(f.ri), _ptr(m.fb_proj), len(m.seqs), _ptr(m.mu), _ptr(m.sd), _ptr(f.stats_scratch)
        st, tag = f.hG[m.first], m.tag
        if f.frames is not None:
            fd = _ptr(f.frames_dev)
            if spec.gaussian:
                check(L.sfsn_gaussian_stats_ragged(ri, fb_tbf, B, F, T, FB, fdrc, m.fg, n, fd, mu, sd, scratch, st), f"sfsn_gaussian_stats_ragged({tag})")
            else:
                check(L.sfsn_laplace_means_ragged(ri, fb_tbf, B, F, T, FB, fdrc, m.fg, n, fd, mu, scratch, st), f"sfsn_laplace_means_ragged({tag})")
        elif spec.gaussian:
            check(L.sfsn_gaussian_stats(ri, fb_tbf, B, F, T, FB, fdrc, m.fg, n, mu, sd, scratch, st), f"sfsn_gaussian_stats({tag})")
        else:
            check(L.sfsn_laplace_means(ri, fb_tbf, B, F, T, FB, fdrc, m.fg, n, mu, scratch, st), f"sfsn_laplace_means({tag})")

    def _features(self, f: _Forward, m: _ModelRun, t0, nt, st, proj) -> bool:
        """The feature rows of one model's chunk.  `proj` = (groups, their chunk-local input-term buffers): True when one launch made
        the rows AND those groups' layer-0 input terms (_stage_featproj), False when the caller still owes the input terms."""
        L = self.lib
        B, F, T, FB, fdrc = m.dims
        z = None
        if m.tag == "fb":
            z, f.zero = f.zero, None  # (the first full-band feature launch of the forward carries the state zeroing)
        if f.cum is None and self._l0_hop is None and self._stage_featproj(m.fg, m.seqs, proj[0], proj[1], f.ri, m.fb_proj, m.dims, t0, nt, z, f.want_layers, st, m.tag):
            if not f.want_layers:  # feature rows a fused launch did not write (layer_outputs "counts" / "none": nobody reads them)
                f.x_skipped[m.tag].update(proj[0])
            return True
        with self.timed("features:" + m.tag, st):
            if m.tag == "fb":
                check(L.sfsn_features_z(_ptr(f.ri), None, B, F, T, 0, fdrc, m.fg, 1, t0, nt, None if z is None else _ptr(z),
                                        0 if z is None else z.numel() * 4, st), "sfsn_features(fb)")
            else:
                check(L.sfsn_features(_ptr(f.ri), _ptr(m.fb_proj), B, F, T, FB, fdrc, m.fg, len(m.seqs), t0, nt, st), "sfsn_features(sb)")
            if f.cum is not None:
                for i, x in enumerate(m.xs):
                    R, I = x.shape[1], x.shape[2]
                    check(L.sfsn_cum_laplace_norm(ctypes.c_void_p(x.data_ptr() + t0 * R * I * 4), nt, R, I, _ptr(f.cum["state"][m.cum0 + i]),
                                                  t0 - f.lead + f.frames_before,
                                                  _ptr(f.cum["scratch"]), st), "sfsn_cum_laplace_norm")
        return False

    def _epilogue(self, f: _Forward, m: _ModelRun, t0, nt, st) -> None:
        """What follows a model's last layer on a chunk: its projection and, behind the sub-band models, the deep filter -- the two in
        one launch where the library covers the shapes (the two-launch epilogue reads the same tensors)."""
        if m.tag == "sb":
            B, F, T = m.dims[:3]
            S = self.spec.num_spks
            if f.epi_chunk == (t0, nt):  # (the chunk's scan launch carried it: _stage_scan_l01)
                f.epi_chunk = None
                f.proj_skipped = not f.write_proj
                return
            if self._stage_projdf(m.seqs, m.d["s8"][-1], m.d["proj"], f.ri, f.enh_ri, f.enh_mag, (B, F, T, S), t0, nt, st, f.write_proj):
                f.proj_skipped = not f.write_proj
                return
        self._stage_proj(m.seqs, m.d["s8"][-1], m.d["proj"], t0, nt, st, m.tag)
        if m.tag == "sb":
            with self.timed("deepfilter", st):
                check(self.lib.sfsn_deepfilter(_ptr(f.ri), B, F, T, S, f.dfg, len(m.seqs), _ptr(f.enh_ri), _ptr(f.enh_mag), t0, nt, st),
                      "sfsn_deepfilter")

    def _run_model(self, f: _Forward, m: _ModelRun, gate_events) -> list:
        """One model over every chunk of the forward.  gate_events: per chunk, what its first launch waits for (the full-band model's
        chunk, on the staged schedules).  Returns the per-chunk completion events (staged schedules; else empty)."""
        use_stack, wide, rpw_stack = self._stack_choice(m.seqs, [x.shape[1] for x in m.xs], f.want_membrane)
        if not f.plan.pipeline and use_stack and self._l0_hop is None:
            return self._run_model_stack(f, m, gate_events, wide, rpw_stack)
        return self._run_model_layers(f, m, gate_events)

    def _run_model_stack(self, f, m, gate_events, wide, rpw_stack) -> list:
        """All layers in one launch per chunk: features, layer 0's input term, the stack scan, the epilogue."""
        seqs, d, xs_, tag, staged = m.seqs, m.d, m.xs, m.tag, f.plan.staged
        g, hg, done = f.gstreams[m.first], f.hG[m.first], []
        for c, (t0, nt) in enumerate(f.plan.bounds):
            if staged and gate_events is not None:
                g.wait_event(gate_events[c])
            xg = self._stack_x_groups(seqs, xs_, nt, wide, rpw_stack or self.stack_rows_per_wg[tag], f.want_membrane)
            zr = [i for i in range(len(seqs)) if i not in xg]
            if not self._features(f, m, t0, nt, hg, (zr, _pick(d["zin"][0], zr))) and zr:
                self._stage_input(_pick(seqs, zr), 0, _pick(xs_, zr), _pick(d["zin"][0], zr), t0, nt, hg, tag)
            self._stage_stack(seqs, d, t0, nt, f.hS[m.first], tag, wide, rpw_stack, xs_=xs_, xg=xg)
            self._epilogue(f, m, t0, nt, hg)
            if staged:
                done.append(_record(g))
        return done

    def _run_model_layers(self, f, m, gate_events) -> list:
        """A launch per layer (and its input product, where the scan does not form it itself) per chunk."""
        seqs, d, xs_, tag, rpw, staged = m.seqs, m.d, m.xs, m.tag, m.rpw, f.plan.staged
        nl = len(seqs[0].cells)
        fused = self._fusable(seqs, rpw, f.want_membrane)
        done = []
        # layer 0: groups whose real-valued input product can run inside the scan / the rest (input product first)
        fx = [i for i in range(len(seqs)) if self._l0_hop is None and self._fusable_x(seqs[i], xs_[i], rpw, f.want_membrane)]
        rest = [i for i in range(len(seqs)) if i not in fx]
        # layers 0 and 1 of a two-layer stack at 16 rows in one launch (the staged schedules and graph capture keep the per-layer launches)
        pair = bool(self.pair16 and self.merge_layer0 and nl == 2 and rpw == 16 and fused and not staged
                    and not torch.cuda.is_current_stream_capturing() and self._l0_hop is None)
        for c, (t0, nt) in enumerate(f.plan.bounds):
            paired = False
            for l in range(nl):
                si = m.first + l
                g, sc = f.gstreams[si], f.sstreams[si]
                # ---- what the scan of this layer consumes
                if l == 0:
                    if staged and gate_events is not None:
                        g.wait_event(gate_events[c])
                    if not self._features(f, m, t0, nt, f.hG[si], (rest, _pick(d["zin"][0], rest))) and rest:
                        self._stage_input(_pick(seqs, rest), 0, _pick(xs_, rest), _pick(d["zin"][0], rest), t0, nt, f.hG[si], tag)
                    if f.l0_alone:
                        self._l0_as_alone(f, m, t0, nt, g, f.hG[si])
                else:
                    f.link(f.sstreams[si - 1], g)  # previous layer's scan of this chunk
                    if not fused:
                        self._stage_input(seqs, l, d["s8"][l - 1], d["zin"][l], t0, nt, f.hG[si], tag)
                f.link(g, sc)
                # ---- the scan(s)
                if l == 0:
                    paired = self._scan_layer0(m, fx, rest, pair, t0, nt, f.hS[si], f)
                elif l == 1 and paired:
                    pass  # (layer 1 of this chunk ran in layer 0's launch)
                elif fused:
                    self._stage_scan_fused(seqs, l, d["states"][l], d["spk"][l], d["s8"], t0, nt, f.hS[si], tag,
                                           cnts=None if d["cnt"] is None else d["cnt"][l])
                else:
                    self._stage_scan(seqs, l, d["zin"][l], d["states"][l], d["spk"][l], d["s8"][l], d["mem"][l], t0, nt, f.hS[si], tag, rpw,
                                     cnts=None if d["cnt"] is None else d["cnt"][l])
                if staged:
                    f.link(sc, g)  # the chunk-local zin buffer is reused by the next chunk's input product
                # ---- after the last layer: projection and whatever follows the model
                if l == nl - 1:
                    self._epilogue(f, m, t0, nt, f.hG[si])
                    if staged:
                        done.append(_record(g))
        return done

    def _scan_layer0(self, m: _ModelRun, fx, rest, pair, t0, nt, st, f=None) -> bool:
        """Layer 0 of a model on one chunk, in as few launches as the library takes: with layer 1 (True: layer 1 ran too), both kinds of
        group in one launch, or the fused-x groups and the rest one after the other."""
        seqs, d, xs_, tag = m.seqs, m.d, m.xs, m.tag
        cn = d["cnt"]
        cn0 = None if cn is None else cn[0]
        # (the chunk's epilogue inside the pair launch: only where _epilogue would take the one-launch epilogue)
        epi = (f, m) if (pair and f is not None and self.pair16_epilogue and self.fuse_projdf and tag == "sb") else None
        if pair and self._stage_scan_l01(seqs, fx, rest, xs_, d, t0, nt, st, tag, cn=cn, epi=epi):
            return True
        if fx and rest and m.rpw == 16 and self.merge_layer0 and self._stage_scan_l0(
                seqs, fx, rest, xs_, d["zin"][0], d["states"][0], d["spk"][0], d["s8"][0], t0, nt, st, tag, cnts=cn0):
            return False  # (both kinds of group in one launch)
        if fx:
            self._stage_scan_fused_x(_pick(seqs, fx), _pick(xs_, fx), _pick(d["states"][0], fx), _pick(d["spk"][0], fx),
                                     _pick(d["s8"][0], fx), t0, nt, st, tag, cnts=None if cn is None else _pick(cn0, fx))
        if rest:
            self._stage_scan(_pick(seqs, rest), 0, _pick(d["zin"][0], rest), _pick(d["states"][0], rest), _pick(d["spk"][0], rest),
                             _pick(d["s8"][0], rest), _pick(d["mem"][0], rest), t0, nt, st, tag, m.rpw,
                             cnts=None if cn is None else _pick(cn0, rest))
        return False

    def _join(self, f: _Forward) -> None:
        """The calling stream waits for every stream of the forward; the forward's deferred error words are collected behind it."""
        if f.plan.staged:
            for s_ in {id(x): x for x in f.sstreams + f.gstreams}.values():
                f.link(s_, f.main)
        if self._defer_err:
            # the error words of this forward's stack launches: one maximum, one copy to pinned memory, on a stream of its own behind
            # the joined forward (nothing of the forward waits for it)
            items, self._defer_err = self._defer_err, None
            self._errors.watch(None, list({id(sc): sc for _, sc in items}.values()), "; ".join(sorted({w for w, _ in items})))
        self._defer_err = None

    def _zero_tail(self, f: _Forward) -> None:
        """A ragged batch: the deep filter has written every frame of the padded batch; what lies past a clip's end is zeroed (2 launches)."""
        B, S, F, T = f.enh_mag.shape
        hm = self._handle(f.main)
        with self.timed("zero_tail", hm):
            check(self.lib.sfsn_zero_tail_frames(_ptr(f.enh_ri), B, S * F, T, 2, _ptr(f.frames_dev), hm), "sfsn_zero_tail_frames(enh_stft)")
            check(self.lib.sfsn_zero_tail_frames(_ptr(f.enh_mag), B, S * F, T, 1, _ptr(f.frames_dev), hm), "sfsn_zero_tail_frames(enh_mag)")

    def _summaries(self, f: _Forward) -> None:
        """layer_outputs="counts": a SpikeSummary in the place of every spike tensor.  SynOPs without the fp32 spike tensors (SURVEY 8f
        rank 1): the scans have counted what they wrote (no launch, no pass over the int8 copies); `count_in_scan = False`: round 3's
        counting launch over the int8 spikes, one launch for all layers; a ragged batch: per clip, over each clip's own frames."""
        spec, fb, sb, xs = self.spec, f.fbm.d, f.sbm.d, f.sbm.xs
        ng, nl_fb, nl_sb = spec.n_groups, spec.fb_layers, spec.sb_layers
        T, B = f.fbm.xs[0].shape[:2]
        tens = [fb["s8"][l][0] for l in range(nl_fb)] + [sb["s8"][l][g] for g in range(ng) for l in range(nl_sb)]
        shapes = [(T, B, self.fb.H)] * nl_fb + [(T, xs[g].shape[1], self.sb[g].H) for g in range(ng) for _ in range(nl_sb)]
        if f.in_scan:
            summ = [SpikeSummary(fb["cnt"][l][0], shapes[l]) for l in range(nl_fb)] + \
                   [SpikeSummary(sb["cnt"][l][g], shapes[nl_fb + g * nl_sb + l]) for g in range(ng) for l in range(nl_sb)]
        elif f.frames is not None:
            rpcs = [1] * nl_fb + [spec.units(g) for g in range(ng) for _ in range(nl_sb)]
            summ = self._count_spikes_ragged(tens, shapes, rpcs, f.frames, f.frames_dev, self._handle(f.main))
        else:
            summ = self._count_spikes(tens, shapes, self._handle(f.main))
        for l in range(nl_fb):
            fb["spk"][l][0] = summ[l]
        for g in range(ng):
            for l in range(nl_sb):
                sb["spk"][l][g] = summ[nl_fb + g * nl_sb + l]

    def _result(self, f: _Forward) -> dict:
        fb, sb, plan = f.fbm.d, f.sbm.d, f.plan
        ng, nl_fb, nl_sb = self.spec.n_groups, self.spec.fb_layers, self.spec.sb_layers

        def outs(m, i, no_proj=False):
            x, pr = m.xs[i], m.d["proj"][i]
            if i in f.x_skipped[m.tag]:  # never written: the entry keeps its shape (compute_neuronops reads size(-1)) and nothing else
                x = torch.empty(x.shape, dtype=x.dtype, device="meta")
            if no_proj:  # (lean modes through sfsn_proj_deepfilter: the coefficient rows stayed in LDS)
                pr = torch.empty(pr.shape, dtype=pr.dtype, device="meta")
            return [x] + [m.d["spk"][l][i] for l in range(len(m.d["spk"]))] + [pr]
        enh, enh_mag = (f.enh[..., f.lead:], f.enh_mag[..., f.lead:]) if f.lead else (f.enh, f.enh_mag)  # (a start: the new frames)
        return dict(enh_stft=enh, enh_mag=enh_mag, fb_all=outs(f.fbm, 0), sb_all=[outs(f.sbm, g, f.proj_skipped) for g in range(ng)],
                    fb_mem=[fb["mem"][l][0] for l in range(nl_fb)], sb_mem=[[sb["mem"][l][g] for l in range(nl_sb)] for g in range(ng)],
                    mu_fb=f.fbm.mu, mu_sb=f.sbm.mu, sd_fb=f.fbm.sd, sd_sb=f.sbm.sd, pipelined=plan.pipeline, overlapped=plan.overlap,
                    n_chunks=len(plan.bounds))
