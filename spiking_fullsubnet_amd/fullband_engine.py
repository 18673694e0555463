"""Host-side driver of the cIRM-GSN path (``modeling_cirm_gsn.Model``): one full-band GSN stack on all n_fft/2 + 1 bins and a
full-spectrum deep filter.  ``Engine`` is built around a full-band model plus sub-band groups; this is the small engine of the other
model, through the same C ABI:

    sfsn_fullband_features         |X|^fdrc over all F bins + LayerNorm             -> x [T][B][F]
    sfsn_fullband_input_proj       layer 0's input term x . W_ih^T + bias_ih         -> zin [T][B][G*Hp]
                                   (sfsn_input_proj_f32 where K = F <= 192)
    sfsn_gsn_stack_scan            every GSN layer in one launch (shared gates; per-layer scans otherwise)
    sfsn_fullband_proj_deepfilter  projection + activation + deep filter + |.|      -> enh [B][S][F][T]
                                   (a ragged batch, ``forward_stft(frames=)``: sfsn_fullband_proj_deepfilter_ragged, which stops at
                                   each clip's own last frame and writes the zeros behind it)

Hidden sizes that are not a multiple of 16 (the recipe's H = 268) are padded to Hp = ceil16(H) when packing: zero rows and columns
in W_ih / W_hh / W_proj, and the padded neurons are held silent (``pad_cell``).  The int8 digit products of the real neurons are
exact integer sums, so the padding changes none of their bits.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, ragged
from ._lib import MAX_COUNT_TENSORS, FusedInput, RowCount, ScanSegment, check
from .engine import ErrorWords, SpikeSummary, _dev, _ptr, fill_segment, fold_batchnorm, pack_w3

ACTIVATIONS = {"tanh": _lib.ACT_TANH, "sigmoid": _lib.ACT_SIGMOID, "relu": _lib.ACT_RELU}


def activation_code(name) -> int:
    """The reference's output activation (modeling_cirm_gsn.py:54-61): only the exact strings "tanh", "sigmoid" and "relu" select
    one; anything else (False, None, "Tanh", ...) is nn.Identity."""
    return ACTIVATIONS.get(name, _lib.ACT_NONE) if isinstance(name, str) else _lib.ACT_NONE


def ceil16(h: int) -> int:
    return (h + 15) // 16 * 16


@dataclass
class FullbandSpec:
    n_fft: int
    fdrc: float
    hidden: int
    layers: int
    df: int
    num_spks: int
    shared: bool
    bn: bool
    ln: bool
    act: int

    @property
    def F(self) -> int:
        return self.n_fft // 2 + 1

    @property
    def P(self) -> int:
        return 2 * self.df * self.num_spks * self.F


def pad_cell(w_ih, w_hh, bias, alpha, beta, H: int, Hp: int, in_pad: int, shared: bool):
    """One GSN cell's parameters padded from H to Hp neurons (numpy, fp32).

    w_ih [G*H, I] -> [G*Hp, in_pad] and w_hh [G*H, H] -> [G*Hp, Hp]: each gate's rows are padded with zero rows, the input and
    recurrent columns with zero columns (the padded inputs are the silent neurons of the layer below).  bias [2H] -> [2Hp]: the
    padded neurons get 0 in the forget half and -1 in the cell half, alpha / beta (folded BatchNorm, or 1 / 0) -> 0 / -1 with BN.
    Without BN the membrane of a padded neuron is c' = 0.5 c - 0.5 (forget gate sigmoid(0), cell input -1): it starts at -0.5 and
    stays in [-1, -0.5]; with BN it is fma(c', 0, -1) = -1.  Either way it never reaches the threshold 0 and never spikes.
    Hp == H returns the arrays unchanged (as fp32 copies)."""
    f32 = np.float32
    G = 1 if shared else 2
    I = w_ih.shape[1]
    wi = np.zeros((G * Hp, in_pad), f32)
    wh = np.zeros((G * Hp, Hp), f32)
    for g in range(G):
        wi[g * Hp:g * Hp + H, :I] = w_ih[g * H:(g + 1) * H]
        wh[g * Hp:g * Hp + H, :H] = w_hh[g * H:(g + 1) * H]
    b = np.zeros(2 * Hp, f32)
    b[:H] = bias[:H]
    b[Hp:Hp + H] = bias[H:]
    b[Hp + H:] = -1.0
    a = np.ones(Hp, f32) if alpha is None else np.zeros(Hp, f32)
    be = np.zeros(Hp, f32) if beta is None else np.full(Hp, -1.0, f32)
    if alpha is not None:
        a[:H], be[:H] = alpha, beta
    return wi, wh, b, a, be


def permute_proj(w: np.ndarray, b: Optional[np.ndarray], F: int, df: int, S: int, Hp: int):
    """W_proj [2 df S F, H] (columns in the reference's (c, d, s, f) order) -> the bin-major row order sfsn_fullband_proj_deepfilter
    reads (include/sfsn.h): row (fb * 2 df S + (c df + d) S + s) * 16 + i = column ((c df + d) S + s) F + fb * 16 + i, zero rows for
    bins >= F, zero columns H..Hp-1.  Returns (W' [NFB * 2 df S * 16, Hp], bias' or None)."""
    NCT, NFB = 2 * df * S, (F + 15) // 16
    P, H = w.shape
    assert P == NCT * F, (w.shape, F, df, S)
    rows = np.full((NFB, NCT, 16), -1, np.int64)
    f = np.arange(NFB * 16).reshape(NFB, 16)
    for j in range(NCT):
        rows[:, j, :] = np.where(f < F, j * F + f, -1)
    rows = rows.reshape(-1)
    wp = np.zeros((rows.size, Hp), np.float32)
    wp[rows >= 0, :H] = w[rows[rows >= 0]]
    bp = None
    if b is not None:
        bp = np.zeros(rows.size, np.float32)
        bp[rows >= 0] = b[rows[rows >= 0]]
    return wp, bp


@dataclass
class _Layer:
    w_ih_f32: Optional[torch.Tensor]  # layer 0: [G*Hp, F] fp32
    w_ih_q: list                      # layers >= 1: per gate (packed, dq) of [Hp, Hp]
    w_hh_q: torch.Tensor
    w_hh_dq: torch.Tensor
    bias: torch.Tensor
    alpha: torch.Tensor
    beta: torch.Tensor


class FullbandEngine:
    """Packed weights + launch sequence of the cIRM-GSN model on one device."""

    def __init__(self, spec: FullbandSpec, state_dict: Dict[str, np.ndarray], device, weight_bits: int = 24):
        if weight_bits not in (24, 16):
            raise ValueError("weight_bits must be 24 (exact) or 16")
        self.spec, self.device, self.weight_bits = spec, torch.device(device), weight_bits
        if self.device.type != "cuda":
            raise RuntimeError("spiking_fullsubnet_amd runs on a HIP device only (no CPU path); move the module to 'cuda'")
        self.lib = _lib.lib()
        H, F = spec.hidden, spec.F
        self.H, self.Hp, self.F = H, ceil16(H), F
        self.HP8 = (self.Hp + 63) // 64 * 64  # bytes of an int8 spike row
        if self.Hp > _lib.MAX_HIDDEN:
            raise NotImplementedError(f"hidden size {H} (padded {self.Hp}): the gfx950 scan holds W_hh register-resident up to "
                                      f"{_lib.MAX_HIDDEN}")
        if F > 320:
            raise NotImplementedError(f"{F} frequency bins: sfsn_fullband_features covers F <= 320 (n_fft <= 638)")
        if spec.num_spks > 4 or spec.df > 16:
            raise NotImplementedError(f"num_spks = {spec.num_spks}, df_order = {spec.df}: sfsn_fullband_proj_deepfilter covers "
                                      "num_spks <= 4 and df_order <= 16")
        sd = {k: np.asarray(v) for k, v in state_dict.items()}
        G, Hp, dev = (1 if spec.shared else 2), self.Hp, self.device
        self.G = G
        self.layers = []
        for l in range(spec.layers):
            p = f"fb_model.sequence_model.layers.{l}.cell."
            alpha = beta = None
            if spec.bn:
                alpha, beta = fold_batchnorm(sd[p + "batchnorm.weight"], sd[p + "batchnorm.bias"], sd[p + "batchnorm.running_mean"],
                                             sd[p + "batchnorm.running_var"])
            wi, wh, b, a, be = pad_cell(sd[p + "weight_ih"], sd[p + "weight_hh"], sd[p + "bias_ih"], alpha, beta, H, Hp,
                                        F if l == 0 else Hp, spec.shared)
            pk, dq = pack_w3(wh, weight_bits)
            layer = _Layer(w_ih_f32=_dev(wi, dev) if l == 0 else None, w_ih_q=[], w_hh_q=_dev(pk, dev), w_hh_dq=_dev(dq, dev),
                           bias=_dev(b, dev), alpha=_dev(a, dev), beta=_dev(be, dev))
            if l > 0:
                for g in range(G):
                    pk, dq = pack_w3(wi[g * Hp:(g + 1) * Hp], weight_bits)
                    layer.w_ih_q.append((_dev(pk, dev), _dev(dq, dev)))
            self.layers.append(layer)
        wp, bp = permute_proj(sd["fb_model.proj.weight"], sd["fb_model.proj.bias"], F, spec.df, spec.num_spks, Hp)
        pk, dq = pack_w3(wp, weight_bits)
        self.proj_q, self.proj_dq, self.proj_b = _dev(pk, dev), _dev(dq, dev), _dev(bp, dev)
        self.ln_w = self.ln_b = None
        if spec.ln:
            self.ln_w = _dev(sd["fb_model.pre_layer_norm.weight"].astype(np.float32), dev)
            self.ln_b = _dev(sd["fb_model.pre_layer_norm.bias"].astype(np.float32), dev)
        self.launches: Dict[str, int] = {}  # launches per C-ABI entry point (tests assert which path ran)
        self.stack_scan = True  # all layers in one sfsn_gsn_stack_scan launch where it applies (False: one scan launch per layer)
        self.stack_lag = 4
        self._ws: Dict[tuple, dict] = {}
        self._errors = ErrorWords(self)  # the stack launches' error words: polled at the next forward

    def _count(self, what: str) -> None:
        self.launches[what] = self.launches.get(what, 0) + 1

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _use_stack(self, B: int) -> bool:
        """The stack launch wants every layer's workgroups resident at once (sfsn_gsn_stack_scan's contract): 4 rows per workgroup
        plus the input-term workgroups for Hp > 256, 8 rows per workgroup otherwise."""
        if not (self.stack_scan and self.spec.shared and self.spec.layers >= 2):
            return False
        n_cu = torch.cuda.get_device_properties(self.device).multi_processor_count
        nl = self.spec.layers
        if self.Hp > 256:
            return (B + 3) // 4 * nl + (B + 15) // 16 * (nl - 1) <= n_cu
        return (B + 7) // 8 * nl <= n_cu

    def _workspace(self, B: int, T: int, stack: bool) -> dict:
        """Scratch of one geometry and stream (reused across forwards): input terms, int8 spikes (pad columns stay zero), stack
        counters (zeroed once; every launch leaves them zeroed)."""
        key = (B, T, stack, torch.cuda.current_stream(self.device).cuda_stream)
        ws = self._ws.get(key)
        if ws is None:
            if len(self._ws) >= 4:
                self._ws.clear()
            ws = self._ws[key] = self._make_workspace(B, T, T, stack)
        return ws

    def _make_workspace(self, B: int, nt: int, T: int, stack: bool) -> dict:
        """Scratch of launches over `nt` frames of a [B, F, T] spectrum: input terms of the nt frames, int8 spikes of all T."""
        dev, nl, Hp, G = self.device, self.spec.layers, self.Hp, self.G
        f32 = dict(dtype=torch.float32, device=dev)
        n_zin = nl if (not stack or Hp > 256) else 1
        ws = dict(zin=[torch.empty((nt, B, G * Hp), **f32) for _ in range(n_zin)],
                  s8=[torch.zeros((T, B, self.HP8), dtype=torch.int8, device=dev) for _ in range(nl)])
        if stack:
            nbytes = self.lib.sfsn_stack_scratch_bytes(nl, 1, B)
            ws["scratch"] = torch.zeros(((nbytes + 3) // 4,), dtype=torch.int32, device=dev)
        return ws

    def check_stack_errors(self) -> None:
        """Raise if a hand-off wait of an earlier stack launch expired (synchronises)."""
        self._errors.check()

    def _launch_frames(self, ri, B: int, T: int, t0: int, nt: int, stack: bool, ws: dict, x, states, spk, proj, enh, mag,
                       frames_dev: Optional[torch.Tensor] = None, mem=None, own_frames=None) -> None:
        """The launch sequence of the model on frames [t0, t0 + nt) of the spectrum ri [B, F, T, 2], on torch's current stream:
        features -> layer 0's input term -> the GSN layers from `states` (updated in place) -> projection + deep filter.
        forward_stft runs it on (0, T) from zero states; a streaming session (fullband_streaming.py) on the `hop` new frames behind
        its history, with the states carried.  x [T, B, F], spk[l] [T, B, Hp] or None, proj [T, B, P] or None, enh [B, S, F, T, 2],
        mag [B, S, F, T] or None are whole-spectrum buffers; ws = _make_workspace(B, nt, T, stack).  frames_dev (int32 [B] on the
        device): a ragged batch -- the last launch is the length-aware one: enh / mag are zero and proj is not written at frames
        >= frames_dev[b].  The launches before it are the same: the model is causal.
        mem (a session's ragged backlog, ``catch_up_ragged``): mem[l] [T, B, Hp], every frame's post-BatchNorm membrane of layer l
        (sfsn_scan_segment.membrane) -- the per-layer launches (``stack`` False: the stack launch has no tap), with fp32 spikes in
        spk[l], which the tap goes with.  own_frames (host ints, with mem): clip b has own_frames[b] <= nt of the new frames and is
        promised the bits of ITS OWN call, so its rows of layer 0's input product take the form that call would (``_l0_as_alone``)."""
        spec, L, Hp, G, F = self.spec, self.lib, self.Hp, self.G, self.F
        st, dev, nl, S = self._stream(), self.device, spec.layers, spec.num_spks
        check(L.sfsn_fullband_features(_ptr(ri), B, F, T, spec.fdrc, _ptr(self.ln_w), _ptr(self.ln_b), 1e-5, _ptr(x), t0, nt, st),
              "sfsn_fullband_features")
        self._count("features")
        # layer 0's input term
        z0, l0 = ws["zin"][0], self.layers[0]
        x_at = ctypes.c_void_p(x.data_ptr() + t0 * B * F * 4)
        for g in range(G):
            args = (x_at, ctypes.c_void_p(l0.w_ih_f32.data_ptr() + g * Hp * F * 4), ctypes.c_void_p(l0.bias.data_ptr() + g * Hp * 4),
                    ctypes.c_void_p(z0.data_ptr() + g * Hp * 4), nt * B, F, Hp, G * Hp, st)
            rc = L.sfsn_input_proj_f32(*args)
            if rc == _lib.SFSN_EUNSUPPORTED:  # K = F > 192 (every n_fft = 512 model): the full-band library's own product
                check(L.sfsn_fullband_input_proj(*args), "sfsn_fullband_input_proj")
                self._count("inproj_wide")
            else:
                check(rc, "sfsn_input_proj_f32")
                self._count("inproj")
                if own_frames is not None:
                    self._l0_as_alone(args, x, z0, g, B, t0, nt, own_frames)
        s8_at = t0 * B * self.HP8  # frame t0 of an int8 spike buffer
        if mem is not None and stack:
            raise ValueError("the membrane tap runs on the per-layer launches (sfsn_gsn_stack_scan requires membrane == NULL)")
        if stack:
            segs = (ScanSegment * nl)()
            fin = (FusedInput * nl)()
            for l in range(nl):
                # layers >= 1 with Hp > 256: the launch's input-term workgroups write their [nt][B][Hp] buffer; Hp <= 256: in-scan
                zin = ws["zin"][0] if l == 0 else (ws["zin"][l] if Hp > 256 else None)
                fill_segment(segs[l], self.layers[l], B, Hp, t0, zin, states[l], ws["s8"][l], spk[l])
                if l > 0:
                    pk, dq = self.layers[l].w_ih_q[0]
                    fin[l].spikes_in, fin[l].w_ih, fin[l].w_ih_dq = ws["s8"][l - 1].data_ptr() + s8_at, pk.data_ptr(), dq.data_ptr()
            rp = 4 if Hp > 256 else 8
            rpw = (ctypes.c_int * nl)(*([rp] * nl))
            scratch = ws["scratch"]
            check(L.sfsn_gsn_stack_scan(segs, fin, nl, 1, nt, Hp, rpw, self.stack_lag, _ptr(scratch), scratch.numel() * 4, st),
                  "sfsn_gsn_stack_scan")
            self._count("stack")
            if not torch.cuda.is_current_stream_capturing():  # the launch's error word, looked at without blocking next time
                self._errors.watch(torch.cuda.current_stream(dev), scratch, f"full-band stack rows={B} frames={nt} rows_per_wg={rp}")
        else:
            for l in range(nl):
                zin = ws["zin"][l]
                if l > 0:
                    for g in range(G):
                        pk, dq = self.layers[l].w_ih_q[g]
                        check(L.sfsn_spike_proj(ctypes.c_void_p(ws["s8"][l - 1].data_ptr() + s8_at), _ptr(pk), _ptr(dq),
                                                ctypes.c_void_p(self.layers[l].bias.data_ptr() + g * Hp * 4),
                                                ctypes.c_void_p(zin.data_ptr() + g * Hp * 4), nt * B, Hp, Hp, G * Hp, st), "sfsn_spike_proj")
                        self._count("spike_proj")
                seg = (ScanSegment * 1)()
                fill_segment(seg[0], self.layers[l], B, Hp, t0, zin, states[l], ws["s8"][l], spk[l], None if mem is None else mem[l])
                check(L.sfsn_gsn_layer_scan(seg, 1, nt, Hp, int(spec.shared), 0, st), "sfsn_gsn_layer_scan")
                self._count("layer_scan")
        args = (_ptr(ri), _ptr(ws["s8"][-1]), Hp, _ptr(self.proj_q), _ptr(self.proj_dq), _ptr(self.proj_b), spec.act, B, F, T, S, spec.df,
                _ptr(proj), _ptr(enh), _ptr(mag), t0, nt)
        if frames_dev is None:
            check(L.sfsn_fullband_proj_deepfilter(*args, st), "sfsn_fullband_proj_deepfilter")
            self._count("projdf")
        else:
            check(L.sfsn_fullband_proj_deepfilter_ragged(*args, _ptr(frames_dev), st), "sfsn_fullband_proj_deepfilter_ragged")
            self._count("projdf_ragged")

    def _l0_as_alone(self, args, x, z0, g: int, B: int, t0: int, nt: int, own_frames) -> None:
        """Behind sfsn_input_proj_f32 on the nt * B rows of a padded batch (K = F <= 192): that product is fp32 below 64 rows per
        call and bf16-split from there on, and the two forms differ in the low bits (include/sfsn.h).  A clip alone has own_frames[b]
        rows, the batch nt * B: where the batch took the split form, the rows of every clip whose own call stays below 64 are done
        again in the fp32 form, in calls below 64 rows (a row's result depends on nothing but the row), as ``Engine`` does for
        ``advance_ragged`` (engine.py, l0_alone).  A clip of 64 rows or more takes the split form alone and in any batch."""
        if nt * B < 64:
            return
        rows = [np.arange(n) * B + b for b, n in enumerate(own_frames) if 0 < n < 64]
        if not rows:
            return
        mine = np.sort(np.concatenate(rows))
        F, Hp, G, P = self.F, self.Hp, self.G, ctypes.c_void_p
        idx = torch.from_numpy(mine.astype(np.int64)).pin_memory().to(self.device, non_blocking=True)
        xr = x[t0:t0 + nt].reshape(-1, F).index_select(0, idx)
        zr = torch.empty((len(mine), Hp), dtype=torch.float32, device=self.device)
        for r0 in range(0, len(mine), 63):
            check(self.lib.sfsn_input_proj_f32(P(xr.data_ptr() + r0 * F * 4), args[1], args[2], P(zr.data_ptr() + r0 * Hp * 4),
                                               min(63, len(mine) - r0), F, Hp, Hp, args[-1]), "sfsn_input_proj_f32")
            self._count("inproj_alone")
        z0.view(-1, G * Hp)[:, g * Hp:(g + 1) * Hp].index_copy_(0, idx, zr)

    @torch.no_grad()
    def forward_stft(self, noisy_cmp: torch.Tensor, want_layers: bool = False, want_counts: bool = False, frames=None,
                     frames_dev: Optional[torch.Tensor] = None) -> dict:
        """complex64 [B, F, T] on the device -> dict(enh_stft complex [B, S, F, T], enh_mag [B, S, F, T] (num_spks == 1) or None,
        all_layers = [x [T, B, F], spikes [T, B, H] per layer, proj [T, B, P]] when want_layers, else None).  want_counts: also
        clip_counts, int64 [layers, B] -- every layer's spikes per clip, counted on the device from the int8 spikes the scans write
        (one sfsn_spike_count_rows launch); without want_layers no fp32 spike or projection tensor is allocated and all_layers is
        [x] + [SpikeSummary(count over the clips, (T, B, H)) per layer] + [proj (T, B, P), shape only (a meta tensor)]: all that
        metric.compute_synops / compute_neuronops read.

        ``frames`` -- a ragged batch (``ragged.py``): a length-B sequence of ints, clip b has ``frames[b]`` frames
        (``1 <= frames[b] <= T``; ``ValueError`` naming the clip otherwise) and the rest of its row is padding.  Over its own frames
        clip b is the clip run alone, bit for bit.  ``enh_stft`` / ``enh_mag`` are zero at frames ``>= frames[b]`` (the length-aware
        epilogue writes the zeros and does no work there); ``clip_counts[l, b]`` counts clip b's own frames and the spike entries of
        ``all_layers`` are ``ragged.ClipSpikeSummary``; with want_layers ``proj`` is zero past a clip's end while ``x`` and the spike
        tensors keep what the model computed on the padding (``ragged.clip_layers`` slices).  The lengths go to the device once,
        without a host synchronisation (``frames_dev``: they are there already, as int32 [B])."""
        spec, L, Hp, G, F = self.spec, self.lib, self.Hp, self.G, self.F
        if noisy_cmp.device != self.device or noisy_cmp.dtype != torch.complex64 or noisy_cmp.ndim != 3 or noisy_cmp.shape[1] != F:
            raise ValueError(f"expected complex64 [B, {F}, T] on {self.device}, got {noisy_cmp.dtype} {tuple(noisy_cmp.shape)} "
                             f"on {noisy_cmp.device}")
        B, _, T = noisy_cmp.shape
        if frames is not None:
            frames = ragged.check_frames(frames, B, T)
            if frames_dev is None:
                frames_dev = ragged.upload(frames, self.device)
        self._errors.poll()
        ri = torch.view_as_real(noisy_cmp.contiguous())
        st, dev, nl, S = self._stream(), self.device, spec.layers, spec.num_spks
        f32 = dict(dtype=torch.float32, device=dev)
        stack = self._use_stack(B)
        ws = self._workspace(B, T, stack)
        x = torch.empty((T, B, F), **f32)
        flat = torch.zeros((nl, 2, B, Hp), **f32)  # zero initial state (modeling_cirm_gsn.py:95-101)
        states = [(flat[l, 0], flat[l, 1]) for l in range(nl)]
        spk = [torch.empty((T, B, Hp), **f32) if want_layers else None for _ in range(nl)]
        enh = torch.empty((B, S, F, T, 2), **f32)
        mag = torch.empty((B, S, F, T), **f32) if S == 1 else None
        # (a ragged batch: the epilogue leaves proj alone past a clip's end, so it starts out zero)
        proj = (torch.empty if frames is None else torch.zeros)((T, B, spec.P), **f32) if want_layers else None
        self._launch_frames(ri, B, T, 0, T, stack, ws, x, states, spk, proj, enh, mag, frames_dev)
        out = dict(enh_stft=torch.view_as_complex(enh), enh_mag=mag, all_layers=None)
        if want_counts:  # SynOPs without the fp32 spike tensors: the workspace's int8 spikes [T][B][HP8] (pad columns zero), a row per clip
            counts = out["clip_counts"] = torch.zeros((nl, B), dtype=torch.int64, device=dev)
            for l0 in range(0, nl, MAX_COUNT_TENSORS):
                arr = (RowCount * min(MAX_COUNT_TENSORS, nl - l0))()
                for j in range(len(arr)):
                    arr[j].spikes_i8, arr[j].T, arr[j].R, arr[j].HP, arr[j].rows_per_clip = _ptr(ws["s8"][l0 + j]), T, B, self.HP8, 1
                    arr[j].counts = _ptr(counts[l0 + j])
                if frames is None:
                    check(L.sfsn_spike_count_rows(arr, len(arr), 0, T, st), "sfsn_spike_count_rows")
                else:  # each clip's own frames
                    check(L.sfsn_spike_count_rows_ragged(arr, len(arr), 0, T, _ptr(frames_dev), B, st), "sfsn_spike_count_rows_ragged")
                self._count("spike_count")
        if want_layers:
            out["all_layers"] = [x] + [s[:, :, :self.H] for s in spk] + [proj]
        elif want_counts:
            if frames is None:
                summaries = [SpikeSummary(c, (T, B, self.H)) for c in counts.sum(1)]
            else:
                summaries = [ragged.ClipSpikeSummary(c, (T, B, self.H), frames) for c in counts]
            out["all_layers"] = [x] + summaries + [torch.empty((T, B, spec.P), dtype=torch.float32, device="meta")]
        return out
