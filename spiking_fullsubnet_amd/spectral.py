"""STFT / inverse STFT of the models on the device kernels (``sfsn_stft`` / ``sfsn_istft``).

Same contract as ``audiozen.acoustics.audio_feature.stft(..., output_type="complex")`` / ``istft(..., input_type="complex")``
(audio_feature.py:236-347): Hann window of ``n_fft``, centred frames, zero padding, ``[B, F, T]`` complex64.  The kernels are
built for the 512-point analysis every reference config uses; any other ``n_fft`` raises ``NotImplementedError`` (the
modules then keep ``torch.stft`` / ``torch.istft``, see ``SpikingFullSubNet.stft``).
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib
from ._lib import check

_windows = {}


def hann(n_fft: int, device) -> torch.Tensor:
    key = (n_fft, str(device))
    if key not in _windows:
        _windows[key] = torch.hann_window(n_fft, device=device)  # audio_feature.py:269,337
    return _windows[key]


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def stft(y: torch.Tensor, n_fft: int, hop_length: int, win_length: Optional[int] = None, window: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 [B, L] on the device -> complex64 [B, n_fft/2+1, 1 + L // hop]."""
    if y.dim() != 2 or y.dtype != torch.float32 or y.device.type != "cuda":
        raise RuntimeError(f"expected a float32 [B, L] tensor on a HIP device, got {y.dtype} {tuple(y.shape)} on {y.device}")
    if win_length not in (None, n_fft):
        raise NotImplementedError("win_length != n_fft")
    B, L = y.shape
    T = 1 + L // hop_length
    w = hann(n_fft, y.device) if window is None else window.to(device=y.device, dtype=torch.float32).contiguous()
    out = torch.empty((B, n_fft // 2 + 1, T), dtype=torch.complex64, device=y.device)
    y = y.contiguous()
    with torch.cuda.device(y.device):  # the C ABI launches on the calling thread's current device
        check(_lib.lib().sfsn_stft(y.data_ptr(), B, L, n_fft, hop_length, w.data_ptr(), torch.view_as_real(out).data_ptr(), T, _stream(y.device)),
              "sfsn_stft")
    return out


def istft(spec: torch.Tensor, n_fft: int, hop_length: int, win_length: Optional[int] = None, window: Optional[torch.Tensor] = None,
          length: Optional[int] = None) -> torch.Tensor:
    """complex64 [B, n_fft/2+1, T] on the device -> float32 [B, length] (default length: (T - 1) * hop, as torch.istft)."""
    if spec.dim() != 3 or spec.dtype != torch.complex64 or spec.device.type != "cuda":
        raise RuntimeError(f"expected a complex64 [B, F, T] tensor on a HIP device, got {spec.dtype} {tuple(spec.shape)} on {spec.device}")
    if win_length not in (None, n_fft):
        raise NotImplementedError("win_length != n_fft")
    B, F, T = spec.shape
    if F != n_fft // 2 + 1:
        raise ValueError(f"expected {n_fft // 2 + 1} frequency bins, got {F}")
    if length is None:
        length = (T - 1) * hop_length
    w = hann(n_fft, spec.device) if window is None else window.to(device=spec.device, dtype=torch.float32).contiguous()
    spec = spec.contiguous()
    out = torch.empty((B, length), dtype=torch.float32, device=spec.device)
    with torch.cuda.device(spec.device):
        check(_lib.lib().sfsn_istft(torch.view_as_real(spec).data_ptr(), B, T, n_fft, hop_length, w.data_ptr(), out.data_ptr(), length,
                                    _stream(spec.device)), "sfsn_istft")
    return out


# ---- outer samples: three times the model's rate, 16-bit PCM (include/sfsn.h; csrc/sfsn_resample_dev.h) ---------------------------
RESAMPLE_TAPS, RESAMPLE_PHASE_TAPS = 96, 32
SAMPLE_FORMATS = {"f32": (_lib.SAMPLE_F32, torch.float32), "s16": (_lib.SAMPLE_S16, torch.int16)}
_taps = {}


def resample_taps_host():
    """``(h float32 [96], g float32 [3, 32])``: the low-pass ``sinc((k - 47.5) / 3) / 3 * kaiser(96, 8)[k]`` normalised to sum 1 in
    float64 and rounded, and its three phases ``3 h[3 j + p]`` formed in float64 and rounded once (numpy arrays)."""
    import numpy as np
    k = np.arange(RESAMPLE_TAPS, dtype=np.float64)
    h = np.sinc((k - 47.5) / 3.0) / 3.0 * np.kaiser(RESAMPLE_TAPS, 8.0)
    h = h / h.sum()
    g = np.stack([3.0 * h[p::3] for p in range(3)])
    return h.astype(np.float32), g.astype(np.float32)


def resample_taps(device):
    """The two tap tables of ``resample_taps_host`` on ``device`` (made once per device, like the Hann window)."""
    key = str(device)
    if key not in _taps:
        h, g = resample_taps_host()
        _taps[key] = (torch.from_numpy(h).to(device), torch.from_numpy(g).contiguous().to(device))
    return _taps[key]


def format_of(name: str):
    """``(SFSN_SAMPLE_* code, torch dtype)`` of ``"f32"`` / ``"s16"``; anything else is a ``ValueError``."""
    if name not in SAMPLE_FORMATS:
        raise ValueError(f"sample_format must be one of {sorted(SAMPLE_FORMATS)}, got {name!r}")
    return SAMPLE_FORMATS[name]


def _filter_state(state, rows: int, width: int, device, what: str):
    if state is None:
        return torch.zeros((rows, width), dtype=torch.float32, device=device)
    if state.dtype != torch.float32 or tuple(state.shape) != (rows, width) or state.device != device or not state.is_contiguous():
        raise RuntimeError(f"{what}: state must be a contiguous float32 [{rows}, {width}] tensor on {device}")
    return state


def resample_down3(x: torch.Tensor, state: Optional[torch.Tensor] = None):
    """48 -> 16 kHz: ``x`` float32 or int16 (``s * 2**-15``) ``[B, 3 n]`` on the device (rows may be strided) ->
    ``(y float32 [B, n], state [B, 96])`` with ``y[m] = sum_k h[k] x[3 m + 2 - k]``.  ``state`` carries the last 93 input samples
    from call to call (``None``: a zero state is made; a given one is updated in place and returned): a signal fed in chunks equals
    the one-shot call bit for bit.  47.5 input samples of group delay."""
    if x.dim() != 2 or x.dtype not in (torch.float32, torch.int16) or x.device.type != "cuda" or x.shape[1] % 3 or x.shape[1] == 0:
        raise RuntimeError(f"expected a float32 or int16 [B, 3 n] tensor on a HIP device, got {x.dtype} {tuple(x.shape)} on {x.device}")
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    B, n = x.shape[0], x.shape[1] // 3
    fmt = _lib.SAMPLE_S16 if x.dtype == torch.int16 else _lib.SAMPLE_F32
    state = _filter_state(state, B, 96, x.device, "resample_down3")
    out = torch.empty((B, n), dtype=torch.float32, device=x.device)
    taps, _ = resample_taps(x.device)
    with torch.cuda.device(x.device):
        check(_lib.lib().sfsn_resample_down3(x.data_ptr(), fmt, B, n, x.stride(0) if B > 1 else x.shape[1], taps.data_ptr(), state.data_ptr(),
                                             out.data_ptr(), _stream(x.device)), "sfsn_resample_down3")
    return out, state


def resample_up3(y: torch.Tensor, state: Optional[torch.Tensor] = None, sample_format: str = "f32", out: Optional[torch.Tensor] = None):
    """16 -> 48 kHz: ``y`` float32 ``[R, n]`` on the device -> ``(z [R, 3 n], state [R, 32])`` with
    ``z[3 m + p] = sum_j 3 h[3 j + p] y[m - j]``; ``sample_format="s16"`` returns int16,
    ``clamp(rint(z * 32768), -32768, 32767)`` (ties to even, NaN -> 0).  ``state`` carries the last 31 values of ``y`` as for
    ``resample_down3``.  ``out``: an ``[R, 3 n]`` tensor of the format to write into (rows may be strided).  47.5 output samples of
    group delay."""
    code, dtype = format_of(sample_format)
    if y.dim() != 2 or y.dtype != torch.float32 or y.device.type != "cuda" or y.shape[1] == 0:
        raise RuntimeError(f"expected a float32 [R, n] tensor on a HIP device, got {y.dtype} {tuple(y.shape)} on {y.device}")
    y = y.contiguous()
    R, n = y.shape
    state = _filter_state(state, R, 32, y.device, "resample_up3")
    if out is None:
        out = torch.empty((R, 3 * n), dtype=dtype, device=y.device)
    elif out.dtype != dtype or tuple(out.shape) != (R, 3 * n) or out.device != y.device or out.stride(1) != 1 or (R > 1 and out.stride(0) < 3 * n):
        raise RuntimeError(f"resample_up3: out must be a {dtype} [{R}, {3 * n}] tensor on {y.device} with unit sample stride")
    _, g = resample_taps(y.device)
    with torch.cuda.device(y.device):
        check(_lib.lib().sfsn_resample_up3(y.data_ptr(), R, n, g.data_ptr(), state.data_ptr(), out.data_ptr(), code,
                                           out.stride(0) if R > 1 else 3 * n, _stream(y.device)), "sfsn_resample_up3")
    return out, state


def _lengths_dev(t: torch.Tensor, n: int, what: str) -> torch.Tensor:
    if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] != n or t.device.type != "cuda":
        raise RuntimeError(f"{what}: expected an int32 [{n}] tensor on the HIP device (ragged.upload)")
    return t.contiguous()


def stft_ragged(y: torch.Tensor, n_fft: int, hop_length: int, clip_len: torch.Tensor) -> torch.Tensor:
    """``stft`` of a padded batch whose clip b has ``clip_len[b]`` samples (int32 [B] on the device): what the buffer holds past a
    clip's end reads as zero.  Frames ``t < 1 + clip_len[b] // hop`` of clip b are the bits of ``stft`` on that clip alone."""
    if y.dim() != 2 or y.dtype != torch.float32 or y.device.type != "cuda":
        raise RuntimeError(f"expected a float32 [B, L] tensor on a HIP device, got {y.dtype} {tuple(y.shape)} on {y.device}")
    B, L = y.shape
    T = 1 + L // hop_length
    w = hann(n_fft, y.device)
    out = torch.empty((B, n_fft // 2 + 1, T), dtype=torch.complex64, device=y.device)
    y, clip_len = y.contiguous(), _lengths_dev(clip_len, B, "clip_len")
    with torch.cuda.device(y.device):
        check(_lib.lib().sfsn_stft_ragged(y.data_ptr(), B, L, n_fft, hop_length, w.data_ptr(), torch.view_as_real(out).data_ptr(), T,
                                          clip_len.data_ptr(), _stream(y.device)), "sfsn_stft_ragged")
    return out


def istft_ragged(spec: torch.Tensor, n_fft: int, hop_length: int, length: int, clip_frames: torch.Tensor, clip_len: torch.Tensor) -> torch.Tensor:
    """``istft`` of a padded batch -> float32 [B, length]: clip b is built from its first ``clip_frames[b]`` frames only and is zero
    from sample ``clip_len[b]`` on (both int32 [B] on the device).  ``out[b, :clip_len[b]]`` has the bits of ``istft`` on
    ``spec[b:b+1, :, :clip_frames[b]]`` with ``length=clip_len[b]``."""
    if spec.dim() != 3 or spec.dtype != torch.complex64 or spec.device.type != "cuda":
        raise RuntimeError(f"expected a complex64 [B, F, T] tensor on a HIP device, got {spec.dtype} {tuple(spec.shape)} on {spec.device}")
    B, F, T = spec.shape
    if F != n_fft // 2 + 1:
        raise ValueError(f"expected {n_fft // 2 + 1} frequency bins, got {F}")
    w = hann(n_fft, spec.device)
    spec = spec.contiguous()
    clip_frames, clip_len = _lengths_dev(clip_frames, B, "clip_frames"), _lengths_dev(clip_len, B, "clip_len")
    out = torch.empty((B, length), dtype=torch.float32, device=spec.device)
    with torch.cuda.device(spec.device):
        check(_lib.lib().sfsn_istft_ragged(torch.view_as_real(spec).data_ptr(), B, T, n_fft, hop_length, w.data_ptr(), out.data_ptr(), length,
                                           clip_frames.data_ptr(), clip_len.data_ptr(), _stream(spec.device)), "sfsn_istft_ragged")
    return out
