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
