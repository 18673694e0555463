"""The intel_ndns recipe's training loss on the device kernel (``sfsn_recipe_loss``).

Drop-ins for ``audiozen/loss.py`` as ``recipes/intel_ndns/spiking_fullsubnet/trainer.py:24-48`` uses it -- same names, arguments
and return values:

* ``freq_MAE(estimation, target)``, ``mag_MAE(estimation, target)``: L1 distances of the 2048-point, hop-512 Hann spectra;
* ``SISNRLoss(return_neg=False)``: scale-invariant SNR in dB, averaged over the rows;
* ``RecipeLoss(sdr_weight=0.001, sdr_offset=100.0)``: the trainer's whole step,
  ``loss = freq_MAE + mag_MAE + 0.001 * (100 - SISNRLoss)``, in ONE kernel call instead of three, with the trainer's dict.

Every call computes the loss AND its gradient with respect to the estimate (two launches, no host synchronisation, deterministic:
include/sfsn.h); ``backward`` only scales the stored gradient.  What the kernel does not cover is refused, never mis-run: CPU
tensors, any dtype but float32, ``win``/``stride`` other than 2048/512, ``srs`` (the per-clip band limits), clips of 1024 samples or
fewer, and a ``target`` that requires a gradient.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import LOSS_FREQ, LOSS_MAG, LOSS_SDR, check

WIN, STRIDE = 2048, 512
_TERM = {LOSS_FREQ: 0, LOSS_MAG: 1, LOSS_SDR: 2}


def _rows(estimation: torch.Tensor, target: torch.Tensor, what: str):
    """The checks every entry point shares; returns both tensors as contiguous [rows, L]."""
    if not isinstance(estimation, torch.Tensor) or not isinstance(target, torch.Tensor):
        raise NotImplementedError(f"{what}: only torch tensors on a HIP device are covered (got {type(estimation).__name__}, "
                                  f"{type(target).__name__}); there is no CPU path")
    if estimation.shape != target.shape:
        raise RuntimeError(f"Dimension mismatch when calculating {what}, input.shape={estimation.shape} vs target.shape={target.shape}")
    if not estimation.is_cuda or not target.is_cuda:
        raise NotImplementedError(f"{what}: CPU tensors are not covered (spiking_fullsubnet_amd has no CPU path); move both to a HIP device")
    if estimation.dtype != torch.float32 or target.dtype != torch.float32:
        raise NotImplementedError(f"{what}: only float32 is covered, got {estimation.dtype} and {target.dtype}")
    if target.requires_grad:
        raise NotImplementedError(f"{what}: only the estimate gets a gradient; a target that requires one is not covered (detach it)")
    if estimation.dim() < 1 or estimation.shape[-1] <= WIN // 2:
        raise NotImplementedError(f"{what}: clips must be longer than {WIN // 2} samples (the reflect padding of the {WIN}-point "
                                  f"frames), got shape {tuple(estimation.shape)}")
    L = estimation.shape[-1]
    return estimation.reshape(-1, L).contiguous(), target.reshape(-1, L).contiguous()


def _spectral_args(what, win, stride, srs):
    if win != WIN or stride != STRIDE:
        raise NotImplementedError(f"{what}: only win={WIN}, stride={STRIDE} (the recipe's) are covered, got win={win}, stride={stride}")
    if srs is not None:
        raise NotImplementedError(f"{what}: srs (per-clip band limits) is not covered; pass srs=None")


class _RecipeLossFn(torch.autograd.Function):
    """(est [rows, L], tgt, c_freq, c_mag, c_sdr, flags, pick, offset) -> (out, terms).  ``terms`` = (freq, mag, sisnr, total) of
    include/sfsn.h, not differentiable.  ``out`` = terms[pick], or with pick None the trainer's
    (freq + mag) + (-c_sdr) * (offset - sisnr); its gradient is the kernel's d total / d est (the constant offset has none)."""

    @staticmethod
    def forward(ctx, est, tgt, c_freq, c_mag, c_sdr, flags, pick, offset):
        rows, L = est.shape
        L_ = _lib.lib()
        nbytes = L_.sfsn_recipe_loss_scratch_bytes(rows, L)
        if nbytes == 0:
            raise NotImplementedError(f"recipe loss: {rows} rows of {L} samples are beyond the kernel's 32-bit indices")
        want_grad = ctx.needs_input_grad[0]
        terms = torch.empty(4, dtype=torch.float32, device=est.device)
        grad = torch.empty_like(est) if want_grad else None
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=est.device)
        with torch.cuda.device(est.device):  # the C ABI launches on the calling thread's current device
            stream = ctypes.c_void_p(torch.cuda.current_stream(est.device).cuda_stream)
            check(L_.sfsn_recipe_loss(est.data_ptr(), tgt.data_ptr(), rows, L, c_freq, c_mag, c_sdr, flags, terms.data_ptr(),
                                      grad.data_ptr() if want_grad else None, scratch.data_ptr(), stream), "sfsn_recipe_loss")
        ctx.stored = grad
        if pick is None:
            out = (terms[0] + terms[1]) + (-c_sdr) * (offset - terms[2])
        else:
            out = terms[pick].clone()
        ctx.mark_non_differentiable(terms)
        return out, terms

    @staticmethod
    def backward(ctx, g_out, _g_terms):
        return (g_out * ctx.stored if ctx.stored is not None else None,) + (None,) * 7


def _single(estimation, target, flag, what, sign=1.0):
    est, tgt = _rows(estimation, target, what)
    w = [0.0, 0.0, 0.0]
    w[_TERM[flag]] = sign
    out, _ = _RecipeLossFn.apply(est, tgt, w[0], w[1], w[2], flag, 3, 0.0)  # total = sign * the one term, exactly
    return out


def freq_MAE(estimation, target, win=2048, stride=512, srs=None, sudo_sr=None):
    """loss.py:138-155 with srs=None: mean |Re E - Re T| + mean |Im E - Im T| over the [-1, L] view's spectra."""
    _spectral_args("freq_MAE", win, stride, srs)
    return _single(estimation, target, LOSS_FREQ, "freq_MAE")


def mag_MAE(estimation, target, win=2048, stride=512, srs=None, sudo_sr=None):
    """loss.py:167-183 with srs=None: mean | |E| - |T| |."""
    _spectral_args("mag_MAE", win, stride, srs)
    return _single(estimation, target, LOSS_MAG, "mag_MAE")


class SISNRLoss(torch.nn.Module):
    """loss.py:11-40: the mean over the rows of 10 log10(|proj|^2 / (|noise|^2 + eps) + eps); ``return_neg`` negates it."""

    def __init__(self, return_neg=False):
        super().__init__()
        self.return_neg = return_neg

    def forward(self, input, target):
        return _single(input, target, LOSS_SDR, "SI-SNR", -1.0 if self.return_neg else 1.0)


class RecipeLoss(torch.nn.Module):
    """The trainer's loss (trainer.py:33-37) in one kernel call: ``forward(enh_y, clean)`` returns
    ``(loss, {"loss", "loss_freq_mae", "loss_mag_mae", "loss_sdr", "loss_sdr_norm"})`` with
    ``loss_sdr_norm = sdr_weight * (sdr_offset - loss_sdr)`` and ``loss = loss_freq_mae + loss_mag_mae + loss_sdr_norm``.
    Only ``loss`` carries a gradient (to ``enh_y``); the components are for logging."""

    def __init__(self, sdr_weight=0.001, sdr_offset=100.0):
        super().__init__()
        self.sdr_weight, self.sdr_offset = float(sdr_weight), float(sdr_offset)

    def forward(self, enh_y, clean):
        est, tgt = _rows(enh_y, clean, "RecipeLoss")
        loss, terms = _RecipeLossFn.apply(est, tgt, 1.0, 1.0, -self.sdr_weight, LOSS_FREQ | LOSS_MAG | LOSS_SDR, None, self.sdr_offset)
        sdr_norm = self.sdr_weight * (self.sdr_offset - terms[2])
        return loss, {"loss": loss, "loss_freq_mae": terms[0], "loss_mag_mae": terms[1], "loss_sdr": terms[2], "loss_sdr_norm": sdr_norm}
