"""The intel_ndns recipe's training loss on the device kernel (``sfsn_recipe_loss``).

Drop-ins for ``audiozen/loss.py`` as ``recipes/intel_ndns/spiking_fullsubnet/trainer.py:24-48`` uses it -- same names, arguments
and return values:

* ``freq_MAE(estimation, target)``, ``mag_MAE(estimation, target)``: L1 distances of the 2048-point, hop-512 Hann spectra;
* ``SISNRLoss(return_neg=False)``: scale-invariant SNR in dB, averaged over the rows;
* ``RecipeLoss(sdr_weight=0.001, sdr_offset=100.0)``: the trainer's whole step,
  ``loss = freq_MAE + mag_MAE + 0.001 * (100 - SISNRLoss)``, in ONE kernel call instead of three, with the trainer's dict.

* ``time_MAE(estimation, target)``: ``F.l1_loss`` of the waveforms, and ``ReverbRecipeLoss()``: the REVERB trainer's step
  (``recipes/reverb/spiking_fullsubnet/trainer.py:34-37``), ``loss = freq_MAE + mag_MAE + F.l1_loss(est_y, ref_y)``, in one kernel call.

Whole utterances (``lengths=``, the companion of ``model.forward_ragged`` and ``PITWrapper(lengths=)``): every entry point takes the
clips' own lengths in one padded batch.  A clip is an element of the leading dimension and all rows of a ``[B, S, L]`` clip share its
length.  ``lengths`` is a sequence or CPU int tensor (checked on the host by ``check_lengths``: one per clip,
``1025 <= L_b <= L``, ``ValueError`` naming the clip; uploaded from pinned memory without a synchronisation) or an int32 ``[B]`` device
tensor (trusted: no host work, the kernel clamps it into the row, so a training step with lengths captures in a graph).  The call is
``sfsn_recipe_loss_ragged``: every row's terms are those of the row alone, a batch term is the mean of the row terms with every row
weighted equally, the gradient is zero past a clip's end and nothing is read there.  ``RecipeLoss.per_clip`` and
``ReverbRecipeLoss.per_clip`` return the per-clip terms for a batched validation loop, left on the device.  With ``lengths=None`` and
no time term the module calls ``sfsn_recipe_loss`` as before.

Every call computes the loss AND its gradient with respect to the estimate (two launches, no host synchronisation, deterministic:
include/sfsn.h); ``backward`` only scales the stored gradient.  What the kernel does not cover is refused, never mis-run: CPU
tensors, any dtype but float32, ``win``/``stride`` other than 2048/512, ``srs`` (the per-clip band limits), clips of 1024 samples or
fewer, and a ``target`` that requires a gradient.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib, ragged
from ._lib import LOSS_FREQ, LOSS_MAG, LOSS_SDR, LOSS_TIME, check

WIN, STRIDE = 2048, 512
_TERM = {LOSS_FREQ: 0, LOSS_MAG: 1, LOSS_SDR: 2, LOSS_TIME: 3}


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


def check_lengths(lengths, batch: int, max_len: int):
    """The clips' lengths in samples as a list of ints (host only).  ``ValueError`` naming the clip for a wrong count, a value that is
    not an integer, ``L_b <= 1024`` (the reflect padding of the 2048-point frames) or ``L_b > max_len`` (the padded length)."""
    lens = ragged._as_ints(lengths, "lengths")
    if len(lens) != batch:
        raise ValueError(f"lengths: expected one length per clip ({batch}), got {len(lens)}")
    for b, n in enumerate(lens):
        if n <= WIN // 2 or n > max_len:
            raise ValueError(f"lengths[{b}] = {n}: clip {b} must have between {WIN // 2 + 1} and {max_len} samples (the padded length)")
    return lens


def _row_lengths(lengths, shape, device):
    """``lengths`` (one per clip, the leading dimension of ``shape``) as the int32 [rows] device tensor the kernel reads."""
    batch = shape[0] if len(shape) > 1 else 1
    per_clip = 1
    for d in shape[1:-1]:
        per_clip *= d
    if torch.is_tensor(lengths) and lengths.is_cuda:
        if lengths.dtype != torch.int32 or tuple(lengths.shape) != (batch,):
            raise ValueError(f"lengths: a device tensor must be int32 of shape [{batch}] (one length per clip), got {lengths.dtype} "
                             f"{tuple(lengths.shape)}")
        if per_clip > 1:
            return lengths.repeat_interleave(per_clip)
        lengths = lengths.contiguous()
        return lengths if lengths.data_ptr() % 16 == 0 else lengths.clone()
    lens = check_lengths(lengths, batch, shape[-1])
    return ragged.upload([n for n in lens for _ in range(per_clip)], device)


def _call_ragged(est, tgt, row_len, c_freq, c_mag, c_sdr, c_time, flags, want_grad, want_rows):
    """One sfsn_recipe_loss_ragged call on contiguous [rows, L] tensors -> (terms [5], row_terms [rows, 4] or None, grad or None)."""
    rows, L = est.shape
    L_ = _lib.lib()
    nbytes = L_.sfsn_recipe_loss_ragged_scratch_bytes(rows, L)
    if nbytes == 0:
        raise NotImplementedError(f"recipe loss: {rows} rows of {L} samples are beyond the kernel's 32-bit indices")
    terms = torch.empty(5, dtype=torch.float32, device=est.device)
    row_terms = torch.empty(rows, 4, dtype=torch.float32, device=est.device) if want_rows else None
    grad = torch.empty_like(est) if want_grad else None
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=est.device)
    ptr = lambda t: t.data_ptr() if t is not None else None
    with torch.cuda.device(est.device):  # the C ABI launches on the calling thread's current device
        stream = ctypes.c_void_p(torch.cuda.current_stream(est.device).cuda_stream)
        check(L_.sfsn_recipe_loss_ragged(est.data_ptr(), tgt.data_ptr(), rows, L, ptr(row_len), c_freq, c_mag, c_sdr, c_time, flags,
                                         terms.data_ptr(), ptr(row_terms), ptr(grad), scratch.data_ptr(), stream), "sfsn_recipe_loss_ragged")
    return terms, row_terms, grad


class _RecipeLossFn(torch.autograd.Function):
    """(est [rows, L], tgt, c_freq, c_mag, c_sdr, c_time, flags, pick, offset, row_len) -> (out, terms).  ``terms`` is not
    differentiable: (freq, mag, sisnr, total) of sfsn_recipe_loss, or -- with row_len (int32 [rows] on the device) or the time term --
    (freq, mag, sisnr, time, total) of sfsn_recipe_loss_ragged (include/sfsn.h).  ``out`` = terms[pick], or with pick None the
    trainer's (freq + mag) + (-c_sdr) * (offset - sisnr); its gradient is the kernel's d total / d est (the constant offset has none)."""

    @staticmethod
    def forward(ctx, est, tgt, c_freq, c_mag, c_sdr, c_time, flags, pick, offset, row_len):
        if row_len is not None or flags & LOSS_TIME:
            terms, _, ctx.stored = _call_ragged(est, tgt, row_len, c_freq, c_mag, c_sdr, c_time, flags, ctx.needs_input_grad[0], False)
            out = (terms[0] + terms[1]) + (-c_sdr) * (offset - terms[2]) if pick is None else terms[pick].clone()
            ctx.mark_non_differentiable(terms)
            return out, terms
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
        return (g_out * ctx.stored if ctx.stored is not None else None,) + (None,) * 9


def _single(estimation, target, flag, what, sign=1.0, lengths=None):
    est, tgt = _rows(estimation, target, what)
    row_len = None if lengths is None else _row_lengths(lengths, estimation.shape, est.device)
    w = [0.0, 0.0, 0.0, 0.0]
    w[_TERM[flag]] = sign
    out, _ = _RecipeLossFn.apply(est, tgt, *w, flag, -1, 0.0, row_len)  # total = sign * the one term, exactly
    return out


def freq_MAE(estimation, target, win=2048, stride=512, srs=None, sudo_sr=None, lengths=None):
    """loss.py:138-155 with srs=None: mean |Re E - Re T| + mean |Im E - Im T| over the [-1, L] view's spectra."""
    _spectral_args("freq_MAE", win, stride, srs)
    return _single(estimation, target, LOSS_FREQ, "freq_MAE", lengths=lengths)


def mag_MAE(estimation, target, win=2048, stride=512, srs=None, sudo_sr=None, lengths=None):
    """loss.py:167-183 with srs=None: mean | |E| - |T| |."""
    _spectral_args("mag_MAE", win, stride, srs)
    return _single(estimation, target, LOSS_MAG, "mag_MAE", lengths=lengths)


def time_MAE(estimation, target, lengths=None):
    """``F.l1_loss(estimation, target)`` as the REVERB trainer uses it; with ``lengths`` the mean over the rows of each row's own
    mean over its clip's samples."""
    return _single(estimation, target, LOSS_TIME, "time_MAE", lengths=lengths)


class SISNRLoss(torch.nn.Module):
    """loss.py:11-40: the mean over the rows of 10 log10(|proj|^2 / (|noise|^2 + eps) + eps); ``return_neg`` negates it."""

    def __init__(self, return_neg=False):
        super().__init__()
        self.return_neg = return_neg

    def forward(self, input, target, lengths=None):
        return _single(input, target, LOSS_SDR, "SI-SNR", -1.0 if self.return_neg else 1.0, lengths)


@torch.no_grad()
def _per_clip_terms(enh_y, clean, lengths, what, c, flags):
    """[B, 4] device tensor: each clip's (freq, mag, sisnr, time), the mean over the clip's rows; forward only, nothing read back."""
    est, tgt = _rows(enh_y, clean, what)
    row_len = None if lengths is None else _row_lengths(lengths, enh_y.shape, est.device)
    _, row_terms, _ = _call_ragged(est, tgt, row_len, *c, flags, False, True)
    batch = enh_y.shape[0] if enh_y.dim() > 1 else 1
    return row_terms.view(batch, -1, 4).mean(1)


class RecipeLoss(torch.nn.Module):
    """The trainer's loss (trainer.py:33-37) in one kernel call: ``forward(enh_y, clean, lengths=None)`` returns
    ``(loss, {"loss", "loss_freq_mae", "loss_mag_mae", "loss_sdr", "loss_sdr_norm"})`` with
    ``loss_sdr_norm = sdr_weight * (sdr_offset - loss_sdr)`` and ``loss = loss_freq_mae + loss_mag_mae + loss_sdr_norm``.
    Only ``loss`` carries a gradient (to ``enh_y``); the components are for logging.  ``per_clip(enh_y, clean, lengths)`` returns the
    same keys as ``[B]`` device tensors, one value per clip, without a gradient."""

    def __init__(self, sdr_weight=0.001, sdr_offset=100.0):
        super().__init__()
        self.sdr_weight, self.sdr_offset = float(sdr_weight), float(sdr_offset)

    def forward(self, enh_y, clean, lengths=None):
        est, tgt = _rows(enh_y, clean, "RecipeLoss")
        row_len = None if lengths is None else _row_lengths(lengths, enh_y.shape, est.device)
        loss, terms = _RecipeLossFn.apply(est, tgt, 1.0, 1.0, -self.sdr_weight, 0.0, LOSS_FREQ | LOSS_MAG | LOSS_SDR, None, self.sdr_offset,
                                          row_len)
        sdr_norm = self.sdr_weight * (self.sdr_offset - terms[2])
        return loss, {"loss": loss, "loss_freq_mae": terms[0], "loss_mag_mae": terms[1], "loss_sdr": terms[2], "loss_sdr_norm": sdr_norm}

    def per_clip(self, enh_y, clean, lengths=None):
        t = _per_clip_terms(enh_y, clean, lengths, "RecipeLoss", (1.0, 1.0, -self.sdr_weight, 0.0), LOSS_FREQ | LOSS_MAG | LOSS_SDR)
        sdr_norm = self.sdr_weight * (self.sdr_offset - t[:, 2])
        return {"loss": (t[:, 0] + t[:, 1]) + sdr_norm, "loss_freq_mae": t[:, 0], "loss_mag_mae": t[:, 1], "loss_sdr": t[:, 2],
                "loss_sdr_norm": sdr_norm}


class ReverbRecipeLoss(torch.nn.Module):
    """The REVERB trainer's loss (recipes/reverb/spiking_fullsubnet/trainer.py:34-37) in one kernel call:
    ``forward(est_y, ref_y, lengths=None)`` returns ``(loss, {"loss", "loss_freq_mae", "loss_mag_mae", "loss_time_mae"})`` with
    ``loss = loss_freq_mae + loss_mag_mae + loss_time_mae``.  Only ``loss`` carries a gradient (to ``est_y``).
    ``per_clip(est_y, ref_y, lengths)`` returns the same keys as ``[B]`` device tensors, without a gradient."""

    _C, _FLAGS = (1.0, 1.0, 0.0, 1.0), LOSS_FREQ | LOSS_MAG | LOSS_TIME

    def forward(self, est_y, ref_y, lengths=None):
        est, tgt = _rows(est_y, ref_y, "ReverbRecipeLoss")
        row_len = None if lengths is None else _row_lengths(lengths, est_y.shape, est.device)
        loss, terms = _RecipeLossFn.apply(est, tgt, *self._C, self._FLAGS, -1, 0.0, row_len)  # the kernel's total: (freq + mag) + time
        return loss, {"loss": loss, "loss_freq_mae": terms[0], "loss_mag_mae": terms[1], "loss_time_mae": terms[3]}

    def per_clip(self, est_y, ref_y, lengths=None):
        t = _per_clip_terms(est_y, ref_y, lengths, "ReverbRecipeLoss", self._C, self._FLAGS)
        return {"loss": (t[:, 0] + t[:, 1]) + t[:, 3], "loss_freq_mae": t[:, 0], "loss_mag_mae": t[:, 1], "loss_time_mae": t[:, 3]}
