"""The wsj0-mix recipes' training loss on the device kernel (``sfsn_pit_sdr``).

Drop-ins for ``audiozen/pit.py`` as ``recipes/wsj0-mix/spiking_fullsubnet/trainer.py:24-33`` uses it -- same names, arguments and
return values:

* ``PairwiseNegSDR(zero_mean=True, EPS=1e-8)``: ``__call__(est, ref)`` returns the pairwise negative SI-SDR ``[B, S, S]`` (dim 1 the
  estimates, dim 2 the references);
* ``PITWrapper(loss_func)``: ``__call__(est, ref)`` returns ``(mean_loss, reordered)`` from ONE kernel call (pairwise losses, the
  search over the permutations, the mean, the reordered estimates and the gradient); ``full(est, ref)`` adds the chosen permutation
  and the pairwise losses for logging.

Every call computes its gradient with respect to ``est`` when one is asked for (two launches, no host synchronisation, deterministic:
include/sfsn.h), so ``training.GraphedTrainStep`` captures it; ``backward`` only scales the stored gradient (``PairwiseNegSDR``: a
second kernel call with the incoming cotangent).  What the kernel does not cover is refused, never mis-run: CPU tensors, any dtype but
float32, a ``ref`` that requires a gradient, more than 4 sources, a ``loss_func`` that is not this module's ``PairwiseNegSDR``, extra
keyword arguments.  ``reordered`` is NOT differentiable here (in the reference it is; its trainers never use that): it is marked so,
and a loss built on it raises in autograd instead of losing the gradient silently.

Ragged batches (``lengths=``, the companion of ``model.forward_ragged``): ``est`` and ``ref`` are one padded batch ``[B, S, L]`` and
clip b is its samples ``[0, L_b)``; what lies past a clip's end is never read.  Every entry point takes ``lengths`` -- a sequence or
CPU int tensor (checked on the host: one per clip, ``2 <= L_b <= L``, ``ValueError`` naming the clip; uploaded without a
synchronisation) or an int32 ``[B]`` device tensor (trusted as it is: no host work, so a training step with lengths captures in a
graph) -- and runs ``sfsn_pit_sdr_ragged``: each clip's ``pair``, ``perm`` and loss have the bits of the call on that clip alone, the
mean loss weighs every clip equally, ``reordered`` and the gradient are zero past a clip's end.  ``PITWrapper.per_clip`` is the
evaluation loops' call: per-clip loss, permutation, pairwise losses, reordered estimates and ``audiozen.metric.SISDR`` of the matched
rows from one forward-only call, all left on the device.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple
from itertools import permutations

import torch

from . import _lib, ragged
from ._lib import check

MAX_SOURCES = 4
PerClip = namedtuple("PerClip", "loss perm pair reordered si_sdr")  # [B], [B, S] int64, [B, S, S], [B, S, L], [B, S]; all on the device


def _inputs(est, ref, what: str):
    """The checks both entry points share; returns both tensors as contiguous [B, S, L]."""
    if not isinstance(est, torch.Tensor) or not isinstance(ref, torch.Tensor):
        raise NotImplementedError(f"{what}: only torch tensors on a HIP device are covered (got {type(est).__name__}, "
                                  f"{type(ref).__name__}); there is no CPU path")
    if ref.shape != est.shape or ref.ndim != 3:
        raise TypeError(f"Inputs must be of shape [batch, n_src, time], got {ref.shape} and {est.shape} instead")
    if not est.is_cuda or not ref.is_cuda:
        raise NotImplementedError(f"{what}: CPU tensors are not covered (spiking_fullsubnet_amd has no CPU path); move both to a HIP device")
    if est.dtype != torch.float32 or ref.dtype != torch.float32:
        raise NotImplementedError(f"{what}: only float32 is covered, got {est.dtype} and {ref.dtype}")
    if ref.requires_grad:
        raise NotImplementedError(f"{what}: only the estimate gets a gradient; a ref that requires one is not covered (detach it)")
    if est.shape[1] > MAX_SOURCES:
        raise NotImplementedError(f"{what}: at most {MAX_SOURCES} sources are covered, got {est.shape[1]}")
    if est.shape[0] < 1 or est.shape[1] < 1 or est.shape[2] < 2:
        raise NotImplementedError(f"{what}: at least one clip, one source and two samples are needed, got shape {tuple(est.shape)}")
    # non-contiguous views are copied; so is a contiguous view whose first element is not 16-byte aligned (the C ABI asks for that)
    est, ref = est.contiguous(), ref.contiguous()
    return (est if est.data_ptr() % 16 == 0 else est.clone()), (ref if ref.data_ptr() % 16 == 0 else ref.clone())


def device_lengths(lengths, batch: int, max_len: int, device, what: str = "lengths"):
    """``lengths`` as the int32 [batch] device tensor the kernel reads, or None for None.  A sequence or CPU int tensor is checked on
    the host (one per clip, ``2 <= L_b <= max_len``; ``ValueError`` naming the clip) and uploaded from pinned memory; a device tensor
    must be int32 of shape [batch] and is trusted (no host work: the kernel clamps it into the row)."""
    if lengths is None:
        return None
    if torch.is_tensor(lengths) and lengths.is_cuda:
        if lengths.dtype != torch.int32 or tuple(lengths.shape) != (batch,):
            raise ValueError(f"{what}: a device tensor must be int32 of shape [{batch}] (one length per clip), got {lengths.dtype} "
                             f"{tuple(lengths.shape)}")
        lengths = lengths.contiguous()
        return lengths if lengths.data_ptr() % 16 == 0 else lengths.clone()
    lens = ragged._as_ints(lengths, what)
    if len(lens) != batch:
        raise ValueError(f"{what}: expected one length per clip ({batch}), got {len(lens)}")
    for b, n in enumerate(lens):
        if n < 2 or n > max_len:
            raise ValueError(f"{what}[{b}] = {n}: clip {b} must have between 2 and {max_len} samples (the padded length)")
    return ragged.upload(lens, device)


def _call(est, ref, zero_mean, eps, pair_cot, want_grad, want_rest, clip_len=None, per_clip=False):
    """One kernel call on contiguous [B, S, L] tensors -> (pair, perm, loss, grad, reordered); those not asked for are None.
    want_rest: False (pairwise mode, or no use for them), "scalars" (perm and loss, which PIT mode requires) or "all" (and reordered).
    clip_len None: sfsn_pit_sdr.  An int32 [B] device tensor: sfsn_pit_sdr_ragged; per_clip then appends (clip_loss, si_sdr)."""
    B, S, L = est.shape
    L_ = _lib.lib()
    nbytes = L_.sfsn_pit_sdr_scratch_bytes(B, S, L)
    if nbytes == 0:
        raise NotImplementedError(f"PIT loss: {B} x {S} x {L} samples are beyond the kernel's 32-bit indices")
    dev = est.device
    pair = torch.empty(B, S, S, dtype=torch.float32, device=dev)
    perm = torch.empty(B, S, dtype=torch.int32, device=dev) if want_rest else None
    loss = torch.empty(1, dtype=torch.float32, device=dev) if want_rest else None
    reordered = torch.empty_like(est) if want_rest == "all" else None
    grad = torch.empty_like(est) if want_grad else None
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None else None
    if clip_len is not None:
        clip_loss = torch.empty(B, dtype=torch.float32, device=dev) if per_clip else None
        si_sdr = torch.empty(B, S, dtype=torch.float32, device=dev) if per_clip else None
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            check(L_.sfsn_pit_sdr_ragged(est.data_ptr(), ref.data_ptr(), B, S, L, clip_len.data_ptr(), 1 if zero_mean else 0, float(eps),
                                         ptr(pair_cot), pair.data_ptr(), ptr(perm), ptr(clip_loss), ptr(loss), ptr(grad), ptr(reordered),
                                         ptr(si_sdr), scratch.data_ptr(), stream), "sfsn_pit_sdr_ragged")
        return (pair, perm, loss, grad, reordered) + ((clip_loss, si_sdr) if per_clip else ())
    with torch.cuda.device(dev):  # the C ABI launches on the calling thread's current device
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        check(L_.sfsn_pit_sdr(est.data_ptr(), ref.data_ptr(), B, S, L, 1 if zero_mean else 0, float(eps), ptr(pair_cot), pair.data_ptr(),
                              ptr(perm), ptr(loss), ptr(grad), ptr(reordered), scratch.data_ptr(), stream), "sfsn_pit_sdr")
    return pair, perm, loss, grad, reordered


class _PairwiseFn(torch.autograd.Function):
    """(est, ref, zero_mean, eps, clip_len) -> pair [B, S, S]; backward is a second kernel call in pairwise mode with the incoming
    cotangent.  clip_len: None or the int32 [B] device tensor of a ragged batch."""

    @staticmethod
    def forward(ctx, est, ref, zero_mean, eps, clip_len):
        ctx.save_for_backward(est, ref)
        ctx.args = (zero_mean, eps, clip_len)
        return _call(est, ref, zero_mean, eps, None, False, "scalars", clip_len)[0]

    @staticmethod
    def backward(ctx, g_pair):
        est, ref = ctx.saved_tensors
        cot = g_pair.to(torch.float32).contiguous()
        grad = _call(est, ref, ctx.args[0], ctx.args[1], cot, True, False, ctx.args[2])[3]
        return grad, None, None, None, None


class _PitFn(torch.autograd.Function):
    """(est, ref, zero_mean, eps, clip_len) -> (mean_loss, reordered, perm, pair); only mean_loss is differentiable (to est)."""

    @staticmethod
    def forward(ctx, est, ref, zero_mean, eps, clip_len):
        pair, perm, loss, grad, reordered = _call(est, ref, zero_mean, eps, None, ctx.needs_input_grad[0], "all", clip_len)
        ctx.stored = grad
        perm = perm.to(torch.int64)
        ctx.mark_non_differentiable(reordered, perm, pair)
        return loss.reshape(()), reordered, perm, pair

    @staticmethod
    def backward(ctx, g_loss, *_):
        return (g_loss * ctx.stored if ctx.stored is not None else None), None, None, None, None


class PairwiseNegSDR:
    """pit.py:6-56: ``-10 log10(|proj|^2 / (|noise|^2 + EPS) + EPS)`` of every (estimate, reference) pair of a clip."""

    def __init__(self, zero_mean=True, EPS=1e-8):
        self.zero_mean = zero_mean
        self.EPS = EPS

    def __call__(self, est, ref, lengths=None):
        est, ref = _inputs(est, ref, "PairwiseNegSDR")
        clip_len = device_lengths(lengths, est.shape[0], est.shape[2], est.device)
        return _PairwiseFn.apply(est, ref, bool(self.zero_mean), float(self.EPS), clip_len)


class PITWrapper:
    """pit.py:59-124 around this module's ``PairwiseNegSDR``: the mean over the clips of the smallest permutation loss, and the
    estimates reordered by the best permutation (first minimum on a tie)."""

    def __init__(self, loss_func):
        if not isinstance(loss_func, PairwiseNegSDR):
            raise NotImplementedError(f"PITWrapper: only this module's PairwiseNegSDR is covered as loss_func (the search runs inside its "
                                      f"kernel), got {type(loss_func).__name__}")
        self.loss_func = loss_func

    @staticmethod
    def find_best_perm(pair_wise_losses):
        """pit.py:63-94 on a [B, S, S] tensor: (min_loss [B], batch_indices [B, S]); torch.min returns the first minimum on a tie.
        A small torch helper for logging, not on the training path (the kernel runs its own search)."""
        S = pair_wise_losses.shape[1]
        perms = torch.tensor(list(permutations(range(S))), dtype=torch.long, device=pair_wise_losses.device)  # [S!, S]
        picked = pair_wise_losses[:, perms, torch.arange(S, device=perms.device)]  # [B, S!, S]: pair[b, p[j], j]
        min_loss, idx = torch.min(picked.sum(-1) / S, dim=1)
        return min_loss, perms[idx]

    @staticmethod
    def reorder_source(source, batch_indices):
        """pit.py:96-106: source [B, S, L] gathered along dim 1 by batch_indices [B, S]."""
        return torch.gather(source, 1, batch_indices[:, :, None].expand(-1, -1, source.shape[2]))

    def full(self, est, ref, lengths=None):
        """(mean_loss, reordered, perm [B, S] int64, pair [B, S, S]) from one kernel call; only mean_loss carries a gradient.
        ``lengths``: the clips' own lengths in a padded batch (module docstring); mean_loss weighs every clip equally."""
        est, ref = _inputs(est, ref, "PITWrapper")
        clip_len = device_lengths(lengths, est.shape[0], est.shape[2], est.device)
        return _PitFn.apply(est, ref, bool(self.loss_func.zero_mean), float(self.loss_func.EPS), clip_len)

    @torch.no_grad()
    def per_clip(self, est, ref, lengths=None):
        """Forward only, one kernel call, nothing read back: ``PerClip(loss [B], perm [B, S] int64, pair [B, S, S], reordered [B, S, L],
        si_sdr [B, S])`` -- each clip's smallest permutation loss and ``audiozen.metric.SISDR`` of reference j against its matched
        estimate.  ``lengths=None``: every clip has the full length."""
        est, ref = _inputs(est, ref, "PITWrapper")
        B, S, L = est.shape
        clip_len = device_lengths(lengths, B, L, est.device)
        if clip_len is None:
            clip_len = torch.full((B,), L, dtype=torch.int32, device=est.device)
        pair, perm, _, _, reordered, clip_loss, si_sdr = _call(est, ref, bool(self.loss_func.zero_mean), float(self.loss_func.EPS), None, False,
                                                               "all", clip_len, per_clip=True)
        return PerClip(clip_loss, perm.to(torch.int64), pair, reordered, si_sdr)

    def __call__(self, est, ref, lengths=None, **kwargs):
        if kwargs:
            raise NotImplementedError(f"PITWrapper: extra keyword arguments are not covered ({sorted(kwargs)}): PairwiseNegSDR takes none")
        mean_loss, reordered, _, _ = self.full(est, ref, lengths)
        return mean_loss, reordered
