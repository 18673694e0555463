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
"""
from __future__ import annotations

import ctypes
from itertools import permutations

import torch

from . import _lib
from ._lib import check

MAX_SOURCES = 4


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


def _call(est, ref, zero_mean, eps, pair_cot, want_grad, want_rest):
    """One sfsn_pit_sdr call on contiguous [B, S, L] tensors -> (pair, perm, loss, grad, reordered); those not asked for are None.
    want_rest: False (pairwise mode, or no use for them), "scalars" (perm and loss, which PIT mode requires) or "all" (and reordered)."""
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
    with torch.cuda.device(dev):  # the C ABI launches on the calling thread's current device
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        check(L_.sfsn_pit_sdr(est.data_ptr(), ref.data_ptr(), B, S, L, 1 if zero_mean else 0, float(eps), ptr(pair_cot), pair.data_ptr(),
                              ptr(perm), ptr(loss), ptr(grad), ptr(reordered), scratch.data_ptr(), stream), "sfsn_pit_sdr")
    return pair, perm, loss, grad, reordered


class _PairwiseFn(torch.autograd.Function):
    """(est, ref, zero_mean, eps) -> pair [B, S, S]; backward is a second kernel call in pairwise mode with the incoming cotangent."""

    @staticmethod
    def forward(ctx, est, ref, zero_mean, eps):
        ctx.save_for_backward(est, ref)
        ctx.args = (zero_mean, eps)
        return _call(est, ref, zero_mean, eps, None, False, "scalars")[0]

    @staticmethod
    def backward(ctx, g_pair):
        est, ref = ctx.saved_tensors
        cot = g_pair.to(torch.float32).contiguous()
        grad = _call(est, ref, ctx.args[0], ctx.args[1], cot, True, False)[3]
        return grad, None, None, None


class _PitFn(torch.autograd.Function):
    """(est, ref, zero_mean, eps) -> (mean_loss, reordered, perm, pair); only mean_loss is differentiable (to est)."""

    @staticmethod
    def forward(ctx, est, ref, zero_mean, eps):
        pair, perm, loss, grad, reordered = _call(est, ref, zero_mean, eps, None, ctx.needs_input_grad[0], "all")
        ctx.stored = grad
        perm = perm.to(torch.int64)
        ctx.mark_non_differentiable(reordered, perm, pair)
        return loss.reshape(()), reordered, perm, pair

    @staticmethod
    def backward(ctx, g_loss, *_):
        return (g_loss * ctx.stored if ctx.stored is not None else None), None, None, None


class PairwiseNegSDR:
    """pit.py:6-56: ``-10 log10(|proj|^2 / (|noise|^2 + EPS) + EPS)`` of every (estimate, reference) pair of a clip."""

    def __init__(self, zero_mean=True, EPS=1e-8):
        self.zero_mean = zero_mean
        self.EPS = EPS

    def __call__(self, est, ref):
        est, ref = _inputs(est, ref, "PairwiseNegSDR")
        return _PairwiseFn.apply(est, ref, bool(self.zero_mean), float(self.EPS))


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

    def full(self, est, ref):
        """(mean_loss, reordered, perm [B, S] int64, pair [B, S, S]) from one kernel call; only mean_loss carries a gradient."""
        est, ref = _inputs(est, ref, "PITWrapper")
        return _PitFn.apply(est, ref, bool(self.loss_func.zero_mean), float(self.loss_func.EPS))

    def __call__(self, est, ref, **kwargs):
        if kwargs:
            raise NotImplementedError(f"PITWrapper: extra keyword arguments are not covered ({sorted(kwargs)}): PairwiseNegSDR takes none")
        mean_loss, reordered, _, _ = self.full(est, ref)
        return mean_loss, reordered
