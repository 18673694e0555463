"""The two energy proxies the recipes log next to the audio metrics, for the outputs of this package's modules.

Drop-ins for ``audiozen.metric.compute_synops`` / ``compute_neuronops`` (audiozen/metric.py:303-340; called at
recipes/intel_ndns/spiking_fullsubnet_freeze_phase/trainer.py:130-135 with the module's ``all_layer_outputs`` lists).
Each list is ``[layer input, spikes of layer 1, ..., spikes of layer L, projection]``; the reference reads, per spike
entry, its firing rate and its last dimension.  Entries may be the fp32 spike tensors (``layer_outputs="tensors"``,
the module default) or ``SpikeSummary`` objects (``layer_outputs="counts"``): exact device-side counts of the int8 spikes
the scan already writes, so the 4 B/spike tensors never exist.

``SISDR`` is the drop-in for ``audiozen.metric.SISDR`` (metric.py:67-101), the wsj0-mix, intel_ndns and REVERB trainers'
``north_star_metric``, on HIP tensors: rows are scored as given (no permutation search), optionally with the clips' own lengths in a
padded batch, by the kernel that scores ragged batches (``sfsn_pit_sdr_ragged``).
"""
from __future__ import annotations

import torch

from .engine import SpikeSummary


class SISDR:
    """``SISDR()(estimate, target, reduce_mean=True, lengths=None)``: the SI-SDR in dB of every row of ``estimate`` against the same
    row of ``target`` -- float32 tensors ``[L]``, ``[S, L]`` or ``[B, S, L]`` on a HIP device.  ``reduce_mean=True`` returns
    ``{"si_sdr": float}``, the mean over the rows as the reference returns it (one host read, the only one); ``reduce_mean=False``
    returns ``{"si_sdr": tensor}`` of the leading shape, left on the device.  ``lengths``: the clips' own lengths when the last
    dimension is padded -- one per clip (``[B]``; one value for ``[L]`` and ``[S, L]``), as ``pit.PITWrapper`` takes them; what lies
    past a clip's end is never read.  Every row is a one-source clip to the kernel, so there is no search and rows match as given."""

    def __call__(self, estimate, target, reduce_mean=True, lengths=None):
        from . import pit
        if not isinstance(estimate, torch.Tensor) or not isinstance(target, torch.Tensor):
            raise NotImplementedError(f"SISDR: only torch tensors on a HIP device are covered (got {type(estimate).__name__}, "
                                      f"{type(target).__name__}); there is no CPU path")
        if estimate.shape != target.shape or not 1 <= estimate.ndim <= 3:
            raise TypeError(f"SISDR: inputs must both be [L], [S, L] or [B, S, L], got {tuple(estimate.shape)} and {tuple(target.shape)}")
        lead = estimate.shape[:-1]
        n = estimate.shape[-1]
        clips = lead[0] if estimate.ndim == 3 else 1
        rows_per_clip = lead[-1] if estimate.ndim >= 2 else 1
        est, ref = pit._inputs(estimate.detach().reshape(-1, 1, n), target.detach().reshape(-1, 1, n), "SISDR")
        if lengths is not None and not torch.is_tensor(lengths) and not hasattr(lengths, "__len__"):
            lengths = [lengths]
        clip_len = pit.device_lengths(lengths, clips, n, est.device)
        if clip_len is None:
            clip_len = torch.full((est.shape[0],), n, dtype=torch.int32, device=est.device)
        elif rows_per_clip > 1:
            clip_len = clip_len.repeat_interleave(rows_per_clip)
        with torch.no_grad():
            val = pit._call(est, ref, True, 1e-8, None, False, "scalars", clip_len, per_clip=True)[6].reshape(lead)
        if reduce_mean:
            return {"si_sdr": val.mean().item()}
        return {"si_sdr": val}


def _rate(x) -> torch.Tensor:
    if isinstance(x, SpikeSummary):
        return x.rate()
    return torch.gt(x, 0).float().mean()  # audiozen/metric.py:306


def compute_synops(fb_all_layer_outputs, sb_all_layer_outputs, shared_weights=True) -> float:
    """sum over spike layers of rate * H * (fan_out + H), fp32 arithmetic as in the reference; doubled for unshared gates."""
    synops = 0.0
    for outs in [fb_all_layer_outputs] + list(sb_all_layer_outputs):
        for i in range(1, len(outs) - 1):
            synops = synops + _rate(outs[i]) * outs[i].size(-1) * (outs[i + 1].size(-1) + outs[i].size(-1))
    synops = float(synops.item()) if isinstance(synops, torch.Tensor) else float(synops)
    return synops if shared_weights else 2 * synops


def compute_neuronops(fb_all_layer_outputs, sb_all_layer_outputs) -> float:
    """audiozen/metric.py:330-340: the sum of the last dimensions of every entry."""
    n = 0.0
    for outs in [fb_all_layer_outputs] + list(sb_all_layer_outputs):
        for o in outs:
            n += o.size(-1)
    return n
