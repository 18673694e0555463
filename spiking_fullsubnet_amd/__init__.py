"""MI355X-native implementation of Spiking-FullSubNet's recurrent inference hot path.

Drop-in modules (same constructor keywords, state-dict names and forward() tuples as the reference):

* ``spiking_fullsubnet_amd.modeling_spiking_fullsubnet.SpikingFullSubNet``  (live recipes)
* ``spiking_fullsubnet_amd.model_low_freq.Separator``                        (frozen recipe / model_zoo checkpoints)
* ``spiking_fullsubnet_amd.modeling_cirm_gsn.Model``                         (the cIRM-GSN baseline recipe)

The intel_ndns recipe's training loss (``freq_MAE``, ``mag_MAE``, ``SISNRLoss`` and the fused ``RecipeLoss``) is in
``spiking_fullsubnet_amd.loss``, with the REVERB recipe's ``ReverbRecipeLoss`` (``time_MAE`` as its third term) and per-clip ``lengths=``
on every entry point; the wsj0-mix recipes' permutation-invariant SI-SDR loss (``PITWrapper(PairwiseNegSDR())``) is in
``spiking_fullsubnet_amd.pit``.  Clips of different lengths run in one forward with ``model.forward_ragged(waves, lengths)``
(``spiking_fullsubnet_amd.ragged``), each bit-identical to the clip run alone, and are scored in one call with
``PITWrapper.per_clip(est, ref, lengths)`` and ``metric.SISDR`` (per-clip permutation, loss and SI-SDR, left on the device).

All compute between ``stft`` and ``istft`` runs in hand-written gfx950 kernels behind the C ABI of
``include/sfsn.h`` (``csrc/libsfsn_hip.so``).  There is no CPU fallback.
"""
from . import _lib  # noqa: F401
from .engine import Engine, PathSpec, SpikeSummary  # noqa: F401
from . import checkpoint, metric  # noqa: F401
from .model_low_freq import Separator  # noqa: F401
from .modeling_spiking_fullsubnet import SpikingFullSubNet  # noqa: F401
from .modeling_cirm_gsn import Model  # noqa: F401
from .streaming import StreamingSession  # noqa: F401
from .clip_state import ClipState  # noqa: F401
from . import loss  # noqa: F401
from .loss import RecipeLoss, ReverbRecipeLoss  # noqa: F401
from . import pit  # noqa: F401
from . import ragged  # noqa: F401
from .pit import PITWrapper, PairwiseNegSDR, PerClip  # noqa: F401
from .metric import SISDR  # noqa: F401

__all__ = ["SpikingFullSubNet", "Separator", "Engine", "PathSpec", "StreamingSession", "Model", "RecipeLoss", "loss", "pit", "PITWrapper",
           "PairwiseNegSDR", "PerClip", "SISDR", "metric", "ragged", "ReverbRecipeLoss", "ClipState"]
