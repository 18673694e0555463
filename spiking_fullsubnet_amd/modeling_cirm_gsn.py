"""Drop-in for ``audiozen.models.cirm_gsn.modeling_cirm_gsn.Model``, the cIRM-GSN baseline of the Intel N-DNS challenge recipes
(``recipes/intel_ndns/cirm_gsn/default.toml``).

Same constructor keywords and defaults (modeling_cirm_gsn.py:162-204), same state-dict names (``fb_model`` is this package's
``modeling_spiking_fullsubnet.SequenceModel``), same initialisation under a fixed seed and the same ``forward(input[B, samples])``
return values (:206-245).  A recipe switches over by changing only

    [model]
    path = "spiking_fullsubnet_amd.modeling_cirm_gsn.Model"

In ``eval()`` mode a GSN model runs everything between ``stft`` and ``istft`` on the gfx950 kernels through ``FullbandEngine``; an
LSTM model runs its sequence model on ATen (``training.sequence_model``) and the deep filter as torch operations.  ``streaming()``
opens a frame-by-frame session of a GSN model (``fullband_streaming.py``); ``forward_ragged(waves, lengths)`` runs a padded batch of
clips of different lengths, every clip as if it ran alone (``ragged.py``).  Spike counts for SynOPs: ``layer_outputs = "counts"``
(the two-speaker ``forward``), ``forward_stft(want_counts=True)`` and ``streaming(count_spikes=True)`` + ``session.spike_summary``.

In ``train()`` mode -- or in ``eval()`` mode with grad enabled and an input that requires grad (or ``autograd_in_eval = True``) --
``forward()`` takes the differentiable path ``training.forward_cirm``: the GSN stack on the one-launch training layer calls of
``csrc/sfsn_train.hip`` (a hidden size that is not a multiple of 16, the recipe's 268, padded to the next one with silent neurons:
``training.PaddedStack``), the deep filter and its backward as one HIP launch each
(``csrc/sfsn_fullband_train.hip``), the rest as ATen operations.  HIP tensors only: on CPU tensors that path raises
``NotImplementedError``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .fullband_engine import FullbandEngine, FullbandSpec, activation_code
from .modeling_spiking_fullsubnet import SequenceModel, _EngineMixin


def deep_filter_torch(cmp: torch.Tensor, coef: torch.Tensor, df: int, S: int) -> torch.Tensor:
    """deepfiltering (modeling_cirm_gsn.py:125-157) with the coefficients in the projection's column order:
    cmp complex [B, F, T], coef [B, 2 df S F, T] -> [B, S, F, T], Y[f, t] = sum_d X[f, t - (df - 1) + d] C[d]."""
    B, F, T = cmp.shape
    c = coef.reshape(B, 2, df, S, F, T)
    cc = torch.complex(c[:, 0], c[:, 1])                                          # [B, df, S, F, T]
    taps = torch.nn.functional.pad(cmp, (df - 1, 0)).unfold(2, T, 1).permute(0, 2, 1, 3)  # [B, df, F, T]
    return (taps[:, :, None] * cc).sum(1)


class Model(_EngineMixin, nn.Module):
    def __init__(self, n_fft, hop_length, win_length, fdrc, input_size, hidden_size, num_layers, proj_size, output_activate_function,
                 df_order, use_pre_layer_norm_fb=True, bn=False, shared_weights=False, sequence_model="LSTM", num_spks=2):
        super().__init__()
        self.fb_model = SequenceModel(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers,
                                      shared_weights=shared_weights, sequence_model=sequence_model,
                                      proj_size=proj_size * num_spks * df_order * 2, output_activate_function=output_activate_function,
                                      bn=bn, use_pre_layer_norm=use_pre_layer_norm_fb)
        self.fb_input_size, self.n_fft, self.hop_length, self.win_length = input_size, n_fft, hop_length, win_length
        self.fdrc, self.df_order, self.num_spks = fdrc, df_order, num_spks
        F = n_fft // 2 + 1
        if input_size != F or proj_size != F:
            # the reference feeds all F bins to the model and re-indexes its output as (c d s f) over F bins (:220-230): any other
            # size fails there inside einops; refuse up front
            raise ValueError(f"input_size ({input_size}) and proj_size ({proj_size}) must both equal n_fft // 2 + 1 = {F}")
        self._fb_spec = FullbandSpec(n_fft=n_fft, fdrc=float(fdrc), hidden=hidden_size, layers=num_layers, df=df_order,
                                     num_spks=num_spks, shared=bool(shared_weights), bn=bool(bn), ln=bool(use_pre_layer_norm_fb),
                                     act=activation_code(output_activate_function))

    def _make_engine(self, state_dict, device):
        return FullbandEngine(self._fb_spec, state_dict, device, weight_bits=self.weight_bits)

    def _kernel_path(self) -> bool:
        return True  # (eval mode without gradients: the engine for GSN, _forward_lstm for LSTM -- both below)

    def streaming(self, batch: int = 1, hop: int = 1, graph: bool = True, one_launch="auto", waveform: bool = False,
                  host_io: bool = False, resident: bool = False, count_spikes: bool = False, resample: int = 1, sample_format: str = "f32"):
        """Frame-by-frame session (``fullband_streaming.FullbandStreamingSession``): ``step(frames [B, F, hop])`` with the GSN states
        and ``df_order - 1`` frames of history kept on the device, bit-identical to the offline forward on the concatenated input.
        ``one_launch``: True = the whole hop in one ``sfsn_fullband_stream_hop`` launch (``NotImplementedError`` where it does not cover
        the model), False = the offline kernels on the new frames (from a HIP graph when ``graph``), "auto" = the faster one that
        applies.  ``waveform=True``: samples in, samples out -- ``step_wave(samples [B, 128])`` returns ``[B, S, 128]`` enhanced samples,
        the frame's STFT, the hop and the inverse STFT in one ``sfsn_fullband_stream_hop_wave`` launch, bit-identical to
        ``model(wave)`` three calls later (``hop == 1``, 512-point frames with hop 128, ``B <= 16``, shared gate weights; anything else
        has no waveform tier: ``NotImplementedError``).  ``host_io=True`` (with ``waveform``): ``step_wave_host`` takes and returns CPU
        tensors through pinned host memory, no copy launch and no stream synchronisation.  ``count_spikes=True`` (spectrum sessions, both
        tiers): per-clip spike counts of every layer, kept on the device as the session runs, for ``session.spike_summary(clips)`` --
        ``metric.compute_synops(session.spike_summary([b]), [], shared_weights=...)`` is clip b's SynOPs; together with ``waveform``
        it raises ``NotImplementedError`` (the waveform launch does not count).  A tick on which only some clips have input:
        ``session.tick(frames, clips)`` / ``tick_wave`` / ``tick_wave_host`` hold every other clip inside the same one launch.
        ``resident`` is not built for this model.  ``resample`` / ``sample_format`` other than ``1`` / ``"f32"`` raise
        ``NotImplementedError`` HERE: outer samples at 48 kHz or as 16-bit PCM, converted inside the same one launch, come from a factory
        of their own, ``streaming_outer(batch, host_io, resample=3, sample_format="s16")``.  GSN models on a HIP device."""
        if resample != 1:
            raise NotImplementedError(f"cIRM-GSN streaming: resample={resample!r} is not built (the Spiking-FullSubNet sessions have it)")
        if sample_format != "f32":
            raise NotImplementedError(f"cIRM-GSN streaming: sample_format={sample_format!r} is not built (the Spiking-FullSubNet sessions have it)")
        if self.fb_model.sequence_model_name == "LSTM":
            raise NotImplementedError("cIRM-GSN streaming covers the GSN sequence model: an LSTM model runs on ATen and has no session")
        if resident:
            raise NotImplementedError("cIRM-GSN streaming: resident=True is not built (the Spiking-FullSubNet sessions have it)")
        self._check_mode()
        if batch < 1 or hop < 1:
            raise ValueError("batch and hop must be positive")
        if next(self.parameters()).device.type != "cuda":
            # (before anything else about these options is judged: host_io without waveform is a ValueError on a HIP module)
            asked = [f"{name}=True: " for name, on in (("waveform", waveform), ("host_io", host_io), ("count_spikes", count_spikes)) if on]
            raise NotImplementedError((asked[0] if asked else "") + "cIRM-GSN streaming has no CPU path: move the module to a HIP "
                                      "device (`.to('cuda')`) first")
        from .fullband_streaming import FullbandStreamingSession
        return FullbandStreamingSession(self.engine(), batch=batch, hop=hop, graph=graph, one_launch=one_launch, owner=self,
                                        waveform=waveform, host_io=host_io, frame=(self.n_fft, self.hop_length, self.win_length),
                                        count_spikes=count_spikes)

    def streaming_outer(self, batch: int = 1, host_io: bool = False, resample: int = 3, sample_format: str = "s16"):
        """A waveform session on the samples a sound card delivers: ``resample=3`` -- 48 kHz in and out, 384 samples per call -- and
        ``sample_format="s16"`` -- int16 tensors in and out; ``(3, "s16")``, ``(3, "f32")`` and ``(1, "s16")`` exist.  The session is
        ``streaming(waveform=True, host_io=host_io)``'s with ``step_wave`` / ``tick_wave`` / ``step_wave_host`` / ``tick_wave_host``
        taking ``[B, 128 * resample]`` of the format and returning ``[B, S, 128 * resample]`` of it; decimation, interpolation and both
        format conversions run inside the hop's one launch (``sfsn_fullband_stream_hop_wave_io``), and call by call the result is
        ``Q(U3(control(D3(x * 2**-15))))`` with ``control`` the plain waveform session on the same calls, bit for bit
        (``fullband_streaming``: outer samples).  The delay is three calls plus 95 outer samples.  ``ValueError``: ``resample`` not 1
        or 3, an unknown format, or ``(1, "f32")``, which is ``streaming(waveform=True)``.  Everything else ``streaming(waveform=True)``
        refuses is refused alike."""
        from . import spectral
        if resample not in (1, 3):
            raise ValueError(f"resample must be 1 or 3 (the session's samples at the model's rate or at three times it), got {resample!r}")
        spectral.format_of(sample_format)
        if resample == 1 and sample_format == "f32":
            raise ValueError("streaming_outer(resample=1, sample_format='f32'): the model's own samples are streaming(waveform=True)")
        if self.fb_model.sequence_model_name == "LSTM":
            raise NotImplementedError("cIRM-GSN streaming covers the GSN sequence model: an LSTM model runs on ATen and has no session")
        self._check_mode()
        if batch < 1:
            raise ValueError("batch and hop must be positive")
        if next(self.parameters()).device.type != "cuda":
            raise NotImplementedError("waveform=True: cIRM-GSN streaming has no CPU path: move the module to a HIP device (`.to('cuda')`) first")
        from .fullband_streaming import FullbandStreamingSession
        return FullbandStreamingSession(self.engine(), batch=batch, hop=1, owner=self, waveform=True, host_io=host_io,
                                        frame=(self.n_fft, self.hop_length, self.win_length), resample=resample, sample_format=sample_format)

    @torch.no_grad()
    def forward_stft(self, noisy_cmp, want_layers=False, want_counts=False, frames=None):
        """The hot path alone (GSN models): complex64 [B, F, T] -> ``FullbandEngine.forward_stft``'s result dict.  ``frames``: a
        ragged batch, clip b has ``frames[b]`` frames."""
        if self.fb_model.sequence_model_name == "LSTM":
            raise NotImplementedError("forward_stft runs the GSN kernels: an LSTM model runs on ATen (call the module itself)")
        self._check_mode(noisy_cmp)
        return self.engine().forward_stft(noisy_cmp, want_layers=want_layers, want_counts=want_counts, frames=frames)

    @torch.no_grad()
    def forward_ragged(self, waves, lengths):
        """Inference on a batch of clips of different lengths (GSN models): ``waves`` float32 [B, Lmax] on the device (what lies past
        a clip's end is ignored), ``lengths`` a sequence or CPU int tensor of B values, ``1 <= L_b <= Lmax`` (``ValueError`` naming
        the clip otherwise).  Returns ``forward()``'s tuple on the padded batch -- ``(enh_y [B, S, Lmax], [layers])`` for
        ``num_spks > 1``, ``(enh_y [B, Lmax], enh_mag [B, F, T])`` for one speaker -- in which every clip is the clip run alone, bit
        for bit: ``enh_y[b, ..., :L_b]`` and ``enh_mag[b, :, :T_b]`` (zero beyond), and ``ragged.clip_layers(layers, [], b, lengths,
        hop=hop_length)[0]`` for clip b's layer list.  Inference only (``_check_mode``)."""
        if self.fb_model.sequence_model_name == "LSTM":
            raise NotImplementedError("forward_ragged runs the GSN kernels: an LSTM model runs on ATen, one clip per call")
        y, res = self._forward_ragged(waves, lengths)
        if self.num_spks > 1:
            return y, [self._layer_list(res, waves.shape[0])]
        return y[:, 0], res["enh_mag"][:, 0]

    def _forward_kwargs(self):
        # (one speaker returns no layer list; two speakers: layer_outputs says what stands in for the fp32 spike tensors)
        return self._layer_kwargs() if self.num_spks > 1 else dict(want_layers=False, want_counts=False)

    def _gaussian_norm(self) -> bool:
        return False

    def _layer_list(self, res, batch_size):
        layers = res["all_layers"]
        if layers is None:  # "none": the list keeps its length and the shapes of its two ends
            T, F, P = res["enh_stft"].shape[-1], self.fb_input_size, self._fb_spec.P
            layers = [torch.empty((T, batch_size, F), device="meta")] + [None] * self._fb_spec.layers + \
                     [torch.empty((T, batch_size, P), device="meta")]
        return layers

    def forward(self, input):
        assert input.ndim == 2, f"Input tensor must be 2D, but got {input.ndim}D."
        if self._wants_autograd(input):
            from . import training
            return training.forward_cirm(self, input)
        with torch.no_grad():
            if self.fb_model.sequence_model_name == "LSTM":
                return self._forward_lstm(input)
            return self._forward_gsn(input)

    def _finish(self, enh_stft, enh_mag, layers, batch_size, sequence_length):
        if self.num_spks > 1:
            enh_y = self._istft(enh_stft.reshape(batch_size * self.num_spks, *enh_stft.shape[2:]), length=sequence_length)
            # the reference returns `_` here, rebound by `fb_output, *_ = self.fb_model(...)` to [all_layer_outputs] (:228, :239)
            return enh_y.reshape(batch_size, self.num_spks, -1), [layers]
        enh_y = self._istft(enh_stft[:, 0], length=sequence_length)
        return enh_y, enh_mag

    def _forward_gsn(self, input):
        batch_size, sequence_length = input.shape
        res = self.engine().forward_stft(self._stft(input), **self._forward_kwargs())
        mag = res["enh_mag"][:, 0] if res["enh_mag"] is not None else None
        layers = self._layer_list(res, batch_size) if self.num_spks > 1 else None
        return self._finish(res["enh_stft"], mag, layers, batch_size, sequence_length)

    def _forward_lstm(self, input):
        from . import training
        batch_size, sequence_length = input.shape
        cmp = self._stft(input)
        coef, layers = training.sequence_model(self.fb_model, torch.abs(cmp) ** self.fdrc, training=False)  # [B, P, T]
        enh = deep_filter_torch(cmp, coef, self.df_order, self.num_spks)
        return self._finish(enh, torch.abs(enh[:, 0]), layers, batch_size, sequence_length)
