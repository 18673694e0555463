"""References and inputs for the ragged-batch tests (clips of different lengths in one padded batch) -- TEST INFRASTRUCTURE ONLY.

* the clip table every ragged test uses, and seeded clips for it;
* fp64 numpy references of what the ragged kernels compute: the MASKED versions of ``oracle.model.istft`` and of the offline
  norms' statistics (``Oracle.laplace_norm`` / ``gaussian_norm``) -- frames ``t >= T_b`` of clip b do not exist;
* ``padded_vs_alone``: what a padded batch WITHOUT lengths gets wrong, measured on the CPU oracle (the reason the feature exists).

tests/test_ragged_host.py pins the two references to the oracle's clip-alone results on the clip table.
"""
from __future__ import annotations

import numpy as np

HOP = 128
N_FFT = 512
# either side of the 16-frame FFT tile and its 3-frame halo, either side of the 64-lane stride of the row sums; 200, 1925, 4133,
# 8200 and 16600 are no multiple of the hop
CLIP_LENGTHS = (200, 1925, 2048, 2400, 4133, 8200, 16600)
CLIP_FRAMES = tuple(1 + L // HOP for L in CLIP_LENGTHS)
assert CLIP_FRAMES == (2, 16, 17, 19, 33, 65, 130)


def clip_waves(seed: int, lengths=CLIP_LENGTHS, gains=None):
    """One 0.05-rms noise clip per length (float32), each from its own stream of the seed; ``gains`` scale them (distinct levels
    give distinct statistics, so a wrong row -> clip index cannot pass)."""
    out = []
    for b, L in enumerate(lengths):
        rng = np.random.default_rng([seed, b])
        w = (0.05 * rng.standard_normal(L)).astype(np.float32)
        out.append(w if gains is None else (w * np.float32(gains[b % len(gains)])).astype(np.float32))
    return out


def pad_batch(waves, junk_seed=None) -> np.ndarray:
    """[B, Lmax] float32: the clips padded to the longest -- with zeros, or (``junk_seed``) with non-zero noise a reader of the
    padding would notice."""
    Lmax = max(len(w) for w in waves)
    if junk_seed is None:
        out = np.zeros((len(waves), Lmax), np.float32)
    else:
        out = (0.5 + np.random.default_rng(junk_seed).random((len(waves), Lmax))).astype(np.float32)
    for b, w in enumerate(waves):
        out[b, :len(w)] = w
    return out


def istft_ref(spec, frames, lengths, out_len=None, n_fft: int = N_FFT, hop: int = HOP) -> np.ndarray:
    """``oracle.model.istft`` with per-clip lengths, in float64 -> float32 [B, out_len]: for clip b only frames ``t < frames[b]``
    are overlap-added (into the sum and into the squared-window envelope), samples ``m >= lengths[b]`` are 0."""
    from oracle import model as omodel
    spec = np.asarray(spec, np.complex128)
    B, F, T = spec.shape
    out_len = max(lengths) if out_len is None else out_len
    win = omodel.hann_window(n_fft).astype(np.float64)
    out = np.zeros((B, out_len), np.float32)
    for b in range(B):
        Tb, Lb = int(frames[b]), int(lengths[b])
        fr = np.fft.irfft(spec[b, :, :Tb].T, n=n_fft, axis=-1) * win  # [Tb, n_fft]
        total = (Tb - 1) * hop + n_fft
        y, env = np.zeros(total), np.zeros(total)
        for t in range(Tb):  # ascending frames, as the oracle and the kernel
            y[t * hop:t * hop + n_fft] += fr[t]
            env[t * hop:t * hop + n_fft] += win * win
        sl = slice(n_fft // 2, n_fft // 2 + Lb)
        out[b, :Lb] = (y[sl] / env[sl]).astype(np.float32)
    return out


def stats_ref(x, frames, gaussian: bool = False):
    """The offline norms' per-clip statistics of a gathered, un-normalised group tensor ``x`` [T, B * N, I] of a padded batch, in
    float64: the mean over clip b's rows and its first ``frames[b]`` frames only (``offline_laplace_norm``) -- ``gaussian``: that
    mean and the UNBIASED standard deviation (``offline_gaussian_norm`` = torch.mean / torch.std).  -> mu [B] (, sd [B])."""
    x = np.asarray(x, np.float64)
    B = len(frames)
    N = x.shape[1] // B
    mu, sd = np.empty(B), np.empty(B)
    for b in range(B):
        v = x[:int(frames[b]), b * N:(b + 1) * N]
        mu[b] = v.mean()
        sd[b] = v.std(ddof=1) if v.size > 1 else np.nan
    return (mu, sd) if gaussian else mu


def model_spec_sd(kw: dict, seed: int):
    """(oracle spec, numpy state dict) of a ``refweights`` configuration, live or frozen."""
    import refweights as rw
    from oracle import model as omodel
    if "fb_freqs" in kw:
        return omodel.spec_from_frozen_kwargs(kw), rw.frozen_state_dict(kw, seed)
    return omodel.spec_from_live_kwargs(kw), rw.live_state_dict(kw, seed)


def synops_of(fb_all, sb_all, shared) -> float:
    from oracle import model as omodel
    return omodel.compute_synops(fb_all, sb_all, shared)


def padded_vs_alone(kw: dict, seed: int = 3, lengths=CLIP_LENGTHS) -> dict:
    """Run the CPU oracle (fp32) on the zero-padded batch WITHOUT lengths and on every clip alone; report, as maxima over the clips:

    ``spikes_equal`` / ``enh_equal``  frames ``t < T_b`` of every spike tensor / of the enhanced spectrum equal bit for bit
    ``wave_err``     max |padded - alone| over the clips' own samples (the inverse STFT overlap-adds the frames past the end)
    ``wave_err_body`` the same without each clip's last n_fft/2 samples
    ``synops_rel``   max relative error of SynOPs taken as a mean over the padded tensors
    """
    from oracle import model as omodel
    spec, sd = model_spec_sd(kw, seed)
    n_fft, hop = kw["n_fft"], kw["hop_length"]
    waves = clip_waves(seed, lengths)
    batch = pad_batch(waves)
    B = len(waves)
    pad = omodel.forward_from_stft(spec, sd, omodel.stft(batch, n_fft, hop), "f32")
    y_pad = omodel.istft(pad["enh_stft"][:, 0], n_fft, hop, length=batch.shape[1])
    syn_pad = synops_of(pad["fb_all"], pad["sb_all"], spec["shared"])
    res = dict(spikes_equal=True, enh_equal=True, wave_err=0.0, wave_err_body=0.0, synops_rel=0.0)
    for b, w in enumerate(waves):
        L, Tb = len(w), 1 + len(w) // hop
        one = omodel.forward_from_stft(spec, sd, omodel.stft(w[None], n_fft, hop), "f32")
        y_one = omodel.istft(one["enh_stft"][:, 0], n_fft, hop, length=L)
        for outs_p, outs_1 in zip([pad["fb_all"]] + pad["sb_all"], [one["fb_all"]] + one["sb_all"]):
            n = outs_1[0].shape[1]
            for p_, o_ in zip(outs_p[1:-1], outs_1[1:-1]):
                res["spikes_equal"] &= bool(np.array_equal(p_[:Tb, b * n:(b + 1) * n], o_))
        res["enh_equal"] &= bool(np.array_equal(pad["enh_stft"][b, :, :, :Tb], one["enh_stft"][0]))
        err = np.abs(y_pad[b, :L] - y_one[0])
        res["wave_err"] = max(res["wave_err"], float(err.max()))
        if L > n_fft // 2:
            res["wave_err_body"] = max(res["wave_err_body"], float(err[:L - n_fft // 2].max()))
        syn_one = synops_of(one["fb_all"], one["sb_all"], spec["shared"])
        res["synops_rel"] = max(res["synops_rel"], abs(syn_pad - syn_one) / syn_one)
    return res
