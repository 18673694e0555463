"""Ragged batches through the modules: ``forward_ragged(waves, lengths)`` and ``forward_stft(stft, frames=...)`` against the same
model run on every clip alone -- bit for bit (``torch.equal``), for every output: waveform, magnitude, every spike tensor and
projection, spike counts and the SynOPs / NeuronOPs made from them, the offline norms' statistics.  The model is causal and the
ragged kernels at its edges skip what a clip does not have, so nothing here needs a tolerance; the two cases that do (the CPU
oracle, the ATen edges of the 256-point configuration) use the tolerances those comparisons already have elsewhere in the suite.

Clip table (tests/raggedref.py): 200 ... 16600 samples = 2, 16, 17, 19, 33, 65, 130 frames at hop 128."""
import numpy as np
import pytest
import torch

import parity
import raggedref as rr
import refweights as rw
from oracle import model as omodel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LENS, FRAMES = list(rr.CLIP_LENGTHS), list(rr.CLIP_FRAMES)
B, LMAX, TMAX = len(LENS), max(LENS), max(FRAMES)
GAINS = (1.0, 0.45, 1.8)  # the clips differ in level, so their statistics differ: a wrong row -> clip index cannot pass
SEED = 3
CONFIGS = dict(LIVE_TINY=rw.LIVE_TINY, LIVE_TINY_2SPK=rw.LIVE_TINY_2SPK, LIVE_TINY_UNSHARED=rw.LIVE_TINY_UNSHARED,
               FROZEN_TINY=rw.FROZEN_TINY, FROZEN_TINY_GAUSS=rw.FROZEN_TINY_GAUSS, FROZEN_TINY_CUM=rw.FROZEN_TINY_CUM)


def build(kw):
    import spiking_fullsubnet_amd as pkg
    frozen = "fb_freqs" in kw
    sd = rw.frozen_state_dict(kw, SEED) if frozen else rw.live_state_dict(kw, SEED)
    m = (pkg.Separator if frozen else pkg.SpikingFullSubNet)(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.eval().to(DEV), sd


def real(x):
    return torch.view_as_real(x) if x.is_complex() else x


def same(a, b, what):
    a, b = real(a), real(b)
    assert a.shape == b.shape, (what, tuple(a.shape), tuple(b.shape))
    if not torch.equal(a, b):
        d = (a.double() - b.double()).abs()
        raise AssertionError(f"{what}: {int((a != b).sum())} of {a.numel()} elements differ, max |diff| {float(d.max()):.3g}")


def unpack(out):
    """forward()'s tuple -> (enhanced_y, enh_mag or None, fb_all, sb_all); two-speaker models return no magnitude."""
    return (out[0], None, out[1], out[2]) if len(out) == 3 else out


class Case:
    """One configuration: the model, the junk-padded batch, and -- computed once, never modified -- the ragged results and the
    clip-alone results in the ``"tensors"`` and ``"counts"`` modes."""

    def __init__(self, name):
        self.kw = CONFIGS[name]
        self.model, self.sd = build(self.kw)
        waves = rr.clip_waves(SEED, gains=GAINS)
        self.batch = torch.from_numpy(rr.pad_batch(waves, junk_seed=SEED + 1)).to(DEV)  # non-zero junk past every end
        self.zero_batch = torch.from_numpy(rr.pad_batch(waves)).to(DEV)
        self.ragged, self.alone = {}, {}
        for mode in ("tensors", "counts"):
            self.model.layer_outputs = mode
            self.ragged[mode] = unpack(self.model.forward_ragged(self.batch, LENS))
            self.alone[mode] = [unpack(self.model(self.batch[b:b + 1, :L].contiguous())) for b, L in enumerate(LENS)]
        self.model.layer_outputs = "tensors"
        torch.cuda.synchronize()


_cases = {}


@pytest.fixture(params=list(CONFIGS))
def case(request):
    if request.param not in _cases:
        _cases[request.param] = Case(request.param)
    return _cases[request.param]


def get_case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


# ---- forward_ragged against every clip alone --------------------------------------------------------------------------------------
def test_waveform_and_magnitude_equal_each_clip_alone(case):
    y, mag, _, _ = case.ragged["tensors"]
    S = case.kw.get("num_spks", 1)
    assert tuple(y.shape) == ((B, S, LMAX) if S > 1 else (B, LMAX))
    for b, (L, T) in enumerate(zip(LENS, FRAMES)):
        y1, mag1, _, _ = case.alone["tensors"][b]
        same(y[b, ..., :L], y1[0], f"enhanced_y of clip {b}")
        assert not bool(y[b, ..., L:].any()), f"enhanced_y of clip {b} is not zero beyond its {L} samples"
        if mag is not None:
            same(mag[b, :, :T], mag1[0], f"enh_mag of clip {b}")
            assert not bool(mag[b, :, T:].any()), f"enh_mag of clip {b} is not zero beyond its {T} frames"


def test_layer_tensors_equal_each_clip_alone(case):
    from spiking_fullsubnet_amd import metric, ragged
    _, _, fb_all, sb_all = case.ragged["tensors"]
    shared = case.kw.get("shared_weights", False)
    for b in range(B):
        fb, sb = ragged.clip_layers(fb_all, sb_all, b, LENS, hop=rr.HOP)
        _, _, fb1, sb1 = case.alone["tensors"][b]
        for i, (x, x1) in enumerate(zip(fb, fb1)):
            same(x, x1, f"fb_all[{i}] of clip {b}")
        for g, (outs, outs1) in enumerate(zip(sb, sb1)):
            assert len(outs) == len(outs1)
            for i, (x, x1) in enumerate(zip(outs, outs1)):
                same(x, x1, f"sb_all[{g}][{i}] of clip {b}")
        assert metric.compute_synops(fb, sb, shared) == metric.compute_synops(fb1, sb1, shared)
        assert metric.compute_neuronops(fb, sb) == metric.compute_neuronops(fb1, sb1)


def test_counts_equal_each_clip_alone(case):
    from spiking_fullsubnet_amd import metric, ragged
    from spiking_fullsubnet_amd.engine import SpikeSummary
    y, mag, fb_all, sb_all = case.ragged["counts"]
    yt, magt, fb_t, sb_t = case.ragged["tensors"]
    same(y, yt, "enhanced_y in the counts mode")
    shared = case.kw.get("shared_weights", False)
    assert isinstance(fb_all[1], ragged.ClipSpikeSummary)
    for b, T in enumerate(FRAMES):
        fb, sb = ragged.clip_layers(fb_all, sb_all, b, FRAMES)
        _, _, fb1, sb1 = case.alone["counts"][b]
        fbt, sbt = ragged.clip_layers(fb_t, sb_t, b, FRAMES)
        for outs, outs1, outst in zip([fb] + sb, [fb1] + sb1, [fbt] + sbt):
            for i in range(1, len(outs) - 1):
                assert isinstance(outs[i], SpikeSummary) and isinstance(outs1[i], SpikeSummary)
                assert outs[i].shape == outs1[i].shape and outs[i].shape[0] == T
                assert int(outs[i].count) == int(outs1[i].count) == int(outst[i].sum()), (b, i)
        assert metric.compute_synops(fb, sb, shared) == metric.compute_synops(fb1, sb1, shared)
        assert metric.compute_neuronops(fb, sb) == metric.compute_neuronops(fb1, sb1)


def test_forward_stft_frames_equals_each_clip_alone(case):
    from spiking_fullsubnet_amd import ragged
    m = case.model
    stft = m._stft(case.zero_batch)
    res = m.forward_stft(stft, frames=FRAMES)
    for b, T in enumerate(FRAMES):
        one = m.forward_stft(stft[b:b + 1, :, :T].contiguous())
        same(res["enh_stft"][b, ..., :T], one["enh_stft"][0], f"enh_stft of clip {b}")
        same(res["enh_mag"][b, ..., :T], one["enh_mag"][0], f"enh_mag of clip {b}")
        assert not bool(real(res["enh_stft"][b, ..., T:]).any()) and not bool(res["enh_mag"][b, ..., T:].any()), b
        fb, sb = ragged.clip_layers(res["fb_all"], res["sb_all"], b, FRAMES)
        for x, x1 in zip(fb + [x for outs in sb for x in outs], one["fb_all"] + [x for outs in one["sb_all"] for x in outs]):
            same(x, x1, f"a layer output of clip {b}")


# ---- the offline norms' statistics ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["FROZEN_TINY", "FROZEN_TINY_GAUSS"])
def test_norm_statistics_are_each_clips_own(name):
    c = get_case(name)
    m = c.model
    stft = m._stft(c.zero_batch)
    got = m.forward_stft(stft, want_layers=False, return_norm_stats=True, frames=FRAMES)["norm_stats"]
    by_wave = m.norm_stats(c.batch, lengths=LENS)  # (junk past every end)
    by_stft = m.norm_stats(stft, lengths=FRAMES)
    assert len(set(got.mu_fb.tolist())) == B
    for b, (L, T) in enumerate(zip(LENS, FRAMES)):
        one = m.norm_stats(c.batch[b:b + 1, :L].contiguous())
        for s in (got, by_wave, by_stft):
            for t, t1 in ((s.mu_fb, one.mu_fb), (s.mu_sb, one.mu_sb), (s.sd_fb, one.sd_fb), (s.sd_sb, one.sd_sb)):
                assert (t is None) == (t1 is None)
                if t is not None:
                    same(t[..., b], t1[..., 0], f"statistics of clip {b}")
    # given statistics are taken as given in a ragged batch too (the statistics launches are skipped)
    a = m.forward_stft(stft, frames=FRAMES, norm_stats=got)
    same(a["enh_stft"], m.forward_stft(stft, frames=FRAMES)["enh_stft"], "enh_stft with the ragged statistics supplied")


def test_a_padded_batch_without_lengths_is_not_the_clips_alone():
    """Guards the file against passing vacuously: FROZEN_TINY's per-clip mean runs over the padding when no lengths are given."""
    c = get_case("FROZEN_TINY")
    y = unpack(c.model(c.zero_batch))[0]
    differs = [not torch.equal(y[b, :L], c.alone["tensors"][b][0][0]) for b, L in enumerate(LENS)]
    assert all(differs[:-1]), differs


# ---- properties of the batch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["LIVE_TINY", "FROZEN_TINY"])
def test_permuting_the_clips_permutes_the_outputs(name):
    c = get_case(name)
    perm = [4, 0, 6, 2, 1, 5, 3]
    y, mag, fb_all, sb_all = c.ragged["tensors"]
    yp, magp, fbp, sbp = c.model.forward_ragged(c.batch[perm].contiguous(), [LENS[i] for i in perm])
    same(yp, y[perm], "enhanced_y")
    same(magp, mag[perm], "enh_mag")
    from spiking_fullsubnet_amd import ragged
    fr = [FRAMES[i] for i in perm]
    for j, b in enumerate(perm):
        fb, sb = ragged.clip_layers(fb_all, sb_all, b, FRAMES)
        fb2, sb2 = ragged.clip_layers(fbp, sbp, j, fr)
        for x, x2 in zip(fb + [x for outs in sb for x in outs], fb2 + [x for outs in sb2 for x in outs]):
            same(x2, x, f"a layer output of clip {b} at position {j}")


@pytest.mark.parametrize("name", ["LIVE_TINY", "LIVE_TINY_2SPK", "FROZEN_TINY", "FROZEN_TINY_GAUSS", "FROZEN_TINY_CUM"])
def test_full_lengths_and_no_frames_are_todays_forward(name):
    c = get_case(name)
    m, L = c.model, 2400
    wave = torch.from_numpy(np.stack(rr.clip_waves(SEED + 2, [L] * 3, gains=GAINS))).to(DEV)
    ref = unpack(m(wave))
    got = unpack(m.forward_ragged(wave, [L] * 3))
    for a, b_ in zip([got[0], got[1]] + got[2] + [x for outs in got[3] for x in outs],
                     [ref[0], ref[1]] + ref[2] + [x for outs in ref[3] for x in outs]):
        if a is not None:
            same(a, b_, "an output with all lengths equal to Lmax")
    stft = m._stft(wave)
    r0, r1, r2 = m.forward_stft(stft), m.forward_stft(stft, frames=None), m.forward_stft(stft, frames=[stft.shape[-1]] * 3)
    for r in (r1, r2):
        same(r["enh_stft"], r0["enh_stft"], "enh_stft")
        same(r["enh_mag"], r0["enh_mag"], "enh_mag")


# ---- against the CPU oracle: the check does not rest on the product alone --------------------------------------------------------
@pytest.mark.parametrize("name", ["LIVE_TINY", "FROZEN_TINY"])
def test_every_clip_of_a_ragged_batch_against_the_oracle(name):
    from spiking_fullsubnet_amd import ragged
    c = get_case(name)
    m = c.model
    spec = omodel.spec_from_frozen_kwargs(c.kw) if "fb_freqs" in c.kw else omodel.spec_from_live_kwargs(c.kw)
    stft = m._stft(c.zero_batch)
    res = m.forward_stft(stft, frames=FRAMES)
    for b, T in enumerate(FRAMES):
        fb, sb = ragged.clip_layers(res["fb_all"], res["sb_all"], b, FRAMES)
        out = dict(enh_stft=res["enh_stft"][b:b + 1, ..., :T].cpu().numpy(), fb_all=[x.cpu().numpy() for x in fb],
                   sb_all=[[x.cpu().numpy() for x in outs] for outs in sb])
        ora = omodel.forward_from_stft(spec, c.sd, stft[b:b + 1, :, :T].cpu().numpy(), "f32", want_membrane=True)
        parity.check_model(out, parity.gold_from_oracle(ora), spec, tag=f"ragged {name} clip {b}: ")


# ---- 256-point frames (wsj0-mix geometry): ATen at the two edges, the model batched ------------------------------------------------
def test_wsj0_geometry_takes_the_aten_edges():
    from spiking_fullsubnet_amd import ragged
    kw = dict(rw.LIVE_WSJ0, fb_hidden_size=48, sb_hidden_size=32, df_orders=[2, 1, 1])
    m, _ = build(kw)
    hop = kw["hop_length"]
    lens = [200, 1925, 2048, 4133]
    frames = ragged.frames_of(lens, hop)
    waves = rr.clip_waves(SEED, lens, gains=GAINS)
    batch = torch.from_numpy(rr.pad_batch(waves, junk_seed=9)).to(DEV)
    assert not m._device_fft(batch)
    y, fb_all, sb_all = m.forward_ragged(batch, lens)
    assert tuple(y.shape) == (len(lens), 2, max(lens))
    stft = m._stft(torch.from_numpy(rr.pad_batch(waves)).to(DEV))
    res = m.forward_stft(stft, frames=frames)
    for b, (L, T) in enumerate(zip(lens, frames)):
        one = m.forward_stft(stft[b:b + 1, :, :T].contiguous())
        same(res["enh_stft"][b, ..., :T], one["enh_stft"][0], f"enh_stft of clip {b}")
        assert not bool(real(res["enh_stft"][b, ..., T:]).any())
        fb, sb = ragged.clip_layers(res["fb_all"], res["sb_all"], b, frames)
        for x, x1 in zip(fb + [x for outs in sb for x in outs], one["fb_all"] + [x for outs in one["sb_all"] for x in outs]):
            same(x, x1, f"a layer output of clip {b}")
        y1 = m(batch[b:b + 1, :L].contiguous())[0]
        ref = y1[0].cpu().numpy()
        np.testing.assert_allclose(y[b, :, :L].cpu().numpy(), ref, atol=3e-6 * np.abs(ref).max(), rtol=0)
        assert not bool(y[b, :, L:].any())


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_bad_lengths_and_modes_are_refused():
    c = get_case("FROZEN_TINY_GAUSS")
    m = c.model
    small = c.batch[:3, :2400].contiguous()
    for lens, msg in (([2400, 0, 100], r"lengths\[1\] = 0"), ([2400, 2401, 100], r"lengths\[1\] = 2401"), ([2400, 100], "one length per clip"),
                      ([2400, 127, 300], r"lengths\[1\] = 127.*one hop")):
        with pytest.raises(ValueError, match=msg):
            m.forward_ragged(small, lens)
    stft = m._stft(small)
    for fr, msg in (([19, 0, 3], r"frames\[1\] = 0"), ([19, 20, 3], r"frames\[1\] = 20"), ([19, 3], "one frame count"), ([19, 1, 3], r"frames\[1\] = 1")):
        with pytest.raises(ValueError, match=msg):
            m.forward_stft(stft, frames=fr)
    with pytest.raises(ValueError, match="CPU int tensor"):
        m.forward_ragged(small, torch.tensor([2400, 300, 200], device=DEV))
    with pytest.raises(RuntimeError):
        m.forward_ragged(small.cpu(), [2400, 300, 200])
    m.train()
    try:
        with pytest.raises(RuntimeError, match="training mode"):
            m.forward_ragged(small, [2400, 300, 200])
    finally:
        m.eval()
    live = get_case("LIVE_TINY").model
    y = live.forward_ragged(small, [2400, 127, 1])[0]  # a single frame is fine without the Gaussian norm
    assert not bool(y[1, 127:].any()) and not bool(y[2, 1:].any())
