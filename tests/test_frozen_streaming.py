"""Streaming the frozen (model_zoo-architecture) front-end with GIVEN normalisation statistics: ``model.streaming(norm_stats=...)``.

The offline Laplace / Gaussian norm divides by per-clip statistics of the whole utterance; everything else of the model is causal.
So a session that is handed a clip's own statistics must reproduce the offline forward of that clip BIT FOR BIT -- no tolerance
anywhere in this file -- in both session tiers (the one-launch hop, the graph-replayed per-kernel sequence) and in every mode the
sessions have.  For statistics that are not the clip's own the yardstick is the offline forward with the same statistics supplied
(``forward_stft(..., norm_stats=...)``), whose feature arithmetic under arbitrary ``mu`` tests/frontback.py holds to fp64."""
import os

import numpy as np
import pytest
import torch

import refweights as rw

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TINY_LAP = dict(rw.FROZEN_TINY, sb_df_orders=[3, 2, 1])  # (the fixture's orders [2, 1, 3] give the last group 384 projections: one launch covers 256)
TINY_GAUSS = dict(TINY_LAP, norm_type="offline_gaussian_norm")
GAINS = (1.0, 0.45, 1.8)  # the clips differ in level, so their statistics differ: a wrong row -> clip index cannot pass


def build(kw, seed, sd=None):
    import spiking_fullsubnet_amd as pkg
    sd = rw.frozen_state_dict(kw, seed) if sd is None else sd
    m = pkg.Separator(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.eval().to(DEV)


def clips(model, B, T, seed):
    """B distinct clips of T frames -> (wave [B, (T - 1) * 128], stft [B, 257, T])."""
    wave = torch.from_numpy(rw.synth_wave(B, T, seed)) * torch.tensor(GAINS[:B]).reshape(B, 1)
    wave = wave.to(DEV)
    return wave, model._stft(wave)[..., :T].contiguous()


def real(x):
    return torch.view_as_real(x) if x.is_complex() else x


def run_spectra(sess, stft):
    hop = sess.hop
    outs = [sess.step(stft[..., t0:t0 + hop].contiguous()) for t0 in range(0, stft.shape[-1], hop)]
    sess.check_errors()
    return torch.cat([e for e, _ in outs], -1), torch.cat([m for _, m in outs], -1)


def cat_stats(items):
    from spiking_fullsubnet_amd.engine import NormStats
    cat = lambda ts: None if ts[0] is None else torch.cat(ts, -1)
    return NormStats(cat([s.mu_fb for s in items]), cat([s.mu_sb for s in items]), cat([s.sd_fb for s in items]), cat([s.sd_sb for s in items]))


def scaled(stats, factors):
    f = torch.tensor(factors, device=DEV)
    return stats._map(lambda t: t * f)


# ---- a clip's own statistics reproduce the offline forward ---------------------------------------------------------------------
@pytest.mark.parametrize("kw,seed,B,hop", [
    (TINY_LAP, 41, 3, 1), (TINY_LAP, 41, 2, 3), (dict(TINY_LAP, shared_weights=False), 42, 3, 2), (TINY_GAUSS, 43, 3, 1),
    (rw.FROZEN_M, 44, 2, 1), (rw.FROZEN_L, 45, 2, 1), (rw.FROZEN_TINY, 31, 2, 1)],
    ids=["tiny-b3", "tiny-hop3", "tiny-unshared-hop2", "tiny-gauss", "baseline_m", "baseline_l", "tiny-per-kernel"])
def test_own_statistics_reproduce_the_offline_forward(kw, seed, B, hop):
    model = build(kw, seed)
    T = 36 * hop
    _, stft = clips(model, B, T, seed)
    off = model.forward_stft(stft, want_layers=False, return_norm_stats=True)
    stats = off["norm_stats"]
    assert stats.mu_fb.shape == (B,) and stats.mu_sb.shape == (len(kw["sb_df_orders"]), B)
    assert (stats.sd_fb is not None) == (kw["norm_type"] == "offline_gaussian_norm")
    assert len(set(stats.mu_fb.tolist())) == B  # distinct clips, distinct statistics
    sess = model.streaming(batch=B, hop=hop, norm_stats=stats)
    assert (sess._hop is None) == (kw is rw.FROZEN_TINY)  # 384 projections in the last group: the per-kernel tier
    if kw is rw.FROZEN_TINY:
        with pytest.raises(NotImplementedError):
            model.streaming(batch=B, hop=hop, norm_stats=stats, one_launch=True)
    stats.mu_fb.zero_()  # the session owns copies: the caller's tensors are the caller's again
    stats.mu_sb.zero_()
    for rep in range(2):
        e, m = run_spectra(sess, stft)
        assert torch.equal(real(e), real(off["enh_stft"])), rep
        assert torch.equal(m, off["enh_mag"]), rep
        sess.reset()


# ---- given statistics are what the session divides by ----------------------------------------------------------------------------
@pytest.mark.parametrize("kw,seed", [(TINY_LAP, 41), (TINY_GAUSS, 43)], ids=["laplace", "gauss"])
def test_given_statistics_are_really_used(kw, seed):
    model = build(kw, seed)
    B, T = 3, 36
    _, stft = clips(model, B, T, seed)
    own = model.forward_stft(stft, want_layers=False, return_norm_stats=True)
    other = scaled(own["norm_stats"], (0.5, 1.7, 1.0))
    ref = model.forward_stft(stft, want_layers=False, norm_stats=other, return_norm_stats=True)
    assert torch.equal(ref["norm_stats"].mu_sb, other.mu_sb)  # (what the forward used, as clones)
    for b in range(B):
        same = torch.equal(real(ref["enh_stft"][b]), real(own["enh_stft"][b]))
        assert same == (b == 2), b
    again = model.forward_stft(stft, want_layers=False, norm_stats=own["norm_stats"])  # supplied == computed, bit for bit
    assert torch.equal(real(again["enh_stft"]), real(own["enh_stft"])) and torch.equal(again["enh_mag"], own["enh_mag"])
    for one_launch in (True, False):
        sess = model.streaming(batch=B, norm_stats=other, one_launch=one_launch)
        assert (sess._hop is not None) == one_launch
        e, m = run_spectra(sess, stft)
        assert torch.equal(real(e), real(ref["enh_stft"])), one_launch
        assert torch.equal(m, ref["enh_mag"]), one_launch


def test_statistics_the_engine_refuses():
    import spiking_fullsubnet_amd as pkg
    from spiking_fullsubnet_amd.engine import NormStats
    model = build(TINY_GAUSS, 43)
    _, stft = clips(model, 2, 8, 43)
    st = model.norm_stats(stft)
    with pytest.raises(ValueError, match="sd_fb is missing"):
        model.forward_stft(stft, norm_stats=NormStats(st.mu_fb, st.mu_sb))
    with pytest.raises(ValueError, match="shape"):
        model.forward_stft(stft[:1], norm_stats=st)
    with pytest.raises(ValueError, match="on cuda:0"):
        model.forward_stft(stft, norm_stats=st.to("cpu"))
    with pytest.raises(ValueError, match="shape"):
        model.streaming(batch=3, norm_stats=st)
    live = pkg.SpikingFullSubNet(**rw.LIVE_TINY).eval().to(DEV)
    with pytest.raises(ValueError, match="takes no utterance statistics"):
        live.engine().forward_stft(stft, norm_stats=st)
    with pytest.raises(ValueError, match="computes no utterance statistics"):
        live.engine().forward_stft(stft, return_norm_stats=True)
    with pytest.raises(ValueError, match="takes no utterance statistics"):
        live.streaming(batch=2).set_norm_stats(st)
    sess = model.streaming(batch=2, norm_stats=st)
    with pytest.raises(ValueError, match="shape"):
        sess.set_norm_stats(st, clips=[1])
    with pytest.raises(IndexError):
        sess.set_norm_stats(st.select([0]), clips=[2])
    with pytest.raises(ValueError, match="distinct"):
        sess.set_norm_stats(st, clips=[1, 1])


# ---- trained weights -------------------------------------------------------------------------------------------------------------
def test_zoo_checkpoint_streams_on_samples(golden_dir):
    """model_zoo baseline_s (trained, offline_laplace_norm), its fixture clip cut to 36 frames, its own statistics: samples in, samples
    out, equal to ``model(wave)`` after the three-call delay."""
    g = np.load(os.path.join(golden_dir, "frozen_s_zoo.npz"))
    model = build(rw.FROZEN_S, None, {k[3:]: g[k] for k in g.files if k.startswith("sd/")})
    T = 36
    wave = torch.from_numpy(g["wave"][:, :(T - 1) * 128].copy()).to(DEV)
    y = model(wave)[0].reshape(1, 1, -1)
    stats = model.norm_stats(wave)
    assert torch.equal(stats.mu_fb, model.norm_stats(model._stft(wave)).mu_fb)
    sess = model.streaming(batch=1, waveform=True, norm_stats=stats)
    outs = [sess.step_wave(wave[:, 128 * c:128 * (c + 1)].contiguous()) for c in range(T - 1)]
    sess.check_errors()
    assert not any(bool(o.any()) for o in outs[:3])
    got = torch.cat(outs[3:], -1)
    assert bool(got.any()) and torch.equal(got, y[..., :got.shape[-1]])


# ---- modes -------------------------------------------------------------------------------------------------------------------------
def test_resident_host_session_and_new_statistics():
    """waveform=True, host_io=True, resident=True over 20 hops; then a new utterance with its own statistics through
    set_norm_stats (which ends the resident launch, as reset() does): equal to the offline samples and to a fresh session."""
    model = build(TINY_LAP, 41)
    B, n = 2, 20
    w1, _ = clips(model, B, n + 1, 41)
    w2, _ = clips(model, B, n + 1, 47)
    w2 = w2 * 0.7
    s1, s2 = model.norm_stats(w1), model.norm_stats(w2)
    assert not torch.equal(s1.mu_fb, s2.mu_fb)
    sess = model.streaming(batch=B, waveform=True, host_io=True, resident=True, idle_ms=2000, norm_stats=s1)

    def run(s, w):
        w = w.cpu()
        return torch.cat([s.step_wave_host(w[:, 128 * c:128 * (c + 1)]).clone() for c in range(n)][3:], -1)

    def offline(w):
        y = model(w)[0].reshape(B, 1, -1).cpu()
        return y[..., :(n - 3) * 128]

    assert torch.equal(run(sess, w1), offline(w1))
    assert sess._res is not None
    sess.set_norm_stats(s2)
    assert sess._res is None
    sess.reset()
    got = run(sess, w2)
    sess.close()
    sess.check_errors()
    assert torch.equal(got, offline(w2))
    fresh = model.streaming(batch=B, waveform=True, host_io=True, norm_stats=s2)
    assert torch.equal(got, run(fresh, w2))
    assert not torch.equal(got, offline(w1))


@pytest.mark.parametrize("one_launch", [True, False], ids=["one-launch", "per-kernel"])
def test_spike_counts_of_a_session_with_given_statistics(one_launch):
    from spiking_fullsubnet_amd import metric
    model = build(TINY_LAP, 41)
    B, T = 2, 12
    _, stft = clips(model, B, T, 41)
    stats = scaled(model.norm_stats(stft), (1.3, 0.8))
    cnt = model.forward_stft(stft, want_layers=False, want_counts=True, norm_stats=stats)
    sess = model.streaming(batch=B, norm_stats=stats, one_launch=one_launch, count_spikes=True)
    run_spectra(sess, stft)
    fb_s, sb_s = sess.spike_summary()
    want = [int(s.count) for s in cnt["fb_all"][1:-1]] + [int(s.count) for l in cnt["sb_all"] for s in l[1:-1]]
    got = [int(s.count) for s in fb_s[1:-1]] + [int(s.count) for l in sb_s for s in l[1:-1]]
    assert got == want and sum(want) > 0
    assert metric.compute_synops(fb_s, sb_s, True) == metric.compute_synops(cnt["fb_all"], cnt["sb_all"], True)


# ---- a new utterance with its own statistics on one clip ---------------------------------------------------------------------------
@pytest.mark.parametrize("one_launch", [True, False], ids=["one-launch", "per-kernel"])
def test_per_clip_restart_with_new_statistics(one_launch):
    model = build(TINY_LAP, 41)
    B, T, cut = 3, 36, 12
    _, stft = clips(model, B, T, 41)
    _, new = clips(model, 1, T - cut, 53)
    new = (new * 2.5).contiguous()
    solo = [model.forward_stft(stft[b:b + 1].contiguous(), want_layers=False, return_norm_stats=True) for b in range(B)]
    solo_new = model.forward_stft(new, want_layers=False, return_norm_stats=True)
    stats = cat_stats([s["norm_stats"] for s in solo])
    sess = model.streaming(batch=B, norm_stats=stats, one_launch=one_launch)
    assert (sess._hop is not None) == one_launch
    outs = []
    for t in range(T):
        x = stft[..., t:t + 1].clone()
        if t == cut:
            sess.reset(clips=[1])
            sess.set_norm_stats(solo_new["norm_stats"], clips=[1])
        if t >= cut:
            x[1] = new[0, :, t - cut:t - cut + 1]
        outs.append(sess.step(x.contiguous()))
    sess.check_errors()
    e, m = torch.cat([o[0] for o in outs], -1), torch.cat([o[1] for o in outs], -1)
    for b in (0, 2):  # the clips that go on: untouched by the restart and by the other clip's new statistics
        assert torch.equal(real(e[b]), real(solo[b]["enh_stft"][0])) and torch.equal(m[b], solo[b]["enh_mag"][0]), b
    # clip 1: the first utterance up to the cut -- under ITS statistics, given: the offline forward of those frames with them
    head = model.forward_stft(stft[1:2, :, :cut].contiguous(), want_layers=False, norm_stats=solo[1]["norm_stats"])
    assert torch.equal(real(e[1, ..., :cut]), real(head["enh_stft"][0])) and torch.equal(m[1, ..., :cut], head["enh_mag"][0])
    assert torch.equal(real(e[1, ..., cut:]), real(solo_new["enh_stft"][0])) and torch.equal(m[1, ..., cut:], solo_new["enh_mag"][0])
