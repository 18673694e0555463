"""Per-clip spike counts of streaming sessions: ``model.streaming(..., count_spikes=True)`` and ``session.spike_summary(clips)``.

Every count is compared with the offline forward of the same utterance run alone with ``layer_outputs="tensors"``:
``gt(x, 0).sum()`` of each layer's fp32 spike tensor over the frames the clip has seen -- a path independent of both counting
kernels.  Counts must be equal; ``compute_synops`` must equal the offline ``layer_outputs="counts"`` value exactly and
``compute_neuronops`` the offline value.  Covered: spectral one-launch hops 1 and 3, waveform with device or host I/O, the resident
launch, separate gate weights, the frozen front-end with the cumulative norm, the graph-replayed per-kernel sequence, a batch split
into two launches, per-clip restarts mid-stream, and a session without counting computing the same outputs bit for bit."""
import numpy as np
import pytest
import torch

import refweights as rw
from test_streaming_clips import TINY_CUM, build_module, current, utterances

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def check_summary(model, summ, st, F, shared):
    """summ = spike_summary([b]) of a clip that has seen frames [0, F) of the utterance whose spectrum is st [257, T]."""
    from spiking_fullsubnet_amd import SpikeSummary, metric
    fb_s, sb_s = summ
    x = st[None, :, :F].contiguous()
    eng = model.engine()
    ten = eng.forward_stft(x, want_layers=True)
    cnt = eng.forward_stft(x, want_layers=False, want_counts=True)
    n = 0
    for got, t, c in zip([fb_s] + list(sb_s), [ten["fb_all"]] + list(ten["sb_all"]), [cnt["fb_all"]] + list(cnt["sb_all"])):
        assert len(got) == len(t) == len(c)
        assert got[0].device.type == "meta" and got[-1].device.type == "meta"
        assert tuple(got[0].shape) == tuple(t[0].shape) and tuple(got[-1].shape) == tuple(t[-1].shape)
        for g_, tt, cc in zip(got[1:-1], t[1:-1], c[1:-1]):
            assert isinstance(g_, SpikeSummary) and tuple(g_.shape) == tuple(tt.shape) == tuple(cc.shape)
            assert int(g_.count) == int(torch.gt(tt, 0).sum()), n
            n += 1
    assert n == len(fb_s) - 2 + sum(len(s) - 2 for s in sb_s)
    assert metric.compute_synops(fb_s, sb_s, shared) == metric.compute_synops(cnt["fb_all"], cnt["sb_all"], shared)
    assert metric.compute_neuronops(fb_s, sb_s) == metric.compute_neuronops(ten["fb_all"], ten["sb_all"])
    return [int(s.count) for s in fb_s[1:-1]] + [int(s.count) for l in sb_s for s in l[1:-1]]


def spectral_run(model, B, hop, plan, n_steps, seed, checks, **skw):
    """Steps through per-clip utterances, restarting clips as planned; at each step in `checks` (after that step) takes every
    clip's spike_summary.  Returns outputs, snapshots [(step, frames, {b: (summary, utterance index)})], spectra, session."""
    T = n_steps * hop
    utt = utterances(B, n_steps, plan, seed)
    stfts = {}
    for b in range(B):
        for i, (_, s) in enumerate(utt[b]):
            w = torch.from_numpy(rw.synth_wave(1, T + 1, s)).to(DEV)
            stfts[(b, i)] = model._stft(w)[..., :T].contiguous()[0]
    sess = model.streaming(batch=B, hop=hop, **skw)
    outs, snaps = [], []
    for k in range(n_steps):
        if k in plan:
            sess.reset(clips=plan[k])
        x = torch.stack([stfts[(b, current(utt[b], k)[0])][..., hop * (k - current(utt[b], k)[1]):][..., :hop] for b in range(B)])
        outs.append(sess.step(x.contiguous()))
        if sess.count_spikes and k in checks:
            snaps.append((k, sess.clip_frames.copy(), {b: (sess.spike_summary([b]), current(utt[b], k)[0]) for b in range(B)}))
    sess.check_errors()
    return outs, snaps, stfts, sess


def wave_run(model, B, plan, n_calls, seed, checks, host=False, **skw):
    utt = utterances(B, n_calls, plan, seed)
    waves = {(b, i): torch.from_numpy(rw.synth_wave(1, n_calls + 1, s)[0]) for b in range(B) for i, (_, s) in enumerate(utt[b])}
    specs = {k: model._stft(v[None].to(DEV))[0] for k, v in waves.items()}
    if not host:
        waves = {k: v.to(DEV) for k, v in waves.items()}
    sess = model.streaming(batch=B, waveform=True, host_io=host, idle_ms=2000, **skw)
    outs, snaps = [], []
    for c in range(n_calls):
        if c in plan:
            sess.reset(clips=plan[c])
        x = torch.stack([waves[(b, current(utt[b], c)[0])][128 * (c - current(utt[b], c)[1]):][:128] for b in range(B)])
        outs.append(sess.step_wave_host(x).clone() if host else sess.step_wave(x.contiguous()))
        if sess.count_spikes and c in checks:
            snaps.append((c, sess.clip_frames.copy(), {b: (sess.spike_summary([b]), current(utt[b], c)[0]) for b in range(B)}))
    sess.check_errors()
    return outs, snaps, specs, sess


def check_snaps(model, kw, snaps, specs):
    shared = kw.get("shared_weights", True)
    seen = 0
    for c, frames, summ in snaps:
        for b, (s, i) in summ.items():
            if frames[b] > 0:
                check_summary(model, s, specs[(b, i)], int(frames[b]), shared)
                seen += 1
            else:  # a clip whose utterance has no frame yet: nothing counted
                assert all(int(x.count) == 0 for x in s[0][1:-1]) and tuple(s[0][1].shape)[0] == 0
    assert seen > 0


def same_outputs(a, b):
    for x, y in zip(a, b):
        if isinstance(x, tuple):
            assert all(torch.equal(torch.view_as_real(p) if p.is_complex() else p, torch.view_as_real(q) if q.is_complex() else q)
                       for p, q in zip(x, y))
        else:
            assert torch.equal(x, y)


# ---- spectral step(): one-launch hops and the graph-replayed per-kernel sequence ------------------------------------------------
@pytest.mark.parametrize("front,kw,seed,B,hop,one_launch", [
    ("live", rw.LIVE_TINY, 11, 3, 1, "auto"), ("live", rw.LIVE_TINY, 11, 3, 3, "auto"), ("live", rw.LIVE_M, 5, 3, 1, "auto"),
    ("live", rw.LIVE_TINY_2SPK, 12, 3, 3, "auto"), ("live", rw.LIVE_TINY_UNSHARED, 7, 3, 1, "auto"), ("frozen", TINY_CUM, 35, 3, 2, "auto"),
    ("live", rw.LIVE_TINY, 11, 3, 1, False), ("live", rw.LIVE_TINY_2SPK, 12, 3, 3, False)])
def test_spectral_session_counts_every_clip(front, kw, seed, B, hop, one_launch):
    model = build_module(front, kw, seed)
    plan = {4: [1], 9: [2, 1]}  # clip 0 never restarts; restarts mid-stream, checked before and after
    outs, snaps, specs, sess = spectral_run(model, B, hop, plan, 14, seed, {6, 13}, one_launch=one_launch, count_spikes=True)
    assert (sess._hop is None) == (one_launch is False)
    check_snaps(model, kw, snaps, specs)
    # two clips at once = the sum of each (clips 1 and 2 restarted together: equal clip_frames)
    both = sess.spike_summary([1, 2])
    one, two = sess.spike_summary([1]), sess.spike_summary([2])
    for x, y, z in zip(both[0][1:-1], one[0][1:-1], two[0][1:-1]):
        assert int(x.count) == int(y.count) + int(z.count) and x.shape[1] == 2 * y.shape[1]
    # counting does not perturb the hop: a session without it computes the same outputs, bit for bit
    if kw is rw.LIVE_M or one_launch is False or hop == 3:
        off, _, _, _ = spectral_run(model, B, hop, plan, 14, seed, set(), one_launch=one_launch)
        same_outputs(outs, off)
    # reset(): every count back to zero
    sess.reset()
    fb, sb = sess.spike_summary()
    assert all(int(s.count) == 0 for s in fb[1:-1] + [x for l in sb for x in l[1:-1]])


# ---- waveform: device I/O, host I/O, the resident launch ---------------------------------------------------------------------
@pytest.mark.parametrize("front,kw,seed,B,host,resident", [
    ("live", rw.LIVE_TINY, 11, 3, False, False), ("live", rw.LIVE_M, 5, 2, False, False), ("live", rw.LIVE_TINY_2SPK, 12, 3, False, False),
    ("live", rw.LIVE_TINY_UNSHARED, 7, 2, False, False), ("frozen", TINY_CUM, 35, 3, False, False),
    ("live", rw.LIVE_TINY, 11, 3, True, False), ("live", rw.LIVE_TINY, 11, 3, True, True), ("live", rw.LIVE_TINY_2SPK, 12, 2, True, True),
    ("live", rw.LIVE_TINY_UNSHARED, 7, 2, True, True)])
def test_waveform_session_counts_every_clip(front, kw, seed, B, host, resident):
    model = build_module(front, kw, seed)
    # clip B-1 restarts inside the session's first calls, clip 1 mid-stream; a check right after a restart sees no frame yet
    plan = {2: [B - 1], 11: [1]}
    outs, snaps, specs, sess = wave_run(model, B, plan, 20, seed, {2, 11, 12, 19}, host=host, resident=resident, count_spikes=True)
    check_snaps(model, kw, snaps, specs)
    if kw is rw.LIVE_M or resident:
        off, _, _, sess_off = wave_run(model, B, plan, 20, seed, set(), host=host, resident=resident)
        same_outputs(outs, off)
        sess_off.close()
    sess.close()


# ---- a batch split into two launches -----------------------------------------------------------------------------------------
def test_counts_of_a_batch_split_into_two_launches():
    B = 64
    model = build_module("live", rw.LIVE_M, 5)
    plan = {3: [1, 40], 6: [63]}
    outs, snaps, specs, sess = spectral_run(model, B, 1, plan, 9, 5, {8}, count_spikes=True)
    parts = [(p["b0"], p["nb"]) for p in sess._hop["parts"]]
    assert len(parts) == 2
    keep = {0, 1, 31, 32, 40, 63}  # (a sample of clips from both parts, restarted or not)
    snaps = [(c, f, {b: v for b, v in s.items() if b in keep}) for c, f, s in snaps]
    check_snaps(model, rw.LIVE_M, snaps, specs)
    all_fb, _ = sess.spike_summary([31, 32])  # clips of both parts together
    one, two = sess.spike_summary([31])[0], sess.spike_summary([32])[0]
    assert all(int(x.count) == int(y.count) + int(z.count) for x, y, z in zip(all_fb[1:-1], one[1:-1], two[1:-1]))


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def test_spike_summary_arguments():
    model = build_module("live", rw.LIVE_TINY, 11)
    st = model._stft(torch.from_numpy(rw.synth_wave(3, 9, 11)).to(DEV))[..., :8].contiguous()
    for one_launch in ("auto", False):
        plain = model.streaming(batch=3, one_launch=one_launch)
        plain.step(st[..., :1].contiguous())
        with pytest.raises(RuntimeError):
            plain.spike_summary()
        sess = model.streaming(batch=3, one_launch=one_launch, count_spikes=True)
        for t in range(4):
            if t == 2:
                sess.reset(clips=[1])
            sess.step(st[..., t:t + 1].contiguous())
        with pytest.raises(ValueError):
            sess.spike_summary()  # clip 1 has seen 2 frames, the others 4
        with pytest.raises(ValueError):
            sess.spike_summary([0, 1])
        with pytest.raises(ValueError):
            sess.spike_summary([])
        for bad in ([3], [-1], torch.tensor([5])):
            with pytest.raises(IndexError):
                sess.spike_summary(bad)
        with pytest.raises(TypeError):
            sess.spike_summary([0.5])
        fb, sb = sess.spike_summary([0, 2])
        assert fb[1].shape == (4, 2, rw.LIVE_TINY["fb_hidden_size"])
        assert sess.spike_summary(np.array([1]))[0][1].shape[0] == 2
