"""Per-clip restarts of a batched streaming session: ``StreamingSession.reset(clips=[...])`` starts a new utterance on the listed
clips at their next call while every other clip goes on bit for bit.  A restarted clip must behave exactly like a fresh session
fed the same input: its outputs are compared with the module's offline forward of that utterance run alone (B = 1) and with a
fresh B = 1 session, in every mode the session has (spectral one-launch hops with hop 1 and 3, the graph-replayed per-kernel
sequence, waveform with device or host I/O, the resident launch, batches split into several launches, the cumulative norm)."""
import numpy as np
import pytest
import torch

import refweights as rw

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TINY_CUM = dict(rw.FROZEN_TINY_CUM, sb_df_orders=[3, 2, 1])


def build_module(front, kw, seed):
    import spiking_fullsubnet_amd as pkg
    sd = rw.live_state_dict(kw, seed) if front == "live" else rw.frozen_state_dict(kw, seed)
    m = (pkg.SpikingFullSubNet if front == "live" else pkg.Separator)(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.eval().to(DEV)


def utterances(B, n_calls, plan, seed):
    """plan {call: [clips restarted before that call]} -> per clip the list of (first call, seed) of its utterances."""
    utt = [[(0, seed * 100 + b)] for b in range(B)]
    for c in sorted(plan):
        for b in plan[c]:
            if utt[b][-1][0] != c:
                utt[b].append((c, seed * 100 + 50 + 7 * c + b))
    return utt


def current(utt_b, c):
    """(index, first call) of the utterance clip b is in at call c."""
    i = max(j for j, (r, _) in enumerate(utt_b) if r <= c)
    return i, utt_b[i][0]


def stream_plan_wave(model, sess, B, n_calls, plan, utt, waves, host):
    """Feed every clip the samples of its current utterance, restarting clips as planned; returns [n_calls] outputs [B, S, 128]."""
    outs = []
    for c in range(n_calls):
        if c in plan:
            sess.reset(clips=plan[c])
        x = torch.stack([waves[(b, current(utt[b], c)[0])][128 * (c - current(utt[b], c)[1]):][:128] for b in range(B)])
        if host:
            outs.append(sess.step_wave_host(x.cpu()).clone())
        else:
            outs.append(sess.step_wave(x.contiguous()))
    return outs


def check_wave(model, kw_S, B, n_calls, plan, utt, waves, outs, make_fresh):
    """Clip b, utterance u started at call r: zeros for calls r .. r+2, then the offline forward of u alone three calls late; the
    same samples from a fresh B = 1 session fed u."""
    for b in range(B):
        for i, (r, _) in enumerate(utt[b]):
            end = utt[b][i + 1][0] if i + 1 < len(utt[b]) else n_calls
            w = waves[(b, i)]
            y = model(w[None].to(DEV))[0].reshape(1, kw_S, -1)[0].cpu()
            got = torch.stack([outs[c][b].cpu() for c in range(r, end)])  # [n, S, 128]
            assert not bool(got[:3].any()), (b, i)
            for k in range(3, end - r):
                assert torch.equal(got[k], y[:, 128 * (k - 3):128 * (k - 2)]), (b, i, r, k)
            if i > 0 or b == 0:  # restarted clips (and one clip that never restarts) against a fresh session
                fresh = make_fresh()
                ref = [fresh.step_wave(w[128 * k:128 * (k + 1)][None].to(DEV).contiguous()).cpu() for k in range(end - r)]
                assert torch.equal(got, torch.stack(ref)[:, 0]), (b, i)


def wave_case(front, kw, seed, B, plan, n_calls=36, host=False, resident=False):
    model = build_module(front, kw, seed)
    S = kw.get("num_spks", 1)
    utt = utterances(B, n_calls, plan, seed)
    waves = {(b, i): torch.from_numpy(rw.synth_wave(1, n_calls + 1, s)[0]) for b in range(B) for i, (_, s) in enumerate(utt[b])}
    if not host:
        waves = {k: v.to(DEV) for k, v in waves.items()}
    sess = model.streaming(batch=B, waveform=True, host_io=host, resident=resident, idle_ms=2000)
    return model, S, utt, waves, sess


# ---- (1) waveform, device I/O ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,seed,B", [(rw.LIVE_TINY, 11, 4), (rw.LIVE_M, 5, 3), (rw.LIVE_TINY_2SPK, 12, 3)])
def test_waveform_clips_restart_inside_the_hop(kw, seed, B):
    # clip 0 never restarts; clip B-1 restarts at call 2 (inside the session's own first three calls), clips 1 and 2 together at
    # call 14, clip 2 also at call 9 and clip 1 again at call 25
    plan = {2: [B - 1], 9: [2], 14: [1, 2], 25: [1]}
    model, S, utt, waves, sess = wave_case("live", kw, seed, B, plan)
    outs = stream_plan_wave(model, sess, B, 36, plan, utt, waves, host=False)
    sess.check_errors()
    assert sess.clip_calls.tolist() == [36 - utt[b][-1][0] for b in range(B)]
    assert sess.clip_frames.tolist() == [35 - utt[b][-1][0] for b in range(B)]
    check_wave(model, S, B, 36, plan, utt, waves, outs, lambda: model.streaming(batch=1, waveform=True))


# ---- (2) spectral step() --------------------------------------------------------------------------------------------------------
def spectral_case(front, kw, seed, B, hop, plan, n_steps, fresh_kw, stall=None, **skw):
    model = build_module(front, kw, seed)
    T = n_steps * hop
    utt = utterances(B, n_steps, plan, seed)
    stfts, offs = {}, {}
    for b in range(B):
        for i, (_, s) in enumerate(utt[b]):
            w = torch.from_numpy(rw.synth_wave(1, T + 1, s)).to(DEV)
            st = model._stft(w)[..., :T].contiguous()
            stfts[(b, i)] = st[0]
            offs[(b, i)] = model.engine().forward_stft(st, want_layers=False)
    sess = model.streaming(batch=B, hop=hop, **skw)
    if stall is not None:
        stall()
    outs = []
    for k in range(n_steps):
        if k in plan:
            sess.reset(clips=plan[k])
        x = torch.stack([stfts[(b, current(utt[b], k)[0])][..., hop * (k - current(utt[b], k)[1]):][..., :hop] for b in range(B)])
        outs.append(sess.step(x.contiguous()))
    if stall is not None:
        assert not torch.cuda.current_stream().query()  # the steps were still queued behind the stall
    sess.check_errors()
    assert sess.clip_frames.tolist() == [hop * (n_steps - utt[b][-1][0]) for b in range(B)]
    for b in range(B):
        for i, (r, _) in enumerate(utt[b]):
            end = utt[b][i + 1][0] if i + 1 < len(utt[b]) else n_steps
            e = torch.cat([outs[k][0][b] for k in range(r, end)], -1)
            m = torch.cat([outs[k][1][b] for k in range(r, end)], -1)
            off = offs[(b, i)]
            n = e.shape[-1]
            assert torch.equal(torch.view_as_real(e), torch.view_as_real(off["enh_stft"][0][..., :n])), (b, i)
            assert torch.equal(m, off["enh_mag"][0][..., :n]), (b, i)
            if i > 0:
                fresh = model.streaming(batch=1, hop=hop, **fresh_kw)
                ref = [fresh.step(stfts[(b, i)][None, :, hop * k:hop * (k + 1)].contiguous())[0] for k in range(end - r)]
                assert torch.equal(torch.view_as_real(e), torch.view_as_real(torch.cat(ref, -1)[0])), (b, i)
    return sess


@pytest.mark.parametrize("kw,seed,B,hop,one_launch", [(rw.LIVE_TINY, 11, 4, 1, "auto"), (rw.LIVE_TINY, 11, 3, 3, "auto"),
                                                      (rw.LIVE_M, 5, 3, 1, "auto"), (rw.LIVE_TINY_2SPK, 12, 3, 3, "auto"),
                                                      (rw.LIVE_TINY, 11, 3, 1, False), (rw.LIVE_TINY_2SPK, 12, 3, 3, False)])
def test_spectral_clips_restart(kw, seed, B, hop, one_launch):
    plan = {1: [2], 7: [1, 2], 12: [1]}
    sess = spectral_case("live", kw, seed, B, hop, plan, 20, dict(one_launch=one_launch), one_launch=one_launch, graph=True)
    assert (sess._hop is None) == (one_launch is False)
    if one_launch is False:
        assert sess._graph is not None


# ---- (3) the cumulative norm: per-clip running sums and denominators -----------------------------------------------------------------
@pytest.mark.parametrize("kw,seed,B,hop", [(TINY_CUM, 35, 3, 1), (TINY_CUM, 35, 3, 2), (rw.FROZEN_M_CUM, 36, 2, 1)])
def test_cumulative_norm_counts_frames_per_clip(kw, seed, B, hop):
    plan = {3: [1], 9: [B - 1], 14: [1]}
    spectral_case("frozen", kw, seed, B, hop, plan, 20, {})
    if hop == 1:
        model, S, utt, waves, sess = wave_case("frozen", kw, seed, B, plan, n_calls=24)
        outs = stream_plan_wave(model, sess, B, 24, plan, utt, waves, host=False)
        sess.check_errors()
        check_wave(model, S, B, 24, plan, utt, waves, outs, lambda: model.streaming(batch=1, waveform=True))


# ---- (4) host I/O and the resident launch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("front,kw,seed,B,resident", [("live", rw.LIVE_TINY, 11, 3, False), ("live", rw.LIVE_TINY, 11, 3, True),
                                                      ("live", rw.LIVE_TINY_2SPK, 12, 3, True), ("frozen", TINY_CUM, 35, 3, True)])
def test_host_io_and_resident_clips_restart(front, kw, seed, B, resident):
    plan = {2: [B - 1], 9: [2], 14: [1, 2], 15: [2], 25: [1]}
    model, S, utt, waves, sess = wave_case(front, kw, seed, B, plan, host=True, resident=resident)
    outs = []
    for c in range(36):
        if c in plan:
            res = sess._res
            sess.reset(clips=plan[c])
            if resident and c > 1:  # the resident launch serves on: not ended, not restarted
                assert sess._res is res and res is not None
                assert sess._hop["host"]["bell_np"][1] == 0
        x = torch.stack([waves[(b, current(utt[b], c)[0])][128 * (c - current(utt[b], c)[1]):][:128] for b in range(B)])
        o = sess.step_wave_host(x)
        assert o.device.type == "cpu"
        outs.append(o.clone())
    sess.check_errors()
    check_wave(model, S, B, 36, plan, utt, waves, outs, lambda: model.streaming(batch=1, waveform=True))
    sess.close()


# ---- (5) a batch split into several launches -----------------------------------------------------------------------------------------
def test_multi_part_batch_restarts_in_every_part():
    # (LIVE_M: B = 64 asks for 284 workgroups, more than one launch may hold on the chip -- two parts of 32 clips)
    B = 64
    model = build_module("live", rw.LIVE_M, 5)
    probe = model.streaming(batch=B)
    parts = [(p["b0"], p["nb"]) for p in probe._hop["parts"]]
    assert len(parts) > 1
    del probe
    plan = {}
    for j, (b0, nb) in enumerate(parts):
        plan.setdefault(3 + 2 * j, []).append(b0 + nb - 1)
        plan.setdefault(9, []).append(b0 + 1)
    spectral_case("live", rw.LIVE_M, 5, B, 1, plan, 16, {})


# ---- (6) restarts queued between unsynchronised steps ----------------------------------------------------------------------------------
def test_restarts_apply_in_stream_order_without_synchronisation():
    """The host runs far ahead of the device (a long matrix product queued first): every reset(clips) is issued while launches
    before it are still queued, and none of them may see the new origin; restarts on consecutive calls included."""
    kw, seed, B = rw.LIVE_TINY, 11, 4
    plan = {1: [3], 2: [3], 5: [0, 1], 6: [1], 7: [1], 13: [2, 2, 0]}
    model, S, utt, waves, sess = wave_case("live", kw, seed, B, plan, n_calls=24)
    a, p = torch.randn((4096, 4096), device=DEV), torch.empty((4096, 4096), device=DEV)
    torch.cuda.synchronize()

    def stall():
        for _ in range(48):
            torch.mm(a, a, out=p)  # (the values do not matter: the device is busy for tens of milliseconds)

    stall()
    outs = stream_plan_wave(model, sess, B, 24, plan, utt, waves, host=False)
    assert not torch.cuda.current_stream().query()  # the steps above were still queued behind the product
    sess.check_errors()
    check_wave(model, S, B, 24, plan, utt, waves, outs, lambda: model.streaming(batch=1, waveform=True))
    # spectral hops, same rule
    plan2 = {2: [0], 3: [0, 2], 8: [1]}
    spectral_case("live", kw, seed, B, 1, plan2, 12, {}, stall=stall)


# ---- (7) argument checks; reset() and reset([]) --------------------------------------------------------------------------------------
def test_reset_clips_arguments_and_full_reset():
    kw, seed, B, T = rw.LIVE_TINY, 11, 3, 12
    model = build_module("live", kw, seed)
    w = torch.from_numpy(rw.synth_wave(B, T + 1, seed)).to(DEV)
    st = model._stft(w)[..., :T].contiguous()
    off = model.engine().forward_stft(st, want_layers=False)
    for one_launch in ("auto", False):
        sess = model.streaming(batch=B, one_launch=one_launch)
        for bad in ([B], [-1], [0, B + 5], torch.tensor([B])):
            with pytest.raises(IndexError):
                sess.reset(clips=bad)
        with pytest.raises(TypeError):
            sess.reset(clips=[0.5])
        outs = []
        for t in range(T):
            if t == 4:
                sess.reset(clips=[])  # nothing happens
                sess.reset(clips=torch.tensor([], dtype=torch.int64))
            if t == 6:
                sess.reset(clips=[1, 2])
            outs.append(sess.step(st[..., t:t + 1].contiguous())[0])
        e = torch.cat(outs, -1)
        assert torch.equal(torch.view_as_real(e[0]), torch.view_as_real(off["enh_stft"][0]))  # clip 0 untouched by either reset
        assert torch.equal(torch.view_as_real(e[1:, ..., :6]), torch.view_as_real(off["enh_stft"][1:, ..., :6]))
        assert sess.clip_frames.tolist() == [T, T - 6, T - 6]
        with pytest.raises(ValueError):
            sess.clip_frames[0] = 0  # read-only
        sess.reset()  # everything: the whole batch starts again
        assert sess.clip_frames.tolist() == [0, 0, 0] and sess.frames_done == 0
        outs = [sess.step(st[..., t:t + 1].contiguous())[0] for t in range(T)]
        sess.check_errors()
        assert torch.equal(torch.view_as_real(torch.cat(outs, -1)), torch.view_as_real(off["enh_stft"]))
