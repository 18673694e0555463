"""``step(frames, clips=...)`` / ``step_wave`` / ``step_wave_host`` with HELD clips (``sfsn_stream_hop_held``; the per-kernel tier's
save / replay / restore): a hop that advances only some clips of the batch leaves every other clip exactly where it was.

Everything is ``torch.equal`` -- the held launch runs the same instructions on the same rows as a launch without holds, so nothing here
needs a tolerance.  The schedule is tests/holdref.py's (its properties are asserted on the CPU by tests/test_stream_hold_host.py); the
fixtures, seeds, spectra and waves are tests/primeref.py's.  Clip b's j-th active tick is fed its frames [j hop, (j + 1) hop) and must
return row b of call j of a CONTROL session of the same batch that steps every clip every time; the held rows of every input are NaN."""
import numpy as np
import pytest
import torch

import holdref as hd
import primeref as pr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = hd.B
_models = {}


def model_of(name, seed=None):
    key = (name, seed)
    if key not in _models:
        import spiking_fullsubnet_amd as pkg
        front, kw, _ = pr.FIXTURES[name]
        m = (pkg.SpikingFullSubNet if front == "live" else pkg.Separator)(**kw)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in pr.state_dict(name, seed).items()}, strict=True)
        _models[key] = m.eval().to(DEV)
    return _models[key]


def own_stats(name, model, stft):
    """The clips' own offline-norm statistics where the fixture's norm needs them (as tests/test_stream_advance.py)."""
    if name != "frozen_tiny":
        return None
    return model.engine().forward_stft(stft, want_layers=False, return_norm_stats=True)["norm_stats"]


def real(x):
    return torch.view_as_real(x) if x.is_complex() else x


def counts_of(summary):
    fb_all, sb_all = summary
    return [int(x.count) for x in fb_all[1:-1]] + [int(x.count) for a in sb_all for x in a[1:-1]]


def same_state(sa, sb, where):
    """Two ``export_state`` results, section by section -- layer 0's membranes included: held or not, it is the same kernel."""
    assert sa.layout == sb.layout and sa.frames.tolist() == sb.frames.tolist(), where
    assert (sa.calls is None) == (sb.calls is None) and (sa.calls is None or sa.calls.tolist() == sb.calls.tolist()), where
    for name, lo, hi in sa.layout:
        assert torch.equal(sa.blob[:, lo:hi], sb.blob[:, lo:hi]), f"{where}: section {name}"


def differs(sa, sb):
    return [name for name, lo, hi in sa.layout if not torch.equal(sa.blob[:, lo:hi], sb.blob[:, lo:hi])]


def nan_frames(sess, rows):
    """[B, F, hop] complex64, NaN everywhere but the given {clip: [F, hop] frames}."""
    x = torch.full((sess.B, sess.F, sess.hop), float("nan"), dtype=torch.complex64, device=DEV)
    for b, v in rows.items():
        x[b] = v
    return x


def frames_of(stft, b, j, hop):
    return stft[b, :, j * hop:(j + 1) * hop]


def run_schedule(sess, stft):
    """THE schedule on a spectral session -> {clip: [(enh row, mag row)] per active tick}; held output rows are checked to be zero."""
    hop, got = sess.hop, {b: [] for b in range(B)}
    for t, fed in hd.feed():
        if t in hd.RESET_BEFORE:
            sess.reset(clips=hd.RESET_BEFORE[t])
        e, m = sess.step(nan_frames(sess, {b: frames_of(stft, b, j, hop) for b, j in fed.items()}), clips=sorted(fed))
        assert e.shape[0] == m.shape[0] == B
        for b in range(B):
            if b in fed:
                got[b].append((e[b], m[b]))
            else:
                assert not bool(real(e[b]).any()) and not bool(m[b].any()), f"tick {t}: held clip {b} has output"
    return got


def run_control(sess, stft, calls):
    """Every clip, every call; clip b is reset where the schedule resets it (holdref.resets)."""
    hop, out = sess.hop, []
    for j in range(calls):
        for b, jr in hd.resets().items():
            if jr == j:
                sess.reset(clips=[b])
        out.append(sess.step(stft[..., j * hop:(j + 1) * hop].contiguous()))
    return out


# ---- 1, 3, 7. the schedule against a control: outputs, bookkeeping, end state, counts --------------------------------------------
CASES = [(n, hop, ol) for n in pr.FIXTURES for hop in (1, 2) for ol in (True, False)
         if not (n == "frozen_tiny_cum" and not ol)]  # (the cumulative norm streams through the one-launch hop only)


@pytest.mark.parametrize("name,hop,one_launch", CASES, ids=[f"{n}-hop{h}-{'one' if o else 'graph'}" for n, h, o in CASES])
def test_the_schedule_equals_a_control_that_steps_every_clip(name, hop, one_launch):
    model = model_of(name)
    stft = torch.from_numpy(pr.spectra(name, B)).to(DEV)
    stats = own_stats(name, model, stft)
    kw = dict(batch=B, hop=hop, one_launch=one_launch, graph=True, count_spikes=True, norm_stats=stats)
    control, sess = model.streaming(**kw), model.streaming(**kw)
    assert (sess._hop is not None) == one_launch and (one_launch or sess._graph is not None)
    calls = hd.active_ticks()[0]
    want = run_control(control, stft, calls)
    control.check_errors()
    # the premise (asserted by the existing suite for these seeds): the control is the offline forward -- clip 2 up to its reset
    off = model.engine().forward_stft(stft, want_layers=False, **({} if stats is None else dict(norm_stats=stats)))
    ce, cm = torch.cat([w[0] for w in want], -1), torch.cat([w[1] for w in want], -1)
    n2 = hd.resets()[2] * hop
    assert torch.equal(real(ce[:2]), real(off["enh_stft"][:2, ..., :calls * hop])) and torch.equal(cm[:2], off["enh_mag"][:2, ..., :calls * hop])
    assert torch.equal(real(ce[2, ..., :n2]), real(off["enh_stft"][2, ..., :n2])) and torch.equal(cm[2, ..., :n2], off["enh_mag"][2, ..., :n2])
    got = run_schedule(sess, stft)
    sess.check_errors()
    for b in range(B):
        assert len(got[b]) == calls
        for j, (e, m) in enumerate(got[b]):
            assert torch.equal(real(e), real(want[j][0][b])) and torch.equal(m, want[j][1][b]), f"clip {b}, active tick {j}"
    # bookkeeping: the active ticks of each clip's current utterance, and nothing else
    ages = [calls, calls, calls - hd.resets()[2]]
    assert sess.clip_frames.tolist() == [a * hop for a in ages] == control.clip_frames.tolist()
    # 3. the end state: every section, layer 0's membranes included; and the spike counts
    same_state(sess.export_state(), control.export_state(), "after the schedule")
    for b in range(B):
        assert counts_of(sess.spike_summary([b])) == counts_of(control.spike_summary([b])), b
    assert sum(counts_of(sess.spike_summary([0]))) > 0


def test_an_empty_list_launches_nothing_and_returns_zeros():
    model = model_of("live_tiny")
    stft = torch.from_numpy(pr.spectra("live_tiny", B)).to(DEV)
    for one_launch in (True, False):
        sess = model.streaming(batch=B, one_launch=one_launch, count_spikes=True)
        sess.step(stft[..., :1].contiguous())
        before, k = sess.export_state(), (sess._hop["parts"][0]["desc"].launch_index if one_launch else None)
        e, m = sess.step(nan_frames(sess, {}), clips=[])
        assert e.shape == (B, 1, sess.F, 1) and not bool(real(e).any()) and not bool(m.any())
        assert sess.frames_done == 1 and sess.clip_frames.tolist() == [1] * B
        assert not one_launch or sess._hop["parts"][0]["desc"].launch_index == k
        same_state(before, sess.export_state(), "an empty tick")


# ---- 2. a held launch changes nothing of the held clip -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,one_launch", [("live_tiny_2spk", True), ("live_tiny_2spk", False), ("frozen_tiny_cum", True),
                                             ("live_tiny_unshared", True)])
def test_a_held_launch_changes_nothing_of_the_held_clip(name, one_launch):
    model = model_of(name)
    stft = torch.from_numpy(pr.spectra(name, B)).to(DEV)
    kw = dict(batch=B, one_launch=one_launch, count_spikes=True)
    sess, control = model.streaming(**kw), model.streaming(**kw)
    for j in range(3):
        sess.step(stft[..., j:j + 1].contiguous())
        control.step(stft[..., j:j + 1].contiguous())
    b = 1
    parities = []
    for j in (3, 4):  # launch 3 (odd) and launch 4 (even) both hold clip b
        if one_launch:
            parities.append(sess._hop["parts"][0]["desc"].launch_index & 1)
        before, cbefore = sess.export_state(clips=[b]), control.export_state(clips=[b])
        sess.step(nan_frames(sess, {c: stft[c, :, j:j + 1] for c in range(B) if c != b}), clips=[c for c in range(B) if c != b])
        control.step(stft[..., j:j + 1].contiguous())
        same_state(before, sess.export_state(clips=[b]), f"launch {j}")
        # (the same tick without the hold does change them: h or c of some layer, the history, the counts)
        changed = differs(cbefore, control.export_state(clips=[b]))
        assert "hist" in changed and ("slots" in changed or "rows" in changed), changed
        assert any(n.endswith(".c") for n in changed), changed
        if name == "frozen_tiny_cum":
            assert "cum" in changed
    assert not one_launch or sorted(parities) == [0, 1]
    sess.check_errors()
    # ... and the others went on: clips 0 and 2 are where the control's are
    same_state(sess.export_state(clips=[0, 2]), control.export_state(clips=[0, 2]), "the active clips")
    assert sess.clip_frames.tolist() == [5, 3, 5]


# ---- 4. waveform ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,host_io", [(n, h) for n in pr.WAVE_FIXTURES for h in (False, True)])
def test_the_schedule_on_waveform_calls(name, host_io):
    model = model_of(name, pr.WAVE_FIXTURES[name])
    S = pr.FIXTURES[name][1].get("num_spks", 1)
    w = torch.from_numpy(pr.waves(name, B)).to(DEV)
    kw = dict(batch=B, waveform=True, count_spikes=True, host_io=host_io)
    control, sess = model.streaming(**kw), model.streaming(**kw)

    def call(s, x, **k):
        return s.step_wave_host(x.cpu(), **k).to(DEV).clone() if host_io else s.step_wave(x, **k)

    calls = hd.active_ticks()[0]
    want = []
    for j in range(calls):
        for b, jr in hd.resets().items():
            if jr == j:
                control.reset(clips=[b])
        want.append(call(control, w[:, 128 * j:128 * (j + 1)].contiguous()))
    control.check_errors()
    y = model(w)[0].reshape(B, S, -1)
    assert not any(bool(o.any()) for o in want[:3])  # the three leading zero calls ...
    for j in range(3, calls):                        # ... then the offline model's samples of three calls earlier (clip 2: up to its reset)
        rows = [0, 1] + ([2] if j < hd.resets()[2] else [])
        assert torch.equal(want[j][rows], y[rows, :, 128 * (j - 3):128 * (j - 2)]), j
    assert 0 not in hd.TICKS[0]  # clip 0 is held at the session's first call, which launches nothing
    seen = [0] * B
    for t, fed in hd.feed():
        if t in hd.RESET_BEFORE:
            sess.reset(clips=hd.RESET_BEFORE[t])
        x = torch.full((B, 128), float("nan"), dtype=torch.float32, device=DEV)
        for b, j in fed.items():
            x[b] = w[b, 128 * j:128 * (j + 1)]
        out = call(sess, x, clips=sorted(fed))  # (host_io: the wait on the done words returns, held clips included)
        assert out.shape == (B, S, 128)
        for b in range(B):
            if b in fed:
                assert torch.equal(out[b], want[fed[b]][b]), f"tick {t}: clip {b}, its call {fed[b]}"
                seen[b] += 1
            else:
                assert not bool(out[b].any()), f"tick {t}: held clip {b} has output"
    sess.check_errors()
    ages = [calls, calls, calls - hd.resets()[2]]
    assert seen == [calls] * B and sess.clip_calls.tolist() == ages == control.clip_calls.tolist()
    assert sess.clip_frames.tolist() == [a - 1 for a in ages]
    same_state(sess.export_state(), control.export_state(), "after the schedule")
    for b in range(B):
        assert counts_of(sess.spike_summary([b])) == counts_of(control.spike_summary([b])), b


def test_a_held_waveform_call_changes_nothing_of_the_held_clip():
    name = "live_tiny_2spk"
    model = model_of(name, pr.WAVE_FIXTURES[name])
    w = torch.from_numpy(pr.waves(name, B)).to(DEV)
    sess = model.streaming(batch=B, waveform=True, count_spikes=True)
    for j in range(5):
        sess.step_wave(w[:, 128 * j:128 * (j + 1)].contiguous())
    for j in (5, 6):  # both launch parities
        before = sess.export_state(clips=[2])
        x = w[:, 128 * j:128 * (j + 1)].clone()
        x[2] = float("nan")
        sess.step_wave(x, clips=[0, 1])
        after = sess.export_state(clips=[2])
        same_state(before, after, f"call {j}")
        assert {"wave", "ola"} <= {n for n, _, _ in after.layout}
    sess.check_errors()
    assert sess.clip_calls.tolist() == [7, 7, 5]


# ---- 5. combinations, also with the launch index near the wrap --------------------------------------------------------------------
def control_outputs(model, stft, hop=1):
    s = model.streaming(batch=B, hop=hop, count_spikes=True)
    outs = [s.step(stft[..., k:k + hop].contiguous()) for k in range(0, pr.T, hop)]
    s.check_errors()
    return torch.cat([o[0] for o in outs], -1), torch.cat([o[1] for o in outs], -1)


def wrapped(sess, wrap):
    if wrap:  # the launch counter about to wrap, or the origins at the edge of the int32 the session's tensor holds them in
        for part in sess._hop["parts"]:
            part["desc"].launch_index = wrap
            part["origin"].fill_(sess._as_i32(wrap))
    return sess


def tick(sess, stft, at, hold=()):
    """One tick: clip b takes its frame at[b] unless held; -> (enh, mag)."""
    rows = {b: stft[b, :, at[b]:at[b] + 1] for b in range(B) if b not in hold}
    out = sess.step(nan_frames(sess, rows), clips=sorted(rows)) if hold else sess.step(nan_frames(sess, rows))
    for b in rows:
        at[b] += 1
    return out


def check_tick(out, es, ms, at_before, hold, where):
    for b in range(B):
        if b in hold:
            assert not bool(real(out[0][b]).any()) and not bool(out[1][b].any()), where
        else:
            t = at_before[b]
            assert torch.equal(real(out[0][b]), real(es[b, ..., t:t + 1])) and torch.equal(out[1][b], ms[b, ..., t:t + 1]), (where, b, t)


COMBOS = [(True, 0), (True, 2 ** 32 - 3), (True, 2 ** 31 + 3), (False, 0)]


@pytest.mark.parametrize("one_launch,wrap", COMBOS)
def test_hold_then_advance_on_the_held_clip_then_step(one_launch, wrap):
    model = model_of("live_tiny")
    stft = torch.from_numpy(pr.spectra("live_tiny", B)).to(DEV)
    es, ms = control_outputs(model, stft)
    sess = wrapped(model.streaming(batch=B, one_launch=one_launch, count_spikes=True), wrap)
    at, N = [0] * B, 9
    for i in range(4):
        hold = (1,) if i >= 2 else ()
        before = list(at)
        check_tick(tick(sess, stft, at, hold), es, ms, before, hold, f"tick {i}")
    assert at == [4, 2, 4] and sess.clip_frames.tolist() == at
    e1, m1 = sess.advance(stft[1:2, :, 2:2 + N], clips=[1])  # the held clip takes a backlog from where it was held
    assert torch.equal(real(e1), real(es[1:2, ..., 2:2 + N])) and torch.equal(m1, ms[1:2, ..., 2:2 + N])
    at[1] += N
    for i in range(6):
        hold = (1,) if i == 0 else ((0, 2) if i == 3 else ())
        before = list(at)
        check_tick(tick(sess, stft, at, hold), es, ms, before, hold, f"tick {i} behind the backlog")
    sess.check_errors()
    assert sess.clip_frames.tolist() == at == [9, 16, 9]


@pytest.mark.parametrize("one_launch,wrap", COMBOS)
def test_hold_then_move_the_clip_to_another_slot_then_step(one_launch, wrap):
    model = model_of("live_tiny")
    stft = torch.from_numpy(pr.spectra("live_tiny", B)).to(DEV)
    es, ms = control_outputs(model, stft)
    sess = wrapped(model.streaming(batch=B, one_launch=one_launch, count_spikes=True), wrap)
    at = [0] * B
    for i in range(5):
        hold = (1,) if i in (1, 2) else ((0,) if i == 4 else ())
        before = list(at)
        check_tick(tick(sess, stft, at, hold), es, ms, before, hold, f"tick {i}")
    assert at == [4, 3, 5]
    state = sess.export_state(clips=[1])  # clip 1 (3 frames, twice held) moves to slot 2; clip 0 (just held) to slot 1
    state0 = sess.export_state(clips=[0])
    sess.import_state(state, clips=[2])
    sess.import_state(state0, clips=[1])
    assert sess.clip_frames.tolist() == [4, 4, 3]
    src = [0, 0, 1]  # whose utterance each slot continues
    at = [4, 4, 3]
    for i in range(6):
        hold = (2,) if i == 1 else ()
        x = nan_frames(sess, {b: stft[src[b], :, at[b]:at[b] + 1] for b in range(B) if b not in hold})
        e, m = sess.step(x, clips=[b for b in range(B) if b not in hold])
        for b in range(B):
            if b in hold:
                assert not bool(real(e[b]).any())
                continue
            assert torch.equal(real(e[b]), real(es[src[b], ..., at[b]:at[b] + 1])) and torch.equal(m[b], ms[src[b], ..., at[b]:at[b] + 1]), (i, b)
            at[b] += 1
    sess.check_errors()
    assert sess.clip_frames.tolist() == at == [10, 10, 8]


@pytest.mark.parametrize("one_launch,wrap", COMBOS)
def test_hold_around_prime(one_launch, wrap):
    model = model_of("live_tiny")
    stft = torch.from_numpy(pr.spectra("live_tiny", B)).to(DEV)
    es, ms = control_outputs(model, stft)
    sess = wrapped(model.streaming(batch=B, one_launch=one_launch, count_spikes=True), wrap)
    at, P = [0] * B, 17
    for i in range(3):
        hold = (1,) if i == 2 else ()
        before = list(at)
        check_tick(tick(sess, stft, at, hold), es, ms, before, hold, f"tick {i}")
    p, _ = sess.prime(stft[1:2, :, :P], clips=[1])  # the held clip starts over from a recorded prefix of its own utterance
    assert torch.equal(real(p), real(es[1:2, ..., :P]))
    at[1] = P
    for i in range(6):
        hold = (1,) if i in (0, 1) else ()  # held in the two launches right behind the prefix (both parities)
        before = list(at)
        check_tick(tick(sess, stft, at, hold), es, ms, before, hold, f"tick {i} behind the prefix")
    sess.check_errors()
    assert sess.clip_frames.tolist() == at == [9, P + 4, 9]


# ---- 6. a session cut into parts -----------------------------------------------------------------------------------------------
def test_a_session_cut_into_parts_sends_each_part_its_slice_of_the_mask():
    name, Bb = "live_tiny", 256
    model = model_of(name)
    stft = torch.from_numpy(pr.spectra(name, 3)).to(DEV)
    off = model.engine().forward_stft(stft, want_layers=False)
    sess = model.streaming(batch=Bb, count_spikes=True)
    parts = [(p["b0"], p["nb"]) for p in sess._hop["parts"]]
    assert len(parts) > 1, "256 clips ask for more workgroups than one launch may hold"
    cut = parts[1][0]
    clips = [5, cut - 1, cut]  # tracked clips (fed the three spectra), either side of the cut; every other clip hears silence
    part0, part1 = set(range(parts[0][0], parts[0][0] + parts[0][1])), set(range(parts[1][0], parts[1][0] + parts[1][1]))
    holds = [set(), {cut - 1, cut},  # clips on either side of the cut
             part0,                  # a whole part held; every other part with nobody held
             part1, {5}, set(), set(), set(), set(), set()]
    at = [0, 0, 0]
    used = set()
    for i, held in enumerate(holds):
        x = torch.zeros((Bb, sess.F, 1), dtype=torch.complex64, device=DEV)
        if held:
            x[sorted(held)] = float("nan")
        for c, b in enumerate(clips):
            if b not in held:
                x[b] = stft[c, :, at[c]:at[c] + 1]
        launched = []
        for nm in ("sfsn_stream_hop", "sfsn_stream_hop_held"):
            launched.append(_counted(sess.eng.lib, nm))
        try:
            e, m = sess.step(x, clips=[b for b in range(Bb) if b not in held]) if held else sess.step(x)
        finally:
            for c_ in launched:
                c_.restore()
        n_held_parts = sum(1 for b0, nb in parts if any(b0 <= b < b0 + nb for b in held))
        assert launched[1].calls == n_held_parts and launched[0].calls == len(parts) - n_held_parts, i  # one launch per part, always
        used.add((launched[0].calls > 0, launched[1].calls > 0))
        for c, b in enumerate(clips):
            if b in held:
                assert not bool(real(e[b]).any()) and not bool(m[b].any()), (i, b)
            else:
                t = at[c]
                assert torch.equal(real(e[b]), real(off["enh_stft"][c, ..., t:t + 1])) and torch.equal(m[b], off["enh_mag"][c, ..., t:t + 1]), (i, b)
                at[c] += 1
        assert not held or not bool(real(e[sorted(held)]).any() or m[sorted(held)].any())
    sess.check_errors()
    assert used == {(True, False), (True, True)} or used == {(True, False), (True, True), (False, True)}
    n = len(holds) - 2
    assert at == [n] * 3 and sess.clip_frames[clips].tolist() == at and sess.clip_frames[0] == len(holds) - 1
    one = model.streaming(batch=3, count_spikes=True)
    for t in range(n):
        one.step(stft[..., t:t + 1].contiguous())
    assert counts_of(sess.spike_summary(clips)) == counts_of(one.spike_summary())
    same_state(sess.export_state(clips=clips), one.export_state(), "the tracked clips")


class _counted:
    """Counts the calls of one entry point of the loaded library (the session looks it up by name on every launch)."""

    def __init__(self, lib, name):
        self.lib, self.name, self.fn, self.calls = lib, name, getattr(lib, name), 0
        setattr(lib, name, self)

    def __call__(self, *a):
        self.calls += 1
        return self.fn(*a)

    def restore(self):
        setattr(self.lib, self.name, self.fn)


# ---- 7. the cumulative norm: a held clip's frame count does not move ---------------------------------------------------------------
def test_cumulative_norm_divides_by_the_held_clips_own_frame_count():
    name = "frozen_tiny_cum"
    model = model_of(name)
    stft = torch.from_numpy(pr.spectra(name, B)).to(DEV)
    off = model.engine().forward_stft(stft, want_layers=False)
    es, ms = off["enh_stft"], off["enh_mag"]
    sess = model.streaming(batch=B)
    at = [0] * B
    for i in range(14):
        hold = (1,) if 3 <= i < 7 else ((0, 1) if i == 8 else ())  # clip 1 held for four launches in a row, and once more
        before = list(at)
        check_tick(tick(sess, stft, at, hold), es, ms, before, hold, f"tick {i}")
    sess.check_errors()
    # clip 1 has seen 9 frames in 14 launches: its running mean divides by 9 I, not by 14 I -- the outputs above are the offline
    # forward's for frame indices 0 .. 8 of ITS utterance, and its sums are those of a clip that only ever stepped 9 frames
    assert sess.clip_frames.tolist() == at == [13, 9, 14]
    alone = model.streaming(batch=1)
    for t in range(9):
        alone.step(stft[1:2, :, t:t + 1].contiguous())
    sa, sb = sess.export_state(clips=[1]), alone.export_state()
    assert "cum" in [n for n, _, _ in sa.layout]
    same_state(sa, sb, "the held clip against a clip that only stepped")


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------
def test_what_a_hold_refuses():
    model = model_of("live_tiny")
    stft = torch.from_numpy(pr.spectra("live_tiny", B)).to(DEV)
    w = torch.from_numpy(pr.waves("live_tiny", B)).to(DEV)
    res = model.streaming(batch=1, waveform=True, host_io=True, resident=True)
    with pytest.raises(NotImplementedError, match="resident"):
        res.step_wave_host(w[:1, :128].cpu(), clips=[0])
    with pytest.raises(NotImplementedError, match="resident"):
        res.step_wave_host(w[:1, :128].cpu(), clips=[])
    res.close()
    for one_launch in (True, False):
        s = model.streaming(batch=B, one_launch=one_launch)
        x = stft[..., :1].contiguous()
        for bad in (3, -1, 300):
            with pytest.raises(ValueError, match=rf"clip index {bad} out of range for a session of 3 clips"):
                s.step(x, clips=[0, bad])
        for wrong in ([0.5], torch.tensor([1.0]), [True], torch.zeros((1, 1), dtype=torch.long), "0", 1):
            with pytest.raises(TypeError):
                s.step(x, clips=wrong)
        assert s.frames_done == 0 and s.clip_frames.tolist() == [0] * B  # nothing above changed the session
        assert not one_launch or s._hop["parts"][0]["desc"].launch_index == 0
    ws = model.streaming(batch=B, waveform=True)
    with pytest.raises(ValueError, match="clip index 7 out of range"):
        ws.step_wave(w[:, :128].contiguous(), clips=[7])
    with pytest.raises(TypeError):
        ws.step_wave(w[:, :128].contiguous(), clips=[0.0])
    assert ws.clip_calls.tolist() == [0] * B
    hs = model.streaming(batch=B, waveform=True, host_io=True)
    with pytest.raises(ValueError, match="clip index 3 out of range"):
        hs.step_wave_host(w[:, :128].cpu(), clips=[3])
    assert hs.clip_calls.tolist() == [0] * B
    from spiking_fullsubnet_amd.modeling_cirm_gsn import Model
    import hopref as hr
    import inspect
    cirm = Model(**hr.CIRM_TINY).eval().to(DEV).streaming()
    assert "clips" not in inspect.signature(cirm.step).parameters  # (out of scope: fullband_streaming.py)


# ---- 9. clips=None is today's call ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_launch", [True, False])
def test_without_clips_the_session_makes_the_calls_it_always_made(one_launch):
    model = model_of("live_tiny")
    stft = torch.from_numpy(pr.spectra("live_tiny", B)).to(DEV)
    plain, keyword, listed = (model.streaming(batch=B, one_launch=one_launch) for _ in range(3))
    lib = plain.eng.lib
    hop_calls, held_calls = _counted(lib, "sfsn_stream_hop"), _counted(lib, "sfsn_stream_hop_held")
    try:
        for j in range(6):
            x = stft[..., j:j + 1].contiguous()
            a = plain.step(x)
            n0 = hop_calls.calls
            b = keyword.step(x, clips=None)
            assert hop_calls.calls - n0 == (1 if one_launch else 0)
            c = listed.step(x, clips=[2, 0, 1, 1])  # every clip listed: nobody is held
            for o in (b, c):
                assert torch.equal(real(a[0]), real(o[0])) and torch.equal(a[1], o[1]), j
    finally:
        hop_calls.restore()
        held_calls.restore()
    assert held_calls.calls == 0 and hop_calls.calls == (18 if one_launch else 0)
    if one_launch:
        assert not keyword._hop["parts"][0]["desc"].clip_start  # still the session-wide counters: nothing was switched
    assert plain.clip_frames.tolist() == keyword.clip_frames.tolist() == listed.clip_frames.tolist() == [6] * B
