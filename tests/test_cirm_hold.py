"""``FullbandStreamingSession.tick`` / ``tick_wave`` / ``tick_wave_host`` (``sfsn_fullband_stream_hop_held`` / ``_wave_held``; the
per-kernel tier's save / replay / restore): a tick that advances only some clips of a cIRM-GSN batch leaves every other clip exactly
where it was.

Everything is ``torch.equal`` -- a held launch runs the same instructions on the same rows as a launch without holds, so nothing here
needs a tolerance.  The schedule is tests/holdref.py's (B = 3, 16 ticks, both launch parities, a clip held before it has ever run, an
empty tick, a clip held in the very launch that would have restarted it); models, spectra and waves are tests/test_cirm_streaming.py's
and tests/test_cirm_waveform.py's.  Clip b's j-th active tick is fed its frames [j hop, (j + 1) hop) and must return row b of call j
of a CONTROL session of the same batch that steps every clip every time; the held rows of every input are NaN."""
import inspect

import pytest
import torch

import holdref as hd
from test_cirm_streaming import TINY, VARIANTS, _spectrum, model, offline
from test_cirm_waveform import noise
from test_cirm_waveform import offline as offline_wave

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = hd.B
MODES = {"one_launch": dict(one_launch=True), "counted": dict(one_launch=True, count_spikes=True), "graph": dict(one_launch=False),
         "graph_counted": dict(one_launch=False, count_spikes=True), "eager": dict(one_launch=False, graph=False)}
F129 = dict(TINY, n_fft=256, hop_length=64, win_length=256, input_size=129, proj_size=129)


def session(m, batch, mode, hop=1):
    skw = MODES[mode]
    s = m.streaming(batch=batch, hop=hop, **skw)
    assert s.one_launch is skw["one_launch"] and (s.one_launch or (s._graph is not None) == skw.get("graph", True))
    return s


def real(x):
    return torch.view_as_real(x) if x.is_complex() else x


def same_out(a, b):
    """(enh, mag or None) pairs, bit for bit."""
    return torch.equal(real(a[0]), real(b[0])) and (a[1] is None) == (b[1] is None) and (a[1] is None or torch.equal(a[1], b[1]))


def row(out, b):
    return out[0][b], (None if out[1] is None else out[1][b])


def is_zero(out):
    return not bool(real(out[0]).any()) and (out[1] is None or not bool(out[1].any()))


def counts_of(summary):
    return [int(x.count) for x in summary[1:-1]]


def same_state(sa, sb, where):
    """Two ``export_state`` results, section by section."""
    assert sa.layout == sb.layout and sa.frames.tolist() == sb.frames.tolist(), where
    assert (sa.calls is None) == (sb.calls is None) and (sa.calls is None or sa.calls.tolist() == sb.calls.tolist()), where
    for name, lo, hi in sa.layout:
        assert torch.equal(sa.blob[:, lo:hi], sb.blob[:, lo:hi]), f"{where}: section {name}"


def differs(sa, sb):
    return [name for name, lo, hi in sa.layout if not torch.equal(sa.blob[:, lo:hi], sb.blob[:, lo:hi])]


def nan_frames(sess, rows):
    """[B, F, hop] complex64, NaN (both parts) everywhere but the given {clip: [F, hop] frames}."""
    x = torch.empty((sess.B, sess.F, sess.hop), dtype=torch.complex64, device=DEV)
    torch.view_as_real(x).fill_(float("nan"))
    for b, v in rows.items():
        x[b] = v
    return x


# ---- 1. the schedule against a control that steps every clip every time -----------------------------------------------------------
@pytest.mark.parametrize("hop", [1, 3])
@pytest.mark.parametrize("mode", list(MODES))
def test_the_schedule_equals_a_control_that_steps_every_clip(mode, hop):
    m = model(**TINY)
    calls = hd.active_ticks()[0]
    assert hd.active_ticks() == [calls] * B
    X = _spectrum(B, 257, calls * hop, 71 + hop)
    control, sess = session(m, B, mode, hop), session(m, B, mode, hop)
    want = []
    for j in range(calls):  # every clip, every call; clip b is reset where the schedule resets it
        for b, jr in hd.resets().items():
            if jr == j:
                control.reset(clips=[b])
        want.append(control.step(X[..., j * hop:(j + 1) * hop].contiguous()))
    control.check_errors()
    # the premise: the control is the offline forward -- clip 2 up to its reset
    off = offline(m, X, ("hold", hop))
    ce, cm = torch.cat([w[0] for w in want], -1), torch.cat([w[1] for w in want], -1)
    n2 = hd.resets()[2] * hop
    assert torch.equal(real(ce[:2]), real(off[0][:2])) and torch.equal(cm[:2], off[1][:2])
    assert torch.equal(real(ce[2, ..., :n2]), real(off[0][2, ..., :n2])) and torch.equal(cm[2, ..., :n2], off[1][2, ..., :n2])
    assert bool(real(ce).any())
    seen = [0] * B
    for t, fed in hd.feed():
        if t in hd.RESET_BEFORE:
            sess.reset(clips=hd.RESET_BEFORE[t])
        x = nan_frames(sess, {b: X[b, :, j * hop:(j + 1) * hop] for b, j in fed.items()})
        out = sess.tick(x, sorted(fed))
        assert out[0].shape == (B, 1, 257, hop) and out[1].shape == (B, 1, 257, hop)
        for b in range(B):
            if b in fed:
                assert same_out(row(out, b), row(want[fed[b]], b)), f"tick {t}: clip {b}, its call {fed[b]}"
                seen[b] += 1
            else:
                assert is_zero(row(out, b)), f"tick {t}: held clip {b} has output"
    sess.check_errors()
    ages = [calls, calls, calls - hd.resets()[2]]
    assert seen == [calls] * B and sess.clip_frames().tolist() == [a * hop for a in ages] == control.clip_frames().tolist()
    same_state(sess.export_state(), control.export_state(), "after the schedule")
    if sess.count_spikes:
        for b in range(B):
            assert counts_of(sess.spike_summary([b])) == counts_of(control.spike_summary([b])), b
        assert sum(counts_of(sess.spike_summary([0]))) > 0


@pytest.mark.parametrize("mode", ["counted", "graph_counted"])
def test_an_empty_list_launches_nothing_and_returns_zeros(mode):
    m = model(**TINY)
    X = _spectrum(B, 257, 2, 73)
    sess = session(m, B, mode)
    sess.step(X[..., :1].contiguous())
    before, launches = sess.export_state(), dict(sess.launches)
    k = sess._hop["desc"].launch_index if sess.one_launch else None
    e, mg = sess.tick(nan_frames(sess, {}), [])
    assert e.shape == (B, 1, 257, 1) and is_zero((e, mg)) and mg.shape == (B, 1, 257, 1)
    assert sess.frames_done == 1 and sess.clip_frames().tolist() == [1] * B and sess.launches == launches
    assert not sess.one_launch or sess._hop["desc"].launch_index == k
    same_state(before, sess.export_state(), "an empty tick")
    two = session(model(**dict(TINY, **VARIANTS["df5_2spk"])), B, mode)
    e, mg = two.tick(nan_frames(two, {}), [])
    assert e.shape == (B, 2, 257, 1) and not bool(real(e).any()) and mg is None  # (S > 1: no magnitudes, as step)


# ---- 2. a held launch changes nothing of the held clip ----------------------------------------------------------------------------
HELD_CASES = [("tiny", "counted"), ("tiny", "graph_counted"), ("df5_2spk", "counted"), ("df1", "counted"), ("no_ln", "counted"),
              ("largest", "counted")]


@pytest.mark.parametrize("name,mode", HELD_CASES, ids=[f"{n}-{md}" for n, md in HELD_CASES])
def test_a_held_launch_changes_nothing_of_the_held_clip(name, mode):
    kw = dict(TINY, **VARIANTS.get(name, {}))
    m = model(**kw)
    X = _spectrum(B, kw["n_fft"] // 2 + 1, 5, 79)
    sess, control = session(m, B, mode), session(m, B, mode)
    if name == "largest":
        d = sess._hop["desc"]
        assert (d.Hp + 31) // 32 + d.n_layers * ((d.Hp // 16 + 7) // 8) + (d.F + 15) // 16 * d.S == 62  # the finishing count over a big grid
    for j in range(3):
        sess.step(X[..., j:j + 1].contiguous())
        control.step(X[..., j:j + 1].contiguous())
    b, others = 1, [0, 2]
    parities = []
    for j in (3, 4):  # launch 3 (odd) and launch 4 (even) both hold clip b
        if sess.one_launch:
            parities.append(sess._hop["desc"].launch_index & 1)
        before, cbefore = sess.export_state(clips=[b]), control.export_state(clips=[b])
        out = sess.tick(nan_frames(sess, {c: X[c, :, j:j + 1] for c in others}), others)
        cout = control.step(X[..., j:j + 1].contiguous())
        assert is_zero(row(out, b)) and all(same_out(row(out, c), row(cout, c)) for c in others), j
        same_state(before, sess.export_state(clips=[b]), f"launch {j}")
        # (the same tick without the hold does change them: the history, some membranes, the counts)
        changed = differs(cbefore, control.export_state(clips=[b]))
        assert ("slots" in changed or "rows" in changed) and any(n.endswith(".c") for n in changed), changed
        assert "hist" in changed or (kw["df_order"] == 1 and sess.one_launch), changed  # (D == 0: the hop keeps no history)
    assert not sess.one_launch or sorted(parities) == [0, 1]
    sess.check_errors()
    same_state(sess.export_state(clips=others), control.export_state(clips=others), "the active clips")
    assert sess.clip_frames().tolist() == [5, 3, 5]


# ---- 3. B = 16 at the recipe geometry: the operand's every column in use ------------------------------------------------------------
def run_ticks(sess, X, holds, want, src=None, at=None):
    """One tick per entry of ``holds`` (the held clips): clip b takes frame at[b] of row src[b] of X unless held, and must return
    the offline forward's frame; -> at."""
    nb, hop = sess.B, sess.hop
    src = list(range(nb)) if src is None else src
    at = [0] * nb if at is None else at
    for i, held in enumerate(holds):
        rows = {b: X[src[b], :, at[b]:at[b] + hop] for b in range(nb) if b not in held}
        out = sess.tick(nan_frames(sess, rows), sorted(rows)) if held else sess.step(nan_frames(sess, rows))
        for b in range(nb):
            if b in held:
                assert is_zero(row(out, b)), (i, b)
            else:
                t = at[b]
                w = (want[0][src[b], ..., t:t + hop], None if want[1] is None else want[1][src[b], ..., t:t + hop])
                assert same_out(row(out, b), w), (i, b, t)
                at[b] += hop
    return at


def test_sixteen_clips_at_the_recipe_geometry():
    from test_cirm_gsn import RECIPE
    m = model(**RECIPE)
    X = _spectrum(16, 257, 12, 27)
    want = offline(m, X, ("recipe", 16, 12))  # (tests/test_cirm_streaming.py's reference of this spectrum)
    sess = session(m, 16, "one_launch")
    ends, middle = {0, 15}, set(range(1, 15))
    at = run_ticks(sess, X, [set(), ends, ends, set(), middle, set(), middle | {15}, {0}, set()], want)
    sess.check_errors()
    assert at == sess.clip_frames().tolist() == [6] + [7] * 14 + [6]


# ---- 4. waveform and host_io ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host_io", [False, True])
def test_the_schedule_on_waveform_calls(host_io):
    m = model(**TINY)
    calls = hd.active_ticks()[0]
    w = noise(B, calls, 97)
    control, sess = (m.streaming(batch=B, waveform=True, host_io=host_io) for _ in range(2))

    def call(s, x, clips=None):
        if clips is None:
            return s.step_wave_host(x.cpu()).to(DEV).clone() if host_io else s.step_wave(x)
        return s.tick_wave_host(x.cpu(), clips).to(DEV).clone() if host_io else s.tick_wave(x, clips)

    want = []
    for j in range(calls):
        for b, jr in hd.resets().items():
            if jr == j:
                control.reset(clips=[b])
        want.append(call(control, w[:, 128 * j:128 * (j + 1)].contiguous()))
    control.check_errors()
    y = offline_wave(m, w, ("hold", B, calls))
    assert not any(bool(o.any()) for o in want[:3])  # the three leading zero calls ...
    for j in range(3, calls):                        # ... then the offline model's samples of three calls earlier (clip 2: up to its reset)
        rows = [0, 1] + ([2] if j < hd.resets()[2] else [])
        assert torch.equal(want[j][rows], y[rows, :, 128 * (j - 3):128 * (j - 2)]), j
    assert bool(want[-1].any())
    assert 0 not in hd.TICKS[0]  # clip 0 is held at the session's first call: here that call is a launch
    seen = [0] * B
    for t, fed in hd.feed():
        if t in hd.RESET_BEFORE:
            sess.reset(clips=hd.RESET_BEFORE[t])
        x = torch.full((B, 128), float("nan"), dtype=torch.float32, device=DEV)
        for b, j in fed.items():
            x[b] = w[b, 128 * j:128 * (j + 1)]
        k = sess._hop["desc"].launch_index
        out = call(sess, x, sorted(fed))  # (host_io: the wait on the done words returns, held clips included)
        assert out.shape == (B, 1, 128)
        assert sess._hop["desc"].launch_index == k + (1 if fed else 0)
        if host_io and fed:  # every completion word, the held clips' too, carries this launch
            assert (sess._hop["wave"]["host"]["done_np"].astype("int64") & 0xFFFFFFFF).tolist() == [k + 1] * B
        for b in range(B):
            if b in fed:  # the three-call delay line counts the clip's own calls
                assert torch.equal(out[b], want[fed[b]][b]), f"tick {t}: clip {b}, its call {fed[b]}"
                seen[b] += 1
            else:
                assert not bool(out[b].any()), f"tick {t}: held clip {b} has output"
    sess.check_errors()
    ages = [calls, calls, calls - hd.resets()[2]]
    assert seen == [calls] * B and sess.clip_calls().tolist() == ages == control.clip_calls().tolist()
    assert sess.clip_frames().tolist() == [a - 1 for a in ages]
    sa = sess.export_state()
    assert {"wave", "ola"} <= {n for n, _, _ in sa.layout}
    same_state(sa, control.export_state(), "after the schedule")


def test_a_held_waveform_call_changes_nothing_of_the_held_clip():
    m = model(**dict(TINY, num_spks=2, df_order=5))
    w = noise(B, 7, 101)
    sess = m.streaming(batch=B, waveform=True)
    for j in range(5):
        sess.step_wave(w[:, 128 * j:128 * (j + 1)].contiguous())
    for j in (5, 6):  # both launch parities
        before = sess.export_state(clips=[2])
        x = w[:, 128 * j:128 * (j + 1)].clone()
        x[2] = float("nan")
        out = sess.tick_wave(x, [0, 1])
        assert out.shape == (B, 2, 128) and not bool(out[2].any()) and bool(out[:2].any())
        same_state(before, sess.export_state(clips=[2]), f"call {j}")
    sess.check_errors()
    assert sess.clip_calls().tolist() == [7, 7, 5]


# ---- 5. combinations, also with the launch index near the wrap ----------------------------------------------------------------------
T5 = 26
COMBOS = [("counted", 0), ("counted", 2 ** 32 - 3), ("counted", 2 ** 31 + 3), ("graph_counted", 0)]


def combo(mode, wrap):
    m = model(**TINY)
    X = _spectrum(B, 257, T5, 103)
    sess = session(m, B, mode)
    if wrap:  # the launch counter about to wrap, or the origins at the edge of the int32 the session's tensor holds them in
        sess._hop["desc"].launch_index = wrap
        sess._hop["origin"].fill_(sess._as_i32(wrap))
    return sess, X, offline(m, X, ("hold", "combos"))


@pytest.mark.parametrize("mode,wrap", COMBOS)
def test_hold_then_catch_up_on_the_held_clip_then_tick(mode, wrap):
    sess, X, want = combo(mode, wrap)
    at = run_ticks(sess, X, [set(), set(), {1}, {1}], want)
    assert at == [4, 2, 4] == sess.clip_frames().tolist()
    N = 9
    e1, m1 = sess.catch_up(X[1:2, :, 2:2 + N], clips=[1])  # the held clip takes a backlog from where it was held
    assert same_out((e1, m1), (want[0][1:2, ..., 2:2 + N], want[1][1:2, ..., 2:2 + N]))
    at[1] += N
    at = run_ticks(sess, X, [{1}, set(), set(), {0, 2}, set(), set()], want, at=at)
    sess.check_errors()
    assert sess.clip_frames().tolist() == at == [9, 16, 9]


@pytest.mark.parametrize("mode,wrap", COMBOS)
def test_hold_then_move_the_clip_to_another_slot_then_tick(mode, wrap):
    sess, X, want = combo(mode, wrap)
    at = run_ticks(sess, X, [set(), {1}, {1}, set(), {0}], want)
    assert at == [4, 3, 5]
    state = sess.export_state(clips=[1])  # clip 1 (3 frames, twice held) moves to slot 2; clip 0 (just held) to slot 1
    state0 = sess.export_state(clips=[0])
    sess.import_state(state, clips=[2])
    sess.import_state(state0, clips=[1])
    assert sess.clip_frames().tolist() == [4, 4, 3]
    at = run_ticks(sess, X, [set(), {2}, set(), {0, 1}, set(), set()], want, src=[0, 0, 1], at=[4, 4, 3])
    sess.check_errors()
    assert sess.clip_frames().tolist() == at == [9, 9, 8]
    for b in range(B):
        assert sum(counts_of(sess.spike_summary([b]))) > 0


@pytest.mark.parametrize("mode,wrap", COMBOS)
def test_holds_right_behind_a_warm_start(mode, wrap):
    sess, X, want = combo(mode, wrap)
    at = run_ticks(sess, X, [set(), set(), {1}], want)
    P = 17
    sess.reset(clips=[1])
    p, _ = sess.catch_up(X[1:2, :, :P], clips=[1])  # the held clip starts over from a recorded prefix of its own utterance
    assert torch.equal(real(p), real(want[0][1:2, ..., :P]))
    at[1] = P
    at = run_ticks(sess, X, [{1}, {1}, set(), set(), {1}, set()], want, at=at)  # held in the two launches right behind it: both parities
    sess.check_errors()
    assert sess.clip_frames().tolist() == at == [9, P + 3, 9]


def test_a_reset_clip_held_until_later_starts_from_zero_state():
    """reset(clips); held for two launches (both parities: the restart is due in each, and stays due); then its utterance begins."""
    sess, X, want = combo("counted", 0)
    run_ticks(sess, X, [set(), set(), set()], want)
    sess.reset(clips=[2])
    tail = offline(model(**TINY), X[:, :, 10:].contiguous(), ("hold", "tail"))
    run_ticks(sess, X, [{2}, {2}], want, at=[3, 3, 0])
    for j in range(4):
        x = nan_frames(sess, {0: X[0, :, 5 + j:6 + j], 1: X[1, :, 5 + j:6 + j], 2: X[2, :, 10 + j:11 + j]})
        out = sess.step(x)
        assert same_out(row(out, 2), (tail[0][2, ..., j:j + 1], tail[1][2, ..., j:j + 1])), j
        assert same_out(row(out, 0), (want[0][0, ..., 5 + j:6 + j], want[1][0, ..., 5 + j:6 + j])), j
    sess.check_errors()
    assert sess.clip_frames().tolist() == [9, 9, 4]


# ---- 6. outside the hop kernel: 17 clips, and 256-point frames ------------------------------------------------------------------------
def test_seventeen_clips_and_f129_take_the_per_kernel_tier():
    m = model(**TINY)
    X = _spectrum(17, 257, 6, 37)
    sess = m.streaming(batch=17, hop=1, one_launch="auto")
    assert sess.one_launch is False
    at = run_ticks(sess, X, [set(), {0, 16}, set(range(1, 16)), {16}, set(), {5}, set()], offline(m, X, ("b17",)))
    sess.check_errors()
    assert at == sess.clip_frames().tolist() == [6] * 5 + [5] + [6] * 10 + [5]
    m = model(**F129)
    X = _spectrum(2, 129, 12, 29)
    sess = m.streaming(batch=2, hop=1, one_launch="auto")
    assert sess.one_launch is False
    at = run_ticks(sess, X, [{0}, set(), {1}, {1}, set(), {0}, set(), set()], offline(m, X, ("outside", "f129")))
    sess.check_errors()
    assert at == sess.clip_frames().tolist() == [6, 6]


# ---- 7. which entry point a tick calls ----------------------------------------------------------------------------------------------
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


PLAIN = {"spectrum": "sfsn_fullband_stream_hop", "counted": "sfsn_fullband_stream_hop_counted", "wave": "sfsn_fullband_stream_hop_wave"}


@pytest.mark.parametrize("kind", list(PLAIN))
def test_which_entry_point_a_tick_calls(kind):
    m = model(**TINY)
    wave = kind == "wave"
    sess = m.streaming(batch=B, waveform=True) if wave else session(m, B, "counted" if kind == "counted" else "one_launch")
    ref = m.streaming(batch=B, waveform=True) if wave else session(m, B, "counted" if kind == "counted" else "one_launch")
    X, w = _spectrum(B, 257, 8, 107), noise(B, 8, 109)
    feed = [w[:, 128 * j:128 * (j + 1)].contiguous() if wave else X[..., j:j + 1].contiguous() for j in range(5)]
    wants = [ref.step_wave(x) if wave else ref.step(x) for x in feed[:3]]
    lib = sess.eng.lib
    held_name = "sfsn_fullband_stream_hop_wave_held" if wave else "sfsn_fullband_stream_hop_held"
    probes = {n: _counted(lib, n) for n in list(PLAIN.values()) + ["sfsn_fullband_stream_hop_held", "sfsn_fullband_stream_hop_wave_held"]}

    def calls():
        return {n: p.calls for n, p in probes.items() if p.calls}

    def tick(j, clips):
        before = calls()
        out = sess.tick_wave(feed[j], clips) if wave else sess.tick(feed[j], clips)
        now = calls()
        return out, {n: now[n] - before.get(n, 0) for n in now if now[n] != before.get(n, 0)}

    try:
        for j, clips in enumerate([None, [2, 0, 1, 1], None]):  # nobody held: only the plain entry, and step's results
            out, made = tick(j, clips)
            assert made == {PLAIN[kind]: 1}, (j, made)
            assert torch.equal(out, wants[j]) if wave else same_out(out, wants[j])
        out, made = tick(3, [0, 2])  # some held: exactly one call of the held entry and none of the plain
        assert made == {held_name: 1}, made
        k = sess._hop["desc"].launch_index
        out, made = tick(4, [])  # an empty list: no call, and the launch index stays
        assert made == {} and sess._hop["desc"].launch_index == k and not bool(real(out if wave else out[0]).any())
    finally:
        for p in probes.values():
            p.restore()
    sess.check_errors()
    assert sess.launches == {"hop": 4}


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------
def test_what_a_tick_refuses():
    m = model(**TINY)
    X, w = _spectrum(B, 257, 1, 113), noise(B, 1, 127)
    for mode in ("one_launch", "graph"):
        s = session(m, B, mode)
        for bad in (3, -1, 300):
            with pytest.raises(ValueError, match=rf"clip index {bad} out of range for a session of 3 clips"):
                s.tick(X, [0, bad])
        for wrong in ([0.5], torch.tensor([1.0]), [True], torch.zeros((1, 1), dtype=torch.long), "0", 1):
            with pytest.raises(TypeError):
                s.tick(X, wrong)
        with pytest.raises(RuntimeError, match="expected complex64"):
            s.tick(X[:2], [0])
        with pytest.raises(RuntimeError, match="waveform=True"):
            s.tick_wave(w, [0])
        with pytest.raises(RuntimeError, match="host_io=True"):
            s.tick_wave_host(w.cpu(), [0])
        assert s.frames_done == 0 and s.clip_frames().tolist() == [0] * B and s.launches == {}  # nothing above changed the session
        assert not s.one_launch or s._hop["desc"].launch_index == 0
        s.check_errors()
    ws = m.streaming(batch=B, waveform=True)
    with pytest.raises(ValueError, match="clip index 7 out of range"):
        ws.tick_wave(w, [7])
    with pytest.raises(TypeError):
        ws.tick_wave(w, [0.0])
    with pytest.raises(RuntimeError, match="step_wave"):
        ws.tick(X, [0])
    with pytest.raises(RuntimeError, match="host_io=True"):
        ws.tick_wave_host(w.cpu(), [0])
    assert ws.clip_calls().tolist() == [0] * B and ws._hop["desc"].launch_index == 0
    hs = m.streaming(batch=B, waveform=True, host_io=True)
    with pytest.raises(ValueError, match="clip index 3 out of range"):
        hs.tick_wave_host(w.cpu(), [3])
    with pytest.raises(RuntimeError, match="step_wave_host"):
        hs.tick_wave(w, [0])
    assert hs.clip_calls().tolist() == [0] * B and hs._hop["desc"].launch_index == 0
    for sess in (ws, hs):
        sess.check_errors()
    assert "clips" not in inspect.signature(ws.step).parameters  # (tests/test_stream_hold.py pins it)


# ---- 9. step and tick share one body: the refusals' order, and a tick of every clip IS the step -------------------------------------
@pytest.mark.parametrize("mode", ["one_launch", "eager"])
def test_the_clip_list_is_refused_first_and_a_tick_of_every_clip_is_the_step(mode):
    m = model(**TINY)
    X = _spectrum(B, 257, 4, 131)
    stepped, ticked = session(m, B, mode), session(m, B, mode)

    def feed(j):
        return X[..., j:j + 1].contiguous()

    def marks(s):
        return dict(s.launches), (s._hop["desc"].launch_index if s.one_launch else None), s.frames_done

    for j in range(4):
        if j == 2:  # a wrong dtype AND an index out of range: the clip list's refusal wins, and nothing was launched or counted
            before = marks(ticked)
            with pytest.raises(ValueError, match="clip index 3 out of range for a session of 3 clips"):
                ticked.tick(feed(j).to(torch.complex128), [0, 3])
            assert marks(ticked) == before and before[2] == 2
        assert same_out(stepped.step(feed(j)), ticked.tick(feed(j), range(B))), j
    for s in (stepped, ticked):
        s.check_errors()
    assert torch.equal(stepped.export_state().blob, ticked.export_state().blob)
    assert stepped.launches == ticked.launches and sum(stepped.launches.values()) >= 4
    assert stepped.clip_frames().tolist() == ticked.clip_frames().tolist() == [4] * B
