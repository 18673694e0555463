"""Moving a clip between cIRM-GSN streaming sessions: ``FullbandStreamingSession.export_state`` / ``import_state`` on the one-launch
spectrum hop, its counted form, the waveform hop (``sfsn_fullband_hop_state_export`` / ``_import``, csrc/sfsn_state.hip) and the graph
tier (stream-ordered row copies).  A moved clip continues bit for bit against a control session that never exported or imported;
every comparison is ``torch.equal``.  cIRM-GSN sessions have no ``prime``: an import is their warm start."""
import numpy as np
import pytest
import torch

from test_cirm_streaming import TINY, _spectrum, model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F129 = dict(TINY, n_fft=256, hop_length=64, win_length=256, input_size=129, proj_size=129)  # 256-point frames: the graph tier only
MODES = {"one_launch": (TINY, dict(one_launch=True)), "counted": (TINY, dict(one_launch=True, count_spikes=True)),
         "graph": (TINY, dict(one_launch=False)), "graph_counted": (TINY, dict(one_launch=False, count_spikes=True)),
         "graph_f129": (F129, dict(one_launch=False))}
TA, TB, NEXT = 16, 14, 9


def session(mode, B):
    kw, skw = MODES[mode]
    s = model(**kw).streaming(batch=B, **skw)
    assert s.one_launch is skw["one_launch"]
    return s


def bins(mode):
    return MODES[mode][0]["input_size"]


def step(sess, X, t, rows=None):
    x = X[:, :, t:t + 1] if rows is None else torch.cat([Xb[b:b + 1, :, tb:tb + 1] for Xb, b, tb in rows])
    e, m = sess.step(x.contiguous())
    return torch.view_as_real(e).clone(), m.clone()


def stream(sess, X, t0, n):
    return [step(sess, X, t) for t in range(t0, t0 + n)]


_CONTROL = {}


def control(mode, B, T, seed):
    """(spectrum, outputs) of a session that never exports or imports; computed once, left unchanged."""
    key = (mode, B, T, seed)
    if key not in _CONTROL:
        X = _spectrum(B, bins(mode), T, seed)
        sess = session(mode, B)
        _CONTROL[key] = (X, stream(sess, X, 0, T))
        sess.check_errors()
    return _CONTROL[key]


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def clip(o, b):
    return o[0][b], o[1][b]


def counts(summary):
    return [int(x.count) for x in summary[1:-1]]


# ---- move: both parities of h and hist_ri on either side ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["one_launch", "counted", "graph", "graph_f129"])
@pytest.mark.parametrize("k,j", [(7, 4), (7, 5), (6, 5), (0, 3), (7, 0)])
def test_a_moved_clip_continues_bit_for_bit(mode, k, j):
    (XA, CA), (XB, CB) = control(mode, 3, TA, 71), control(mode, 2, TB, 72)
    A, B = session(mode, 3), session(mode, 2)
    stream(A, XA, 0, k)
    if k == 0:
        A.reset()
    stream(B, XB, 0, j)
    state = A.export_state(clips=[1])
    assert len(state) == 1 and state.frames.tolist() == [k] and state.calls is None and state.blob.shape[1] % 16 == 0
    B.import_state(state, clips=[0])
    assert B.clip_frames().tolist() == [k, j] and A.clip_frames().tolist() == [k] * 3
    for i in range(NEXT):
        a = step(A, XA, k + i)
        b = step(B, None, None, rows=[(XA, 1, k + i), (XB, 1, j + i)])
        assert same(a, CA[k + i]), ("A", i)
        assert same(clip(b, 0), clip(CA[k + i], 1)), ("moved", i)
        assert same(clip(b, 1), clip(CB[j + i], 1)), ("B slot 1", i)
    A.check_errors()
    B.check_errors()
    assert float(CA[TA - 1][0].abs().max()) > 0
    if "counted" in mode:
        C = session(mode, 3)
        stream(C, XA, 0, k + NEXT)
        assert counts(B.spike_summary([0])) == counts(C.spike_summary([1])) and sum(counts(B.spike_summary([0]))) > 0


@pytest.mark.parametrize("mode", ["one_launch", "graph"])
def test_rewind_and_fork(mode):
    (X, C), k = control(mode, 3, TA, 71), 6
    A = session(mode, 3)
    stream(A, X, 0, k)
    state = A.export_state()
    first = stream(A, X, k, 5)
    A.import_state(state)
    assert A.clip_frames().tolist() == [k] * 3
    again = stream(A, X, k, 5)
    for i in range(5):
        assert same(first[i], again[i]) and same(first[i], C[k + i]), i
    # fork: clip 0's state at frame k into two slots of another session
    B = session(mode, 3)
    stream(B, _spectrum(3, bins(mode), 3, 73), 0, 3)
    B.import_state(state.select([0, 0]), clips=[2, 0])
    for i in range(3):
        o = step(B, None, None, rows=[(X, 0, k + i), (X, 1, k + i), (X, 0, k + i)])
        assert same(clip(o, 0), clip(o, 2)) and same(clip(o, 0), clip(C[k + i], 0)), i
    o = step(B, None, None, rows=[(X, 0, k + 3), (X, 1, k + 3), (X, 2, k + 3)])
    assert same(clip(o, 0), clip(C[k + 3], 0)) and not torch.equal(o[0][0], o[0][2])
    B.check_errors()


# ---- the waveform hop ------------------------------------------------------------------------------------------------------------------
def samples(B, calls, seed):
    return torch.from_numpy((0.05 * np.random.default_rng(seed).standard_normal((B, 128 * calls))).astype(np.float32)).to(DEV)


def wave_calls(sess, W, c0, n, host, rows=None):
    outs = []
    for c in range(c0, c0 + n):
        x = W[:, 128 * c:128 * (c + 1)] if rows is None else torch.cat([Wb[b:b + 1, 128 * (cb + c - c0):128 * (cb + c - c0 + 1)] for Wb, b, cb in rows])
        outs.append(sess.step_wave_host(x.cpu()).clone() if host else sess.step_wave(x.contiguous()).cpu())
    return outs


_WCONTROL = {}


def wave_control(B, calls, seed, host):
    key = (B, calls, seed, host)
    if key not in _WCONTROL:
        sess = model(**TINY).streaming(batch=B, waveform=True, host_io=host)
        _WCONTROL[key] = wave_calls(sess, samples(B, calls, seed), 0, calls, host)
        sess.check_errors()
    return _WCONTROL[key]


@pytest.mark.parametrize("c,j,host", [(c, j, False) for c in (1, 2, 3, 9) for j in (0, 4, 5)] + [(1, 0, True), (9, 4, True)])
def test_waveform_clips_move(c, j, host):
    """Exported at the clip's call c (1: no frame yet), imported into a session at call count j (0: never called; 4 and 5: both
    parities): the outputs equal the unmoved control's, the muted first calls included."""
    m, n = model(**TINY), 7
    WA, WB = samples(3, 16, 81), samples(2, 12, 82)
    CA, CB = wave_control(3, 16, 81, host), wave_control(2, 12, 82, host)
    A, B = (m.streaming(batch=b, waveform=True, host_io=host) for b in (3, 2))
    wave_calls(A, WA, 0, c, host)
    wave_calls(B, WB, 0, j, host)
    state = A.export_state([1])
    assert state.calls.tolist() == [c] and state.frames.tolist() == [c - 1] and {"wave", "ola", "hist"} <= set(state.sections())
    B.import_state(state, [0])
    assert B.clip_calls().tolist() == [c, j]
    outs = wave_calls(B, None, 0, n, host, rows=[(WA, 1, c), (WB, 1, j)])
    for i in range(n):
        assert torch.equal(outs[i][0], CA[c + i][1]), ("moved", i)
        assert torch.equal(outs[i][1], CB[j + i][1]), ("other", i)
    assert any(bool(outs[i][0].any()) for i in range(n))
    B.check_errors()
    assert B.clip_calls().tolist() == [c + n, j + n] and B.clip_frames().tolist() == [c + n - 1, j + n - 1]


# ---- non-vacuity -----------------------------------------------------------------------------------------------------------------------
# mode -> (seed of the input, k).  With 20 neurons per layer a zeroed membrane or last-spike row of ONE layer often flips no spike of
# the last layer within ten frames (measured over seeds 91 .. 95 and k = 9, 13: 2 to 5 of 10 inputs exercise every section, the same
# ones in the one-launch and the graph tier), so each mode names an input under which every section matters.
ZERO_CASES = {"counted": (92, 9), "wave": (92, 9), "graph_counted": (92, 9), "graph_f129": (91, 9)}


def zeroed_sections(mode, seed, k, n=10):
    """Import the state of frame / call k with each section zeroed in turn -> (sections, those all zero at export, those whose zeroing
    left the next n steps as they were).  The unmodified state must reproduce the truth."""
    if mode == "wave":
        m = model(**TINY)
        A, B = (m.streaming(batch=2, waveform=True) for _ in range(2))
        W = samples(2, k + n, seed)
        run = lambda s, c0, cnt: wave_calls(s, W, c0, cnt, False)  # noqa: E731
        differ = lambda x, y: any(not torch.equal(p, q) for p, q in zip(x, y))  # noqa: E731
    else:
        A, B = session(mode, 2), session(mode, 2)
        X = _spectrum(2, bins(mode), k + n, seed)
        run = lambda s, c0, cnt: stream(s, X, c0, cnt)  # noqa: E731
        differ = lambda x, y: any(not same(p, q) for p, q in zip(x, y))  # noqa: E731
    counted = "counted" in mode
    run(A, 0, k)
    state = A.export_state()
    truth = run(A, k, n)
    truth_counts = counts(A.spike_summary()) if counted else None
    secs = state.sections()
    B.import_state(state)
    assert not differ(run(B, k, n), truth)
    zero, unchanged = [], []
    for sec, (a, b) in secs.items():
        if not bool(state.blob[:, a:b].any()):
            zero.append(sec)
            continue
        broken = state.clone()
        broken.blob[:, a:b] = 0
        B.import_state(broken)
        got = run(B, k, n)
        if sec in ("slots", "rows"):  # (counts are read by nothing: the outputs stay, the summary moves)
            if counts(B.spike_summary()) == truth_counts or differ(got, truth):
                unchanged.append(sec)
        elif not differ(got, truth):
            unchanged.append(sec)
    B.check_errors()
    return secs, zero, unchanged


@pytest.mark.parametrize("mode", sorted(ZERO_CASES))
def test_zeroing_any_section_changes_the_continuation(mode):
    """A control import whose one section is zeroed must make the continuation differ from the truth (for the spike counts: in
    spike_summary).  Seed and k are chosen so that every section is non-zero at export, which is asserted first."""
    seed, k = ZERO_CASES[mode]
    secs, zero, unchanged = zeroed_sections(mode, seed, k)
    want = {"hist", "l0.h", "l2.c"} | ({"wave", "ola"} if mode == "wave" else set()) | ({"slots"} if mode == "counted" else set()) | \
        ({"rows"} if mode == "graph_counted" else set())
    assert want <= set(secs)
    print(f"MIGRATE_SECTIONS cirm {mode}: {sorted(secs)}; zero at export {zero}; zeroing changed nothing {unchanged}")
    assert not zero, f"sections all zero at export: the inputs do not exercise them: {zero}"
    assert not unchanged, f"zeroing changed nothing: {unchanged}"


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    m = model(**TINY)
    A = session("one_launch", 3)
    X, C = control("one_launch", 3, TA, 71)
    stream(A, X, 0, 3)
    state = A.export_state([0, 1])
    for make, field in ((lambda: m.streaming(batch=2, hop=2, one_launch=True), "hop"), (lambda: session("graph", 2), "tier"),
                        (lambda: m.streaming(batch=2, waveform=True), "waveform"), (lambda: session("counted", 2), "count_spikes"),
                        (lambda: model(**dict(TINY, num_layers=2)).streaming(batch=2, one_launch=True), "layers")):
        with pytest.raises(ValueError, match=field):
            make().import_state(state, [0, 1])
    B = session("one_launch", 2)
    with pytest.raises(RuntimeError, match=r"\.to\("):
        B.import_state(state.to("cpu"), [0, 1])
    with pytest.raises(RuntimeError, match="2 clips for 1"):
        B.import_state(state, [1])
    with pytest.raises(ValueError, match="distinct"):
        B.import_state(state, [0, 0])
    with pytest.raises(IndexError):
        B.import_state(state, [0, 2])
    with pytest.raises(TypeError):
        B.import_state(state, [0, 1.5])
    with pytest.raises(TypeError):
        B.import_state(state.blob, [0, 1])
    assert not hasattr(B, "prime")  # (tests/test_stream_prime.py pins it: import is these sessions' warm start)
    B.import_state(state.to("cpu").to(DEV), [1, 0])
    o = step(B, None, None, rows=[(X, 1, 3), (X, 0, 3)])
    assert same(clip(o, 0), clip(C[3], 1)) and same(clip(o, 1), clip(C[3], 0))
