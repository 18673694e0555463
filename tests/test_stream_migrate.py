"""Moving a clip between streaming sessions: ``StreamingSession.export_state`` / ``import_state`` (``ClipState``; the one-launch tier's
``sfsn_hop_state_export`` / ``sfsn_hop_state_import``, csrc/sfsn_state.hip).  The state is copied, so a moved clip must continue bit for
bit -- against a control session that streamed the same clip without ever exporting or importing -- while every clip that did not
move goes on bit for bit as well.  Every comparison is ``torch.equal``; there is no tolerance in this file."""
import functools

import pytest
import torch

import refweights as rw
from test_streaming_clips import DEV, TINY_CUM, build_module

pytestmark = pytest.mark.gpu

TIERS = [pytest.param(True, id="one_launch"), pytest.param(False, id="per_kernel")]
MODELS = {"live": ("live", rw.LIVE_TINY, 11), "2spk": ("live", rw.LIVE_TINY_2SPK, 12), "cum": ("frozen", TINY_CUM, 7),
          "frozen": ("frozen", rw.FROZEN_TINY, 3),  # (384 projections in its last group: the per-kernel tier only)
          "lap": ("frozen", dict(rw.FROZEN_TINY, sb_df_orders=[3, 2, 1]), 3)}


@functools.lru_cache(maxsize=None)
def model_of(name):
    return build_module(*MODELS[name])


@functools.lru_cache(maxsize=None)
def waves(name, B, calls, seed):
    return torch.from_numpy(rw.synth_wave(B, calls + 1, seed, modulated=True)).to(DEV)  # [B, 128 * calls]


@functools.lru_cache(maxsize=None)
def spectra(name, B, T, seed):
    return model_of(name)._stft(waves(name, B, T, seed))[..., :T].contiguous()  # complex64 [B, F, T]


def step(sess, X, t, rows=None):
    """One hop-1 step on frame t of X (or of the per-clip (X, t) pairs in ``rows``) -> (enh as reals, mag), copies."""
    x = X[:, :, t:t + 1] if rows is None else torch.cat([Xb[b:b + 1, :, tb:tb + 1] for Xb, b, tb in rows])
    e, m = sess.step(x.contiguous())
    return torch.view_as_real(e).clone(), m.clone()


def stream(sess, X, t0, n):
    return [step(sess, X, t) for t in range(t0, t0 + n)]


_CONTROL = {}


def control(name, tier, B, T, seed, **kw):
    """The outputs of a session that streams ``spectra(name, B, T, seed)`` and never exports or imports; computed once, left unchanged."""
    key = (name, tier, B, T, seed, tuple(sorted(kw.items())))
    if key not in _CONTROL:
        sess = model_of(name).streaming(batch=B, one_launch=tier, **kw)
        assert (sess._hop is not None) is tier
        _CONTROL[key] = stream(sess, spectra(name, B, T, seed), 0, T)
        sess.check_errors()
    return _CONTROL[key]


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def clip(o, b):
    return o[0][b], o[1][b]


def counts(summary):
    fb_all, sb_all = summary
    return [int(x.count) for x in fb_all[1:-1]] + [int(x.count) for g in sb_all for x in g[1:-1]]


TA, TB, NEXT = 16, 14, 9


# ---- move ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("k,j", [(7, 4), (7, 5), (0, 3), (7, 0), (6, 5)])
def test_a_moved_clip_continues_bit_for_bit(tier, k, j):
    """Clip 1 of A (B = 3, k frames in) into slot 0 of B (B = 2, j frames of other input in): equal and different launch parities,
    k = 0 (exported straight after reset), j = 0 (B never stepped)."""
    m = model_of("live")
    XA, XB = spectra("live", 3, TA, 21), spectra("live", 2, TB, 22)
    CA, CB = control("live", tier, 3, TA, 21), control("live", tier, 2, TB, 22)
    A, B = m.streaming(batch=3, one_launch=tier), m.streaming(batch=2, one_launch=tier)
    stream(A, XA, 0, k)
    if k == 0:
        A.reset()
    stream(B, XB, 0, j)
    state = A.export_state(clips=[1])
    assert len(state) == 1 and state.frames.tolist() == [k] and state.calls is None and state.stats is None
    assert state.blob.dtype == torch.uint8 and state.blob.shape[1] % 16 == 0 and state.blob.device == torch.device(DEV)
    B.import_state(state, clips=[0])
    assert B.clip_frames.tolist() == [k, j] and A.clip_frames.tolist() == [k] * 3
    for i in range(NEXT):
        a = step(A, XA, k + i)
        b = step(B, None, None, rows=[(XA, 1, k + i), (XB, 1, j + i)])
        assert same(a, CA[k + i]), ("A", i)                          # A's clips: a control that never exported
        assert same(clip(b, 0), clip(CA[k + i], 1)), ("moved", i)    # the moved clip: A's clip 1, enh_stft and enh_mag
        assert same(clip(b, 1), clip(CB[j + i], 1)), ("B slot 1", i)  # B's other clip: a control that never saw an import
    A.check_errors()
    B.check_errors()
    assert B.clip_frames.tolist() == [k + NEXT, j + NEXT]
    assert float(CA[TA - 1][0].abs().max()) > 0


@pytest.mark.parametrize("tier", TIERS)
def test_rewind(tier):
    """Export at frame k, stream 5 frames, import back into the same slots, stream the same 5 frames again: identical outputs."""
    m, k = model_of("live"), 6
    X, C = spectra("live", 3, TA, 21), control("live", tier, 3, TA, 21)
    A = m.streaming(batch=3, one_launch=tier)
    stream(A, X, 0, k)
    state = A.export_state()
    first = stream(A, X, k, 5)
    assert A.clip_frames.tolist() == [k + 5] * 3
    A.import_state(state)
    assert A.clip_frames.tolist() == [k] * 3
    again = stream(A, X, k, 5)
    for i in range(5):
        assert same(first[i], again[i]) and same(first[i], C[k + i]), i
    # rewinding one clip only: the others go on
    state = A.export_state([2]).to("cpu")
    stream(A, X, k + 5, 2)
    A.import_state(state.to(DEV), [2])
    o = step(A, None, None, rows=[(X, 0, k + 7), (X, 1, k + 7), (X, 2, k + 5)])
    assert same(clip(o, 0), clip(C[k + 7], 0)) and same(clip(o, 1), clip(C[k + 7], 1)) and same(clip(o, 2), clip(C[k + 5], 2))
    assert A.clip_frames.tolist() == [k + 8, k + 8, k + 6]
    A.check_errors()


@pytest.mark.parametrize("tier", TIERS)
def test_fork(tier):
    """One state into two slots: identical input gives identical output, different input different output."""
    m, k = model_of("live"), 6
    X, C = spectra("live", 3, TA, 21), control("live", tier, 3, TA, 21)
    A, B = m.streaming(batch=3, one_launch=tier), m.streaming(batch=3, one_launch=tier)
    stream(A, X, 0, k)
    stream(B, spectra("live", 3, TA, 23), 0, 3)
    one = A.export_state([0])
    B.import_state(one.select([0, 0]), clips=[2, 0])
    for i in range(4):
        o = step(B, None, None, rows=[(X, 0, k + i), (X, 1, k + i), (X, 0, k + i)])
        assert same(clip(o, 0), clip(o, 2)) and same(clip(o, 0), clip(C[k + i], 0)), i
    o = step(B, None, None, rows=[(X, 0, k + 4), (X, 1, k + 4), (X, 2, k + 4)])
    assert same(clip(o, 0), clip(C[k + 4], 0)) and not torch.equal(o[0][0], o[0][2])
    B.check_errors()


# ---- waveform sessions -----------------------------------------------------------------------------------------------------------------
def wave_calls(sess, W, c0, n, host, rows=None):
    outs = []
    for c in range(c0, c0 + n):
        x = W[:, 128 * c:128 * (c + 1)] if rows is None else torch.cat([Wb[b:b + 1, 128 * (cb + c - c0):128 * (cb + c - c0 + 1)] for Wb, b, cb in rows])
        outs.append(sess.step_wave_host(x.cpu()).clone() if host else sess.step_wave(x.contiguous()).cpu())
    return outs


_WCONTROL = {}


def wave_control(name, B, calls, seed, host):
    key = (name, B, calls, seed, host)
    if key not in _WCONTROL:
        sess = model_of(name).streaming(batch=B, waveform=True, host_io=host)
        _WCONTROL[key] = wave_calls(sess, waves(name, B, calls, seed), 0, calls, host)
        sess.check_errors()
    return _WCONTROL[key]


WAVE_CASES = ([("live", c, j, False) for c in (1, 2, 3, 9) for j in (0, 4)] +
              [("live", 1, 0, True), ("live", 1, 4, True), ("live", 9, 0, True), ("live", 2, 3, True)] +  # host_io without resident
              [("2spk", 1, 4, False), ("2spk", 9, 0, False), ("2spk", 9, 4, False)])                       # two ola rows per clip


@pytest.mark.parametrize("name,c,j,host", WAVE_CASES)
def test_waveform_clips_move(name, c, j, host):
    """A clip exported at its call c (1: no frame yet) into a session at call count j (0: never called): step_wave's outputs equal the
    unmoved control's from there on, the muted first calls included.  ``2spk``: two overlap-add rows per clip."""
    m, n = model_of(name), 7
    WA, WB = waves(name, 3, 16, 31), waves(name, 2, 12, 32)
    CA, CB = wave_control(name, 3, 16, 31, host), wave_control(name, 2, 12, 32, host)
    A, B = (m.streaming(batch=b, waveform=True, host_io=host) for b in (3, 2))
    wave_calls(A, WA, 0, c, host)
    wave_calls(B, WB, 0, j, host)
    state = A.export_state([1])
    assert state.calls.tolist() == [c] and state.frames.tolist() == [max(c - 1, 0)] and {"wave", "ola"} <= set(state.sections())
    B.import_state(state, [0])
    # a session never called counts its first call as made: the other clip's utterance begins with the next call
    assert B.clip_calls.tolist() == [c, j]
    outs = wave_calls(B, None, 0, n, host, rows=[(WA, 1, c), (WB, 1, j)])
    for i in range(n):
        assert torch.equal(outs[i][0], CA[c + i][1]), ("moved", i)
        assert torch.equal(outs[i][1], CB[j + i][1]), ("other", i)
    assert any(bool(outs[i][0].any()) for i in range(n))
    B.check_errors()
    assert B.clip_calls.tolist() == [c + n, j + n] and B.clip_frames.tolist() == [c + n - 1, j + n - 1]
    A.close()
    B.close()


# ---- spike counts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", TIERS)
def test_spike_counts_follow_the_clip(tier):
    m, k, j = model_of("live"), 7, 4
    XA, XB = spectra("live", 3, TA, 21), spectra("live", 2, TB, 22)
    A, B, C = (m.streaming(batch=b, one_launch=tier, count_spikes=True) for b in (3, 2, 3))
    stream(A, XA, 0, k)
    stream(C, XA, 0, k)
    stream(B, XB, 0, j)
    other = counts(B.spike_summary([1]))
    B.import_state(A.export_state([1]), [0])
    assert counts(B.spike_summary([0])) == counts(C.spike_summary([1])) and sum(counts(B.spike_summary([0]))) > 0
    assert counts(B.spike_summary([1])) == other
    for i in range(5):
        step(C, XA, k + i)
        step(B, None, None, rows=[(XA, 1, k + i), (XB, 1, j + i)])
    assert counts(B.spike_summary([0])) == counts(C.spike_summary([1]))
    fb, _ = B.spike_summary([0])
    assert fb[1].size(0) == k + 5  # the summary's frame count is the clip's, not the session's


# ---- norms -----------------------------------------------------------------------------------------------------------------------------
def test_the_cumulative_norms_denominator_follows_the_clip():
    m, k, j = model_of("cum"), 7, 4
    XA, XB = spectra("cum", 3, TA, 41), spectra("cum", 2, TB, 42)
    CA, CB = control("cum", True, 3, TA, 41), control("cum", True, 2, TB, 42)
    A, B = m.streaming(batch=3), m.streaming(batch=2)
    stream(A, XA, 0, k)
    stream(B, XB, 0, j)
    state = A.export_state([1])
    a, b = state.sections()["cum"]
    assert bool(state.blob[:, a:b].any())
    B.import_state(state, [0])
    for i in range(NEXT):
        o = step(B, None, None, rows=[(XA, 1, k + i), (XB, 1, j + i)])
        assert same(clip(o, 0), clip(CA[k + i], 1)) and same(clip(o, 1), clip(CB[j + i], 1)), i
    B.check_errors()


@pytest.mark.parametrize("name,tier", [("frozen", False), ("lap", True), ("lap", False)], ids=["frozen_tiny", "one_launch", "per_kernel"])
def test_given_statistics_follow_the_clip(name, tier):
    m, k, j = model_of(name), 7, 4
    XA, XB = spectra(name, 3, TA, 51), spectra(name, 2, TB, 52)
    SA, SB = m.norm_stats(XA), m.norm_stats(XB)
    CA, CB = control_stats(m, tier, XA, SA), control_stats(m, tier, XB, SB)
    A, B = m.streaming(batch=3, one_launch=tier, norm_stats=SA), m.streaming(batch=2, one_launch=tier, norm_stats=SB)
    assert (A._hop is not None) is tier and len(set(SA.mu_fb.tolist() + SB.mu_fb.tolist())) == 5  # distinct clips, distinct statistics
    stream(A, XA, 0, k)
    stream(B, XB, 0, j)
    state = A.export_state([1])
    assert torch.equal(state.stats[0], SA.mu_fb[1:2]) and torch.equal(state.stats[1], SA.mu_sb[:, 1:2])
    B.import_state(state, [0])
    assert torch.equal(B._stats.mu_fb, torch.stack([SA.mu_fb[1], SB.mu_fb[1]]))  # the other clip keeps its own
    for i in range(NEXT):
        o = step(B, None, None, rows=[(XA, 1, k + i), (XB, 1, j + i)])
        assert same(clip(o, 0), clip(CA[k + i], 1)) and same(clip(o, 1), clip(CB[j + i], 1)), i
    B.check_errors()


def control_stats(m, tier, X, stats):
    sess = m.streaming(batch=X.shape[0], one_launch=tier, norm_stats=stats)
    return stream(sess, X, 0, X.shape[2])


# ---- parked in host memory ----------------------------------------------------------------------------------------------------------------
def test_a_state_parked_in_host_memory_comes_back_the_same_bits(tmp_path):
    m, k = model_of("live"), 7
    X, C = spectra("live", 3, TA, 21), control("live", True, 3, TA, 21)
    A = m.streaming(batch=3)
    stream(A, X, 0, k)
    state = A.export_state([2, 0])
    parked = state.to("cpu")
    assert parked.device.type == "cpu" and torch.equal(parked.blob, state.blob.cpu())
    torch.save(parked, tmp_path / "call.pt")
    back = torch.load(tmp_path / "call.pt", weights_only=False).to(DEV)
    assert torch.equal(back.blob, state.blob) and back.signature == state.signature
    B = m.streaming(batch=2)
    B.import_state(back, [0, 1])  # row 0 = A's clip 2, row 1 = A's clip 0
    for i in range(4):
        o = step(B, None, None, rows=[(X, 2, k + i), (X, 0, k + i)])
        assert same(clip(o, 0), clip(C[k + i], 2)) and same(clip(o, 1), clip(C[k + i], 0)), i


# ---- non-vacuity: every section of the blob is needed ----------------------------------------------------------------------------------
# (name, one-launch tier, waveform, seed of the input, k).  The tiny models forget: a zeroed membrane or last-spike row of ONE layer often
# flips no spike of the last layer within a dozen frames (measured over seeds 61 .. 65 and k = 9, 13: 1 of 10 inputs exercises every
# section of the two-speaker model, 3 of 10 of the cumulative-norm one, 8 of 10 of the live model in either tier), so each case
# names an input under which every section matters.  What is asserted is the same for any input.
ZERO_CASES = {"live_wave": ("live", True, True, 61, 9), "2spk_wave": ("2spk", True, True, 62, 13), "cum": ("cum", True, False, 62, 9),
              "per_kernel": ("live", False, False, 61, 9)}


def zeroed_sections(name, tier, waveform, seed, k, n=12):
    """Import the state of frame / call k with each section zeroed in turn -> (sections, those all zero at export, those whose zeroing
    left the next n steps as they were).  The unmodified state must reproduce the truth."""
    m = model_of(name)
    kw = dict(waveform=True) if waveform else dict(one_launch=tier)
    A, B = m.streaming(batch=2, count_spikes=True, **kw), m.streaming(batch=2, count_spikes=True, **kw)
    if waveform:
        W = waves(name, 2, k + n, seed)
        run = lambda s, c0, cnt: wave_calls(s, W, c0, cnt, False)  # noqa: E731
        differ = lambda x, y: any(not torch.equal(p, q) for p, q in zip(x, y))  # noqa: E731
    else:
        X = spectra(name, 2, k + n, seed)
        run = lambda s, c0, cnt: stream(s, X, c0, cnt)  # noqa: E731
        differ = lambda x, y: any(not same(p, q) for p, q in zip(x, y))  # noqa: E731
    run(A, 0, k)
    state = A.export_state()
    truth = run(A, k, n)
    truth_counts = counts(A.spike_summary())
    secs = state.sections()
    B.import_state(state)
    assert not differ(run(B, k, n), truth) and counts(B.spike_summary()) == truth_counts  # the unmodified state: the truth
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


@pytest.mark.parametrize("case", sorted(ZERO_CASES))
def test_zeroing_any_section_changes_the_continuation(case):
    """A control import whose one section is zeroed must make the continuation differ from the truth -- in the outputs, for the spike
    counts in spike_summary -- or the moves above could pass on inputs that never exercise that section (no history without
    max(df) > 1, no second overlap-add row without a second speaker, no running sums without the cumulative norm).  Seed and k
    are chosen so that every section is non-zero at export, which is asserted first."""
    name, tier, waveform, seed, k = ZERO_CASES[case]
    secs, zero, unchanged = zeroed_sections(name, tier, waveform, seed, k)
    want = {"hist"} | ({"wave", "ola"} if waveform else set()) | ({"cum"} if name == "cum" else set()) | ({"slots"} if tier else {"rows"})
    assert want <= set(secs) and any(s.endswith(".h") for s in secs) and any(s.endswith(".c") for s in secs)
    print(f"MIGRATE_SECTIONS {case}: {sorted(secs)}; zero at export {zero}; zeroing changed nothing {unchanged}")
    assert not zero, f"sections all zero at export: the inputs do not exercise them: {zero}"
    assert not unchanged, f"zeroing changed nothing: {unchanged}"


# ---- a batch cut into several launches ---------------------------------------------------------------------------------------------------
def test_clips_move_across_the_parts_of_a_session_and_between_one_and_two_parts():
    m, k, Bbig = model_of("live"), 6, 256
    X, C = spectra("live", 3, TA, 21), control("live", True, 3, TA, 21)
    big = m.streaming(batch=Bbig)
    parts = [(p["b0"], p["nb"]) for p in big._hop["parts"]]
    assert len(parts) > 1, "256 clips ask for more workgroups than one launch may hold"
    small = m.streaming(batch=3)
    stream(small, X, 0, k)
    cut = parts[1][0]
    junk = torch.zeros((Bbig, big.F, 1), dtype=torch.complex64, device=DEV)
    for _ in range(3):
        big.step(junk)
    # one part -> two parts: the three clips land on either side of the cut, in the caller's order
    slots = [cut, 5, cut - 1]
    big.import_state(small.export_state([0, 1, 2]), slots)
    for i in range(2):
        x = junk.clone()
        x[slots] = X[:, :, k + i:k + i + 1]
        e, mg = big.step(x)
        for r, b in enumerate(slots):
            assert same((torch.view_as_real(e)[b], mg[b]), clip(C[k + i], r)), (i, b)
    # across the parts of one session (clip cut - 1 -> the last clip), and two parts -> one part
    big.import_state(big.export_state([cut - 1]), [Bbig - 1])
    back = m.streaming(batch=2)
    back.import_state(big.export_state([cut, Bbig - 1]), [1, 0])
    x = junk.clone()
    x[Bbig - 1] = X[2, :, k + 2:k + 3]
    e, mg = big.step(x)
    assert same((torch.view_as_real(e)[Bbig - 1], mg[Bbig - 1]), clip(C[k + 2], 2))
    o = step(back, None, None, rows=[(X, 2, k + 2), (X, 0, k + 2)])
    assert same(clip(o, 0), clip(C[k + 2], 2)) and same(clip(o, 1), clip(C[k + 2], 0))
    big.check_errors()
    assert big.clip_frames[[cut, 5, Bbig - 1, 0]].tolist() == [k + 3, k + 3, k + 3, 6]


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    m = model_of("live")
    A = m.streaming(batch=3)
    X = spectra("live", 3, TA, 21)
    stream(A, X, 0, 3)
    state = A.export_state([0, 1])
    for make, field in ((lambda: m.streaming(batch=2, hop=2), "hop"), (lambda: m.streaming(batch=2, one_launch=False), "tier"),
                        (lambda: m.streaming(batch=2, waveform=True), "waveform"), (lambda: m.streaming(batch=2, count_spikes=True), "count_spikes"),
                        (lambda: model_of("2spk").streaming(batch=2), "df")):
        with pytest.raises(ValueError, match=field):
            make().import_state(state, [0, 1])
    B = m.streaming(batch=2)
    with pytest.raises(RuntimeError, match=r"\.to\("):
        B.import_state(state.to("cpu"), [0, 1])
    with pytest.raises(RuntimeError, match="2 clips for 1"):
        B.import_state(state, [0])
    with pytest.raises(ValueError, match="distinct"):
        B.import_state(state, [1, 1])
    with pytest.raises(IndexError):
        B.import_state(state, [0, 2])
    with pytest.raises(IndexError):
        A.export_state([3])
    for bad in ([0.0, 1.0], [True, False], torch.zeros((2, 1), dtype=torch.long)):
        with pytest.raises(TypeError):
            B.import_state(state, bad)
    with pytest.raises(TypeError):
        B.import_state(state.blob, [0, 1])
    with pytest.raises(ValueError):
        A.export_state([])
    R = m.streaming(batch=1, waveform=True, host_io=True, resident=True)
    with pytest.raises(NotImplementedError):
        R.export_state()
    with pytest.raises(NotImplementedError):
        R.import_state(state, [0])
    R.close()
    # nothing above touched B: it still continues a correct import
    B.import_state(state, [1, 0])
    C = control("live", True, 3, TA, 21)
    o = step(B, None, None, rows=[(X, 1, 3), (X, 0, 3)])
    assert same(clip(o, 0), clip(C[3], 1)) and same(clip(o, 1), clip(C[3], 0))
