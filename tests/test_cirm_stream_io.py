"""cIRM-GSN waveform sessions whose OUTER samples differ from the model's: ``Model.streaming_outer(resample=3, sample_format="s16")`` --
48 kHz and 16-bit PCM in and out, converted inside the hop's one launch (``sfsn_fullband_stream_hop_wave_io``).

As for the sibling (tests/test_stream_io.py), what such a session returns is DEFINED by a composition of things that are tested on their
own: ``spectral.resample_down3`` (D3), a plain float32 waveform session of the same module on the same calls (``control``),
``spectral.resample_up3`` (U3) and the quantiser Q, with the two filter states carried per clip; resets and holds are applied to the
composition's states.  Everything is ``torch.equal``: the launch calls the functions the stand-alone kernels call
(csrc/sfsn_resample_dev.h), so nothing here has a tolerance.  Tiny models (tests/golden/cirm_tiny*.npz), 12 calls.

Batches, the smallest at which the roles differ: B = 3 -- a partial STFT workgroup, with S = 2 six pairs in one inverse-STFT workgroup;
B = 9 -- wave 0 of the STFT workgroup owns clips 0 and 8, so its decimator window is reused behind the wave barrier; B = 16 with S = 2 --
32 pairs, four inverse-STFT workgroups, every STFT wave twice."""
import numpy as np
import pytest
import torch

from test_cirm_waveform import _fixture
from test_stream_io import COMBOS, Q, outer_samples

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CALLS = 12
IDS = [f"x{r}-{f}" for r, f in COMBOS]
ONE, TWO = "cirm_tiny.npz", "cirm_tiny_2spk.npz"


def model_of(fname):
    return _fixture(fname)[0]


def dtype_of(fmt):
    return torch.int16 if fmt == "s16" else torch.float32


class Composition:
    """Q(U3(control(D3(x * 2**-15)))) call by call, with per-clip resets and holds: the definition the sessions are checked against."""

    def __init__(self, model, B, resample, fmt):
        from spiking_fullsubnet_amd import spectral
        self.sp, self.B, self.resample, self.fmt = spectral, B, resample, fmt
        self.control = model.streaming(batch=B, waveform=True)
        self.S = self.control.S
        self.dec = torch.zeros((B, 96), device=DEV)
        self.int = torch.zeros((B * self.S, 32), device=DEV)

    def reset(self, clips):
        self.control.reset(clips=clips)
        for b in clips:
            self.dec[b].zero_()
            self.int[b * self.S:(b + 1) * self.S].zero_()

    def step(self, x, clips=None):
        """x: [B, 128 * resample] of the format (CPU or device) -> (float result [B, S, 128 * resample], the same as the format)."""
        x = x.to(DEV)
        held = [] if clips is None else [b for b in range(self.B) if b not in clips]
        dec0, int0 = self.dec.clone(), self.int.clone()
        if self.resample == 3:
            y, _ = self.sp.resample_down3(x, self.dec)
        else:
            y = x.to(torch.float32) * (1.0 / 32768.0) if x.dtype == torch.int16 else x
        y = torch.nan_to_num(y, nan=0.0) if held else y  # (a held row's samples reach nothing; keep the control's input finite)
        out = self.control.step_wave(y.contiguous()) if clips is None else self.control.tick_wave(y.contiguous(), clips)
        if self.resample == 3:
            z, _ = self.sp.resample_up3(out.reshape(self.B * self.S, 128), self.int)
            z = z.view(self.B, self.S, 384)
        else:
            z = out
        for b in held:  # a held clip: zeros out, neither filter moves
            self.dec[b] = dec0[b]
            self.int[b * self.S:(b + 1) * self.S] = int0[b * self.S:(b + 1) * self.S]
            z[b] = 0.0
        return z, (Q(z) if self.fmt == "s16" else z)


def open_session(model, B, resample, fmt, host=False):
    return model.streaming_outer(batch=B, host_io=host, resample=resample, sample_format=fmt)


def call(sess, x, host, clips=None):
    if host:
        return (sess.step_wave_host(x) if clips is None else sess.tick_wave_host(x, clips)).clone()
    x = x.to(DEV)
    return (sess.step_wave(x) if clips is None else sess.tick_wave(x, clips)).cpu()


def sections_equal(a, b, where, names=None):
    sa, sb = a.sections(), b.sections()
    for name, (lo, hi) in sa.items():
        if names is not None and name not in names:
            continue
        blo, bhi = sb[name]
        assert torch.equal(a.blob[:, lo:hi], b.blob[:, blo:bhi]), f"{where}: section {name}"


CASES = [(ONE, 3), (TWO, 3), (ONE, 9), (TWO, 16)]


@pytest.mark.parametrize("host", (False, True), ids=["device", "host_io"])
@pytest.mark.parametrize("resample,fmt", COMBOS, ids=IDS)
@pytest.mark.parametrize("fname,B", CASES, ids=[f"{n[:-4]}-B{b}" for n, b in CASES])
def test_results_equal_the_composition(fname, B, resample, fmt, host):
    model = model_of(fname)
    sess, ref = open_session(model, B, resample, fmt, host), Composition(model, B, resample, fmt)
    S, n = ref.S, 128 * resample
    assert (sess.resample, sess.sample_format, sess._io, sess._outer) == (resample, fmt, True, n)
    later = False
    for c, x in enumerate(outer_samples(B, resample, fmt)):
        got = call(sess, x, host)
        zf, want = ref.step(x)
        assert got.dtype == dtype_of(fmt) and tuple(got.shape) == (B, S, n)
        assert torch.equal(got, want.cpu()), f"call {c}"
        if fmt == "s16":
            assert torch.equal(got, Q(zf).cpu()), f"call {c}: int16 is Q of the float result"
        if c < 3:
            assert not bool(got.any()), f"call {c}: the three-call delay"
        else:
            later = later or bool(got.any())
    assert later, "the compared result is not zero after call 3"
    sess.check_errors()
    assert sess.launches == {"hop": CALLS}, "one launch per call"
    st = sess.export_state()
    sections_equal(ref.control.export_state(), st, "after 12 calls")
    if resample == 3:
        lo, hi = st.sections()["dec"]
        assert torch.equal(st.blob[:, lo:hi].contiguous().view(torch.float32), ref.dec)
        lo, hi = st.sections()["int"]
        assert torch.equal(st.blob[:, lo:hi].contiguous().view(torch.float32).view(B * S, 32), ref.int)


@pytest.mark.parametrize("host", (False, True), ids=["device", "host_io"])
@pytest.mark.parametrize("resample,fmt", COMBOS, ids=IDS)
def test_a_hold_and_a_restart_reach_the_filters(resample, fmt, host):
    """Clip 1 is held on calls 4-6 with NaN (int16: the minimum) in its row, and restarts at call 7: it must not ring."""
    B = 3
    model = model_of(TWO)
    sess, ref = open_session(model, B, resample, fmt, host), Composition(model, B, resample, fmt)
    xs = outer_samples(B, resample, fmt, calls=CALLS)
    feed = 0  # clip 1's own next block
    fresh = None
    for c in range(CALLS):
        x = xs[c].clone()
        if c == 7:
            sess.reset(clips=[1])
            ref.reset([1])
            fresh = open_session(model, B, resample, fmt, host)  # every clip of it starts where clip 1 restarts
        if 4 <= c <= 6:
            x[1] = float("nan") if fmt == "f32" else -32768
            before = sess.export_state(clips=[1])
            got = call(sess, x, host, clips=[0, 2])
            after = sess.export_state(clips=[1])
            assert before.layout == after.layout and torch.equal(before.blob, after.blob), f"call {c}: clip 1's filter and model state"
            assert before.calls.tolist() == after.calls.tolist()
            assert not bool(got[1].any()), f"call {c}: the held clip's rows are zero"
            want = ref.step(x, clips=[0, 2])[1].cpu()
        else:
            x[1] = xs[feed][1]
            feed += 1
            got = call(sess, x, host)
            want = ref.step(x)[1].cpu()
        assert got.dtype == dtype_of(fmt) and tuple(got.shape) == (B, ref.S, 128 * resample)
        assert torch.equal(got, want), f"call {c}"
        if fresh is not None:
            assert torch.equal(call(fresh, x, host)[1], got[1]), f"call {c}: clip 1 is a fresh session's clip, filter included"
            if c < 10:
                assert not bool(got[1].any()), f"call {c}: the restarted clip rings"
    assert bool(got[1].any())
    assert sess.clip_calls().tolist() == [CALLS, CALLS - 7, CALLS]
    assert sess.launches == {"hop": CALLS}, "holds and restarts add no launch"
    sess.check_errors()


@pytest.mark.parametrize("resample,fmt", COMBOS, ids=IDS)
def test_export_import_continues_bit_for_bit(resample, fmt):
    B = 3
    model = model_of(TWO)
    a = open_session(model, B, resample, fmt)
    xs = outer_samples(B, resample, fmt)
    for c in range(6):
        call(a, xs[c], False)
    state = a.export_state(clips=[2])
    names = list(state.sections())
    assert (names[-2:] == ["dec", "int"]) == (resample == 3) and ("dec" in names) == (resample == 3)
    others = {"moved": state}
    if resample == 3:
        for sec in ("dec", "int"):
            z = state.clone()
            lo, hi = z.sections()[sec]
            assert bool(z.blob[:, lo:hi].any()), f"{sec}: the carried samples are not zero after six calls"
            z.blob[:, lo:hi] = 0
            others[sec] = z
    sessions = {}
    for k, st in others.items():
        s2 = open_session(model, B, resample, fmt)
        call(s2, xs[0], False)  # the session is running when the clip arrives
        s2.import_state(st, clips=[0])
        sessions[k] = s2
    same = {k: True for k in sessions}
    for c in range(6, CALLS):
        want = call(a, xs[c], False)[2]
        for k, s2 in sessions.items():
            x = xs[c].clone()
            x[0] = xs[c][2]
            same[k] = same[k] and torch.equal(call(s2, x, False)[0], want)
    assert same.pop("moved"), "the moved clip continues bit for bit in another slot of another session"
    for k, v in same.items():
        assert not v, f"a state with its {k!r} section zeroed must not continue alike"
    # a state moves only between sessions of the same options
    plain = model.streaming(batch=B, waveform=True)
    with pytest.raises(ValueError, match="resample|sample_format"):
        plain.import_state(state, clips=[0])
    other = [cmb for cmb in COMBOS if cmb != (resample, fmt)][0]
    with pytest.raises(ValueError, match="resample|sample_format"):
        open_session(model, B, *other).import_state(state, clips=[0])
    with pytest.raises(ValueError, match="resample|sample_format"):
        a.import_state(plain.export_state(clips=[0]), clips=[0])


def test_a_plain_session_is_what_it_was():
    """Its launches, its signature and its blob: nothing of the options reaches a session opened without them."""
    import dataclasses
    from spiking_fullsubnet_amd import clip_state
    model = model_of(ONE)
    B = 3
    a = model.streaming(batch=B, waveform=True)
    assert not a._io and a._hop["io"] is None and a._hop["io_ref"] is None and (a.resample, a.sample_format, a._outer) == (1, "f32", 128)
    names = []
    launch = a._launch
    a._launch = lambda name, *args: (names.append(name), launch(name, *args))[1]
    xs = outer_samples(B, 1, "f32", calls=6)
    for c, x in enumerate(xs):
        out = a.step_wave(x.to(DEV)) if c != 4 else a.tick_wave(x.to(DEV), [0, 2])
        assert out.dtype == torch.float32 and tuple(out.shape) == (B, 1, 128)
    assert names == ["sfsn_fullband_stream_hop_wave"] * 4 + ["sfsn_fullband_stream_hop_wave_held", "sfsn_fullband_stream_hop_wave"]
    eng = a.eng
    want = [("model", "cirm_gsn"), ("tier", "one_launch"), ("hop", 1), ("waveform", True), ("count_spikes", False), ("F", 257), ("Hp", eng.Hp)]
    want += [(k, v) for k, v in dataclasses.asdict(eng.spec).items() if k != "bn"]
    assert a._state_signature() == tuple(want)
    st = a.export_state()
    layout, nbytes = clip_state.fullband_sections(eng.spec.layers, eng.Hp, False, 257, eng.spec.df - 1, True, 1)
    assert st.layout == layout and st.blob.shape[1] == nbytes and st.signature == tuple((str(k), v) for k, v in want)
    assert "dec" not in st.sections() and "int" not in st.sections()
    # and an io session's head IS that blob: the same sections at the same places, the filters behind them
    b = open_session(model, B, 3, "s16")
    lb, nb = b._state_layout()
    assert lb[:-2] == layout and [n for n, _, _ in lb[-2:]] == ["dec", "int"] and lb[-2][1] == nbytes and nb == nbytes + 96 * 4 + 32 * 4
    assert dict(b._state_signature())["resample"] == 3 and dict(b._state_signature())["sample_format"] == "s16"


def test_refusals():
    model = model_of(ONE)
    sess = open_session(model, 2, 3, "s16")
    x = torch.zeros((2, 384), dtype=torch.int16, device=DEV)
    for fn in (sess.step_wave, lambda t: sess.tick_wave(t, [0])):
        with pytest.raises(RuntimeError, match=r"int16 \(resample=3, sample_format='s16'\) \(2, 384\)"):
            fn(torch.zeros((2, 128), device=DEV))
        with pytest.raises(RuntimeError, match=r"int16 \(resample=3, sample_format='s16'\) \(2, 384\)"):
            fn(x.to(torch.float32))
        with pytest.raises(RuntimeError, match=r"int16 \(resample=3, sample_format='s16'\) \(2, 384\)"):
            fn(torch.zeros((2, 128), dtype=torch.int16, device=DEV))
    with pytest.raises(RuntimeError, match="host_io=True"):
        sess.step_wave_host(x.cpu())
    hs = open_session(model, 2, 3, "s16", host=True)
    for fn in (hs.step_wave_host, lambda t: hs.tick_wave_host(t, [1])):
        with pytest.raises(RuntimeError, match=r"int16 \(2, 384\) \(resample=3, sample_format='s16'\)"):
            fn(torch.zeros((2, 384)))
        with pytest.raises(RuntimeError, match=r"int16 \(2, 384\)"):
            fn(torch.zeros((2, 128), dtype=torch.int16))
    with pytest.raises(RuntimeError, match="use step_wave_host"):
        hs.step_wave(x)
    f3 = open_session(model, 2, 3, "f32")
    with pytest.raises(RuntimeError, match=r"float32 \(resample=3, sample_format='f32'\) \(2, 384\)"):
        f3.step_wave(torch.zeros((2, 128), device=DEV))
    assert sess.launches == {} and hs.launches == {} and f3.launches == {}, "a refused call launches nothing"
    assert not bool(sess.step_wave(x).any())
    # the backlog's own refusals
    with pytest.raises(RuntimeError, match=r"int16 \(resample=3, sample_format='s16'\)"):
        sess.catch_up_wave(torch.zeros((2, 768), device=DEV))
    with pytest.raises(ValueError, match="multiple of 384"):
        sess.catch_up_wave(torch.zeros((2, 512), dtype=torch.int16, device=DEV))
    with pytest.raises(NotImplementedError, match=r"catch_up_wave_ragged.*resample=3.*sample_format='s16'"):
        sess.catch_up_wave_ragged(torch.zeros((2, 768), dtype=torch.int16, device=DEV), [768, 384])
    # the factory: what streaming(waveform=True) refuses is refused alike, and streaming() itself keeps refusing the options
    with pytest.raises(NotImplementedError, match="waveform=True.*B=17"):
        model.streaming_outer(batch=17)
    with pytest.raises(ValueError, match=r"streaming\(waveform=True\)"):
        model.streaming_outer(resample=1, sample_format="f32")
    with pytest.raises(NotImplementedError, match="resample=3"):
        model.streaming(batch=1, waveform=True, resample=3)


KINDS = ("running", "one_call", "no_call")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", (1, 2, 5))
@pytest.mark.parametrize("resample,fmt", COMBOS, ids=IDS)
def test_a_backlog_equals_the_calls_it_replaces(resample, fmt, c, kind):
    """``catch_up_wave`` on clips [2, 0] of one session against ``c`` ``tick_wave`` calls of those clips on another, both with the same
    six calls behind them: the results, every section of ``export_state`` (both filters included) and three more calls are equal.
    ``one_call``: the clips restarted and have made one call since (the backlog crosses the mute boundary); ``no_call``: none."""
    B, n = 3, 128 * resample
    model = model_of(TWO)
    a, b = open_session(model, B, resample, fmt), open_session(model, B, resample, fmt)
    xs = [x.to(DEV) for x in outer_samples(B, resample, fmt, calls=6 + 1 + c + 3)]
    for s in (a, b):
        for x in xs[:6]:
            s.step_wave(x)
        if kind != "running":
            s.reset(clips=[0, 2])
        if kind == "one_call":
            assert not bool(s.tick_wave(xs[6], [0, 2]).any())
    assert a.clip_calls().tolist() == [dict(running=6, one_call=1, no_call=0)[kind], 6, dict(running=6, one_call=1, no_call=0)[kind]]
    blocks = xs[7:7 + c]
    backlog = torch.cat(blocks, dim=1)[[2, 0]].contiguous()  # rows in the caller's order
    launches = dict(a.launches)
    got = a.catch_up_wave(backlog, clips=[2, 0])
    assert a.launches.get("hop", 0) == launches.get("hop", 0), "the backlog makes no hop launch"
    want = torch.cat([b.tick_wave(x, [0, 2]) for x in blocks], dim=-1)[[2, 0]]
    assert got.dtype == dtype_of(fmt) and tuple(got.shape) == (2, a.S, n * c)
    assert torch.equal(got, want)
    if kind == "running" or c >= 3:
        assert bool(got.any())
    assert a.clip_calls().tolist() == b.clip_calls().tolist() and a.clip_frames().tolist() == b.clip_frames().tolist()
    sa, sb = a.export_state(), b.export_state()
    assert sa.layout == sb.layout and sa.calls.tolist() == sb.calls.tolist()
    # (a clip whose only call so far is its first has no frame yet: what the model stages and the accumulator hold for it is whatever
    # that launch left there -- include/sfsn.h, k == -1: "discarded by the next launch" -- and the backlog leaves those rows alone,
    # as it does on a plain session; its samples and both filters are defined, and three calls later everything is)
    defined = ("wave", "dec", "int") if kind == "no_call" and c == 1 else None
    sections_equal(sa, sb, f"after the backlog ({kind}, c={c})", defined)
    for x in xs[7 + c:]:
        assert torch.equal(a.step_wave(x), b.step_wave(x))
    sections_equal(a.export_state(), b.export_state(), "three calls later")
    a.check_errors()
    b.check_errors()


def test_a_backlog_of_mixed_kinds_is_refused():
    B = 3
    model = model_of(ONE)
    sess = open_session(model, B, 3, "s16")
    xs = [x.to(DEV) for x in outer_samples(B, 3, "s16", calls=3)]
    for x in xs[:2]:
        sess.step_wave(x)
    sess.reset(clips=[0])
    before = sess.export_state()
    with pytest.raises(ValueError, match="clip 0 has made no call in its current utterance and clip 2 has"):
        sess.catch_up_wave(torch.cat([xs[2], xs[2]], dim=1)[[0, 2]].contiguous(), clips=[0, 2])
    assert torch.equal(before.blob, sess.export_state().blob), "a refused backlog changes nothing"
