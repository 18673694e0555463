"""Waveform sessions whose OUTER samples differ from the model's: ``model.streaming(waveform=True, resample=3, sample_format="s16")`` --
48 kHz and 16-bit PCM in and out, converted inside the hop's one launch (``sfsn_stream_hop_io``).

What such a session returns is DEFINED by a composition of things that are tested on their own: ``spectral.resample_down3`` (D3), a
plain float32 waveform session of the same model on the same calls (``control``), ``spectral.resample_up3`` (U3) and the quantiser Q,
with the two filter states carried per clip.  Everything is ``torch.equal``: the launch calls the functions the stand-alone kernels
call (csrc/sfsn_resample_dev.h), so nothing here has a tolerance.  Tiny models, 12 calls."""
import numpy as np
import pytest
import torch

import primeref as pr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CALLS = 12
COMBOS = [(3, "s16"), (3, "f32"), (1, "s16")]
_models = {}


def model_of(name):
    if name not in _models:
        import spiking_fullsubnet_amd as pkg
        front, kw, _ = pr.FIXTURES[name]
        m = (pkg.SpikingFullSubNet if front == "live" else pkg.Separator)(**kw)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in pr.state_dict(name).items()}, strict=True)
        _models[name] = m.eval().to(DEV)
    return _models[name]


def outer_samples(B, resample, fmt, calls=CALLS, seed=1):
    """[calls][B, 128 * resample] CPU tensors of the session's format; clip b is the same whatever B is."""
    n = 128 * resample
    rows = []
    for b in range(B):
        rng = np.random.default_rng(7919 * seed + b)
        t = np.arange(calls * n) / (16000.0 * resample)
        x = 0.25 * np.sin(2 * np.pi * (300.0 + 90.0 * b) * t) * (1.0 + 0.5 * np.sin(2 * np.pi * 3.0 * t)) + 0.1 * rng.standard_normal(calls * n)
        rows.append(x)
    x = np.stack(rows)
    x = np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16) if fmt == "s16" else x.astype(np.float32)
    return [torch.from_numpy(np.ascontiguousarray(x[:, c * n:(c + 1) * n])) for c in range(calls)]


def Q(v):
    """clamp(rint(v * 32768), -32768, 32767) as int16, ties to even, NaN -> 0 (torch.round rounds half to even)."""
    r = torch.round(v * 32768.0)
    r = torch.where(torch.isnan(r), torch.zeros_like(r), r)
    return torch.clamp(r, -32768.0, 32767.0).to(torch.int16)


class Composition:
    """Q(U3(control(D3(x * 2**-15)))) call by call, with per-clip resets and holds: the definition the sessions are checked against."""

    def __init__(self, model, B, resample, fmt):
        from spiking_fullsubnet_amd import spectral
        self.sp, self.B, self.resample, self.fmt = spectral, B, resample, fmt
        self.control = model.streaming(batch=B, waveform=True)
        self.S = self.control.eng.spec.num_spks
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
        out = self.control.step_wave(y.contiguous(), clips=clips)
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


def open_session(model, B, resample, fmt, host):
    return model.streaming(batch=B, waveform=True, host_io=host, resample=resample, sample_format=fmt)


def call(sess, x, host, clips=None):
    if host:
        return sess.step_wave_host(x, clips=clips).clone()
    return sess.step_wave(x.to(DEV), clips=clips).cpu()


def shared_sections_equal(a, b, where):
    sa, sb = a.sections(), b.sections()
    for name, (lo, hi) in sa.items():
        blo, bhi = sb[name]
        assert torch.equal(a.blob[:, lo:hi], b.blob[:, blo:bhi]), f"{where}: section {name}"


CASES = [("live_tiny", 3), ("live_tiny_2spk", 3), ("live_tiny", 17)]


@pytest.mark.parametrize("host", (False, True), ids=["device", "host_io"])
@pytest.mark.parametrize("resample,fmt", COMBOS, ids=[f"x{r}-{f}" for r, f in COMBOS])
@pytest.mark.parametrize("name,B", CASES, ids=[f"{n}-B{b}" for n, b in CASES])
def test_results_equal_the_composition(name, B, resample, fmt, host):
    model = model_of(name)
    sess, ref = open_session(model, B, resample, fmt, host), Composition(model, B, resample, fmt)
    S, n = ref.S, 128 * resample
    nonzero = False
    for c, x in enumerate(outer_samples(B, resample, fmt)):
        got = call(sess, x, host)
        zf, want = ref.step(x)
        assert got.dtype == (torch.int16 if fmt == "s16" else torch.float32) and tuple(got.shape) == (B, S, n)
        assert torch.equal(got, want.cpu()), f"call {c}"
        if fmt == "s16":
            assert torch.equal(got, Q(zf).cpu()), f"call {c}: int16 is Q of the float result"
        if c < 3:
            assert not bool(got.any()), f"call {c}: the three-call delay"
        nonzero = nonzero or bool(got.any())
    assert nonzero
    sess.check_errors()
    st = sess.export_state()
    shared_sections_equal(ref.control.export_state(), st, "after 12 calls")
    if resample == 3:
        lo, hi = st.sections()["dec"]
        assert torch.equal(st.blob[:, lo:hi].contiguous().view(torch.float32), ref.dec)
        lo, hi = st.sections()["int"]
        assert torch.equal(st.blob[:, lo:hi].contiguous().view(torch.float32).view(B * S, 32), ref.int)


@pytest.mark.parametrize("host", (False, True), ids=["device", "host_io"])
@pytest.mark.parametrize("resample,fmt", COMBOS, ids=[f"x{r}-{f}" for r, f in COMBOS])
def test_reset_of_one_clip_reaches_the_filters(resample, fmt, host):
    name, B = "live_tiny_2spk", 3
    model = model_of(name)
    sess, ref = open_session(model, B, resample, fmt, host), Composition(model, B, resample, fmt)
    fresh = None
    for c, x in enumerate(outer_samples(B, resample, fmt)):
        if c == 5:
            sess.reset(clips=[1])
            ref.reset([1])
            fresh = open_session(model, B, resample, fmt, host)  # every clip of it starts where clip 1 restarts
        got = call(sess, x, host)
        assert torch.equal(got, ref.step(x)[1].cpu()), f"call {c}"
        if fresh is not None:
            assert torch.equal(call(fresh, x, host)[1], got[1]), f"call {c}: clip 1 is a fresh session's clip, filter included"
    assert sess.clip_calls.tolist() == [CALLS, CALLS - 5, CALLS]


@pytest.mark.parametrize("host", (False, True), ids=["device", "host_io"])
@pytest.mark.parametrize("resample,fmt", COMBOS, ids=[f"x{r}-{f}" for r, f in COMBOS])
def test_a_held_clip_keeps_its_filters_and_its_place(resample, fmt, host):
    name, B = "live_tiny", 3
    model = model_of(name)
    sess, ref = open_session(model, B, resample, fmt, host), Composition(model, B, resample, fmt)
    xs = outer_samples(B, resample, fmt, calls=CALLS + 1)
    feed = 0  # clip 1's own next block
    for c in range(CALLS):
        x = xs[c].clone()
        if c in (0, 6):  # clip 1 is held at the session's first call and in the middle
            x[1] = xs[feed][1] * 0 + (float("nan") if fmt == "f32" else 12345)
            before = sess.export_state(clips=[1])
            got = call(sess, x, host, clips=[0, 2])
            after = sess.export_state(clips=[1])
            assert before.layout == after.layout and torch.equal(before.blob, after.blob), f"call {c}: clip 1's filter and model state"
            assert before.calls.tolist() == after.calls.tolist()
            assert got.dtype == (torch.int16 if fmt == "s16" else torch.float32) and tuple(got[1].shape) == (ref.S, 128 * resample)
            assert not bool(got[1].any()), f"call {c}: the held clip's row is zero"
            want = ref.step(x, clips=[0, 2])[1].cpu()
        else:
            x[1] = xs[feed][1]
            feed += 1
            got = call(sess, x, host)
            want = ref.step(x)[1].cpu()
        assert torch.equal(got, want), f"call {c}"
    assert sess.clip_calls.tolist() == [CALLS, CALLS - 2, CALLS]


@pytest.mark.parametrize("resample,fmt", COMBOS, ids=[f"x{r}-{f}" for r, f in COMBOS])
def test_export_import_continues_bit_for_bit(resample, fmt):
    name, B = "live_tiny_2spk", 3
    model = model_of(name)
    a = open_session(model, B, resample, fmt, False)
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
        s2 = open_session(model, B, resample, fmt, False)
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
    plain = model.streaming(batch=B, waveform=True)
    with pytest.raises(ValueError, match="resample|sample_format"):
        plain.import_state(state, clips=[0])


def test_the_default_session_is_the_explicit_plain_one():
    model = model_of("live_tiny")
    a = model.streaming(batch=3, waveform=True)
    b = model.streaming(batch=3, waveform=True, resample=1, sample_format="f32")
    assert not a._io and not b._io and a._state_signature() == b._state_signature()
    assert all(part["io"] is None for part in b._hop["parts"])  # today's launch
    for x in outer_samples(3, 1, "f32", calls=6):
        assert torch.equal(a.step_wave(x.to(DEV)), b.step_wave(x.to(DEV)))


def test_refusals():
    import spiking_fullsubnet_amd as pkg
    model = model_of("live_tiny")
    with pytest.raises(ValueError, match="resample must be 1 or 3"):
        model.streaming(batch=1, waveform=True, resample=2)
    with pytest.raises(ValueError, match="sample_format"):
        model.streaming(batch=1, waveform=True, sample_format="s24")
    with pytest.raises(ValueError, match="waveform=True"):
        model.streaming(batch=1, resample=3)
    with pytest.raises(NotImplementedError, match="resident=True"):
        model.streaming(batch=1, waveform=True, host_io=True, resident=True, resample=3)
    with pytest.raises(NotImplementedError, match="resident=True"):
        model.streaming(batch=1, waveform=True, host_io=True, resident=True, sample_format="s16")
    sess = model.streaming(batch=2, waveform=True, resample=3, sample_format="s16")
    x = torch.zeros((2, 384), dtype=torch.int16, device=DEV)
    for what, fn in (("prime_wave", lambda: sess.prime_wave(torch.zeros((2, 512), device=DEV))),
                     ("advance_wave", lambda: sess.advance_wave(torch.zeros((2, 512), device=DEV))),
                     ("advance_wave_ragged", lambda: sess.advance_wave_ragged(torch.zeros((2, 512), device=DEV), [512, 256]))):
        with pytest.raises(NotImplementedError, match=what + ".*resample=3.*sample_format='s16'"):
            fn()
    with pytest.raises(RuntimeError, match=r"int16 \(resample=3, sample_format='s16'\) \(2, 384\)"):
        sess.step_wave(torch.zeros((2, 128), device=DEV))
    with pytest.raises(RuntimeError, match=r"int16 \(resample=3, sample_format='s16'\) \(2, 384\)"):
        sess.step_wave(x.to(torch.float32))
    hs = model.streaming(batch=2, waveform=True, host_io=True, resample=3, sample_format="s16")
    with pytest.raises(RuntimeError, match=r"int16 \(2, 384\) \(resample=3, sample_format='s16'\)"):
        hs.step_wave_host(torch.zeros((2, 384)))
    with pytest.raises(RuntimeError, match=r"int16 \(2, 384\)"):
        hs.step_wave_host(torch.zeros((2, 128), dtype=torch.int16))
    assert not bool(sess.step_wave(x).any())
    from test_cirm_streaming import TINY, model as cirm_model
    cirm = cirm_model(**TINY)
    with pytest.raises(NotImplementedError, match="resample=3"):
        cirm.streaming(batch=1, waveform=True, resample=3)
    with pytest.raises(NotImplementedError, match="sample_format='s16'"):
        cirm.streaming(batch=1, waveform=True, sample_format="s16")
