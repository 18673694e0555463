"""``StreamingSession.advance_ragged`` / ``advance_wave_ragged`` with ``sfsn_hop_advance_ragged``: one call runs a backlog of ITS OWN
length per clip.  The whole specification is the sequence of single-clip calls ``advance(stft[i:i+1, :, :frames[i]],
clips=[clips[i]])``: two sessions with the same past, one makes the ragged call, the control makes the single-clip calls, and then

* the results are ``torch.equal`` over each clip's own range and zero behind it (NaN is planted in every input row past its length,
  and the allocator's free blocks are filled with a sentinel first, so "zero" is something the call wrote);
* ``export_state`` is equal section by section with NO exception -- the layer-0 membranes included: both sides run the offline kernels;
* ``clip_frames`` / ``clip_calls`` and the spike counts are equal;
* three more launches on both give the same outputs and the same state again.

The fixtures, seeds and inputs are tests/primeref.py's; the lengths come from ``primeref.prefix_lengths``, so that one call mixes a clip
below the deep filter's reach, clips that leave on different parities of the double-buffered state, and the longest row.  An
implementation that takes any clip's state from the last padded frame fails every comparison here."""
import ctypes

import pytest
import torch

import hopref as hr
import primeref as pr
from test_stream_advance import book, model_of, own_stats, real

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 3


def lengths(hop, name):
    """(below the reach where a launch is shorter than it, an odd / even number of launches, the longest) from prefix_lengths."""
    Ns = pr.prefix_lengths(hop, pr.df_reach(name))
    odd = 17 if hop == 1 else 18
    assert Ns[0] == hop and odd in Ns and Ns[-1] == 40
    assert (Ns[0] // hop) % 2 != (40 // hop) % 2 or (odd // hop) % 2 != (40 // hop) % 2  # (both parities of the launch count)
    return (Ns[0], odd, 40)


def sentinel_the_free_blocks():
    """Fill what the caching allocator will hand out next with 0x5A bytes: a result the call did not write shows."""
    big = torch.empty((8 << 20,), dtype=torch.uint8, device=DEV)
    big.fill_(0x5A)
    del big


def same_state(a, b, where):
    """``export_state`` of two sessions, section by section, no exception."""
    sa, sb = a.export_state(), b.export_state()
    assert sa.layout == sb.layout and sa.frames.tolist() == sb.frames.tolist(), where
    assert (sa.calls is None) == (sb.calls is None) and (sa.calls is None or sa.calls.tolist() == sb.calls.tolist()), where
    for name, lo, hi in sa.layout:
        assert torch.equal(sa.blob[:, lo:hi], sb.blob[:, lo:hi]), f"{where}: section {name}"


def planted(rows, lens, unit=1):
    """The padded input: row i keeps its first lens[i] * unit entries of the last axis, NaN behind."""
    x = rows.clone()
    for i, n in enumerate(lens):
        x[i, ..., n * unit:] = float("nan")
    return x


def near_wrap(sess, k):
    for part in sess._hop["parts"]:
        part["desc"].launch_index = k
        part["origin"].fill_(sess._as_i32(k))


def ragged_against_singles(sess, control, stft, at, lens, clips, where):
    """One ragged call on `sess` against the single-clip calls on `control`; clip clips[i] takes lens[i] frames from its frame at[i]."""
    Nmax = max(lens)
    rows = torch.zeros((len(clips), stft.shape[1], Nmax), dtype=stft.dtype, device=DEV)
    for i, (b, t, n) in enumerate(zip(clips, at, lens)):
        rows[i, :, :n] = stft[b, :, t:t + n]
    sentinel_the_free_blocks()
    e, m = sess.advance_ragged(planted(rows, lens), list(lens), clips=None if clips == list(range(sess.B)) else clips)
    assert e.shape[0] == len(clips) and e.shape[-1] == Nmax and m.shape == e.shape, where
    for i, (b, n) in enumerate(zip(clips, lens)):
        ce, cm = control.advance(rows[i:i + 1, :, :n].contiguous(), clips=[b])
        assert torch.equal(real(e[i:i + 1, ..., :n]), real(ce)) and torch.equal(m[i:i + 1, ..., :n], cm), f"{where}: clip {b}"
        assert not bool(real(e[i, ..., n:]).any()) and not bool(m[i, ..., n:].any()), f"{where}: clip {b} is not zero behind its frames"
    sess.check_errors()
    control.check_errors()
    assert book(sess) == book(control), where
    same_state(sess, control, where)


def step_both(sess, control, stft, at, n_launches, where, clips=None):
    """The same launches on both sessions, clip b reading on from frame at[b]."""
    hop = sess.hop
    for j in range(n_launches):
        x = torch.stack([stft[b, :, at[b] + j * hop:at[b] + (j + 1) * hop] for b in range(sess.B)]).contiguous()
        kw = {} if clips is None else dict(clips=clips)
        (e, m), (ce, cm) = sess.step(x, **kw), control.step(x, **kw)
        sel = list(range(sess.B)) if clips is None else clips
        assert torch.equal(real(e[sel]), real(ce[sel])) and torch.equal(m[sel], cm[sel]), f"{where}: launch {j} behind the backlog"
    sess.check_errors()
    control.check_errors()
    assert book(sess) == book(control), where
    same_state(sess, control, f"{where}, three launches on")


# ---- 1. every clip of the session, lengths mixed and permuted, both tiers -----------------------------------------------------------
CASES = [(n, hop, ol) for n in ("live_tiny", "live_tiny_2spk", "live_tiny_unshared", "frozen_tiny") for hop in (1, 2) for ol in (True, False)]


@pytest.mark.parametrize("name,hop,one_launch", CASES, ids=[f"{n}-hop{h}-{'one' if o else 'graph'}" for n, h, o in CASES])
def test_one_ragged_call_equals_the_single_clip_calls(name, hop, one_launch):
    model = model_of(name)
    stft = torch.from_numpy(pr.spectra(name, B)).to(DEV)
    stats = own_stats(name, model, stft)
    kw = dict(batch=B, hop=hop, one_launch=one_launch, graph=True, count_spikes=True, norm_stats=stats)
    sess, control = model.streaming(**kw), model.streaming(**kw)
    assert (sess._hop is not None) == one_launch
    a, b, c = lengths(hop, name)
    for lens in ((a, b, c), (c, a, b)):
        where = f"lengths {lens}"
        k0 = 5 * hop  # an odd number of launches behind
        for s in (sess, control):
            s.reset()
            for k in range(0, k0, hop):
                s.step(stft[..., k:k + hop].contiguous())
        ragged_against_singles(sess, control, stft, [k0] * B, lens, list(range(B)), where)
        assert sess.clip_frames.tolist() == [k0 + n for n in lens]
        step_both(sess, control, stft, [k0 + n for n in lens], 3, where)


@pytest.mark.parametrize("one_launch", [True, False])
def test_a_clip_long_enough_to_take_the_split_input_product_alone(one_launch):
    """The layer-0 input product takes its bf16-split form from 64 row-frames on (include/sfsn.h): the full-band model of a clip alone
    has one row per frame, so a backlog of 70 frames takes it and the shorter ones beside it do not -- each clip's membranes are still
    those of its own call."""
    name, hop, frames = "live_tiny", 1, 96
    model = model_of(name)
    stft = torch.from_numpy(pr.spectra(name, B, frames)).to(DEV)
    kw = dict(batch=B, hop=hop, one_launch=one_launch, graph=True, count_spikes=True)
    sess, control = model.streaming(**kw), model.streaming(**kw)
    k0, lens = 5, (17, 70, 1)
    for s in (sess, control):
        for k in range(k0):
            s.step(stft[..., k:k + 1].contiguous())
    ragged_against_singles(sess, control, stft, [k0] * B, lens, list(range(B)), f"lengths {lens}")
    step_both(sess, control, stft, [k0 + n for n in lens], 3, f"lengths {lens}")


# ---- 2. some clips listed, not in ascending order; one unlisted clip steps on; a fresh clip, a restarted clip; the counter's wrap --------
@pytest.mark.parametrize("name,hop,one_launch,wrap", [("live_tiny", 1, True, 0), ("live_tiny", 1, True, 2 ** 32 - 3), ("live_tiny", 2, True, 2 ** 32 - 3),
                                                     ("live_tiny", 1, True, 2 ** 31 + 3), ("live_tiny", 1, False, 0),
                                                     ("live_tiny_2spk", 2, False, 0), ("frozen_tiny", 2, True, 0)])
def test_listed_clips_in_any_order_fresh_and_restarted_clips_and_the_wrap(name, hop, one_launch, wrap):
    model = model_of(name)
    stft = torch.from_numpy(pr.spectra(name, B)).to(DEV)
    stats = own_stats(name, model, stft)
    kw = dict(batch=B, hop=hop, one_launch=one_launch, graph=True, count_spikes=True, norm_stats=stats)
    sess, control = model.streaming(**kw), model.streaming(**kw)
    a, b, c = lengths(hop, name)
    n0 = 7
    for s in (sess, control):
        if wrap:
            near_wrap(s, wrap)
        for k in range(n0):  # clips 0 and 1 make 7 launches (the counter wraps inside them); clip 2 is held from the start: never stepped
            s.step(stft[..., k * hop:(k + 1) * hop].contiguous(), clips=[0, 1])
    t = n0 * hop
    assert sess.clip_frames.tolist() == [t, t, 0]
    # (a) clips 2 and 0, in that order: a fresh clip with the longest backlog and a running one below the reach; clip 1 is not listed
    ragged_against_singles(sess, control, stft, [0, t], (c, a), [2, 0], "clips [2, 0]")
    assert sess.clip_frames.tolist() == [t + a, t, c]
    at = [t + a, t, c]
    step_both(sess, control, stft, at, 3, "clips [2, 0]")  # everybody steps on: the unlisted clip from where it was
    at = [x + 3 * hop for x in at]
    # (b) clip 1 restarted -- its rows still hold the old utterance -- and listed with the odd backlog beside two running clips
    for s in (sess, control):
        s.reset(clips=[1])
    other = 4  # the restarted clip's new utterance: clip 1's own frames from another place
    ragged_against_singles(sess, control, stft, [other, at[2], at[0]], (b, a, a + hop), [1, 2, 0], "restarted clip 1")
    assert sess.clip_frames.tolist() == [at[0] + a + hop, b, at[2] + a]
    at = [at[0] + a + hop, other + b, at[2] + a]
    step_both(sess, control, stft, at, 3, "restarted clip 1")
    # a restarted clip that advances equals a fresh session that primes
    fresh = model.streaming(**dict(kw, batch=1, norm_stats=None if stats is None else stats.select([1])))
    fresh.prime(stft[1:2, :, other:other + b].contiguous())
    x = stft[1:2, :, at[1] + 3 * hop:at[1] + 4 * hop].contiguous()
    e, _ = sess.step(torch.cat([x, x, x]).contiguous(), clips=[1])
    f, _ = fresh.step(stft[1:2, :, other + b:other + b + hop].contiguous())
    f, _ = fresh.step(stft[1:2, :, other + b + hop:other + b + 2 * hop].contiguous())
    f, _ = fresh.step(stft[1:2, :, other + b + 2 * hop:other + b + 3 * hop].contiguous())
    f, _ = fresh.step(x)
    assert torch.equal(real(e[1:2]), real(f))


def test_a_session_cut_into_parts_takes_each_parts_clips_with_their_own_lengths():
    name, big, k0 = "live_tiny", 256, 3
    model = model_of(name)
    stft = torch.from_numpy(pr.spectra(name, B)).to(DEV)
    sess, control = model.streaming(batch=big, count_spikes=True), model.streaming(batch=big, count_spikes=True)
    parts = [(p["b0"], p["nb"]) for p in sess._hop["parts"]]
    assert len(parts) > 1, "256 clips ask for more workgroups than one launch may hold"
    clips = [parts[1][0], 5, parts[1][0] - 1]  # clips of two parts, either side of the cut, not in ascending order
    for s in (sess, control):
        for t in range(k0):
            x = torch.zeros((big, s.F, 1), dtype=torch.complex64, device=DEV)
            x[clips] = stft[..., t:t + 1]
            s.step(x)
    lens = (17, 40, 1)
    rows = torch.stack([stft[i, :, k0:k0 + 40] for i in range(B)])
    e, m = sess.advance_ragged(planted(rows, lens), lens, clips=clips)
    for i, (b, n) in enumerate(zip(clips, lens)):
        ce, cm = control.advance(rows[i:i + 1, :, :n].contiguous(), clips=[b])
        assert torch.equal(real(e[i:i + 1, ..., :n]), real(ce)) and torch.equal(m[i:i + 1, ..., :n], cm), b
        assert not bool(real(e[i, ..., n:]).any()) and not bool(m[i, ..., n:].any()), b
    sess.check_errors()
    assert sess.clip_frames[clips].tolist() == [k0 + n for n in lens] and sess.clip_frames[0] == k0
    assert sess.clip_frames.tolist() == control.clip_frames.tolist()
    same_state(sess, control, "a session cut into parts")
    x = torch.zeros((big, sess.F, 1), dtype=torch.complex64, device=DEV)
    x[clips] = torch.stack([stft[i, :, k0 + n:k0 + n + 1] for i, n in enumerate(lens)])
    (e, _), (ce, _) = sess.step(x), control.step(x)
    assert torch.equal(real(e), real(ce))
    same_state(sess, control, "a session cut into parts, one launch on")


# ---- 3. equal lengths are `advance`; a shorter longest row is padded with zeros ---------------------------------------------------------
@pytest.mark.parametrize("one_launch", [True, False])
def test_equal_lengths_delegate_to_advance(one_launch):
    name, hop = "live_tiny", 2
    model = model_of(name)
    stft = torch.from_numpy(pr.spectra(name, B)).to(DEV)
    kw = dict(batch=B, hop=hop, one_launch=one_launch, count_spikes=True)
    sess, control = model.streaming(**kw), model.streaming(**kw)
    for s in (sess, control):
        s.step(stft[..., :hop].contiguous())
    rows = stft[..., hop:hop + 12]
    e, m = sess.advance_ragged(planted(rows, [8, 8, 8]), torch.tensor([8, 8, 8]))
    ce, cm = control.advance(rows[..., :8].contiguous())
    assert e.shape[-1] == 12 and torch.equal(real(e[..., :8]), real(ce)) and torch.equal(m[..., :8], cm)
    assert not bool(real(e[..., 8:]).any()) and not bool(m[..., 8:].any())
    assert book(sess) == book(control)
    same_state(sess, control, "equal lengths")
    # different lengths below a longer tensor: the forward runs on the longest clip's frames, the result has the tensor's
    e, m = sess.advance_ragged(planted(stft[..., hop + 8:hop + 20], [2, 6, 4]), [2, 6, 4])
    assert e.shape[-1] == 12 and not bool(real(e[..., 6:]).any())
    for i, n in enumerate((2, 6, 4)):
        ce, _ = control.advance(stft[i:i + 1, :, hop + 8:hop + 8 + n].contiguous(), clips=[i])
        assert torch.equal(real(e[i:i + 1, ..., :n]), real(ce)) and not bool(real(e[i, ..., n:]).any())
    same_state(sess, control, "a tensor longer than the longest clip")


# ---- 4. waveform sessions -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,host_io", [("live_tiny", False), ("live_tiny_2spk", False), ("live_tiny", True)])
def test_one_ragged_wave_call_equals_the_single_clip_calls(name, host_io):
    model = model_of(name, pr.WAVE_FIXTURES[name])
    S = pr.FIXTURES[name][1].get("num_spks", 1)
    w = torch.from_numpy(pr.waves(name, B)).to(DEV)
    kw = dict(batch=B, waveform=True, count_spikes=True, host_io=host_io)

    def call(s, x):
        return s.step_wave_host(x.cpu()).to(DEV).clone() if host_io else s.step_wave(x)

    sess, control = model.streaming(**kw), model.streaming(**kw)
    m0 = 4  # calls behind (launch index 3: odd)
    for cs in ((1, 4, 19), (19, 1, 4)):
        where = f"calls {cs}"
        for s in (sess, control):
            s.reset()
            for k in range(m0):
                call(s, w[:, 128 * k:128 * (k + 1)].contiguous())
        cmax = max(cs)
        rows = w[:, 128 * m0:128 * (m0 + cmax)]
        sentinel_the_free_blocks()
        r = sess.advance_wave_ragged(planted(rows, cs, 128), [128 * c for c in cs])
        assert r.shape == (B, S, 128 * cmax) and r.device.type == "cuda", where
        for b, c in enumerate(cs):
            cr = control.advance_wave(rows[b:b + 1, :128 * c].contiguous(), clips=[b])
            assert torch.equal(r[b:b + 1, :, :128 * c], cr), f"{where}: clip {b}"
            assert not bool(r[b, :, 128 * c:].any()), f"{where}: clip {b} is not zero behind its samples"
        assert sess.clip_calls.tolist() == [m0 + c for c in cs]
        assert book(sess) == book(control), where
        same_state(sess, control, where)
        for j in range(3):
            x = torch.stack([w[b, 128 * (m0 + c + j):128 * (m0 + c + j + 1)] for b, c in enumerate(cs)]).contiguous()
            assert torch.equal(call(sess, x), call(control, x)), f"{where}: call {j} behind the backlog"
        sess.check_errors()
        control.check_errors()
        assert book(sess) == book(control), where
        same_state(sess, control, f"{where}, three calls on")
    # clips listed out of order, one unlisted
    r = sess.advance_wave_ragged(planted(w[[2, 0], 128 * 20:128 * 23], (3, 1), 128), [384, 128], clips=[2, 0])
    for i, (b, c) in enumerate(((2, 3), (0, 1))):
        cr = control.advance_wave(w[b:b + 1, 128 * 20:128 * (20 + c)].contiguous(), clips=[b])
        assert torch.equal(r[i:i + 1, :, :128 * c], cr) and not bool(r[i, :, 128 * c:].any())
    same_state(sess, control, "clips [2, 0]")


# ---- 5. the cumulative norm is refused, and what else needs a device to be refused ---------------------------------------------------
def test_the_cumulative_norm_raises_and_nothing_moves():
    name = "frozen_tiny_cum"
    model = model_of(name)
    stft = torch.from_numpy(pr.spectra(name, B)).to(DEV)
    sess, control = model.streaming(batch=B), model.streaming(batch=B)  # (the cumulative norm streams through the one-launch hop only)
    assert sess._hop is not None
    for s in (sess, control):
        s.step(stft[..., :1].contiguous())
    with pytest.raises(NotImplementedError, match="one `advance` call per length"):
        sess.advance_ragged(stft[..., 1:41], [1, 17, 40])
    assert sess.clip_frames.tolist() == [1, 1, 1]
    same_state(sess, control, "after the refusal")
    e, _ = sess.advance_ragged(stft[..., 1:41], [17, 17, 17])  # equal lengths are `advance`, which this model has
    ce, _ = control.advance(stft[..., 1:18].contiguous())
    assert torch.equal(real(e[..., :17]), real(ce)) and not bool(real(e[..., 17:]).any())
    same_state(sess, control, "equal lengths")
    wname = "frozen_tiny_cum"
    wmodel = model_of(wname, pr.WAVE_FIXTURES[wname])
    w = torch.from_numpy(pr.waves(wname, B)).to(DEV)
    ws = wmodel.streaming(batch=B, waveform=True)
    ws.step_wave(w[:, :128].contiguous())
    with pytest.raises(NotImplementedError, match="one `advance` call per length"):
        ws.advance_wave_ragged(w[:, 128:128 * 5], [128, 256, 512])
    assert ws.clip_calls.tolist() == [1, 1, 1]


def test_what_the_launch_and_the_sessions_refuse():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    model = model_of("live_tiny")
    sess = model.streaming(batch=B, hop=2, one_launch=True)
    ref, D = sess._hop["parts"][0]["ref"], sess.D
    fn = L.sfsn_hop_advance_ragged

    def call(src, clips=(1,)):
        return fn(ref, (ctypes.c_int * len(clips))(*clips), len(clips), ctypes.byref(src), None)

    for Nmax, T in ((3, D + 3), (0, D), (4, D + 3)):  # not a multiple of hop; no frame; rows shorter than [history | new]
        bad = _lib.AdvanceRaggedSrc()
        bad.Bp, bad.Nmax, bad.T = 1, Nmax, T
        assert call(bad) == _lib.SFSN_EINVAL
    ok = _lib.AdvanceRaggedSrc()
    ok.Bp, ok.Nmax, ok.T = 1, 4, D + 4
    assert call(ok) == _lib.SFSN_EINVAL                       # valid geometry, NULL tensors: refused, not launched
    assert call(ok, (3,)) == _lib.SFSN_EINVAL and call(ok, (-1,)) == _lib.SFSN_EINVAL
    assert call(ok, (0, 1)) == _lib.SFSN_EINVAL               # more clips than the tensors have rows
    two = _lib.AdvanceRaggedSrc()
    two.Bp, two.Nmax, two.T = 2, 4, D + 4
    assert call(two, (1, 1)) == _lib.SFSN_EINVAL              # listed twice
    cum = model_of("frozen_tiny_cum").streaming(batch=B, one_launch=True)
    assert fn(cum._hop["parts"][0]["ref"], (ctypes.c_int * 1)(0), 1, ctypes.byref(ok), None) == _lib.SFSN_EUNSUPPORTED
    torch.cuda.synchronize()
    sess.check_errors()
    # the engine keeps its refusal for callers that do not ask for per-clip ends, and asks for frames where they do
    stft = torch.from_numpy(pr.spectra("live_tiny", B)).to(DEV)
    eng = model.engine()
    with pytest.raises(ValueError, match="ragged"):
        eng.forward_stft(stft, frames=[60, 50, 40], _end_state=True)
    with pytest.raises(ValueError, match="ragged"):
        eng.forward_stft(stft, frames=[60, 50, 40], _end_state=eng._start_buffers(B, 58, 2))
    start = eng._start_buffers(B, 58, 2, per_clip_ends=True)
    with pytest.raises(ValueError, match="needs frames"):
        eng.forward_stft(start["stft"], _end_state=start)
    with pytest.raises(ValueError, match=r"frames\[1\] = 59"):
        eng.forward_stft(start["stft"], frames=[58, 59, 1], _end_state=start)  # (counted in NEW frames: 58 at most)
    # resident sessions refuse, cIRM-GSN sessions have no such method
    w = torch.from_numpy(pr.waves("live_tiny", B)).to(DEV)
    res = model.streaming(batch=1, waveform=True, host_io=True, resident=True)
    with pytest.raises(NotImplementedError, match="resident"):
        res.advance_wave_ragged(w[:1, :256], [256])
    with pytest.raises(NotImplementedError, match="resident"):
        res.advance_ragged(stft[:1, :, :4], [4])
    res.close()
    from spiking_fullsubnet_amd.modeling_cirm_gsn import Model
    cirm = Model(**hr.CIRM_TINY).eval().to(DEV).streaming()
    assert not hasattr(cirm, "advance_ragged") and not hasattr(cirm, "advance_wave_ragged")
    # a waveform clip without a call in its utterance, on a real session
    ws = model.streaming(batch=B, waveform=True)
    ws.step_wave(w[:, :128].contiguous())
    ws.reset(clips=[2])
    with pytest.raises(ValueError, match=r"clip 2\b.*prime_wave"):
        ws.advance_wave_ragged(w[:, 128:512], [128, 256, 384])
    assert ws.clip_calls.tolist() == [1, 1, 0]
