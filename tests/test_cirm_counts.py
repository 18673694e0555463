"""Spike counts of the cIRM-GSN model: streaming sessions opened with ``count_spikes=True`` (the counting one-launch hop
``sfsn_fullband_stream_hop_counted`` and the per-kernel sequence with its ``sfsn_spike_count_rows`` launch, from a graph or eager) and
the offline ``forward_stft(want_counts=True)``.

Every comparison is an exact integer.  The references are independent of the counting kernels: the reference implementation's own
spike tensors in ``golden/cirm_tiny*.npz`` (no membrane of theirs sits within 1e-4 of the threshold, so the kernels' spikes are the
reference's bit for bit) and, at the recipe's width, ``gt(x, 0).sum()`` of the offline forward's fp32 spike tensors."""
import functools
import os

import numpy as np
import pytest
import torch

import parity
from test_cirm_gsn import RECIPE
from test_cirm_streaming import GOLD, _fixture, _spectrum, model, offline

pytestmark = pytest.mark.gpu

# per layer [clip 0, clip 1] over the fixtures' 24 frames, out of 24 * 20 = 480 possible spikes each (counted from the fixtures on a CPU)
FIXTURE_COUNTS = {"cirm_tiny.npz": [[89, 92], [276, 272], [176, 177]], "cirm_tiny_2spk.npz": [[63, 64], [296, 180], [166, 189]]}
TIERS = {"one_launch": dict(one_launch=True), "graph": dict(one_launch=False, graph=True), "eager": dict(one_launch=False, graph=False)}
NL, H, T_FIX = 3, 20, 24


@functools.lru_cache(maxsize=None)
def gold_spikes(fname):
    """The reference's spikes of a fixture, bool [layer][T, B, H]; guarded against an emptied or near-threshold fixture."""
    g = np.load(os.path.join(GOLD, fname))
    spk = [parity.unpack(g[f"spikes_packed/{l}"], (T_FIX, 2, H)) for l in range(NL)]
    for l in range(NL):
        assert tuple(int(v) for v in g[f"spikes_shape/{l}"]) == (T_FIX, 2, H)
        assert not parity.unpack(g[f"near{parity.TAU:g}/{l}"], (T_FIX, 2, H)).any()
        per_clip = spk[l].sum((0, 2)).tolist()
        assert per_clip == FIXTURE_COUNTS[fname][l]
        assert all(0 < c < T_FIX * H for c in per_clip) and per_clip[0] != per_clip[1]  # neither silent nor saturated; clips differ
    return spk


def want(fname, b, frames):
    """Per layer, the reference's spike count of clip b over its first `frames` frames."""
    return [int(s[:frames, b].sum()) for s in gold_spikes(fname)]


def counts_of(summary):
    return [int(s.count) for s in summary[1:-1]]


def check_summary(summary, T, nb, P, hidden=H, F=257):
    from spiking_fullsubnet_amd.engine import SpikeSummary
    assert tuple(summary[0].shape) == (T, nb, F) and tuple(summary[-1].shape) == (T, nb, P)
    assert all(isinstance(s, SpikeSummary) and tuple(s.shape) == (T, nb, hidden) for s in summary[1:-1])


# ---- 1. against the reference's spikes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,T", [(1, 24), (3, 24), (5, 20)])
@pytest.mark.parametrize("tier", sorted(TIERS))
@pytest.mark.parametrize("fname", sorted(FIXTURE_COUNTS))
def test_fixtures(fname, tier, hop, T):
    m, stft = _fixture(fname)
    stft = stft[:, :, :T].contiguous()
    sess = m.streaming(batch=2, hop=hop, count_spikes=True, **TIERS[tier])
    assert sess.one_launch is (tier == "one_launch") and sess.count_spikes
    n = T // hop
    outs, mags, looked = [], [], 0
    for i in range(n):
        e, mg = sess.step(stft[:, :, i * hop:(i + 1) * hop].contiguous())
        outs.append(e)
        mags.append(mg)
        if i + 1 in (1, n // 2, n):  # two intermediate steps and the last one
            seen = (i + 1) * hop
            for b in range(2):
                s = sess.spike_summary([b])
                check_summary(s, seen, 1, m._fb_spec.P)
                assert counts_of(s) == want(fname, b, seen), (fname, tier, hop, b, seen)
            looked += 1
    assert looked == 3
    sess.check_errors()
    ref = offline(m, stft, (fname, T))
    assert torch.equal(torch.view_as_real(torch.cat(outs, -1)), torch.view_as_real(ref[0]))
    if m.num_spks == 1:
        assert torch.equal(torch.cat(mags, -1), ref[1])
    if tier == "one_launch":
        assert sess.launches == {"hop": n}
    else:
        assert sess.launches["spike_count"] == n and sess.launches["projdf"] == n and "hop" not in sess.launches
    whole = sess.spike_summary()
    check_summary(whole, T, 2, m._fb_spec.P)
    assert counts_of(whole) == [a + b for a, b in zip(want(fname, 0, T), want(fname, 1, T))]
    sess.reset()  # a whole reset zeroes the counts: the utterance again gives the same numbers, not twice them
    for i in range(n):
        sess.step(stft[:, :, i * hop:(i + 1) * hop].contiguous())
    assert [counts_of(sess.spike_summary([b])) for b in range(2)] == [want(fname, b, T) for b in range(2)]


# ---- 2. one clip restarts while the other goes on ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["one_launch", "graph"])
@pytest.mark.parametrize("fname", sorted(FIXTURE_COUNTS))
def test_restart(fname, tier):
    m, stft = _fixture(fname)
    sess = m.streaming(batch=2, hop=1, count_spikes=True, **TIERS[tier])
    for i in range(T_FIX):
        if i == 10:
            sess.reset(clips=[1])
        frame = torch.stack([stft[0, :, i:i + 1], stft[1, :, i - 10:i - 9] if i >= 10 else stft[1, :, i:i + 1]])
        sess.step(frame.contiguous())
    sess.check_errors()
    assert sess.clip_frames().tolist() == [24, 14]
    s0, s1 = sess.spike_summary([0]), sess.spike_summary([1])
    check_summary(s0, 24, 1, m._fb_spec.P)
    check_summary(s1, 14, 1, m._fb_spec.P)
    assert counts_of(s0) == want(fname, 0, 24)
    assert counts_of(s1) == want(fname, 1, 14)
    with pytest.raises(ValueError, match="different numbers of frames"):
        sess.spike_summary([0, 1])
    with pytest.raises(ValueError, match="different numbers of frames"):
        sess.spike_summary()
    with pytest.raises(IndexError):
        sess.spike_summary([2])
    with pytest.raises(TypeError):
        sess.spike_summary([0.5])
    with pytest.raises(ValueError, match="no clip"):
        sess.spike_summary([])


def test_a_session_that_does_not_count_says_so():
    m, _ = _fixture("cirm_tiny.npz")
    for kw in TIERS.values():
        sess = m.streaming(batch=2, hop=1, **kw)
        assert not sess.count_spikes
        with pytest.raises(RuntimeError, match="count_spikes=True"):
            sess.spike_summary()


def test_counting_waveform_session_is_refused():
    m, _ = _fixture("cirm_tiny.npz")
    with pytest.raises(NotImplementedError, match="count_spikes"):
        m.streaming(batch=1, waveform=True, count_spikes=True)


# ---- 3. the recipe's width: H = 268 padded to 272 (17 tiles, five 64-byte k slices) -----------------------------------------------------
_RECIPE_REF = {}


def recipe_ref(m, stft, key):
    """Per-clip counts [layers, B] from the offline forward's fp32 spike tensors (other kernels than either counting path), once."""
    if key not in _RECIPE_REF:
        res = m.engine().forward_stft(stft, want_layers=True)
        m.engine().check_stack_errors()
        spk = res["all_layers"][1:-1]
        assert all(tuple(s.shape) == (stft.shape[2], stft.shape[0], 268) for s in spk)
        _RECIPE_REF[key] = (torch.stack([torch.gt(s, 0).sum((0, 2)) for s in spk]).cpu(), spk[0].numel(), res["enh_stft"].clone())
    return _RECIPE_REF[key]


@pytest.mark.parametrize("tier", ["one_launch", "graph"])
@pytest.mark.parametrize("B,T", [(3, 12), (16, 6)])
def test_recipe_width(B, T, tier):
    m = model(**RECIPE)
    stft = _spectrum(B, 257, T, 11 + B)
    ref, numel, enh = recipe_ref(m, stft, (B, T))
    for l in range(RECIPE["num_layers"]):  # the comparison is not empty: no layer silent, none saturated
        assert 0 < int(ref[l].sum()) < numel, (l, ref[l].tolist(), numel)
    sess = m.streaming(batch=B, hop=1, count_spikes=True, **TIERS[tier])
    assert sess.one_launch is (tier == "one_launch")
    outs = [sess.step(stft[:, :, t:t + 1].contiguous())[0] for t in range(T)]
    sess.check_errors()
    assert torch.equal(torch.view_as_real(torch.cat(outs, -1)), torch.view_as_real(enh))
    got = torch.tensor([counts_of(sess.spike_summary([b])) for b in range(B)]).T
    assert torch.equal(got, ref), (got.tolist(), ref.tolist())
    whole = sess.spike_summary()
    check_summary(whole, T, B, m._fb_spec.P, hidden=268)  # the model's hidden size: the four pad neurons are not in the denominator
    assert counts_of(whole) == ref.sum(1).tolist()
    off = m.forward_stft(stft, want_counts=True)
    assert torch.equal(off["clip_counts"].cpu(), ref)


# ---- 4. offline ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", sorted(FIXTURE_COUNTS))
def test_offline_counts(fname):
    from spiking_fullsubnet_amd import metric
    m, stft = _fixture(fname)
    gold_spikes(fname)
    before = dict(m.engine().launches)
    res = m.forward_stft(stft, want_counts=True)
    m.engine().check_stack_errors()
    assert m.engine().launches.get("spike_count", 0) - before.get("spike_count", 0) == 1  # one launch for all layers
    assert res["clip_counts"].dtype == torch.int64 and res["clip_counts"].tolist() == FIXTURE_COUNTS[fname]
    lay = res["all_layers"]
    check_summary(lay, T_FIX, 2, m._fb_spec.P)
    assert lay[-1].device.type == "meta"  # the fp32 projection rows were never allocated
    assert counts_of(lay) == [sum(c) for c in FIXTURE_COUNTS[fname]]
    ref = offline(m, stft, (fname, T_FIX))
    assert torch.equal(torch.view_as_real(res["enh_stft"]), torch.view_as_real(ref[0]))
    # SynOPs: a session's whole-batch summary == the offline counts exactly, == the fp32 tensors' value to the metric test's bound
    sess = m.streaming(batch=2, hop=3, count_spikes=True, one_launch=True)
    for t in range(0, T_FIX, 3):
        sess.step(stft[:, :, t:t + 3].contiguous())
    sess.check_errors()
    summ = sess.spike_summary()
    ten = m.forward_stft(stft, want_layers=True)["all_layers"]
    syn = metric.compute_synops(lay, [], shared_weights=True)
    assert syn > 0
    assert metric.compute_synops(summ, [], shared_weights=True) == syn
    assert syn == pytest.approx(metric.compute_synops(ten, [], shared_weights=True), rel=1e-6)
    assert metric.compute_neuronops(summ, []) == metric.compute_neuronops(lay, []) == metric.compute_neuronops(ten, [])
    # both options together: the tensors, and the per-clip counts beside them
    both = m.forward_stft(stft, want_layers=True, want_counts=True)
    assert both["clip_counts"].tolist() == FIXTURE_COUNTS[fname] and torch.is_tensor(both["all_layers"][1])


def test_two_speaker_forward_honours_layer_outputs():
    from spiking_fullsubnet_amd import metric
    fname = "cirm_tiny_2spk.npz"
    m, _ = _fixture(fname)
    wave = torch.from_numpy(np.load(os.path.join(GOLD, fname))["wave"]).cuda()
    assert m.layer_outputs == "tensors"
    y_t, (ten,) = m(wave)
    try:
        m.layer_outputs = "counts"
        y_c, (cnt,) = m(wave)
        m.layer_outputs = "none"
        y_n, (non,) = m(wave)
        m.layer_outputs = "spikes"
        with pytest.raises(ValueError, match="layer_outputs"):
            m(wave)
    finally:
        del m.layer_outputs  # (back to the class default: the module is shared with other tests)
    assert m.layer_outputs == "tensors"
    assert torch.equal(y_c, y_t) and torch.equal(y_n, y_t)
    assert all(torch.is_tensor(t) and t.device.type == "cuda" for t in ten)
    check_summary(cnt, T_FIX, 2, m._fb_spec.P)
    assert counts_of(cnt) == [sum(c) for c in FIXTURE_COUNTS[fname]]
    assert counts_of(cnt) == [int(torch.gt(t, 0).sum()) for t in ten[1:-1]]
    assert len(non) == len(ten) and all(s is None for s in non[1:-1])
    assert tuple(non[0].shape) == tuple(ten[0].shape) and tuple(non[-1].shape) == tuple(ten[-1].shape)
    assert metric.compute_synops(cnt, [], shared_weights=True) == pytest.approx(metric.compute_synops(ten, [], shared_weights=True), rel=1e-6)
