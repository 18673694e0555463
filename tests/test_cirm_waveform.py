"""cIRM-GSN streaming on samples (``modeling_cirm_gsn.Model.streaming(waveform=True)``): 128 samples per clip in, 128 enhanced samples
per clip and speaker out, one ``sfsn_fullband_stream_hop_wave`` launch per call.  Every comparison with the offline forward is
``torch.equal`` against ``model(wave)`` of the same module on the same samples: the model path is bit-identical already
(tests/test_cirm_streaming.py) and the in-launch transforms are the offline transforms' code, so there is no tolerance.  Call c
returns the samples that entered with call c - 3; with n calls the comparison covers the first 128 (n - 3) output samples (the last
three hops of the offline clip depend on frames a stream of n calls does not have yet)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import refweights as rw
from test_cirm_gsn import RECIPE, recipe_model

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
TINY = dict(RECIPE, hidden_size=20, num_layers=3)
HOP = 128


@functools.lru_cache(maxsize=None)
def _fixture(fname):
    from spiking_fullsubnet_amd.modeling_cirm_gsn import Model
    gold = np.load(os.path.join(GOLD, fname))
    m = Model(**json.loads(str(gold["kwargs"])))
    m.load_state_dict({k[3:]: torch.from_numpy(np.asarray(gold[k])) for k in gold.files if k.startswith("sd/")}, strict=True)
    return m.eval().cuda(), torch.from_numpy(gold["wave"]).cuda(), torch.from_numpy(gold["enh_y"]).cuda()


@functools.lru_cache(maxsize=None)
def _model(items):
    return recipe_model(**dict(items))[0].cuda()


def model(**kw):
    m = _model(tuple(sorted(kw.items())))
    assert m.spectral_backend == "device"  # the offline side runs the device transforms
    return m


def noise(B, calls, seed):
    """Seeded noise of `calls` hops per clip (0.05 * randn: well below an amplitude of 0.5)."""
    x = rw.synth_wave(B, calls + 1, seed=seed)
    assert x.shape == (B, calls * HOP) and float(np.abs(x).max()) <= 0.5
    return torch.from_numpy(x).cuda()


_REF = {}


def offline(m, wave, key):
    """``model(wave)`` as [B, S, samples], computed once per key and left unchanged."""
    if key not in _REF:
        y = m(wave)[0]
        m.engine().check_stack_errors()
        _REF[key] = y.reshape(wave.shape[0], m.num_spks, -1).clone()
    return _REF[key]


def stream(sess, wave, host=False):
    """The session's outputs for the calls that `wave` [B, 128 n] makes, concatenated: [B, S, 128 n]."""
    outs = []
    for c in range(wave.shape[1] // HOP):
        x = wave[:, c * HOP:(c + 1) * HOP].contiguous()
        outs.append(sess.step_wave_host(x).clone() if host else sess.step_wave(x))
    return torch.cat(outs, -1)


def assert_same(got, want):
    """got == want bit for bit, and the comparison is not empty."""
    assert got.shape == want.shape and want.numel() > 0
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert torch.equal(got, want)


def assert_delayed(got, ref):
    """A stream of n calls against the offline forward of its samples: three zero hops, then the first 128 (n - 3) samples."""
    n = got.shape[-1]
    assert not got[..., :3 * HOP].any()
    assert_same(got[..., 3 * HOP:], ref[..., :n - 3 * HOP])


# ---- 1. the reference's fixtures ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", ["cirm_tiny.npz", "cirm_tiny_2spk.npz"])
def test_fixtures(fname):
    m, wave, enh_y = _fixture(fname)
    assert m.spectral_backend == "device"
    B, S = wave.shape[0], m.num_spks
    assert wave.shape == (2, 23 * HOP)
    ref = offline(m, wave, fname)
    sess = m.streaming(batch=B, waveform=True)
    assert sess.one_launch is True and sess.waveform
    got = stream(sess, wave)
    assert got.shape == (B, S, 23 * HOP)
    assert_delayed(got, ref)
    gold = enh_y.reshape(B, S, -1)[..., :2560]
    assert torch.isfinite(gold).all() and float(gold.abs().max()) > 0
    torch.testing.assert_close(got[..., 3 * HOP:], gold, rtol=2e-4, atol=1e-4)  # tests/test_cirm_gsn.py's bound for enh_y
    assert sess.launches == {"hop": 23}
    sess.reset()
    assert torch.equal(stream(sess, wave), got)
    sess.check_errors()


# ---- 2. batch shapes that change the work split -------------------------------------------------------------------------------------
SHAPES = {
    "b1": (TINY, 1, 24),
    "b9": (TINY, 9, 24),  # a wave of the STFT workgroup serves two clips
    "b16_2spk_df5": (dict(TINY, num_spks=2, df_order=5), 16, 24),  # 32 (clip, speaker) pairs: four inverse-STFT workgroups, deepest history
    "recipe_b1": (RECIPE, 1, 30),
    "recipe_b3": (RECIPE, 3, 30),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_batch_shapes(name):
    kw, B, calls = SHAPES[name]
    m = model(**kw)
    wave = noise(B, calls, 41 + B)
    sess = m.streaming(batch=B, waveform=True)
    got = stream(sess, wave)
    assert got.shape == (B, kw["num_spks"], calls * HOP)
    assert_delayed(got, offline(m, wave, ("shape", name)))
    assert sess.launches == {"hop": calls}
    sess.check_errors()


# ---- 3. more launches than the tag's period (127) -----------------------------------------------------------------------------------
def test_tag_period():
    m = model(**TINY)
    calls, cut = 140, 60
    wave = noise(2, calls, 53)
    whole = offline(m, wave, ("period", "whole"))
    head = offline(m, wave[:, :cut * HOP].contiguous(), ("period", "head"))
    tail = offline(m, wave[:, cut * HOP:].contiguous(), ("period", "tail"))
    sess = m.streaming(batch=2, waveform=True)
    a = stream(sess, wave[:, :cut * HOP])
    sess.reset(clips=[0])
    b = stream(sess, wave[:, cut * HOP:])
    got = torch.cat([a, b], -1)
    assert_delayed(got[1:2], whole[1:2])  # clip 1 never noticed
    assert_delayed(a[0:1], head[0:1])  # clip 0 up to its call 59: the offline forward of its first 60 calls' samples
    assert_delayed(b[0:1], tail[0:1])  # three zero hops, then the offline forward of its samples from call 60 on
    assert sess.launches == {"hop": calls}
    sess.check_errors()


# ---- 4. per-clip restart and whole reset (tests/test_cirm_streaming.py::test_per_clip_restart, on samples) ---------------------------
def test_per_clip_restart():
    m = model(**TINY)
    calls, cut = 30, 12
    wave = noise(3, calls, 59)
    whole = offline(m, wave, ("restart", "whole"))
    tail = offline(m, wave[:, cut * HOP:].contiguous(), ("restart", "tail"))
    sess = m.streaming(batch=3, waveform=True)
    assert sess.clip_frames().tolist() == [0, 0, 0]

    def run():
        a = stream(sess, wave[:, :cut * HOP])
        assert sess.clip_frames().tolist() == [cut - 1] * 3  # a clip's first call has no frame yet
        sess.reset(clips=[1])
        assert sess.clip_frames().tolist() == [cut - 1, 0, cut - 1]
        b = stream(sess, wave[:, cut * HOP:])
        return a, b

    a, b = run()
    assert sess.clip_frames().tolist() == [calls - 1, calls - cut - 1, calls - 1]
    for c in (0, 2):
        assert_delayed(torch.cat([a, b], -1)[c:c + 1], whole[c:c + 1])
    assert_delayed(a[1:2], whole[1:2, :, :cut * HOP])
    assert_delayed(b[1:2], tail[1:2])
    sess.reset()
    assert sess.clip_frames().tolist() == [0, 0, 0]
    a2, b2 = run()
    assert torch.equal(a, a2) and torch.equal(b, b2)
    sess.check_errors()


# ---- 5. samples on the host ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S", [(1, 1), (3, 2)])
def test_host_io(B, S):
    kw = dict(TINY, num_spks=S)
    m = model(**kw)
    calls = 30
    wave = noise(B, calls, 61 + B)
    ref = offline(m, wave, ("host", B, S))
    dev_sess = m.streaming(batch=B, waveform=True)
    want = stream(dev_sess, wave)
    dev_sess.check_errors()
    sess = m.streaming(batch=B, waveform=True, host_io=True)
    first = sess.step_wave_host(wave[:, :HOP].cpu())
    assert first.device.type == "cpu" and first.shape == (B, S, HOP)
    sess.reset()
    got = stream(sess, wave.cpu(), host=True)
    assert got.device.type == "cpu" and got.dtype == torch.float32
    assert_same(got, want.cpu())
    assert_delayed(got, ref.cpu())
    assert sess.launches == {"hop": calls + 1}
    sess.check_errors()


# ---- 6. refusals on a HIP module -----------------------------------------------------------------------------------------------------
def test_refusals():
    m = model(**TINY)
    with pytest.raises(ValueError, match="host_io goes with waveform=True"):
        m.streaming(host_io=True)
    with pytest.raises(NotImplementedError, match="hop=2"):
        m.streaming(waveform=True, hop=2)
    with pytest.raises(NotImplementedError, match="B=17"):
        m.streaming(waveform=True, batch=17)
    with pytest.raises(ValueError, match="one-launch"):
        m.streaming(waveform=True, one_launch=False)
    with pytest.raises(NotImplementedError, match="shared_weights=False"):
        model(**dict(TINY, shared_weights=False)).streaming(waveform=True)
    for opt in ("resident", "count_spikes"):
        with pytest.raises(NotImplementedError, match=opt):
            m.streaming(waveform=True, **{opt: True})
    wsess = m.streaming(batch=1, waveform=True)
    with pytest.raises(RuntimeError, match="step_wave"):
        wsess.step(torch.zeros((1, 257, 1), dtype=torch.complex64, device="cuda"))
    ssess = m.streaming(batch=1)
    with pytest.raises(RuntimeError, match="waveform=True"):
        ssess.step_wave(torch.zeros((1, HOP), device="cuda"))
    with pytest.raises(RuntimeError, match="host_io=True"):
        wsess.step_wave_host(torch.zeros((1, HOP)))
    wsess.check_errors()
    ssess.check_errors()
