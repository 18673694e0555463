"""cIRM-GSN frame by frame (``modeling_cirm_gsn.Model.streaming``): both tiers of ``FullbandStreamingSession`` -- the one-launch hop
``sfsn_fullband_stream_hop`` and the per-kernel sequence -- against the offline forward on the concatenated input.  Every comparison
is ``torch.equal`` with ``model.engine().forward_stft(stft)``: the integer digit sums are exact and every fp32 expression is the same
expression in the same order, so there is no tolerance."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from test_cirm_gsn import RECIPE, recipe_model

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
TINY = dict(RECIPE, hidden_size=20, num_layers=3)


def _spectrum(B, F, T, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(((rng.standard_normal((B, F, T)) + 1j * rng.standard_normal((B, F, T))) * 0.5).astype(np.complex64)).cuda()


@functools.lru_cache(maxsize=None)
def _fixture(fname):
    from spiking_fullsubnet_amd.modeling_cirm_gsn import Model
    gold = np.load(os.path.join(GOLD, fname))
    m = Model(**json.loads(str(gold["kwargs"])))
    m.load_state_dict({k[3:]: torch.from_numpy(np.asarray(gold[k])) for k in gold.files if k.startswith("sd/")}, strict=True)
    return m.eval().cuda(), torch.from_numpy(gold["stft"]).cuda()


@functools.lru_cache(maxsize=None)
def _model(items):
    return recipe_model(**dict(items))[0].cuda()


def model(**kw):
    return _model(tuple(sorted(kw.items())))


_REF = {}


def offline(m, stft, key):
    """The offline forward of a spectrum, computed once per key and left unchanged."""
    if key not in _REF:
        res = m.engine().forward_stft(stft)
        m.engine().check_stack_errors()
        _REF[key] = (res["enh_stft"].clone(), None if res["enh_mag"] is None else res["enh_mag"].clone())
    return _REF[key]


def stream(sess, stft, hop):
    outs, mags = [], []
    for t in range(0, stft.shape[2], hop):
        e, mg = sess.step(stft[:, :, t:t + hop].contiguous())
        outs.append(e)
        mags.append(mg)
    sess.check_errors()
    return torch.cat(outs, -1), (None if mags[0] is None else torch.cat(mags, -1))


def assert_equal(got, want, S):
    assert got[0].shape == want[0].shape
    assert torch.isfinite(torch.view_as_real(want[0])).all() and float(want[0].abs().max()) > 0  # (the comparison is not empty)
    assert torch.equal(torch.view_as_real(got[0]), torch.view_as_real(want[0]))
    if S == 1:
        assert torch.equal(got[1], want[1])
    else:
        assert got[1] is None


# ---- 1. the reference's fixtures ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,T", [(1, 24), (3, 24), (5, 20)])
@pytest.mark.parametrize("one_launch", [True, False])
@pytest.mark.parametrize("fname", ["cirm_tiny.npz", "cirm_tiny_2spk.npz"])
def test_fixtures(fname, one_launch, hop, T):
    m, stft = _fixture(fname)
    stft = stft[:, :, :T].contiguous()
    S = m.num_spks
    sess = m.streaming(batch=stft.shape[0], hop=hop, one_launch=one_launch)
    assert sess.one_launch is one_launch
    got = stream(sess, stft, hop)
    assert_equal(got, offline(m, stft, (fname, T)), S)
    if one_launch:
        assert sess.launches == {"hop": T // hop}
    else:
        assert sess.launches["features"] == T // hop and sess.launches["projdf"] == T // hop and "hop" not in sess.launches
    assert sess.clip_frames().tolist() == [T] * stft.shape[0]


# ---- 2. the recipe's geometry -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["one_launch", "graph", "eager"])
@pytest.mark.parametrize("B,T", [(3, 47), (16, 12)])
def test_recipe_geometry(B, T, mode):
    m = model(**RECIPE)
    stft = _spectrum(B, 257, T, 11 + B)
    sess = m.streaming(batch=B, hop=1, one_launch=mode == "one_launch", graph=mode != "eager")
    assert sess.one_launch is (mode == "one_launch")
    assert_equal(stream(sess, stft, 1), offline(m, stft, ("recipe", B, T)), 1)


# ---- 3. variants at H = 20, F = 257 (and two other widths) -------------------------------------------------------------------------------------------------
VARIANTS = {
    "no_bn": dict(bn=False), "no_ln": dict(use_pre_layer_norm_fb=False), "tanh": dict(output_activate_function="tanh"),
    "sigmoid": dict(output_activate_function="sigmoid"), "relu": dict(output_activate_function="relu"), "one_layer": dict(num_layers=1),
    "df1": dict(df_order=1), "df5_2spk": dict(df_order=5, num_spks=2), "h48_4layers": dict(hidden_size=48, num_layers=4),
    # other widths inside the hop kernel's coverage: F = 201 (four feature slots per lane offline, a 9-bin last block) and the largest
    # geometry it takes (F = 320, Hp = 320, 4 layers, df 5, two speakers: 62 workgroups)
    "f201": dict(n_fft=400, hop_length=100, win_length=400, input_size=201, proj_size=201),
    "largest": dict(n_fft=638, hop_length=160, win_length=638, input_size=320, proj_size=320, hidden_size=320, num_layers=4, df_order=5,
                    num_spks=2),
}


@pytest.mark.parametrize("one_launch", [True, False])
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_variants(name, one_launch):
    kw = dict(TINY, **VARIANTS[name])
    m = model(**kw)
    stft = _spectrum(2, kw["n_fft"] // 2 + 1, 14, 23)
    sess = m.streaming(batch=2, hop=2, one_launch=one_launch)
    assert sess.one_launch is one_launch
    assert_equal(stream(sess, stft, 2), offline(m, stft, ("variant", name)), kw["num_spks"])


@pytest.mark.parametrize("name,over", [("unshared", dict(shared_weights=False)),
                                       ("f129", dict(n_fft=256, hop_length=64, win_length=256, input_size=129, proj_size=129))])
def test_outside_the_hop_kernel(name, over):
    """Separate gate weights and F <= 192: equal whichever tier serves them; one_launch=True works or refuses, never mis-runs."""
    kw = dict(TINY, **over)
    m = model(**kw)
    F = kw["n_fft"] // 2 + 1
    stft = _spectrum(2, F, 12, 29)
    want = offline(m, stft, ("outside", name))
    sess = m.streaming(batch=2, hop=1, one_launch="auto")
    assert_equal(stream(sess, stft, 1), want, 1)
    try:
        sess = m.streaming(batch=2, hop=1, one_launch=True)
    except NotImplementedError:
        return
    assert sess.one_launch is True
    assert_equal(stream(sess, stft, 1), want, 1)


# ---- 4. per-clip restart ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_launch", [True, False])
def test_per_clip_restart(one_launch):
    m = model(**TINY)
    stft = _spectrum(3, 257, 20, 31)
    whole = offline(m, stft, ("restart", "whole"))
    tail = offline(m, stft[:, :, 10:].contiguous(), ("restart", "tail"))
    sess = m.streaming(batch=3, hop=1, one_launch=one_launch)

    def run():
        a = stream(sess, stft[:, :, :10].contiguous(), 1)
        sess.reset(clips=[1])
        assert sess.clip_frames().tolist() == [10, 0, 10]
        b = stream(sess, stft[:, :, 10:].contiguous(), 1)
        return a, b

    a, b = run()
    assert sess.clip_frames().tolist() == [20, 10, 20]
    for c in (0, 2):
        assert torch.equal(torch.view_as_real(torch.cat([a[0], b[0]], -1)[c]), torch.view_as_real(whole[0][c]))
        assert torch.equal(torch.cat([a[1], b[1]], -1)[c], whole[1][c])
    assert torch.equal(torch.view_as_real(a[0][1]), torch.view_as_real(whole[0][1, :, :, :10]))
    assert torch.equal(torch.view_as_real(b[0][1]), torch.view_as_real(tail[0][1]))
    assert torch.equal(b[1][1], tail[1][1])
    sess.reset()
    assert sess.clip_frames().tolist() == [0, 0, 0]
    a2, b2 = run()
    for x, y in ((a, a2), (b, b2)):
        assert torch.equal(torch.view_as_real(x[0]), torch.view_as_real(y[0])) and torch.equal(x[1], y[1])


# ---- 5. more clips than the hop kernel takes ----------------------------------------------------------------------------------------
def test_seventeen_clips():
    m = model(**TINY)
    stft = _spectrum(17, 257, 6, 37)
    sess = m.streaming(batch=17, hop=1, one_launch="auto")
    assert sess.one_launch is False
    assert_equal(stream(sess, stft, 1), offline(m, stft, ("b17",)), 1)
    with pytest.raises(NotImplementedError, match="B=17"):
        m.streaming(batch=17, hop=1, one_launch=True)


def test_auto_takes_the_hop_kernel_where_it_is_the_default():
    from spiking_fullsubnet_amd import fullband_streaming
    sess = model(**TINY).streaming(batch=1, hop=1)
    assert sess.one_launch is fullband_streaming.AUTO_ONE_LAUNCH
