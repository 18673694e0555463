"""cIRM-GSN on the gfx950 kernels (spiking_fullsubnet_amd.modeling_cirm_gsn.Model): the two new entry points against sfsn_spike_proj
and the CPU oracle, the whole module against an oracle composition at the recipe's geometry and against the reference's own outputs
(tests/golden/cirm_tiny*.npz, made by tests/golden/make_golden_cirm.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import parity
from oracle import Oracle

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
RECIPE = dict(n_fft=512, hop_length=128, win_length=512, fdrc=0.5, input_size=257, hidden_size=268, num_layers=4, proj_size=257,
              output_activate_function=False, df_order=3, use_pre_layer_norm_fb=True, bn=True, shared_weights=True, sequence_model="GSN",
              num_spks=1)


def _lib():
    from spiking_fullsubnet_amd import _lib as L
    return L


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def recipe_model(seed=7, **over):
    """The recipe's model (H = 268, 4 layers, P = 1542, BatchNorm, shared gates) under a seed, with BatchNorm statistics and
    LayerNorm affine parameters moved away from their identity initial values."""
    from spiking_fullsubnet_amd.modeling_cirm_gsn import Model
    kw = dict(RECIPE, **over)
    torch.manual_seed(seed)
    m = Model(**kw)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.weight.copy_(1.0 + 0.3 * torch.rand(mod.num_features, generator=g))
                mod.bias.copy_(0.2 * torch.randn(mod.num_features, generator=g))
                mod.running_mean.copy_(0.1 * torch.randn(mod.num_features, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(mod.num_features, generator=g))
            if isinstance(mod, torch.nn.LayerNorm):
                mod.weight.copy_(1.0 + 0.2 * torch.randn(mod.normalized_shape, generator=g))
                mod.bias.copy_(0.1 * torch.randn(mod.normalized_shape, generator=g))
    return m.eval(), kw


def random_spectrum(B, F, T, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((B, F, T)) + 1j * rng.standard_normal((B, F, T))) * 0.5).astype(np.complex64)


# ---- the fused epilogue ------------------------------------------------------------------------------------------------------
def _epilogue_case(F, S, df, H=272, B=2, T=40, act=0, seed=0):
    from spiking_fullsubnet_amd.engine import pack_w3
    from spiking_fullsubnet_amd.fullband_engine import permute_proj
    rng = np.random.default_rng(seed)
    P, HP8 = 2 * df * S * F, (H + 63) // 64 * 64
    s8 = np.zeros((T, B, HP8), np.int8)
    s8[:, :, :H] = rng.random((T, B, H)) < 0.3
    w = (rng.standard_normal((P, H)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(P) * 0.1).astype(np.float32)
    wp, bp = permute_proj(w, b, F, df, S, H)
    pk, dq = pack_w3(wp)
    stft = random_spectrum(B, F, T, seed + 1)
    dev = "cuda"
    t = dict(s8=torch.from_numpy(s8).to(dev), pk=torch.from_numpy(pk).to(dev), dq=torch.from_numpy(dq).to(dev),
             bp=torch.from_numpy(bp).to(dev), ri=torch.view_as_real(torch.from_numpy(stft).to(dev)).contiguous())
    return dict(F=F, S=S, df=df, H=H, B=B, T=T, P=P, act=act, w=w, b=b, s8=s8, stft=stft, t=t)


def _run_epilogue(c, t0=0, nt=None, want_proj=True, want_mag=True):
    L = _lib()
    B, S, F, T, P = c["B"], c["S"], c["F"], c["T"], c["P"]
    nt = T - t0 if nt is None else nt
    t = c["t"]
    enh = torch.full((B, S, F, T, 2), float("nan"), device="cuda")
    mag = torch.full((B, S, F, T), float("nan"), device="cuda") if want_mag else None
    proj = torch.full((T, B, P), float("nan"), device="cuda") if want_proj else None
    rc = L.lib().sfsn_fullband_proj_deepfilter(_p(t["ri"]), _p(t["s8"]), c["H"], _p(t["pk"]), _p(t["dq"]), _p(t["bp"]), c["act"], B, F, T, S,
                                               c["df"], _p(proj), _p(enh), _p(mag), t0, nt, None)
    assert rc == 0, L.lib().sfsn_strerror(rc)
    torch.cuda.synchronize()
    return (enh.cpu().numpy(), None if mag is None else mag.cpu().numpy(), None if proj is None else proj.cpu().numpy())


def _spike_proj_rows(c):
    """The coefficient rows as sfsn_spike_proj computes them, 256 output columns per call (each row is its own exact sum)."""
    from spiking_fullsubnet_amd.engine import pack_w3
    L = _lib()
    T, B, P, H = c["T"], c["B"], c["P"], c["H"]
    out = np.empty((T, B, P), np.float32)
    s8 = c["t"]["s8"]
    for n0 in range(0, P, 256):
        n1 = min(P, n0 + 256)
        pk, dq = pack_w3(c["w"][n0:n1])
        pk, dq = torch.from_numpy(pk).cuda(), torch.from_numpy(dq).cuda()
        bias = torch.from_numpy(np.ascontiguousarray(c["b"][n0:n1])).cuda()
        y = torch.empty((T * B, n1 - n0), device="cuda")
        rc = L.lib().sfsn_spike_proj(_p(s8), _p(pk), _p(dq), _p(bias), _p(y), T * B, H, n1 - n0, n1 - n0, None)
        assert rc == 0, L.lib().sfsn_strerror(rc)
        out[:, :, n0:n1] = y.cpu().numpy().reshape(T, B, n1 - n0)
    return out


def _oracle_filter(c, proj):
    """Oracle("f32").deepfilter_group + finish_spectrum fed `proj` permuted into its (c, f, d, s) layout, N = 1, fc = F."""
    o = Oracle("f32")
    T, B, F, S, df = c["T"], c["B"], c["F"], c["S"], c["df"]
    perm = proj.reshape(T, B, 2, df, S, F).transpose(0, 1, 2, 5, 3, 4).reshape(T, B, 2 * F * df * S)
    enh = np.zeros((B, S, F, T), np.complex64)
    o.deepfilter_group(c["stft"], perm, enh, 0, 1, F, df, S)
    mag = o.finish_spectrum(c["stft"], enh, F)
    return enh, mag


@pytest.mark.parametrize("F,S,df", [(257, 1, 3), (257, 2, 5), (129, 1, 1), (129, 2, 3), (257, 1, 5)])
def test_epilogue_rows_and_filter_bit_exact(F, S, df):
    c = _epilogue_case(F, S, df, seed=F + 10 * S + df)
    enh, mag, proj = _run_epilogue(c)
    ref_rows = _spike_proj_rows(c)
    assert np.array_equal(proj, ref_rows), f"coefficient rows differ from sfsn_spike_proj in {int((proj != ref_rows).sum())} places"
    enh_ref, mag_ref = _oracle_filter(c, proj)
    enh_c = enh[..., 0] + 1j * enh[..., 1]
    assert np.array_equal(enh[..., 0], enh_ref.real) and np.array_equal(enh[..., 1], enh_ref.imag), \
        f"enh differs from the oracle: max {np.abs(enh_c - enh_ref).max():.3g}"
    assert np.array_equal(mag, mag_ref), f"enh_mag differs from the oracle's hypotf: max {np.abs(mag - mag_ref).max():.3g}"


def test_epilogue_window_and_nullable_outputs():
    c = _epilogue_case(257, 2, 3, B=3, T=45, seed=5)
    enh_full, _, proj_full = _run_epilogue(c)
    enh, mag, proj = _run_epilogue(c, t0=7, nt=21)
    inside, outside = slice(7, 28), np.r_[0:7, 28:45]
    assert np.array_equal(enh[:, :, :, inside], enh_full[:, :, :, inside])
    assert np.isnan(enh[:, :, :, outside]).all() and np.isnan(mag[:, :, :, outside]).all()
    assert np.array_equal(proj[inside], proj_full[inside]) and np.isnan(proj[outside]).all()
    enh2, mag2, proj2 = _run_epilogue(c, want_proj=False, want_mag=False)
    assert proj2 is None and mag2 is None and np.array_equal(enh2, enh_full)


@pytest.mark.parametrize("act,fn", [(1, torch.tanh), (2, torch.sigmoid), (3, torch.relu)])
def test_epilogue_activations(act, fn):
    """df = 1 and X = 1 + 0i: the filtered value is the activated coefficient itself."""
    c = _epilogue_case(129, 1, 1, act=act, seed=3)
    c["stft"] = np.ones_like(c["stft"])
    c["t"]["ri"] = torch.view_as_real(torch.from_numpy(c["stft"]).cuda()).contiguous()
    enh, _, proj = _run_epilogue(c)
    T, B, F = c["T"], c["B"], c["F"]
    want = fn(torch.from_numpy(proj)).numpy().reshape(T, B, 2, F).transpose(1, 2, 3, 0)  # [B, c, F, T]
    got = np.stack([enh[:, 0, :, :, 0], enh[:, 0, :, :, 1]], 1)
    ulp = np.spacing(np.abs(want).astype(np.float32))
    assert (np.abs(got - want) <= 4 * ulp).all(), f"activation {act}: max {np.abs(got - want).max():.3g}"


def test_new_entry_points_check_arguments():
    L = _lib()
    lib = L.lib()
    c = _epilogue_case(257, 1, 3, B=1, T=16)
    t = c["t"]
    enh = torch.empty((1, 1, 257, 16, 2), device="cuda")
    x = torch.empty((16, 1, 257), device="cuda")
    args = lambda **k: [k.get("ri", _p(t["ri"])), _p(t["s8"]), k.get("H", 272), _p(t["pk"]), _p(t["dq"]), None, k.get("act", 0), 1, 257, 16,
                        1, k.get("df", 3), None, k.get("enh", _p(enh)), None, k.get("t0", 0), k.get("nt", 16), None]
    assert lib.sfsn_fullband_proj_deepfilter(*args(ri=None)) == L.SFSN_EINVAL
    assert lib.sfsn_fullband_proj_deepfilter(*args(enh=None)) == L.SFSN_EINVAL
    assert lib.sfsn_fullband_proj_deepfilter(*args(act=4)) == L.SFSN_EINVAL
    assert lib.sfsn_fullband_proj_deepfilter(*args(t0=4, nt=13)) == L.SFSN_EINVAL
    assert lib.sfsn_fullband_proj_deepfilter(*args(H=400)) == L.SFSN_EUNSUPPORTED
    assert lib.sfsn_fullband_proj_deepfilter(*args(df=17)) == L.SFSN_EUNSUPPORTED
    assert lib.sfsn_fullband_features(_p(t["ri"]), 1, 257, 16, 0.5, None, None, 1e-5, None, 0, 16, None) == L.SFSN_EINVAL
    assert lib.sfsn_fullband_features(_p(t["ri"]), 1, 257, 16, 0.5, _p(x), None, 1e-5, _p(x), 0, 16, None) == L.SFSN_EINVAL
    assert lib.sfsn_fullband_features(_p(t["ri"]), 1, 257, 16, 0.5, None, None, 1e-5, _p(x), 10, 7, None) == L.SFSN_EINVAL
    assert lib.sfsn_fullband_features(_p(t["ri"]), 1, 400, 16, 0.5, None, None, 1e-5, _p(x), 0, 16, None) == L.SFSN_EUNSUPPORTED
    torch.cuda.synchronize()


# ---- the feature kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,ln", [(257, True), (257, False), (129, True)])
def test_features_against_oracle(F, ln):
    L = _lib()
    B, T = 3, 70
    stft = random_spectrum(B, F, T, F)
    rng = np.random.default_rng(1)
    w = (1 + 0.2 * rng.standard_normal(F)).astype(np.float32)
    b = (0.1 * rng.standard_normal(F)).astype(np.float32)
    ri = torch.view_as_real(torch.from_numpy(stft).cuda()).contiguous()
    wt, bt = torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()
    x = torch.full((T, B, F), float("nan"), device="cuda")
    rc = L.lib().sfsn_fullband_features(_p(ri), B, F, T, 0.5, _p(wt) if ln else None, _p(bt) if ln else None, 1e-5, _p(x), 0, T, None)
    assert rc == 0
    torch.cuda.synchronize()
    o = Oracle("f32")
    mag = o.front_mag(np.concatenate([stft, np.zeros((B, 1, T), np.complex64)], 1), 0.5)  # [B, F, T]: the padded bin is dropped
    ref = np.ascontiguousarray(mag.transpose(2, 0, 1))
    if ln:
        ref = o.layer_norm(ref, w, b)
    parity.check_continuous(x.cpu().numpy(), ref, np.full(B, T), f"features F={F} ln={ln}")


# ---- the module ----------------------------------------------------------------------------------------------------------------
def test_recipe_geometry_against_oracle_composition():
    m, kw = recipe_model()
    m = m.cuda()
    B, T, F = 3, 48, 257
    stft = random_spectrum(B, F, T, 11)
    res = m.engine().forward_stft(torch.from_numpy(stft).cuda(), want_layers=True)
    torch.cuda.synchronize()
    eng = m.engine()
    assert eng.launches.get("stack", 0) == 1 and eng.launches.get("projdf", 0) == 1 and eng.launches.get("features", 0) == 1
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    o = Oracle("f32")
    mag = o.front_mag(np.concatenate([stft, np.zeros((B, 1, T), np.complex64)], 1), kw["fdrc"])
    x = o.layer_norm(np.ascontiguousarray(mag.transpose(2, 0, 1)), sd["fb_model.pre_layer_norm.weight"], sd["fb_model.pre_layer_norm.bias"])
    outs = [r.cpu().numpy() for r in res["all_layers"]]
    parity.check_continuous(outs[0], x, np.full(B, T), "cirm/x")
    stats, t_valid, h = [], np.full(B, T), x
    for l in range(kw["num_layers"]):
        p = f"fb_model.sequence_model.layers.{l}.cell."
        bn = tuple(sd[p + "batchnorm." + n] for n in ("weight", "bias", "running_mean", "running_var"))
        spk, mem, _, _ = o.gsn_layer(h, sd[p + "weight_ih"], sd[p + "weight_hh"], sd[p + "bias_ih"], bn=bn, shared=True)
        t_valid, st = parity.check_chain(outs[1 + l], spk, np.abs(mem) < parity.TAU, t_valid, f"cirm/L{l}")
        stats.append(st)
        h = spk
    proj = o.linear(h, sd["fb_model.proj.weight"], sd["fb_model.proj.bias"])
    parity.check_continuous(outs[-1], proj, t_valid, "cirm/proj")
    c = dict(T=T, B=B, F=F, S=1, df=kw["df_order"], stft=stft)
    enh_ref, mag_ref = _oracle_filter(c, proj)
    enh = res["enh_stft"].cpu().numpy()
    mag = res["enh_mag"].cpu().numpy()
    tb = lambda a: np.ascontiguousarray(a[:, 0].transpose(2, 0, 1))  # [B, S, F, T] -> [T, B, F]: rows = clips
    parity.check_continuous(tb(enh.real), tb(enh_ref.real), t_valid, "cirm/enh.re")
    parity.check_continuous(tb(enh.imag), tb(enh_ref.imag), t_valid, "cirm/enh.im")
    parity.check_continuous(tb(mag), tb(mag_ref), t_valid, "cirm/enh_mag")
    parity.report("cirm_gsn_recipe_B3_T48", stats)
    assert min(s["spike_agreement"] for s in stats) >= 0.999


def _golden_model(gold):
    import json
    from spiking_fullsubnet_amd.modeling_cirm_gsn import Model
    kw = json.loads(str(gold["kwargs"]))
    m = Model(**kw)
    m.load_state_dict({k[3:]: torch.from_numpy(np.asarray(gold[k])) for k in gold.files if k.startswith("sd/")}, strict=True)
    return m.eval().cuda(), kw


@pytest.mark.parametrize("fname", ["cirm_tiny.npz", "cirm_tiny_2spk.npz"])
def test_module_against_reference_fixture(fname):
    gold = np.load(os.path.join(GOLD, fname))
    m, kw = _golden_model(gold)
    S = kw["num_spks"]
    stft = torch.from_numpy(gold["stft"]).cuda()
    res = m.engine().forward_stft(stft, want_layers=True)
    outs = [r.cpu().numpy() for r in res["all_layers"]]
    B, T = gold["stft"].shape[0], gold["stft"].shape[2]
    parity.check_continuous(outs[0], gold["x"], np.full(B, T), f"{fname}/x")
    t_valid, stats = np.full(B, T), []
    for l in range(kw["num_layers"]):
        shape = tuple(int(v) for v in gold[f"spikes_shape/{l}"])
        ref, near = parity.unpack(gold[f"spikes_packed/{l}"], shape), parity.unpack(gold[f"near{parity.TAU:g}/{l}"], shape)
        t_valid, st = parity.check_chain(outs[1 + l], ref, near, t_valid, f"{fname}/L{l}")
        stats.append(st)
    enh, enh_ref = res["enh_stft"].cpu().numpy(), gold["enh_stft"]
    for b in range(B):
        tv = int(t_valid[b])
        err = np.abs(enh[b, :, :, :tv] - enh_ref[b, :, :, :tv])
        assert (err <= parity.ATOL + parity.REL * np.abs(enh_ref[b, :, :, :tv])).all(), f"{fname}: enh clip {b}: {err.max():.3g}"
    parity.report(f"cirm_{fname}", stats)
    wave = torch.from_numpy(gold["wave"]).cuda()
    out = m(wave)
    assert isinstance(out, tuple) and len(out) == 2
    if S == 1:
        enh_y, enh_mag = out
        assert enh_y.shape == gold["enh_y"].shape and enh_mag.shape == gold["enh_mag"].shape
        np.testing.assert_allclose(enh_mag.cpu().numpy(), gold["enh_mag"], rtol=2e-4, atol=1e-4)  # includes the device STFT
    else:
        enh_y, rest = out
        assert enh_y.shape == gold["enh_y"].shape and isinstance(rest, list) and len(rest) == 1
        layers = rest[0]
        assert isinstance(layers, list) and len(layers) == kw["num_layers"] + 2
        assert tuple(layers[0].shape) == (T, B, 257) and all(tuple(s.shape) == (T, B, kw["hidden_size"]) for s in layers[1:-1])
        assert tuple(layers[-1].shape) == (T, B, 2 * kw["df_order"] * S * 257)
    np.testing.assert_allclose(enh_y.cpu().numpy(), gold["enh_y"], rtol=2e-4, atol=1e-4)


def test_full_size_deterministic():
    m, _ = recipe_model(seed=3)
    m = m.cuda()
    B, T = 64, 1000
    wave = torch.from_numpy(np.random.default_rng(2).standard_normal((B, (T - 1) * 128)).astype(np.float32) * 0.1).cuda()
    y1, mag1 = m(wave)
    y2, mag2 = m(wave)
    m.engine().check_stack_errors()
    assert torch.isfinite(y1).all() and torch.isfinite(mag1).all()
    assert torch.equal(y1, y2) and torch.equal(mag1, mag2)
    eng = m.engine()
    assert eng.launches["stack"] == 2 and eng.launches["projdf"] == 2 and eng.launches["features"] == 2
    assert eng.launches.get("layer_scan", 0) == 0


def test_lstm_eval_runs():
    from spiking_fullsubnet_amd.modeling_cirm_gsn import Model, deep_filter_torch
    torch.manual_seed(0)
    m = Model(512, 128, 512, 0.5, 257, 32, 2, 257, "tanh", 3, sequence_model="LSTM", num_spks=1).eval().cuda()
    wave = torch.randn(2, 127 * 128, device="cuda") * 0.1
    y, mag = m(wave)
    assert y.shape == wave.shape and mag.shape == (2, 257, 128) and torch.isfinite(y).all()
    m2 = Model(512, 128, 512, 0.5, 257, 32, 2, 257, None, 2, sequence_model="LSTM", num_spks=2).eval().cuda()
    y2, rest = m2(wave)
    assert y2.shape == (2, 2, wave.shape[1]) and rest == [[]]
    # the torch deep filter against the reference's unfold + einsum form on the same coefficients
    cmp = torch.randn(2, 257, 20, dtype=torch.complex64)
    coef = torch.randn(2, 2 * 3 * 2 * 257, 20)
    got = deep_filter_torch(cmp, coef, 3, 2)
    c = coef.reshape(2, 2, 3, 2, 257, 20)
    want = torch.zeros(2, 2, 257, 20, dtype=torch.complex64)
    for d in range(3):
        sh = torch.nn.functional.pad(cmp, (2 - d, 0))[..., :20]
        want += sh[:, None] * torch.complex(c[:, 0, d], c[:, 1, d])
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)
