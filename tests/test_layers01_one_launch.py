"""sfsn_gsn_layer_scan_l01: layers 0 and 1 of a two-layer stack in ONE launch at 16 rows per workgroup (gsn_scan_l01_kernel: the
layer-0 workgroups publish their progress, the layer-1 workgroups trail them).  Through the C ABI against sfsn_gsn_layer_scan_l0 (or,
where one of the layer-0 lists is empty, the single entry point) followed by sfsn_gsn_layer_scan_fused on the same inputs: both layers'
fp32 spikes, int8 spikes, final h / c and the spike counts, all for exact equality; after every launch the error word and every
progress counter of the scratch buffer are 0; then the engine's forward with the launch on and off.  No test makes a workgroup wait
for data that never comes."""
import numpy as np
import pytest
import torch

import refweights as rw
from test_hip_parity import DEV, _p, _t, build_module, make_layer

pytestmark = pytest.mark.gpu

TMAX = 64
# the consumer's prologue requests A = 6 frames and its ring holds D = 7: below, at and just above A, the ring wrap, and more than two
# wraps plus the lag
TS = (1, 2, 5, 6, 7, 8, 64)


@pytest.fixture(scope="module")
def hip():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    assert L.sfsn_device_count() >= 1
    return L


def _group(rng, H, R, I, fused_x):
    """One group's two layers: weights, T = 64 frames of layer-0 input (feature rows x, or the input term zin = x.W_ih^T + b_f), states."""
    sd, alpha, beta, _ = make_layer(rng, I, H, True, True)
    sd1, alpha1, beta1, _ = make_layer(rng, H, H, True, True)
    x = rng.standard_normal((TMAX, R, I)).astype(np.float32)
    g = dict(R=R, I=I, H=H, fused_x=fused_x, sd=(sd, sd1), alpha=(alpha, alpha1), beta=(beta, beta1),
             h0=[(rng.random((R, H)) > 0.5).astype(np.float32) for _ in range(2)], c0=[rng.standard_normal((R, H)).astype(np.float32) for _ in range(2)])
    g["inp"] = x if fused_x else (x @ sd["weight_ih"].astype(np.float32).T + sd["bias_ih"][:H]).astype(np.float32)
    return g


_CASES = {}


def _case(seed, H, fx, zs):
    """The groups of a case and their weights / inputs on the device: made once, read-only, shared by every run of the case."""
    key = (seed, H, tuple(fx), tuple(zs))
    if key not in _CASES:
        from spiking_fullsubnet_amd.engine import pack_w3
        rng = np.random.default_rng(seed)
        groups = [_group(rng, H, R, I, True) for I, R in fx] + [_group(rng, H, R, 20, False) for R in zs]
        for g in groups:
            w = []
            for l in range(2):
                pk, dq = pack_w3(g["sd"][l]["weight_hh"])
                w.append(dict(pk=_t(pk), dq=_t(dq), bias=_t(g["sd"][l]["bias_ih"]), alpha=_t(g["alpha"][l]), beta=_t(g["beta"][l])))
            w[0]["wih"] = _t(g["sd"][0]["weight_ih"].astype(np.float32))
            pki, dqi = pack_w3(g["sd"][1]["weight_ih"])
            w[1]["pki"], w[1]["dqi"] = _t(pki), _t(dqi)
            g["w"], g["inp_dev"] = w, _t(g["inp"])
        _CASES[key] = groups
    groups = _CASES[key]
    return [g for g in groups if g["fused_x"]], [g for g in groups if not g["fused_x"]]


def _scratch(hip, gx, gz):
    nbytes = hip.sfsn_stack_scratch_bytes(2, len(gx) + len(gz), sum(g["R"] for g in gx + gz))
    return torch.zeros((nbytes // 4,), dtype=torch.int32, device=DEV)


def _run(hip, gx, gz, pair, want_f32, cuts, lag=4, scratch=None):
    """The frames [cuts[0], cuts[-1]) of every group, fed piece by piece (state carried in the h / c tensors): one launch per piece
    (pair, on `scratch`) or the per-layer calls.  Per group: layer 0's, then layer 1's (fp32 spikes or None, int8 spikes, h, c, count)."""
    from spiking_fullsubnet_amd._lib import FusedInput, FusedX, ScanSegment, check
    T, H = cuts[-1] - cuts[0], (gx + gz)[0]["H"]
    HP = (H + 63) // 64 * 64
    nx, nz = len(gx), len(gz)
    dev = []
    for g in gx + gz:
        dev.append([dict(h=_t(g["h0"][l]), c=_t(g["c0"][l]), spk=torch.full((T, g["R"], H), float("nan"), device=DEV) if want_f32 else None,
                         s8=torch.zeros((T, g["R"], HP), dtype=torch.int8, device=DEV), cnt=torch.zeros((1,), dtype=torch.int64, device=DEV))
                    for l in range(2)])
    for a, b in zip(cuts[:-1], cuts[1:]):
        t0, nt = a - cuts[0], b - a
        sx, sz, fin = (ScanSegment * max(nx, 1))(), (ScanSegment * max(nz, 1))(), (FusedX * max(nx, 1))()
        s1, fin1 = (ScanSegment * (nx + nz))(), (FusedInput * (nx + nz))()
        for k, (g, d) in enumerate(zip(gx + gz, dev)):
            R = g["R"]
            for l, s in enumerate((sx[k] if k < nx else sz[k - nx], s1[k])):
                w, o = g["w"][l], d[l]
                s.w_hh, s.w_dq, s.bias, s.bn_alpha, s.bn_beta = _p(w["pk"]), _p(w["dq"]), _p(w["bias"]), _p(w["alpha"]), _p(w["beta"])
                s.h_state, s.c_state, s.membrane, s.R, s.zin = _p(o["h"]), _p(o["c"]), None, R, None
                s.spikes_f32 = o["spk"].data_ptr() + t0 * R * H * 4 if want_f32 else None
                s.spikes_i8 = o["s8"].data_ptr() + t0 * R * HP
                s.spike_count = None if want_f32 else _p(o["cnt"])
            inp = g["inp_dev"].data_ptr() + (cuts[0] + t0) * R * (g["I"] if g["fused_x"] else H) * 4
            if g["fused_x"]:
                fin[k].x, fin[k].w_ih, fin[k].I = inp, g["w"][0]["wih"].data_ptr(), g["I"]
            else:
                sz[k - nx].zin = inp
            fin1[k].spikes_in = d[0]["s8"].data_ptr() + t0 * R * HP
            fin1[k].w_ih, fin1[k].w_ih_dq = g["w"][1]["pki"].data_ptr(), g["w"][1]["dqi"].data_ptr()
        if pair:
            check(hip.sfsn_gsn_layer_scan_l01(sx if nx else None, fin if nx else None, nx, sz if nz else None, nz, s1, fin1, nt, H, 1, lag,
                                              _p(scratch), scratch.numel() * 4, None), "sfsn_gsn_layer_scan_l01")
            torch.cuda.synchronize()
            words = scratch.cpu().numpy()
            assert words[0] == 0, "a hand-off wait expired"
            assert not words.any(), "the exit of the launch left a progress counter (or the exit counter) behind"
        else:
            if nx and nz:
                check(hip.sfsn_gsn_layer_scan_l0(sx, fin, nx, sz, nz, nt, H, 1, None), "sfsn_gsn_layer_scan_l0")
            elif nx:
                check(hip.sfsn_gsn_layer_scan_fused_x(sx, fin, nx, nt, H, None), "sfsn_gsn_layer_scan_fused_x")
            else:
                check(hip.sfsn_gsn_layer_scan(sz, nz, nt, H, 1, 16, None), "sfsn_gsn_layer_scan")
            check(hip.sfsn_gsn_layer_scan_fused(s1, fin1, nx + nz, nt, H, None), "sfsn_gsn_layer_scan_fused")
    torch.cuda.synchronize()
    return [sum(((o["spk"].cpu().numpy() if want_f32 else None, o["s8"].cpu().numpy(), o["h"].cpu().numpy(), o["c"].cpu().numpy(), int(o["cnt"][0]))
                 for o in d), ()) for d in dev]


NAMES = ("layer 0 fp32 spikes", "layer 0 int8 spikes", "layer 0 h", "layer 0 c", "layer 0 count",
         "layer 1 fp32 spikes", "layer 1 int8 spikes", "layer 1 h", "layer 1 c", "layer 1 count")


def _same(new, old, tag):
    assert len(new) == len(old)
    for k, (a, b) in enumerate(zip(new, old)):
        for u, v, nm in zip(a, b, NAMES):
            if u is None or v is None:
                assert u is None and v is None, f"{tag} group {k}: {nm}"
            else:
                np.testing.assert_array_equal(u, v, err_msg=f"{tag} group {k}: {nm}")


# fused-x segments (I, R): two 32-wide k-chunks (I = 38) and one (I = 30), one and two workgroups; plain segments R: a half-filled last
# workgroup (24) and a half-filled only one (8); one and two segments of either kind; either layer-0 list alone
LAYOUTS = {"x38r16_z24": ([(38, 16)], [24]), "x30r32_z8": ([(30, 32)], [8]), "x38r32_x30r16_z24_z8": ([(38, 32), (30, 16)], [24, 8]),
           "x38r32": ([(38, 32)], []), "z24": ([], [24])}
_REF = {}


def _ref(hip, H, layout, T, f32):
    """The per-layer calls' results: computed once per (case, T, output mode), shared by the lags, never written to."""
    key = (H, layout, T, f32)
    if key not in _REF:
        fx, zs = LAYOUTS[layout]
        gx, gz = _case(1000 * H + len(layout), H, fx, zs)
        _REF[key] = _run(hip, gx, gz, False, f32, [0, T])
    return _REF[key]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("H", [224, 192, 144])  # KS 4 + tail step (the benchmark's instantiation), KS 3 without, KS 3 + tail step
def test_one_launch_equals_the_per_layer_calls(hip, H, layout):
    fx, zs = LAYOUTS[layout]
    gx, gz = _case(1000 * H + len(layout), H, fx, zs)
    scratch = _scratch(hip, gx, gz)  # ONE buffer for every launch of the case: each starts on what the previous one left
    seen = False
    for T in TS:
        for f32 in (True, False):
            old = _ref(hip, H, layout, T, f32)
            for lag in ((4, 0, 1) if T in (8, 64) else (4,)):  # the engine's default; at the two longest counts also 0 and 1
                new = _run(hip, gx, gz, True, f32, [0, T], lag=lag, scratch=scratch)
                _same(new, old, f"H={H} {layout} T={T} lag={lag} fp32 spikes {f32}")
            if f32:
                spikes = [(int(r[0].sum()), int(r[5].sum())) for r in new]
                assert not any(np.isnan(r[0]).any() or np.isnan(r[5]).any() for r in new)
            else:
                assert [(r[4], r[9]) for r in new] == spikes, "the counts are not the numbers of spikes written"
            seen = seen or all(r[1].any() and r[6].any() for r in new)
            for r in new:
                assert not r[1][:, :, H:].any() and not r[6][:, :, H:].any()  # pad columns
    assert seen, "the case cannot tell a launch that writes nothing"


@pytest.mark.parametrize("H", [224, 192])
def test_one_launch_carries_the_state_over_pieces(hip, H):
    fx, zs = LAYOUTS["x38r32_x30r16_z24_z8"]
    gx, gz = _case(31 + H, H, fx, zs)
    scratch = _scratch(hip, gx, gz)
    for f32 in (True, False):
        new, old = _run(hip, gx, gz, True, f32, [0, 5, 11], scratch=scratch), _run(hip, gx, gz, False, f32, [0, 5, 11])
        _same(new, old, f"H={H} 5 + 6 frames, fp32 spikes {f32}")
        _same(new, _run(hip, gx, gz, True, f32, [0, 11], scratch=scratch), f"H={H} 5 + 6 frames against 11, fp32 spikes {f32}")


def test_forward_with_layers_0_and_1_in_one_launch_is_bit_identical():
    """forward_stft of the live baseline_m model at the timed region's geometry (8 rows per full-band, 16 per sub-band workgroup), B = 4,
    T = 40, with Engine.pair16 on and off, in both output modes: every returned tensor and count."""
    kw = rw.LIVE_M
    model = build_module("live", kw, rw.live_state_dict(kw, 5))
    stft = model._stft(torch.from_numpy(rw.synth_wave(4, 40, 5)).to(DEV))
    eng = model.engine()
    was = eng.pair16
    eng.stack_scan, eng.rows_per_wg = False, (8, 16)  # (64 sub-band rows alone on the chip would take the stack launch: not the path in question)
    try:
        outs, launches = [], []
        for on in (True, False):
            eng.pair16 = on
            eng.launches = {}
            outs.append((eng.forward_stft(stft, pipeline=False), eng.forward_stft(stft, want_layers=False, want_counts=True, pipeline=False)))
            torch.cuda.synchronize()
            eng.check_stack_errors()
            launches.append(dict(eng.launches))
    finally:
        eng.pair16, eng.rows_per_wg = was, (0, 0)
    on, off = launches
    assert on.get("l01_pair", 0) >= 1 and on.get("fused", 0) > 0 and on.get("fused_x", 0) > 0 and on.get("l0_merged", 0) > 0, on
    assert off.get("l01_pair", 0) == 0, off
    assert (off.get("fused"), off.get("fused_x"), off.get("l0_merged")) == (on["fused"], on["fused_x"], on["l0_merged"]), (on, off)
    (a, al), (b, bl) = outs
    assert torch.equal(torch.view_as_real(a["enh_stft"]), torch.view_as_real(b["enh_stft"])) and torch.equal(a["enh_mag"], b["enh_mag"])
    assert torch.equal(torch.view_as_real(al["enh_stft"]), torch.view_as_real(bl["enh_stft"])) and torch.equal(al["enh_mag"], bl["enh_mag"])
    assert torch.equal(torch.view_as_real(a["enh_stft"]), torch.view_as_real(al["enh_stft"]))
    for x, y in zip(a["fb_all"] + sum(a["sb_all"], []), b["fb_all"] + sum(b["sb_all"], [])):
        assert torch.equal(x, y)
    for x, y, z in zip(a["fb_all"] + sum(a["sb_all"], []), al["fb_all"] + sum(al["sb_all"], []), bl["fb_all"] + sum(bl["sb_all"], [])):
        if not torch.is_tensor(y):
            assert int(y.count.item()) == int(z.count.item()) == int((x > 0).sum().item())
