"""sfsn_gsn_layer_scan_l0: layer 0 of the fused-x groups and of the groups with an input term in ONE launch at 16 rows per workgroup
(gsn_scan_l0_kernel: a workgroup runs scan3y_role or round 2's body, whichever its segment's own entry point would have launched).
Through the C ABI against sfsn_gsn_layer_scan_fused_x + sfsn_gsn_layer_scan(rows_per_wg = 16) on the same inputs: fp32 spikes, int8
spikes, final h / c and the spike counts, all for exact equality; then the engine's forward with the launch on and off."""
import numpy as np
import pytest
import torch

import refweights as rw
from test_hip_parity import DEV, _p, _t, build_module, make_layer

pytestmark = pytest.mark.gpu

TMAX = 64
TS = (1, 2, 5, 64)  # the prologue alone, one two-step trip, an odd count, more than two wraps of either role's ring


@pytest.fixture(scope="module")
def hip():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    assert L.sfsn_device_count() >= 1
    return L


def _group(rng, H, R, I, fused_x):
    """One group's layer 0: weights, T = 64 frames of input (feature rows x, or the ABI's input term zin = x.W_ih^T + b_f), state."""
    sd, alpha, beta, _ = make_layer(rng, I, H, True, True)
    x = rng.standard_normal((TMAX, R, I)).astype(np.float32)
    g = dict(sd=sd, alpha=alpha, beta=beta, R=R, I=I, H=H, fused_x=fused_x,
             h0=(rng.random((R, H)) > 0.5).astype(np.float32), c0=rng.standard_normal((R, H)).astype(np.float32))
    g["inp"] = x if fused_x else (x @ sd["weight_ih"].astype(np.float32).T + sd["bias_ih"][:H]).astype(np.float32)
    return g


def _case(seed, H, fx, zs):
    rng = np.random.default_rng(seed)
    return [_group(rng, H, R, I, True) for I, R in fx], [_group(rng, H, R, 20, False) for R in zs]


def _run(hip, gx, gz, merged, want_f32, cuts):
    """The frames [cuts[0], cuts[-1]) of every group, fed piece by piece (state carried in the h / c tensors), as one launch per piece
    (merged) or as the two calls.  Per group: (fp32 spikes or None, int8 spikes, h, c, count)."""
    from spiking_fullsubnet_amd._lib import FusedX, ScanSegment, check
    from spiking_fullsubnet_amd.engine import pack_w3
    T, H, HP = cuts[-1] - cuts[0], gx[0]["H"], (gx[0]["H"] + 63) // 64 * 64
    dev = []
    for g in gx + gz:
        pk, dq = pack_w3(g["sd"]["weight_hh"])
        dev.append(dict(pk=_t(pk), dq=_t(dq), wih=_t(g["sd"]["weight_ih"].astype(np.float32)), bias=_t(g["sd"]["bias_ih"]), alpha=_t(g["alpha"]),
                        beta=_t(g["beta"]), inp=_t(g["inp"][cuts[0]:cuts[-1]]), h=_t(g["h0"]), c=_t(g["c0"]),
                        spk=torch.full((T, g["R"], H), float("nan"), device=DEV) if want_f32 else None,
                        s8=torch.zeros((T, g["R"], HP), dtype=torch.int8, device=DEV), cnt=torch.zeros((1,), dtype=torch.int64, device=DEV)))
    for a, b in zip(cuts[:-1], cuts[1:]):
        t0, nt = a - cuts[0], b - a
        sx, sz, fin = (ScanSegment * len(gx))(), (ScanSegment * len(gz))(), (FusedX * len(gx))()
        for k, (g, d) in enumerate(zip(gx + gz, dev)):
            s = sx[k] if k < len(gx) else sz[k - len(gx)]
            R = g["R"]
            s.w_hh, s.w_dq, s.bias, s.bn_alpha, s.bn_beta = _p(d["pk"]), _p(d["dq"]), _p(d["bias"]), _p(d["alpha"]), _p(d["beta"])
            s.h_state, s.c_state, s.membrane, s.R = _p(d["h"]), _p(d["c"]), None, R
            s.spikes_f32 = d["spk"].data_ptr() + t0 * R * H * 4 if want_f32 else None
            s.spikes_i8 = d["s8"].data_ptr() + t0 * R * HP
            s.spike_count = None if want_f32 else _p(d["cnt"])
            if g["fused_x"]:
                s.zin = None
                fin[k].x, fin[k].w_ih, fin[k].I = d["inp"].data_ptr() + t0 * R * g["I"] * 4, d["wih"].data_ptr(), g["I"]
            else:
                s.zin = d["inp"].data_ptr() + t0 * R * H * 4
        if merged:
            check(hip.sfsn_gsn_layer_scan_l0(sx, fin, len(gx), sz, len(gz), nt, H, 1, None), "sfsn_gsn_layer_scan_l0")
        else:
            check(hip.sfsn_gsn_layer_scan_fused_x(sx, fin, len(gx), nt, H, None), "sfsn_gsn_layer_scan_fused_x")
            check(hip.sfsn_gsn_layer_scan(sz, len(gz), nt, H, 1, 16, None), "sfsn_gsn_layer_scan")
    torch.cuda.synchronize()
    return [(d["spk"].cpu().numpy() if want_f32 else None, d["s8"].cpu().numpy(), d["h"].cpu().numpy(), d["c"].cpu().numpy(), int(d["cnt"][0]))
            for d in dev]


def _same(new, old, tag):
    assert len(new) == len(old)
    for k, (a, b) in enumerate(zip(new, old)):
        for u, v, nm in zip(a, b, ("fp32 spikes", "int8 spikes", "h", "c", "count")):
            if u is None or v is None:
                assert u is None and v is None, f"{tag} group {k}: {nm}"
            else:
                np.testing.assert_array_equal(u, v, err_msg=f"{tag} group {k}: {nm}")


# fused-x segments (I, R): two 32-wide k-chunks (I = 38) and one (I = 30), one and two workgroups; plain segments R: a half-filled last
# workgroup (24) and a half-filled only one (8); one and two segments of either kind
LAYOUTS = {"x38r16_z24": ([(38, 16)], [24]), "x30r32_z8": ([(30, 32)], [8]), "x38r32_x30r16_z24_z8": ([(38, 32), (30, 16)], [24, 8])}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("H", [224, 192, 144])  # KS 4 + tail step (the benchmark's instantiation), KS 3 without, KS 3 + tail step
def test_one_launch_equals_the_two_calls(hip, H, layout):
    fx, zs = LAYOUTS[layout]
    gx, gz = _case(1000 * H + len(layout), H, fx, zs)
    seen = False
    for T in TS:
        for f32 in (True, False):
            new, old = _run(hip, gx, gz, True, f32, [0, T]), _run(hip, gx, gz, False, f32, [0, T])
            _same(new, old, f"H={H} {layout} T={T} fp32 spikes {f32}")
            if f32:
                spikes = [int(r[0].sum()) for r in new]
                assert not any(np.isnan(r[0]).any() for r in new)
            else:
                assert [r[4] for r in new] == spikes, "the counts are not the numbers of spikes written"
            seen = seen or all(r[1].any() for r in new)
            assert not any(r[1][:, :, H:].any() for r in new)
    assert seen, "the case cannot tell a launch that writes nothing"


@pytest.mark.parametrize("H", [224, 192])
def test_one_launch_carries_the_state_over_pieces(hip, H):
    fx, zs = LAYOUTS["x38r32_x30r16_z24_z8"]
    gx, gz = _case(31 + H, H, fx, zs)
    for f32 in (True, False):
        new, old = _run(hip, gx, gz, True, f32, [0, 5, 11]), _run(hip, gx, gz, False, f32, [0, 5, 11])
        _same(new, old, f"H={H} 5 + 6 frames, fp32 spikes {f32}")
        _same(new, _run(hip, gx, gz, True, f32, [0, 11]), f"H={H} 5 + 6 frames against 11, fp32 spikes {f32}")


def test_forward_with_the_one_launch_layer_0_is_bit_identical():
    """forward_stft of the live baseline_m model at the timed region's geometry (8 rows per full-band, 16 per sub-band workgroup), B = 4
    (sub-band rows 32 / 24 / 8: group 0 takes the fused-x role), with Engine.merge_layer0 on and off: every returned tensor."""
    kw = rw.LIVE_M
    model = build_module("live", kw, rw.live_state_dict(kw, 5))
    stft = model._stft(torch.from_numpy(rw.synth_wave(4, 40, 5)).to(DEV))
    eng = model.engine()
    eng.stack_scan, eng.rows_per_wg = False, (8, 16)  # (64 sub-band rows alone on the chip would take the stack launch: not the path in question)
    try:
        outs, launches = [], []
        for on in (True, False):
            eng.merge_layer0 = on
            eng.launches = {}
            outs.append((eng.forward_stft(stft, pipeline=False), eng.forward_stft(stft, want_layers=False, want_counts=True, pipeline=False)))
            torch.cuda.synchronize()
            launches.append(dict(eng.launches))
    finally:
        eng.merge_layer0, eng.rows_per_wg = True, (0, 0)
    on, off = launches
    # the fused-x scan ran in every forward; with the switch on inside the one launch (no separate call), with it off on its own
    # (`fused_x` counts the layer-0 launches that ran the fused-x scan, `l0_merged` those of them that were the one launch)
    assert on.get("l0_merged", 0) >= 2 and on.get("fused_x", 0) - on["l0_merged"] == 0, on
    assert off.get("l0_merged", 0) == 0 and off.get("fused_x", 0) == on["fused_x"], off
    (a, al), (b, bl) = outs
    assert torch.equal(torch.view_as_real(a["enh_stft"]), torch.view_as_real(b["enh_stft"])) and torch.equal(a["enh_mag"], b["enh_mag"])
    assert torch.equal(torch.view_as_real(al["enh_stft"]), torch.view_as_real(bl["enh_stft"])) and torch.equal(al["enh_mag"], bl["enh_mag"])
    assert torch.equal(torch.view_as_real(a["enh_stft"]), torch.view_as_real(al["enh_stft"]))
    for x, y in zip(a["fb_all"] + sum(a["sb_all"], []), b["fb_all"] + sum(b["sb_all"], [])):
        assert torch.equal(x, y)
    for x, y, z in zip(a["fb_all"] + sum(a["sb_all"], []), al["fb_all"] + sum(al["sb_all"], []), bl["fb_all"] + sum(bl["sb_all"], [])):
        if not torch.is_tensor(y):
            assert int(y.count.item()) == int(z.count.item()) == int((x > 0).sum().item())
