"""sfsn_gsn_layer_scan_l01_projdf: layers 0 and 1 of a two-layer sub-band stack AND the sub-band epilogue (projection + deep filter +
pass-through + |.|) in ONE launch (gsn_scan_l01e_kernel: layer 1 publishes its int8 rows, a few epilogue workgroups follow it a
16-frame tile or two behind).  Through the C ABI against sfsn_gsn_layer_scan_l01 followed by sfsn_proj_deepfilter on the same inputs:
both layers' fp32 and int8 spikes, final h / c, the spike counts, the coefficient rows, the enhanced spectrum and its magnitude, all
for exact equality; after every launch the error word and every progress counter of the scratch buffer are 0; every launch of a case
runs on one scratch buffer, twice in a row.  Then the engine's forward with the launch on and off.  No test makes a workgroup wait for
data that never comes."""
import zlib

import numpy as np
import pytest
import torch

import refweights as rw
from test_hip_parity import DEV, _p, _t, build_module
from test_layers01_one_launch import _case

pytestmark = pytest.mark.gpu

F = 129


@pytest.fixture(scope="module")
def hip():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    assert L.sfsn_device_count() >= 1
    return L


_EPI = {}


def _epi(key, groups, B, S, T):
    """Per group (n_units = R / B): fc, df, the packed projection W_p [P][H] and its bias; the noisy spectrum [B][F][T][2].  Made once."""
    k = (key, B, S, T)
    if k not in _EPI:
        from spiking_fullsubnet_amd.engine import pack_w3
        rng = np.random.default_rng(zlib.crc32(repr(k).encode()))
        out = []
        for i, g in enumerate(groups):
            fc, df = ((4, 5), (2, 3), (1, 4))[i % 3]  # P = 40 S (3 / 5 column tiles), 12 S (one, mostly padding), 8 S
            P = 2 * fc * df * S
            wp = (rng.standard_normal((P, g["H"])) * 0.1).astype(np.float32)
            pk, dq = pack_w3(wp)
            out.append(dict(fc=fc, df=df, P=P, n_units=g["R"] // B, pk=_t(pk), dq=_t(dq), bias=_t(rng.standard_normal(P).astype(np.float32))))
        assert all(o["n_units"] * B == g["R"] for o, g in zip(out, groups)) and sum(o["n_units"] * o["fc"] for o in out) < F
        _EPI[k] = (out, _t(rng.standard_normal((B, F, T, 2)).astype(np.float32)))
    return _EPI[k]


def _run(hip, gx, gz, B, S, one, want_f32, cuts, key, lag=4, scratch=None, want_proj=True):
    """The frames [0, cuts[-1]) piece by piece: `one` = the one launch per piece on `scratch`, else sfsn_gsn_layer_scan_l01 +
    sfsn_proj_deepfilter.  Returns every output as host arrays."""
    from spiking_fullsubnet_amd._lib import FusedInput, FusedX, ProjDfGroup, ScanSegment, check
    groups = gx + gz
    T, H = cuts[-1], groups[0]["H"]
    HP = (H + 63) // 64 * 64
    nx, nz = len(gx), len(gz)
    epi, stft = _epi(key, groups, B, S, T)
    dev = []
    for g in groups:
        dev.append([dict(h=_t(g["h0"][l]), c=_t(g["c0"][l]), spk=torch.full((T, g["R"], H), float("nan"), device=DEV) if want_f32 else None,
                         s8=torch.zeros((T, g["R"], HP), dtype=torch.int8, device=DEV), cnt=torch.zeros((1,), dtype=torch.int64, device=DEV))
                    for l in range(2)])
    projs = [torch.full((T, g["R"], e["P"]), float("nan"), device=DEV) for g, e in zip(groups, epi)]
    enh = torch.full((B, S, F, T, 2), float("nan"), device=DEV)
    mag = torch.full((B, S, F, T), float("nan"), device=DEV)
    own = scratch is None
    if own:
        nbytes = hip.sfsn_stack_scratch_bytes(2, len(groups), sum(g["R"] for g in groups))
        scratch = torch.zeros((nbytes // 4,), dtype=torch.int32, device=DEV)
    arr = (ProjDfGroup * len(groups))()
    for a, e, d, y in zip(arr, epi, dev, projs):
        a.spikes_i8, a.w_packed, a.w_dq, a.bias = _p(d[1]["s8"]), _p(e["pk"]), _p(e["dq"]), _p(e["bias"])
        a.proj, a.n_units, a.fc, a.df = (_p(y) if want_proj else None), e["n_units"], e["fc"], e["df"]
    for t0, t1 in zip(cuts[:-1], cuts[1:]):
        nt = t1 - t0
        sx, sz, fin = (ScanSegment * max(nx, 1))(), (ScanSegment * max(nz, 1))(), (FusedX * max(nx, 1))()
        s1, fin1 = (ScanSegment * (nx + nz))(), (FusedInput * (nx + nz))()
        for k, (g, d) in enumerate(zip(groups, dev)):
            R = g["R"]
            for l, s in enumerate((sx[k] if k < nx else sz[k - nx], s1[k])):
                w, o = g["w"][l], d[l]
                s.w_hh, s.w_dq, s.bias, s.bn_alpha, s.bn_beta = _p(w["pk"]), _p(w["dq"]), _p(w["bias"]), _p(w["alpha"]), _p(w["beta"])
                s.h_state, s.c_state, s.membrane, s.R, s.zin = _p(o["h"]), _p(o["c"]), None, R, None
                s.spikes_f32 = o["spk"].data_ptr() + t0 * R * H * 4 if want_f32 else None
                s.spikes_i8 = o["s8"].data_ptr() + t0 * R * HP
                s.spike_count = None if want_f32 else _p(o["cnt"])
            inp = g["inp_dev"].data_ptr() + t0 * R * (g["I"] if g["fused_x"] else H) * 4
            if g["fused_x"]:
                fin[k].x, fin[k].w_ih, fin[k].I = inp, g["w"][0]["wih"].data_ptr(), g["I"]
            else:
                sz[k - nx].zin = inp
            fin1[k].spikes_in = d[0]["s8"].data_ptr() + t0 * R * HP
            fin1[k].w_ih, fin1[k].w_ih_dq = g["w"][1]["pki"].data_ptr(), g["w"][1]["dqi"].data_ptr()
        scan = (sx if nx else None, fin if nx else None, nx, sz if nz else None, nz, s1, fin1)
        if one:
            check(hip.sfsn_gsn_layer_scan_l01_projdf(*scan, H, 1, lag, _p(scratch), scratch.numel() * 4, _p(stft), B, F, T, S, arr, len(groups),
                                                     _p(enh), _p(mag), t0, nt, None), "sfsn_gsn_layer_scan_l01_projdf")
        else:
            check(hip.sfsn_gsn_layer_scan_l01(*scan, nt, H, 1, lag, _p(scratch), scratch.numel() * 4, None), "sfsn_gsn_layer_scan_l01")
            check(hip.sfsn_proj_deepfilter(_p(stft), B, F, T, S, H, arr, len(groups), _p(enh), _p(mag), t0, nt, None), "sfsn_proj_deepfilter")
        torch.cuda.synchronize()
        words = scratch.cpu().numpy()
        assert words[0] == 0, "a hand-off wait expired"
        assert not words.any(), "the exit of the launch left a progress counter (or the exit counter) behind"
    out = {}
    for k, d in enumerate(dev):
        for l, o in enumerate(d):
            for nm in ("spk", "s8", "h", "c", "cnt"):
                if o[nm] is not None:
                    out[f"group {k} layer {l} {nm}"] = o[nm].cpu().numpy()
    for k, y in enumerate(projs):
        out[f"group {k} coefficient rows"] = y.cpu().numpy()
    out["enh_stft"], out["enh_mag"] = enh.cpu().numpy(), mag.cpu().numpy()
    return out


def _same(new, old, tag):
    assert new.keys() == old.keys()
    for k in new:
        np.testing.assert_array_equal(new[k], old[k], err_msg=f"{tag}: {k}")  # (NaN = never written, in both or in neither)


# (B, fused-x segments (I, R), input-term segments R): the rows a clip's units take against the 16-row blocks of layer 1 --
#   3 units at B = 6: 18 rows, clip 5 straddles blocks 0 and 1 (beside 8 units per clip on the fused-x side: 48 rows);
#   8 units at B = 3: 24 rows, the last block half full (beside 16 units per clip: 48 rows); alone; the fused-x group alone;
#   2 units at B = 1: one block with 2 live rows
LAYOUTS = {"b6_x48_z18": (6, [(38, 48)], [18]), "b3_x48_z24": (3, [(30, 48)], [24]), "b3_z24": (3, [], [24]), "b3_x48": (3, [(38, 48)], []),
           "b1_z2": (1, [], [2])}
TS = (1, 2, 15, 16, 17, 33, 40)


def _groups(H, layout):
    B, fx, zs = LAYOUTS[layout]
    return (B,) + tuple(_case(7000 * H + len(layout), H, fx, zs))


def _scratch(hip, gx, gz):
    nbytes = hip.sfsn_stack_scratch_bytes(2, len(gx) + len(gz), sum(g["R"] for g in gx + gz))
    return torch.zeros((nbytes // 4,), dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("H", [224, 192])  # KS 4 + tail step (and the OFF form without fp32 spikes), KS 3
def test_one_launch_equals_the_pair_launch_and_the_epilogue_launch(hip, H, layout):
    B, gx, gz = _groups(H, layout)
    scratch = _scratch(hip, gx, gz)
    key = (H, layout)
    wrote = False
    for T in TS:
        for f32 in (True, False):
            for S in ((1, 2) if T in (17, 40) else (1,)):
                old = _run(hip, gx, gz, B, S, False, f32, [0, T], key)
                for lag in ((4, 0, 1) if T in (17, 40) and S == 1 else (4,)):
                    for rep in range(2):  # twice in a row on the one scratch buffer
                        new = _run(hip, gx, gz, B, S, True, f32, [0, T], key, lag=lag, scratch=scratch)
                        _same(new, old, f"H={H} {layout} T={T} S={S} lag={lag} fp32 spikes {f32} run {rep}")
                assert not np.isnan(new["enh_stft"]).any() and not np.isnan(new["enh_mag"]).any()
                assert all(not np.isnan(v).any() for k, v in new.items() if k.endswith("coefficient rows"))
                wrote = wrote or bool(np.abs(new["enh_mag"][:, :, :4]).sum() > 0)
    assert wrote, "the case cannot tell a launch that writes nothing"


@pytest.mark.parametrize("H", [224, 192])
def test_coefficient_rows_may_stay_unwritten(hip, H):
    B, gx, gz = _groups(H, "b6_x48_z18")
    scratch = _scratch(hip, gx, gz)
    for f32 in (True, False):
        old = _run(hip, gx, gz, B, 1, False, f32, [0, 33], (H, "noproj"), want_proj=False)
        new = _run(hip, gx, gz, B, 1, True, f32, [0, 33], (H, "noproj"), scratch=scratch, want_proj=False)
        _same(new, old, f"H={H} proj = NULL fp32 spikes {f32}")
        assert all(np.isnan(v).all() for k, v in new.items() if k.endswith("coefficient rows"))


@pytest.mark.parametrize("wgs", ["1", "500"])  # one workgroup per job owns every clip; more workgroups than tiles (one per clip is the cap)
@pytest.mark.parametrize("H", [224, 192])
def test_number_of_epilogue_workgroups(hip, H, wgs, monkeypatch):
    B, gx, gz = _groups(H, "b6_x48_z18")
    scratch = _scratch(hip, gx, gz)
    T = 64 if wgs == "1" else 16
    old = _run(hip, gx, gz, B, 1, False, True, [0, T], (H, "wgs"))
    monkeypatch.setenv("SFSN_L01E_WGS", wgs)
    for rep in range(2):
        _same(_run(hip, gx, gz, B, 1, True, True, [0, T], (H, "wgs"), scratch=scratch), old, f"H={H} SFSN_L01E_WGS={wgs} run {rep}")


@pytest.mark.parametrize("H", [224, 192])
def test_two_chunks_equal_one(hip, H):
    """24 + 16 frames as two calls against 40 in one: t0 > 0, the filter taps (df = 5 and 3) reach back before t0."""
    B, gx, gz = _groups(H, "b6_x48_z18")
    scratch = _scratch(hip, gx, gz)
    for f32 in (True, False):
        whole = _run(hip, gx, gz, B, 1, True, f32, [0, 40], (H, "chunks"), scratch=scratch)
        _same(_run(hip, gx, gz, B, 1, True, f32, [0, 24, 40], (H, "chunks"), scratch=scratch), whole, f"H={H} 24 + 16 against 40, fp32 spikes {f32}")
        _same(_run(hip, gx, gz, B, 1, False, f32, [0, 24, 40], (H, "chunks")), whole, f"H={H} the two launches in two chunks, fp32 spikes {f32}")


def _equal(a, b, path="result"):
    if a is None or isinstance(a, (bool, int, float, str)):
        assert a == b, path
    elif torch.is_tensor(a):
        assert torch.is_tensor(b) and a.shape == b.shape and a.device.type == b.device.type, path
        if a.device.type != "meta":
            x, y = (torch.view_as_real(a), torch.view_as_real(b)) if a.is_complex() else (a, b)
            assert torch.equal(x, y), path
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (u, v) in enumerate(zip(a, b)):
            _equal(u, v, f"{path}[{i}]")
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            _equal(a[k], b[k], f"{path}[{k!r}]")
    elif hasattr(a, "count"):
        assert int(a.count.item()) == int(b.count.item()), path
    else:
        assert a == b, path


def test_forward_with_the_epilogue_in_the_scan_launch_is_bit_identical():
    """forward_stft of the live baseline_m model at the timed region's geometry, B = 4, T = 40, with Engine.pair16_epilogue on and off:
    every tensor of the result, also for a ragged batch and in the lean mode with and without the coefficient rows."""
    kw = rw.LIVE_M
    model = build_module("live", kw, rw.live_state_dict(kw, 5))
    stft = model._stft(torch.from_numpy(rw.synth_wave(4, 40, 5)).to(DEV))
    eng = model.engine()
    was = eng.pair16_epilogue, eng.lean_skips_proj, eng.pair16
    eng.stack_scan, eng.rows_per_wg, eng.pair16 = False, (8, 16), True
    calls = (dict(), dict(frames=[40, 23, 40, 7]), dict(want_layers=False, want_counts=True), dict(want_layers=False, want_counts=True, lean=True))
    try:
        outs, launches = [], []
        for on in (True, False):
            eng.pair16_epilogue = on
            eng.launches = {}
            res = []
            for c in calls:
                c = dict(c)
                eng.lean_skips_proj = c.pop("lean", False)
                res.append(eng.forward_stft(stft, pipeline=False, **c))
            torch.cuda.synchronize()
            eng.check_stack_errors()
            outs.append(res)
            launches.append(dict(eng.launches))
    finally:
        eng.pair16_epilogue, eng.lean_skips_proj, eng.pair16 = was
        eng.rows_per_wg = (0, 0)
    on, off = launches
    assert on.get("l01_projdf", 0) >= len(calls) and on["l01_projdf"] == on.get("l01_pair") == off.get("l01_pair") and on.get("projdf") == off.get("projdf"), (on, off)
    assert off.get("l01_projdf", 0) == 0, off
    for i, (a, b) in enumerate(zip(*outs)):
        _equal(a, b, f"call {i}")
