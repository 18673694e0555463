"""The kernels around the scans against the fp64 reference of tests/frontback.py, under its derived per-element bounds: sfsn_features
(default body, SFSN_FEAT_ROWS=wave, sfsn_features_proj with rows-only jobs), sfsn_laplace_means, sfsn_gaussian_stats and the chain into
sfsn_features, sfsn_cum_laplace_norm, sfsn_deepfilter (both kernels, every reason for the generic one), sfsn_proj_deepfilter,
sfsn_hist_shift, sfsn_fullband_input_proj.  Every output buffer starts as NaN canaries: rows and frames outside [t0, t0 + nt), columns
beyond ldz and the floats behind the end of a buffer must still hold them.  Every test prints its worst error / tolerance per entry
point; the criterion is <= 1."""
import ctypes

import numpy as np
import pytest
import torch

import frontback as fbk

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 64  # canary floats behind every output buffer


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _p(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off)


def _canary(*shape):
    """A NaN-filled tensor of `shape` with PAD more NaNs behind it: (view, whole buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + PAD,), float("nan"), device=DEV)
    return buf[:n].view(*shape), buf


class Fails(list):
    """Bound violations of one test: all of them are collected (and printed) before the test fails, so that one run shows every
    bin, row and frame that is outside."""

    def note(self, ratio, *info):
        if not ratio <= 1.0:
            self.append((info, ratio))
            print("OUTSIDE THE BOUND:", info, ratio)

    def done(self):
        assert not self, (len(self), self[:12])


def _tail_ok(buf):
    return bool(torch.isnan(buf[-PAD:]).all())


def _all_nan(t):
    return t.numel() == 0 or bool(torch.isnan(t).all())


@pytest.fixture(scope="module")
def hip():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    assert L.sfsn_device_count() >= 1
    return L


NORM_ID = dict(none=0, layernorm=1, laplace=2, gaussian=4)


def _fill_group(g, geo, norm, pr, keep):
    g.lo, g.n_units, g.ctr, g.nbr, g.ctr_fb, g.nbr_fb = geo
    g.norm = NORM_ID[norm]
    g.ln_eps = 1e-5
    if norm == "layernorm":
        w, b = _t(pr[0]), _t(pr[1])
        keep += [w, b]
        g.ln_w, g.ln_b, g.ln_eps = w.data_ptr(), b.data_ptr(), pr[2]
    elif norm == "laplace":
        mu = pr[0] if torch.is_tensor(pr[0]) else _t(np.asarray(pr[0], np.float32))
        keep.append(mu)
        g.mu = mu.data_ptr()
    elif norm == "gaussian":
        mu = pr[0] if torch.is_tensor(pr[0]) else _t(np.asarray(pr[0], np.float32))
        sd = pr[2] if torch.is_tensor(pr[2]) else _t(np.asarray(pr[2], np.float32))
        keep += [mu, sd]
        g.mu, g.ln_w = mu.data_ptr(), sd.data_ptr()


def _run_features(hip, monkeypatch, how, ri, fb, B, F, T, FB, fdrc, groups, norm, params, t0, nt):
    """One of the three ways to produce the rows; returns ([(x, buffer)], rc)."""
    from spiking_fullsubnet_amd._lib import FeatProjJob, FeatureGroup, check
    n = len(groups)
    keep, outs = [], []
    fg, jobs = (FeatureGroup * n)(), (FeatProjJob * n)()
    for i, (geo, pr) in enumerate(zip(groups, params)):
        x, buf = _canary(T, B * geo[1], sum(fbk.widths(geo)))
        outs.append((x, buf))
        for g in (fg[i], jobs[i].feat):
            _fill_group(g, geo, norm, pr, keep)
            g.x = x.data_ptr()
    monkeypatch.delenv("SFSN_FEAT_ROWS", raising=False)
    if how == "featproj":
        rc = hip.sfsn_features_proj(_p(ri), _p(fb), B, F, T, FB, fdrc, jobs, n, t0, nt, None, 0, None)
    else:
        if how == "wave":
            monkeypatch.setenv("SFSN_FEAT_ROWS", "wave")
        rc = hip.sfsn_features(_p(ri), _p(fb), B, F, T, FB, fdrc, fg, n, t0, nt, None)
        monkeypatch.delenv("SFSN_FEAT_ROWS", raising=False)
        check(rc, "sfsn_features")
    torch.cuda.synchronize()
    return outs, rc


def _check_rows(fails, outs, refs, groups, fb_np, nf, FB, t0, nt, norm, tag):
    """Window rows inside the bound, everything else still NaN; SFSN_NORM_NONE: the full-band part bit for bit."""
    worst = 0.0
    for (x, buf), (y, tol), geo in zip(outs, refs, groups):
        assert _all_nan(x[:t0]) and _all_nan(x[t0 + nt:]) and _tail_ok(buf), (tag, geo)
        got = x[t0:t0 + nt].cpu().numpy()
        r = fbk.worst(got, y[t0:t0 + nt], tol[t0:t0 + nt])
        worst = max(worst, r)
        fails.note(r, tag, geo)
        I1, I2 = fbk.widths(geo)
        if norm == "none" and I2:
            fi = fbk.group_index(nf, FB, geo)[1]
            want = fb_np[t0:t0 + nt][:, :, fi].reshape(nt, -1, I2)  # [nt][B][N][I2] -> rows
            assert np.array_equal(got[:, :, I1:].view(np.int32), np.ascontiguousarray(want).view(np.int32)), (tag, geo)
    return worst


@pytest.mark.parametrize("norm", ["none", "layernorm", "laplace", "gaussian"])
def test_features_against_fp64(hip, monkeypatch, norm):
    from spiking_fullsubnet_amd import _lib
    worst = dict(default=0.0, wave=0.0, featproj=0.0)
    taken, fails = 0, Fails()
    for name, B, F, T, FB, groups, t0, nt, fdrc in fbk.FEATURE_CASES:
        ri_np, fb_np = fbk.make_inputs(len(name), B, F, T, FB)
        params = fbk.make_norm_params(7, groups, B, norm)
        refs = fbk.feature_reference(ri_np, fb_np, FB, groups, fdrc, norm, params, B)
        ri, fb = _t(ri_np), (None if fb_np is None else _t(fb_np))
        for how in ("default", "wave", "featproj"):
            outs, rc = _run_features(hip, monkeypatch, how, ri, fb, B, F, T, FB, fdrc, groups, norm, params, t0, nt)
            if how == "featproj" and rc != 0:
                assert rc == _lib.SFSN_EUNSUPPORTED, rc
                assert all(_all_nan(b) for _, b in outs), name  # a refused call writes nothing
                continue
            taken += how == "featproj"
            worst[how] = max(worst[how], _check_rows(fails, outs, refs, groups, fb_np, F - 1, FB, t0, nt, norm, (name, norm, how)))
    print(f"sfsn_features[{norm}] worst error/tolerance: default {worst['default']:.3f}  wave-per-row {worst['wave']:.3f}  "
          f"sfsn_features_proj (rows only, {taken} cases) {worst['featproj']:.3f}")
    fails.done()
    assert taken >= 2


def _stats_call(hip, kind, ri, fb, B, F, T, FB, fdrc, groups):
    from spiking_fullsubnet_amd._lib import FeatureGroup, check
    n = len(groups)
    fg = (FeatureGroup * n)()
    for g, geo in zip(fg, groups):
        g.lo, g.n_units, g.ctr, g.nbr, g.ctr_fb, g.nbr_fb = geo
    mu, mub = _canary(n, B)
    rows = B * (F - 1 + FB)
    if kind == "laplace":
        scratch, scb = _canary(rows)  # exactly the documented size
        check(hip.sfsn_laplace_means(_p(ri), _p(fb), B, F, T, FB, fdrc, fg, n, _p(mu), _p(scratch), None), "sfsn_laplace_means")
        torch.cuda.synchronize()
        assert _tail_ok(mub) and _tail_ok(scb)
        return mu, None
    sd, sdb = _canary(n, B)
    scratch, scb = _canary(5 * rows + 2)  # exactly the documented size (8-byte aligned)
    check(hip.sfsn_gaussian_stats(_p(ri), _p(fb), B, F, T, FB, fdrc, fg, n, _p(mu), _p(sd), _p(scratch), None), "sfsn_gaussian_stats")
    torch.cuda.synchronize()
    assert _tail_ok(mub) and _tail_ok(sdb) and _tail_ok(scb)
    return mu, sd


def test_laplace_means_and_gaussian_stats_against_fp64(hip):
    w = dict(laplace=0.0, mean=0.0, sd=0.0)
    fails = Fails()
    for name, B, F, T, FB, groups, fdrc in fbk.STATS_CASES:
        ri_np, fb_np = fbk.make_inputs(len(name), B, F, T, FB, near_const=True)
        refs = fbk.stats_reference(ri_np, fb_np, FB, groups, fdrc, B, T >= 2)
        ri, fb = _t(ri_np), _t(fb_np)
        mu = _stats_call(hip, "laplace", ri, fb, B, F, T, FB, fdrc, groups)[0].cpu().numpy()
        for i, r in enumerate(refs):
            q = fbk.worst(mu[i], r["mu"], r["dmu"])
            w["laplace"] = max(w["laplace"], q)
            fails.note(q, name, "laplace", groups[i], mu[i], r["mu"])
            if B >= 2:
                assert mu[i][1] == 0.0  # the silent clip
        if T < 2:
            continue
        m, sd = _stats_call(hip, "gaussian", ri, fb, B, F, T, FB, fdrc, groups)
        m, sd = m.cpu().numpy(), sd.cpu().numpy()
        for i, r in enumerate(refs):
            qm, qs = fbk.worst(m[i], r["m"], r["dm"]), fbk.worst(sd[i], r["sd"], r["dsd"])
            w["mean"], w["sd"] = max(w["mean"], qm), max(w["sd"], qs)
            fails.note(qm, name, "gaussian mean", groups[i], m[i], r["m"])
            fails.note(qs, name, "gaussian sd", groups[i], sd[i], r["sd"])
            if B >= 2:
                assert m[i][1] == 0.0 and sd[i][1] == 0.0
    print(f"sfsn_laplace_means worst error/tolerance {w['laplace']:.3f}; sfsn_gaussian_stats mean {w['mean']:.3f} sd {w['sd']:.3f}")
    fails.done()


@pytest.mark.parametrize("norm", ["laplace", "gaussian"])
def test_statistics_into_features_chain_against_fp64(hip, monkeypatch, norm):
    """What the engine runs for the frozen front-ends: the statistics launch, then sfsn_features reading them on the device."""
    worst, fails = 0.0, Fails()
    for name, B, F, T, FB, groups, fdrc in fbk.STATS_CASES:
        if norm == "gaussian" and T < 2:
            continue
        ri_np, fb_np = fbk.make_inputs(len(name), B, F, T, FB)
        st = fbk.stats_reference(ri_np, fb_np, FB, groups, fdrc, B, norm == "gaussian")
        pref = [(s["mu"], s["dmu"]) if norm == "laplace" else (s["m"], s["dm"], s["sd"], s["dsd"]) for s in st]
        refs = fbk.feature_reference(ri_np, fb_np, FB, groups, fdrc, norm, pref, B)
        ri, fb = _t(ri_np), _t(fb_np)
        mu, sd = _stats_call(hip, norm, ri, fb, B, F, T, FB, fdrc, groups)
        pk = [(mu[i], None, None if sd is None else sd[i], None) for i in range(len(groups))]
        outs, _ = _run_features(hip, monkeypatch, "default", ri, fb, B, F, T, FB, fdrc, groups, norm, pk, 0, T)
        worst = max(worst, _check_rows(fails, outs, refs, groups, fb_np, F - 1, FB, 0, T, norm, (name, norm, "chain")))
        for (x, _), geo in zip(outs, groups):  # the silent clip: 0 / EPS = 0, never NaN
            n = geo[1]
            assert B < 2 or bool((x[:, n:2 * n] == 0).all()), (name, geo)
    print(f"statistics -> sfsn_features[{norm}] worst error/tolerance {worst:.3f}")
    fails.done()


def _cumlap(hip, x_np, frames_before, state_np):
    from spiking_fullsubnet_amd._lib import check
    T, R, I = x_np.shape
    x, xb = _canary(T, R, I)
    x.copy_(_t(x_np))
    scratch, sb = _canary(T, R)
    state = None if state_np is None else _t(np.asarray(state_np, np.float32))
    check(hip.sfsn_cum_laplace_norm(_p(x), T, R, I, _p(state), frames_before, _p(scratch), None), "sfsn_cum_laplace_norm")
    torch.cuda.synchronize()
    assert _tail_ok(xb) and _tail_ok(sb)
    return x.cpu().numpy(), None if state is None else state.cpu().numpy()


def test_cumulative_laplace_norm_against_fp64_and_in_pieces(hip):
    worst = ws = 0.0
    fails = Fails()
    for T, R, I, pieces in fbk.CUM_CASES:
        x = fbk.make_cum_input(T + R + I, T, R, I)
        y, tol, last, dlast = fbk.cum_laplace(x)
        got, st = _cumlap(hip, x, 0, np.zeros(R))
        r, rs = fbk.worst(got, y, tol), fbk.worst(st, last, dlast)
        worst, ws = max(worst, r), max(ws, rs)
        fails.note(r, T, R, I, "rows")
        fails.note(rs, T, R, I, "carried sums")
        assert T < 4 or np.all(got[:max(T // 4, 1), 0] == 0)  # the row that starts silent
        g0, _ = _cumlap(hip, x, 0, None)
        assert np.array_equal(g0.view(np.int32), got.view(np.int32)), (T, R, I, "cum_state NULL")
        t, carried, parts = 0, np.zeros(R, np.float32), []
        for n in pieces:
            yp, carried = _cumlap(hip, x[t:t + n], t, carried)
            parts.append(yp)
            t += n
        assert np.array_equal(np.concatenate(parts).view(np.int32), got.view(np.int32)), (T, R, I, "pieces")
        assert np.array_equal(carried.view(np.int32), st.view(np.int32)), (T, R, I, "carried sums")
        # a sequence that starts from carried sums and frames seen before
        c0 = (np.abs(np.random.default_rng(T).standard_normal(R)) * 50 * I).astype(np.float32)
        y1, tol1, _, _ = fbk.cum_laplace(x, 7, c0)
        g1, _ = _cumlap(hip, x, 7, c0)
        r1 = fbk.worst(g1, y1, tol1)
        worst = max(worst, r1)
        fails.note(r1, T, R, I, "carried in")
    print(f"sfsn_cum_laplace_norm worst error/tolerance rows {worst:.3f} carried sums {ws:.3f}")
    fails.done()


def _upload_proj(p_np, offset):
    """The coefficient tensor on the device; offset: 4 bytes behind a 16-byte boundary."""
    if not offset:
        return _t(p_np), None
    buf = torch.empty(p_np.size + 1, device=DEV)
    v = buf[1:].view(*p_np.shape)
    v.copy_(_t(p_np))
    assert v.data_ptr() % 16 == 4
    return v, buf


def _check_df(fails, enh, mag, ri_np, ref, t0, nt, tag):
    e_ref, m_ref, tol, tm, f0 = ref
    (e, eb), (m, mb) = enh, mag
    assert _all_nan(e[:, :, :, :t0]) and _all_nan(e[:, :, :, t0 + nt:]) and _tail_ok(eb), tag
    got = e[:, :, :, t0:t0 + nt].cpu().numpy()
    r = fbk.worst(got, e_ref[:, :, :, t0:t0 + nt], tol[:, :, :, t0:t0 + nt])
    fails.note(r, tag, "spectrum")
    want = np.broadcast_to(ri_np[:, None, f0:, t0:t0 + nt], got[:, :, f0:].shape)
    assert np.array_equal(got[:, :, f0:].view(np.int32), np.ascontiguousarray(want).view(np.int32)), (tag, "pass-through bins")
    rm = 0.0
    if m is not None:
        assert _all_nan(m[:, :, :, :t0]) and _all_nan(m[:, :, :, t0 + nt:]) and _tail_ok(mb), tag
        rm = fbk.worst(m[:, :, :, t0:t0 + nt].cpu().numpy(), m_ref[:, :, :, t0:t0 + nt], tm[:, :, :, t0:t0 + nt])
        fails.note(rm, tag, "magnitude")
    return r, rm, got


def test_deepfilter_against_fp64(hip):
    from spiking_fullsubnet_amd._lib import DfGroup, check
    w = dict(pass_=[0.0, 0.0], generic=[0.0, 0.0])
    fails = Fails()
    for name, B, F, T, S, groups, t0, nt, off in fbk.DF_CASES:
        ri_np, projs = fbk.make_df_case(len(name), B, F, T, S, groups)
        ref = fbk.deepfilter(ri_np, S, [(p,) + g for p, g in zip(projs, groups)])
        kind, _ = fbk.df_dispatch(groups, S, not off)
        ri = _t(ri_np)
        dev = [_upload_proj(p, off) for p in projs]
        dfg = (DfGroup * len(groups))()
        for a, (pt, _), (N, fc, df) in zip(dfg, dev, groups):
            a.proj, a.n_units, a.fc, a.df = pt.data_ptr(), N, fc, df
        enh, mag = _canary(B, S, F, T, 2), _canary(B, S, F, T)
        check(hip.sfsn_deepfilter(_p(ri), B, F, T, S, dfg, len(groups), _p(enh[0]), _p(mag[0]), t0, nt, None), "sfsn_deepfilter")
        torch.cuda.synchronize()
        r, rm, got = _check_df(fails, enh, mag, ri_np, ref, t0, nt, name)
        key = "pass_" if kind == "pass" else "generic"
        w[key] = [max(w[key][0], r), max(w[key][1], rm)]
        enh2 = _canary(B, S, F, T, 2)
        check(hip.sfsn_deepfilter(_p(ri), B, F, T, S, dfg, len(groups), _p(enh2[0]), None, t0, nt, None), "sfsn_deepfilter (no magnitude)")
        torch.cuda.synchronize()
        _, _, got2 = _check_df(fails, enh2, (None, None), ri_np, ref, t0, nt, name + " enh_mag NULL")
        assert np.array_equal(got.view(np.int32), got2.view(np.int32)), name
    print(f"sfsn_deepfilter worst error/tolerance: pass kernel spectrum {w['pass_'][0]:.3f} magnitude {w['pass_'][1]:.3f}; "
          f"generic kernel spectrum {w['generic'][0]:.3f} magnitude {w['generic'][1]:.3f}")
    fails.done()


def test_proj_deepfilter_spectrum_is_the_fp64_filter_of_the_rows_it_wrote(hip):
    from spiking_fullsubnet_amd import _lib
    from spiking_fullsubnet_amd._lib import ProjDfGroup
    from spiking_fullsubnet_amd.engine import pack_w3
    H, HP = 64, 64
    worst, taken, fails = [0.0, 0.0], [], Fails()
    for name, B, F, T, S, groups, t0, nt, off in fbk.DF_CASES:
        if off:
            continue
        rng = np.random.default_rng(len(name))
        ri_np, _ = fbk.make_df_case(len(name), B, F, T, S, groups)
        ri = _t(ri_np)
        arr, keep, rows = (ProjDfGroup * len(groups))(), [], []
        for a, (N, fc, df) in zip(arr, groups):
            P = 2 * fc * df * S
            s8 = np.zeros((T, B * N, HP), np.int8)
            s8[:, :, :H] = rng.random((T, B * N, H)) < 0.3
            pk, dq = pack_w3((rng.standard_normal((P, H)) * 0.2).astype(np.float32))
            ts = [_t(s8), _t(pk), _t(dq), _t(rng.standard_normal(P).astype(np.float32))]
            y = _canary(T, B * N, P)
            keep.append(ts)
            rows.append(y)
            a.spikes_i8, a.w_packed, a.w_dq, a.bias, a.proj = ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), ts[3].data_ptr(), y[0].data_ptr()
            a.n_units, a.fc, a.df = N, fc, df
        enh, mag = _canary(B, S, F, T, 2), _canary(B, S, F, T)
        rc = hip.sfsn_proj_deepfilter(_p(ri), B, F, T, S, H, arr, len(groups), _p(enh[0]), _p(mag[0]), t0, nt, None)
        torch.cuda.synchronize()
        if rc != 0:
            assert rc == _lib.SFSN_EUNSUPPORTED, (name, rc)
            assert _all_nan(enh[1]) and _all_nan(mag[1]) and all(_all_nan(b) for _, b in rows), name
            continue
        taken.append(name)
        projs = []
        for (y, yb) in rows:
            assert _all_nan(y[:t0]) and _all_nan(y[t0 + nt:]) and _tail_ok(yb) and not bool(torch.isnan(y[t0:t0 + nt]).any()), name
            projs.append(np.nan_to_num(y.cpu().numpy(), nan=0.0))
        ref = fbk.deepfilter(ri_np, S, [(p,) + g for p, g in zip(projs, groups)])
        r, rm, _ = _check_df(fails, enh, mag, ri_np, ref, t0, nt, name + " (proj_deepfilter)")
        worst = [max(worst[0], r), max(worst[1], rm)]
    print(f"sfsn_proj_deepfilter worst error/tolerance spectrum {worst[0]:.3f} magnitude {worst[1]:.3f} on {taken}")
    fails.done()
    assert len(taken) >= 3, taken


def test_hist_shift_equals_numpy_for_every_depth_and_hop(hip):
    from spiking_fullsubnet_amd import _lib
    from spiking_fullsubnet_amd._lib import check
    rng = np.random.default_rng(16)
    n = 0
    for rows in fbk.HIST_ROWS:
        for D in range(0, 16):
            for hop in range(1, 17 - D):
                h_np = rng.standard_normal((rows, D + hop, 2)).astype(np.float32)
                i_np = rng.standard_normal((rows, hop, 2)).astype(np.float32)
                h, hb = _canary(rows, D + hop, 2)
                h.copy_(_t(h_np))
                inp = _t(i_np)
                check(hip.sfsn_hist_shift(_p(h), _p(inp), rows, D, hop, None), "sfsn_hist_shift")
                torch.cuda.synchronize()
                assert _tail_ok(hb), (rows, D, hop)
                assert np.array_equal(h.cpu().numpy().view(np.int32), fbk.hist_shift(h_np, i_np, D, hop).view(np.int32)), (rows, D, hop)
                n += 1
        for D, hop in ((16, 1), (0, 17), (9, 8)):
            h, hb = _canary(rows, D + hop, 2)
            inp = _t(rng.standard_normal((rows, hop, 2)).astype(np.float32))
            assert hip.sfsn_hist_shift(_p(h), _p(inp), rows, D, hop, None) == _lib.SFSN_EUNSUPPORTED
            torch.cuda.synchronize()
            assert _all_nan(hb), (rows, D, hop)  # nothing written
    print(f"sfsn_hist_shift: {n} (rows, D, hop) combinations bit-equal to numpy")


def test_fullband_input_proj_against_fp64(hip):
    from spiking_fullsubnet_amd._lib import check
    worst, k, fails = 0.0, 0, Fails()
    for M in fbk.INPROJ_M:
        for K in fbk.INPROJ_K:
            for N in fbk.INPROJ_N:
                rng = np.random.default_rng(M + K + N)
                x = rng.standard_normal((M, K)).astype(np.float32)
                w = (0.25 * rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
                b = (rng.uniform(1.0, 2.0, N) * rng.choice([-1.0, 1.0], N)).astype(np.float32) if k % 2 == 0 else None
                k += 1
                ldz = N + 3
                ref, tol = fbk.linear(x, w, b)
                z, zb = _canary(M, ldz)
                xt, wt, bt = _t(x), _t(w), (None if b is None else _t(b))
                check(hip.sfsn_fullband_input_proj(_p(xt), _p(wt), _p(bt), _p(z), M, K, N, ldz, None), "sfsn_fullband_input_proj")
                torch.cuda.synchronize()
                assert _all_nan(z[:, N:]) and _tail_ok(zb), (M, K, N)
                r = fbk.worst(z[:, :N].cpu().numpy(), ref, tol)
                worst = max(worst, r)
                fails.note(r, M, K, N)
    print(f"sfsn_fullband_input_proj worst error/tolerance {worst:.3f} over {k} shapes")
    fails.done()
