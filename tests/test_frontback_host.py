"""CPU checks of tests/frontback.py itself, before a GPU is involved: the numpy restatement equals Oracle("f64") wherever the oracle has
the primitive; an fp32 evaluation of the same formulas sits inside every bound with half of it to spare (so the bounds are attainable),
and still inside with the magnitudes perturbed by the kernels' allowance; every mutant of the reference is rejected by at least one case
of the tables (so the bounds bite); the bounds are not vacuous; the deep-filter table reaches both kernels for every reason."""
import numpy as np
import pytest

import frontback as fbk
from oracle import Oracle

NORMS = ["none", "layernorm", "laplace", "gaussian"]


def _cplx(ri):
    return ri[..., 0].astype(np.float64) + 1j * ri[..., 1].astype(np.float64)


def _close(a, b, rel=1e-14):
    """Two fp64 evaluations agree to `rel` of the tensor's largest value.  1e-14 everywhere but where rows are ill-conditioned (LayerNorm
    of a constant row, Gaussian rows of a clip with one non-zero bin) or the two sides sum in another order (deep filter taps): 1e-13."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b))) <= rel * max(float(np.max(np.abs(b))), 1e-300)


# geometries the oracle can express (ctr_fb == ctr, a full-band part present): the recipes' and ones with full-band neighbours / a top edge
ORACLE_GEOS = [(2, 257, 12, 64, fbk.M_GROUPS), (2, 129, 9, 32, fbk.WSJ0_GROUPS),
               (3, 257, 7, 48, [(0, 8, 4, 15, 4, 1), (32, 3, 32, 15, 32, 7), (192, 2, 32, 7, 32, 7)]),
               (1, 33, 5, 32, [(0, 8, 4, 3, 4, 1)]), (2, 257, 6, 128, [(0, 2, 64, 64, 64, 0), (0, 40, 2, 3, 2, 0)])]


def test_restatement_equals_the_fp64_oracle():
    o = Oracle("f64")
    for B, F, T, FB, groups in ORACLE_GEOS:
        ri, fb = fbk.make_inputs(5, B, F, T, FB)
        nf = F - 1
        for fdrc in (0.5, 0.3, 1.0):
            assert _close(fbk.magnitude(ri, fdrc), o.front_mag(_cplx(ri), float(np.float32(fdrc)))), (F, fdrc)
        mag = fbk.magnitude(ri, 0.5)
        # integer index maps: gather a tensor whose value IS its index
        code_m = np.broadcast_to(np.arange(nf, dtype=np.float64)[None, :, None], (B, nf, T))
        code_f = np.broadcast_to(np.arange(FB, dtype=np.float64)[None, None, :], (T, B, FB))
        for geo in groups:
            lo, n, ctr, nbr, cfb, nfb = geo
            assert np.array_equal(fbk.gather(code_m, code_f, FB, geo), o.gather_group(code_m, code_f, lo, lo + n * ctr, ctr, nbr, cfb, nfb))
            x = fbk.gather(mag, fb.astype(np.float64), FB, geo)
            assert np.array_equal(x, o.gather_group(mag, fb, lo, lo + n * ctr, ctr, nbr, cfb, nfb))
            I = x.shape[-1]
            rng = np.random.default_rng(I)
            w, b = rng.uniform(0.5, 1.5, I), rng.standard_normal(I) * 0.1
            y, _ = fbk.layer_norm(x, np.zeros_like(x), w, b, 1e-5)
            assert _close(y, o.layer_norm(x, w, b, 1e-5), 1e-13)
            mu, _ = fbk.laplace_mean(x, np.zeros_like(x), B)
            yo, muo = o.laplace_norm(x, B)
            assert _close(mu, muo) and _close(fbk.laplace_rows(x, np.zeros_like(x), mu, np.zeros(B), B)[0], yo)
            m, _, sd, _ = fbk.gaussian_stats(x, np.zeros_like(x), B)
            yo, muo = o.gaussian_norm(x, B)
            assert _close(m, muo)
            assert _close(fbk.gaussian_rows(x, np.zeros_like(x), m, np.zeros(B), sd, np.zeros(B), B)[0], yo, 1e-13)
            assert _close(fbk.cum_laplace(x)[0], o.cum_laplace_norm(x))
    for name, B, F, T, S, groups, t0, nt, off in fbk.DF_CASES:
        ri, projs = fbk.make_df_case(3, B, F, T, S, groups)
        enh, mag, _, _, f0 = fbk.deepfilter(ri, S, [(p,) + g for p, g in zip(projs, groups)])
        eo = np.zeros((B, S, F, T), np.complex128)
        lo = 0
        for p, (N, fc, df) in zip(projs, groups):
            o.deepfilter_group(_cplx(ri), p, eo, lo, N, fc, df, S)
            lo += N * fc
        mo = o.finish_spectrum(_cplx(ri), eo, lo)
        assert lo == f0 and _close(enh[..., 0], eo.real, 1e-13) and _close(enh[..., 1], eo.imag, 1e-13), name
        assert _close(mag, mo, 1e-13), name


def _feature_runs(case, norm, **kw):
    name, B, F, T, FB, groups, t0, nt, fdrc = case
    ri, fb = fbk.make_inputs(len(name), B, F, T, FB)
    params = fbk.make_norm_params(7, groups, B, norm)
    return ri, fb, params, fbk.feature_reference(ri, fb, FB, groups, fdrc, norm, params, B, **kw)


def _ratio(outs, refs):
    return max(fbk.worst(y, r, t) for (y, _), (r, t) in zip(outs, refs))


@pytest.mark.parametrize("norm", NORMS)
def test_fp32_evaluation_is_inside_the_feature_bounds_and_they_are_not_vacuous(norm):
    o32 = Oracle("f32")
    for case in fbk.FEATURE_CASES:
        name, B, F, T, FB, groups, t0, nt, fdrc = case
        ri, fb, params, refs = _feature_runs(case, norm)
        f32 = fbk.feature_reference(ri, fb, FB, groups, fdrc, norm, params, B, dt=np.float32)
        r = _ratio(f32, refs)
        rng = np.random.default_rng(1)
        scale = 1 + rng.uniform(-1, 1, (B, F - 1, T)) * (fbk.a_mag(fdrc) - 1) * fbk.U  # (+ 1u for the rounding to fp32)
        rp = _ratio(fbk.feature_reference(ri, fb, FB, groups, fdrc, norm, params, B, dt=np.float32, mag_scale=scale), refs)
        tol = np.concatenate([t.ravel() for _, t in refs])
        ref = np.concatenate([y.ravel() for y, _ in refs])
        share = fbk.vacuous_share(tol, ref)
        print(f"{name:24s} {norm:9s} fp32 {r:.3f} perturbed {rp:.3f} vacuous {share:.4f} median tol {np.median(tol):.2e}")
        assert r <= 0.5 and rp <= 1.0 and share <= 0.02, (name, norm, r, rp, share)
        if norm in ("none", "layernorm"):  # the fp32 oracle for every group it can express (ctr_fb == ctr)
            m32 = o32.front_mag(_cplx(ri), float(np.float32(fdrc)))
            for geo, pr, (yr, tr) in zip(groups, params, refs):
                lo, n, ctr, nbr, cfb, nfb = geo
                if cfb != ctr:
                    continue
                yo = o32.gather_group(m32, fb, lo, lo + n * ctr, ctr, nbr, cfb, nfb)
                if norm == "layernorm":
                    yo = o32.layer_norm(yo, pr[0], pr[1], pr[2])
                assert fbk.worst(yo, yr, tr) <= 0.5, (name, geo, norm, "fp32 oracle")


GATHER_MUTANTS = ["edge_repeat", "fb_noreflect", "fb_nomod", "k_ctr"]


@pytest.mark.parametrize("mut", GATHER_MUTANTS + ["unbiased", "eps_outside"])
def test_feature_mutants_are_rejected(mut):
    norms = ["none", "layernorm"] if mut in GATHER_MUTANTS else ["layernorm"]
    for norm in norms:
        hit = []
        for case in fbk.FEATURE_CASES:
            name, B, F, T, FB, groups, t0, nt, fdrc = case
            ri, fb, params, refs = _feature_runs(case, norm)
            with np.errstate(all="ignore"):
                bad = fbk.feature_reference(ri, fb, FB, groups, fdrc, norm, params, B, mut=mut)
            r = _ratio(bad, refs)
            if r > 1:
                hit.append((name, r))
        print(mut, norm, hit)
        assert hit, (mut, norm)


def test_statistics_bounds_hold_for_fp32_bite_and_are_not_vacuous():
    mut_hit = dict(biased_sd=0, n_ctr=0)
    for name, B, F, T, FB, groups, fdrc in fbk.STATS_CASES:
        gauss = T >= 2
        ri, fb = fbk.make_inputs(len(name), B, F, T, FB, near_const=True)
        refs = fbk.stats_reference(ri, fb, FB, groups, fdrc, B, gauss)
        rng = np.random.default_rng(2)
        scale = 1 + rng.uniform(-1, 1, (B, F - 1, T)) * (fbk.a_mag(fdrc) - 1) * fbk.U
        for tag, sc, lim in (("fp32", None, 0.5), ("perturbed", scale, 1.0)):
            got = fbk.stats_fp32(ri, fb, FB, groups, fdrc, B, sc, gauss)
            r_mu = max(fbk.worst(g["mu"], r["mu"], r["dmu"]) for g, r in zip(got, refs))
            r_sd = max(fbk.worst(g["sd"], r["sd"], r["dsd"]) for g, r in zip(got, refs)) if gauss else 0.0
            r_m = max(fbk.worst(g["m"], r["m"], r["dm"]) for g, r in zip(got, refs)) if gauss else 0.0
            print(f"{name:18s} {tag:9s} laplace mu {r_mu:.3f} gaussian mean {r_m:.3f} sd {r_sd:.3f}")
            assert max(r_mu, r_m, r_sd) <= lim, (name, tag, r_mu, r_m, r_sd)
        for geo, r in zip(groups, refs):
            assert np.all(np.isfinite(r["mu"])) and fbk.vacuous_share(r["dmu"], r["mu"]) <= 0.02, (name, geo)
            if B >= 2:
                assert r["mu"][1] == 0.0 and r["dmu"][1] == 0.0  # the silent clip: exactly zero, and the bound says so
            if gauss:
                assert fbk.vacuous_share(r["dsd"], r["sd"]) <= 0.02 and fbk.vacuous_share(r["dm"], r["m"]) <= 0.02, (name, geo, r["dsd"], r["sd"])
                _, _, sdb, _ = fbk.gaussian_stats(r["x"], r["e"], B, mut="biased_sd")
                mut_hit["biased_sd"] += fbk.worst(sdb, r["sd"], r["dsd"]) > 1
            if fbk.widths(geo)[1] or geo[3]:
                mub, _ = fbk.laplace_mean(r["x"], r["e"], B, mut_ctr=geo[2])
                mut_hit["n_ctr"] += fbk.worst(mub, r["mu"], r["dmu"]) > 1
        if B >= 4 and gauss:  # the nearly constant clip is what it is meant to be
            ratio = refs[0]["sd"][3] / refs[0]["m"][3]
            assert 3e-5 < ratio < 3e-4, ratio
    assert all(v > 0 for v in mut_hit.values()), mut_hit


@pytest.mark.parametrize("norm", ["laplace", "gaussian"])
def test_statistics_into_features_chain_bound_is_not_vacuous(norm):
    for name, B, F, T, FB, groups, fdrc in fbk.STATS_CASES:
        if norm == "gaussian" and T < 2:
            continue
        ri, fb = fbk.make_inputs(len(name), B, F, T, FB)
        st = fbk.stats_reference(ri, fb, FB, groups, fdrc, B, norm == "gaussian")
        params = [(s["mu"], s["dmu"]) if norm == "laplace" else (s["m"], s["dm"], s["sd"], s["dsd"]) for s in st]
        refs = fbk.feature_reference(ri, fb, FB, groups, fdrc, norm, params, B)
        g32 = fbk.stats_fp32(ri, fb, FB, groups, fdrc, B, None, norm == "gaussian")
        p32 = [(g["mu"], None) if norm == "laplace" else (g["m"], None, g["sd"], None) for g in g32]
        f32 = fbk.feature_reference(ri, fb, FB, groups, fdrc, norm, p32, B, dt=np.float32)
        r = _ratio(f32, refs)
        tol = np.concatenate([t.ravel() for _, t in refs])
        ref = np.concatenate([y.ravel() for y, _ in refs])
        print(f"{name:18s} {norm:9s} chain fp32 {r:.3f} vacuous {fbk.vacuous_share(tol, ref):.4f}")
        assert np.all(np.isfinite(ref)) and r <= 0.5 and fbk.vacuous_share(tol, ref) <= 0.02, (name, r)
        # the fp32 oracle forms the statistics and the rows itself, for every group it can express (ctr_fb == ctr)
        o32 = Oracle("f32")
        m32 = o32.front_mag(_cplx(ri), float(np.float32(fdrc)))
        for geo, s_, (yr, tr) in zip(groups, st, refs):
            lo, n, ctr, nbr, cfb, nfb = geo
            if cfb != ctr:
                continue
            x32 = o32.gather_group(m32, fb, lo, lo + n * ctr, ctr, nbr, cfb, nfb)
            yo, muo = o32.laplace_norm(x32, B) if norm == "laplace" else o32.gaussian_norm(x32, B)
            rm = fbk.worst(muo, s_["mu"], s_["dmu"]) if norm == "laplace" else fbk.worst(muo, s_["m"], s_["dm"])
            assert fbk.worst(yo, yr, tr) <= 0.5 and rm <= 0.5, (name, geo, norm, "fp32 oracle", fbk.worst(yo, yr, tr), rm)


def test_cumulative_norm_bound_holds_bites_and_pieces_agree():
    hit = 0
    for T, R, I, pieces in fbk.CUM_CASES:
        x = fbk.make_cum_input(T + R + I, T, R, I)
        y, tol, last, _ = fbk.cum_laplace(x)
        y32 = fbk.cum_laplace(x, dt=np.float32)[0]
        r = fbk.worst(y32, y, tol)
        share = fbk.vacuous_share(tol, y)
        print(f"T {T:4d} R {R:4d} I {I:4d} fp32 {r:.3f} vacuous {share:.4f}")
        assert np.all(np.isfinite(y)) and r <= 0.5 and share <= 0.02, (T, R, I, r, share)
        assert fbk.worst(Oracle("f32").cum_laplace_norm(x), y, tol) <= 0.5, (T, R, I, "fp32 oracle")
        assert T < 4 or np.all(y[:max(T // 4, 1), 0] == 0)  # the row that starts silent: 0 / EPS = 0
        # fed in pieces with the carried sums and frames_before: the same values
        t, carried, parts = 0, None, []
        for n in pieces:
            yp, _, carried, _ = fbk.cum_laplace(x[t:t + n], t, carried)
            parts.append(yp)
            t += n
        assert t == T and np.max(np.abs(np.concatenate(parts) - y) / (np.abs(y) + 1e-300)) < 1e-13
        if T > 1:
            hit += fbk.worst(fbk.cum_laplace(x, mut="div_t")[0], y, tol) > 1
    assert hit >= 3


DF_MUTANTS = ["taps_desc", "hist_nonzero", "swap_reim", "speaker_outer", "pass_late"]


def test_deep_filter_bound_holds_for_fp32_bites_and_the_table_reaches_every_branch():
    hits = {m: 0 for m in DF_MUTANTS}
    reasons, passes = set(), []
    for name, B, F, T, S, groups, t0, nt, off in fbk.DF_CASES:
        ri, projs = fbk.make_df_case(len(name), B, F, T, S, groups)
        gl = [(p,) + g for p, g in zip(projs, groups)]
        enh, mag, tol, tm, f0 = fbk.deepfilter(ri, S, gl)
        e32, m32, _, _, _ = fbk.deepfilter(ri, S, gl, dt=np.float32)
        r, rm = fbk.worst(e32, enh, tol), fbk.worst(m32, mag, tm)
        share = max(fbk.vacuous_share(tol, enh), fbk.vacuous_share(tm, mag))
        print(f"{name:22s} fp32 spectrum {r:.3f} magnitude {rm:.3f} vacuous {share:.4f} dispatch {fbk.df_dispatch(groups, S, not off)}")
        assert r <= 0.5 and rm <= 0.5 and share <= 0.02, (name, r, rm, share)
        o32 = Oracle("f32")  # the fp32 oracle has every one of these shapes
        eo, lo = np.zeros((B, S, F, T), np.complex64), 0
        for p, (N, fc, df) in zip(projs, groups):
            o32.deepfilter_group(_cplx(ri), p, eo, lo, N, fc, df, S)
            lo += N * fc
        mo = o32.finish_spectrum(_cplx(ri), eo, lo)
        ro = max(fbk.worst(eo.real, enh[..., 0], tol[..., 0]), fbk.worst(eo.imag, enh[..., 1], tol[..., 1]), fbk.worst(mo, mag, tm))
        assert ro <= 0.5, (name, "fp32 oracle", ro)
        assert np.array_equal(enh[:, :, f0:], np.broadcast_to(ri[:, None, f0:].astype(np.float64), enh[:, :, f0:].shape))
        for m in DF_MUTANTS:
            hits[m] += fbk.worst(fbk.deepfilter(ri, S, gl, mut=m)[0], enh, tol) > 1
        kind, what = fbk.df_dispatch(groups, S, not off)
        if kind == "generic":
            reasons.add(what)
        else:
            passes += what
    assert all(v > 0 for v in hits.values()), hits
    assert reasons == {"P%4", "align", "passes", "tile"}, reasons
    assert 1 in passes and any(p > 1 for p in passes), passes
    # the two shapes the table names for P % 4 != 0, the 48 KB tile of fc = 64, df = 5, and more than DF_MAX_PASSES passes
    assert fbk.df_dispatch([(5, 1, 3)], 1) == ("generic", "P%4") and fbk.df_dispatch([(4, 3, 1)], 1) == ("generic", "P%4")
    assert fbk.df_dispatch([(2, 64, 5)], 1) == ("generic", "tile") and fbk.df_dispatch([(49, 4, 16)], 1) == ("generic", "passes")
    assert fbk.df_dispatch([(8, 4, 5), (3, 32, 3), (2, 64, 1)], 1) == ("pass", [2, 3, 2])
    assert fbk.df_dispatch([(8, 4, 5), (3, 32, 3), (2, 64, 1)], 1, aligned=False) == ("generic", "align")


def test_input_product_bound_holds_for_fp32_and_is_not_vacuous():
    for M in fbk.INPROJ_M:
        for K in fbk.INPROJ_K:
            for N in fbk.INPROJ_N:
                rng = np.random.default_rng(M + K + N)
                x = rng.standard_normal((M, K)).astype(np.float32)
                w = (0.25 * rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
                b = (rng.uniform(1.0, 2.0, N) * rng.choice([-1.0, 1.0], N)).astype(np.float32)
                z, tol = fbk.linear(x, w, b)
                z32 = Oracle("f32").linear(x, w, b)
                assert fbk.worst(z32, z, tol) <= 0.5 and fbk.vacuous_share(tol, z) <= 0.02, (M, K, N)
                # a product that dropped its last column or its bias is outside
                assert fbk.worst(fbk.linear(x[:, :-1], w[:, :-1], b)[0] if K > 1 else z - b, z, tol) > 1


def test_history_shift_reference():
    h = np.arange(2 * 5 * 2, dtype=np.float32).reshape(2, 5, 2)
    i = -np.arange(2 * 2 * 2, dtype=np.float32).reshape(2, 2, 2) - 1
    out = fbk.hist_shift(h, i, 3, 2)
    assert np.array_equal(out[:, :3], h[:, 2:]) and np.array_equal(out[:, 3:], i)
    assert np.array_equal(fbk.hist_shift(h[:, :2], i, 0, 2), i)
