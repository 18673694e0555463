"""Reference, tolerances and inputs for the kernels AROUND the scans: the feature prologue (sfsn_features, sfsn_features_proj with
rows-only jobs), the normalisation statistics (sfsn_laplace_means, sfsn_gaussian_stats, sfsn_cum_laplace_norm), the deep-filter
epilogue (sfsn_deepfilter, sfsn_proj_deepfilter), sfsn_hist_shift and sfsn_fullband_input_proj.

A helper module like parity.py (not a conftest).  Three parts:

* an fp64 numpy restatement of every operation, written from the formulas of include/sfsn.h (not from the kernels);
  test_frontback_host.py checks it against Oracle("f64") wherever the oracle has the primitive;
* per-element forward-error bounds.  Every bound is evaluated from fp64 reference quantities with u = 2^-24 (the fp32 unit
  roundoff; "1 ulp" of a hardware approximation is 2u relative) and gamma(n) = n u / (1 - n u); each function's docstring carries its
  derivation.  No constant here is fitted to what a kernel returns.  First-order analyses drop O(u^2) terms, which are below
  1e-5 of the bound: every bound is multiplied by SECOND_ORDER = 1.001 to cover them.  Every fp32 operation counts 1u (additions,
  products, fma, and the division: the build pins correctly rounded division), with ONE deviation: the LAST rounding of a result counts
  2u.  That is a consequence of the host test's criterion, not of the kernels: a correctly rounded fp32 reference may use up to 1.0 of
  a 1u bound on a value that is exact before it is stored, and the host test must show it at <= 0.5;
* one seeded input generator and the case tables both test files walk.

Every reference function takes `dt`: np.float64 is the reference, np.float32 evaluates the same formulas in fp32 numpy (the
"implementation" the host test uses to show that the bounds are attainable before a GPU is involved), and `mut` selects a
deliberately wrong variant (the host test shows that each one is rejected).
"""
import numpy as np

U = 2.0 ** -24
EPS = 2.220446049250313e-16  # the reference's EPSILON (np.finfo(np.float64).eps); exactly representable in fp32 (2^-52)
SECOND_ORDER = 1.001
POWF_ULP = 2  # ASSUMED: no accuracy table of the device powf ships with the ROCm tree; a kernel outside it is a finding, not a constant to widen
A_ABS = 3     # see a_mag


def gamma(n):
    return n * U / (1.0 - n * U)


# ----------------------------------------------------------------------------------------------------------------------
# geometry
# ----------------------------------------------------------------------------------------------------------------------
def reflect(f, nf, mut=None):
    """sfsn.h: f < 0 -> -f, f > nf - 1 -> 2 (nf - 1) - f (a reflection WITHOUT repeating the edge bin)."""
    f = np.asarray(f)
    if mut == "edge_repeat":
        return np.where(f < 0, -f - 1, np.where(f > nf - 1, 2 * nf - 1 - f, f))
    return np.where(f < 0, -f, np.where(f > nf - 1, 2 * (nf - 1) - f, f))


def widths(geo):
    lo, n, ctr, nbr, cfb, nfb = geo
    I1 = ctr + 2 * nbr
    return I1, (cfb + 2 * nfb if cfb else 0)


def group_index(nf, FB, geo, mut=None):
    """Integer index maps of one group: (magnitude bins [N][I1], full-band columns [N][I2]).
    j < I1: reflect(lo + k ctr - nbr + j);  j' < I2: reflect(lo + k ctr_fb - nbr_fb + j') % FB."""
    lo, n, ctr, nbr, cfb, nfb = geo
    I1, I2 = widths(geo)
    k = np.arange(n)[:, None]
    mi = reflect(lo + k * ctr - nbr + np.arange(I1)[None, :], nf, mut)
    step = ctr if mut == "k_ctr" else cfb
    fi = lo + k * step - nfb + np.arange(I2)[None, :]
    if mut != "fb_noreflect":
        fi = reflect(fi, nf, mut)
    if mut != "fb_nomod" and FB:
        fi = fi % FB
    return mi, fi


def magnitude(ri, fdrc, dt=np.float64):
    """|X|^fdrc on bins 0 .. F-2 (the Nyquist bin is dropped): ri [B][F][T][2] -> [B][F-1][T]."""
    ri = np.asarray(ri, dt)[:, :-1]
    m = np.hypot(ri[..., 0], ri[..., 1])  # (fp32: hypotf, the oracle's arithmetic)
    # the ABI takes fdrc as a float: the exponent IS that fp32 value (0.3f differs from 0.3 by 4e-8, which |ln m| <= 14 multiplies)
    return np.sqrt(m) if fdrc == 0.5 else (m.copy() if fdrc == 1.0 else np.power(m, dt(np.float32(fdrc))))


def a_mag(fdrc):
    """Relative error of the kernels' compressed magnitude, in units of u, from counting the roundings of compress_mag:
    fast_abs2 = v_sqrt(fma(re, re, im * im)): the product and the fma round once each, so the sum of squares is 2u off, the square
    root halves that (1u) and adds its own 1 ulp = 2u: |X| carries A_ABS = 3u.  fdrc = 0.5 takes a second v_sqrt: 3/2 + 2 = 3.5 -> 4.
    Any other exponent goes through powf: the input's 3u is multiplied by fdrc, powf adds POWF_ULP ulp = 2 POWF_ULP u (2 ulp is an
    assumption: no accuracy table for the device powf is at hand)."""
    return 4.0 if fdrc == 0.5 else float(np.ceil(A_ABS * fdrc + 2 * POWF_ULP))


def gather(mag, fb, FB, geo, mut=None):
    """x [T][B*N][I] of one group from mag [B][nf][T] and fb [T][B][FB] (None: no full-band part may be asked for)."""
    B, nf, T = mag.shape
    mi, fi = group_index(nf, FB, geo, mut)
    n = geo[1]
    x1 = np.transpose(mag[:, mi, :], (3, 0, 1, 2))  # [T][B][N][I1]
    if fi.shape[1] == 0:
        return np.ascontiguousarray(x1.reshape(T, B * n, -1))
    if mut in ("fb_nomod", "fb_noreflect"):  # what a kernel that forgot the wrap reads: whatever follows (or precedes) in memory
        flat = fb.reshape(-1)
        pos = (np.arange(T)[:, None, None, None] * B + np.arange(B)[None, :, None, None]) * FB + fi[None, None]
        x2 = flat[np.clip(pos, 0, flat.size - 1)]
    else:
        x2 = fb[:, :, fi]  # [T][B][N][I2]
    return np.ascontiguousarray(np.concatenate([x1, x2.astype(mag.dtype)], -1).reshape(T, B * n, -1))


def gather_err(mag, FB, geo, fdrc):
    """Absolute input-error bound of the gathered rows: a_mag u |x| on the magnitude part, 0 on the full-band part (a copy)."""
    B, nf, T = mag.shape
    return gather(a_mag(fdrc) * U * np.abs(mag), np.zeros((T, B, max(FB, 1))), FB, geo)


# ----------------------------------------------------------------------------------------------------------------------
# normalisations: every function returns (value, absolute error bound[, ...])
# ----------------------------------------------------------------------------------------------------------------------
def layer_norm(x, e, w, b, eps, dt=np.float64, mut=None):
    """y_i = (x_i - mean) rstd w_i + b_i, rstd = 1 / sqrt(var + eps), var biased.  Bound, with e_i the input error of x_i:

    mean: the kernels add the I elements as a tree (feat_row_tree = tree16 / tree4, or in-lane slots + wave_sum): NU - 1 in-leaf
      additions (NU = ceil(I / 64); the first addition to the literal 0 is exact) and six levels, so an element passes through at
      most d_s = min(NU + 5, I - 1) roundings.  inv_I = 1 / I and the product round once each unless I is a power of two (both exact):
      c_I = 2 or 0.       |dmean| <= mean(e) + (d_s + c_I) u mean|x|  =: dm.
    centred value: the input errors are common to x_i and the mean: |d(x_i - mean)| <= (1 - 1/I) e_i + (mean(e) - e_i / I)
      + (d_s + c_I) u mean|x| + u |x_i - mean| (the subtraction)  =: dc_i + u |x_i - mean|.
    variance: a shift of the mean by dm changes it by dm^2 only (second order in the shift); the input errors change it by at most
      (2 / I) sum |x_i - mean| e_i + mean(e^2); roundings: 2u (two uses of the rounded difference) + 1u (square) + d_s u (tree) + c_I u, all on
      var, then 1u on var + eps.  rstd is v_rsq_f32, 1 ulp = 2u.  With q = var + eps:
      rho = [(1 / I) sum |x_i - mean| e_i + (dm^2 + mean(e^2)) / 2] / q + ((3 + d_s + c_I) var / q + 1) u / 2 + 2u    (relative error of rstd).
    output: two products and the final addition round once each:
      |dy_i| <= |w_i| rstd dc_i + |w_i| |x_i - mean| rstd (rho + 3u) + 2u |y_i|  (the last rounding: 1 ulp).
    A single-element row (I = 1) has dc = 0 and x - mean = 0: y = b exactly."""
    x = np.asarray(x, dt)
    w, b = np.asarray(w, dt), np.asarray(b, dt)
    I = x.shape[-1]
    mean = x.mean(-1, keepdims=True)
    xc = x - mean
    var = (xc * xc).sum(-1, keepdims=True) / dt(max(I - 1, 1) if mut == "unbiased" else I)
    rstd = 1 / (np.sqrt(var) + dt(eps)) if mut == "eps_outside" else 1 / np.sqrt(var + dt(eps))
    y = (xc * rstd) * w + b
    if dt != np.float64 or mut is not None:
        return y, None
    NU = (I + 63) // 64
    d_s = min(NU + 5, I - 1)
    c_I = 0 if I & (I - 1) == 0 else 2
    me = e.mean(-1, keepdims=True)
    rnd = (d_s + c_I) * U * np.abs(x).mean(-1, keepdims=True)
    dm = me + rnd
    dc = (1 - 1 / I) * e + (me - e / I) + rnd
    q = var + eps
    rho = ((np.abs(xc) * e).mean(-1, keepdims=True) + (dm * dm + (e * e).mean(-1, keepdims=True)) / 2) / q + ((3 + d_s + c_I) * var / q + 1) * U / 2 + 2 * U
    tol = np.abs(w) * rstd * dc + np.abs(w) * np.abs(xc) * rstd * (rho + 3 * U) + 2 * U * np.abs(y)
    return y, tol * SECOND_ORDER


def laplace_rows(x, e, mu, dmu, B, dt=np.float64):
    """y = x / (mu[b] + EPS).  The denominator's addition rounds once (1u), the division is correctly rounded and ends the formula
    (the last rounding: 2u); an error dmu of mu moves y by |y| dmu / (mu + EPS):  |dy| <= e / den + |y| (3u + dmu / den)."""
    x = np.asarray(x, dt)
    T, R, I = x.shape
    den = (np.asarray(mu, dt) + dt(EPS))[None, :, None, None]
    y = (x.reshape(T, B, R // B, I) / den).reshape(T, R, I)
    if dt != np.float64:
        return y, None
    d64 = np.broadcast_to(den, (T, B, R // B, I)).reshape(T, R, I)
    rel = np.broadcast_to((np.asarray(dmu, np.float64)[None, :, None, None] / den), (T, B, R // B, I)).reshape(T, R, I)
    return y, (e / d64 + np.abs(y) * (3 * U + rel)) * SECOND_ORDER


def gaussian_rows(x, e, mu, dmu, sd, dsd, B, dt=np.float64):
    """y = (x - mu[b]) / (sd[b] + EPS).  Numerator: |d| <= e + dmu + u |x - mu| (the subtraction); denominator 1u + dsd / den; the
    division ends the formula (the last rounding: 2u):  |dy| <= (e + dmu) / den + |y| (4u + dsd / den)."""
    x = np.asarray(x, dt)
    T, R, I = x.shape
    sh = (T, B, R // B, I)
    den = (np.asarray(sd, dt) + dt(EPS))[None, :, None, None]
    y = ((x.reshape(sh) - np.asarray(mu, dt)[None, :, None, None]) / den).reshape(T, R, I)
    if dt != np.float64:
        return y, None
    bc = lambda v: np.broadcast_to(np.asarray(v, np.float64)[None, :, None, None], sh).reshape(T, R, I)
    d64 = bc(np.asarray(sd, np.float64) + EPS)
    return y, ((e + bc(dmu)) / d64 + np.abs(y) * (4 * U + bc(dsd) / d64)) * SECOND_ORDER


def laplace_mean(x, e, B, dt=np.float64, mut_ctr=None):
    """mu[b] = mean over (T, N, I) of the gathered group tensor.  The kernels sum each spectrum row over time in fp64, round the row sum to
    fp32 (1u of the row sum, and sum |row sums| / n <= mean|x|), combine the rows in fp64 and round the mean to fp32:
    |dmu| <= mean(e) + u mean|x| + 2u |mu| (the last rounding: 1 ulp) + n 2^-53 mean|x| (fp64 accumulation of n terms, any order)."""
    x = np.asarray(x, dt)
    T, R, I = x.shape
    x4 = x.reshape(T, B, R // B, I)
    n = T * (R // B) * (mut_ctr if mut_ctr else I)
    mu = x4.sum((0, 2, 3), dtype=dt) / dt(n)
    if dt != np.float64:
        return mu, None
    ma = np.abs(x4).mean((0, 2, 3))
    tol = e.reshape(x4.shape).mean((0, 2, 3)) + U * ma + 2 * U * np.abs(mu) + n * 2.0 ** -53 * ma
    return mu, tol * SECOND_ORDER


def gaussian_stats(x, e, B, dt=np.float64, mut=None):
    """mean and UNBIASED standard deviation per clip over (T, N, I).  The kernels keep sums and sums of squares in fp64 and form
    var = (s2 - n m^2) / (n - 1) in fp64, so the fp32 part of the error is the input error and the final rounding:
    mean: |dm| <= mean(e) + 2u |m| (the last rounding: 1 ulp) + c64, c64 = n 2^-53 mean|x|.
    variance: the input errors move it by at most dv = [2 sum |x_i - m| e_i + sum e_i^2] / (n - 1) (exact expansion of the sample
      variance of x + delta); the fp64 cancellation in s2 - n m^2 costs (n + 4) 2^-53 on each of two terms of size n mean(x^2): relative to
      the variance that is the factor mean(x^2) / var:  dv64 = 2 (n + 4) 2^-53 n mean(x^2) / (n - 1).
    standard deviation: sd - sqrt(max(var - dv - dv64, 0)) (the larger of the two one-sided changes of the square root) + 2u sd (the
      final rounding: 1 ulp) + 2^-52 sd (fp64 sqrt)."""
    x = np.asarray(x, dt)
    T, R, I = x.shape
    x4 = x.reshape(T, B, R // B, I)
    n = T * (R // B) * I
    m = x4.sum((0, 2, 3), dtype=dt) / dt(n)
    xc = x4 - m[None, :, None, None]
    var = (xc * xc).sum((0, 2, 3), dtype=dt) / dt(n if mut == "biased_sd" else n - 1)
    sd = np.sqrt(var)
    if dt != np.float64 or mut is not None:
        return m, None, sd, None
    e4 = e.reshape(x4.shape)
    ma = np.abs(x4).mean((0, 2, 3))
    dm = e4.mean((0, 2, 3)) + 2 * U * np.abs(m) + n * 2.0 ** -53 * ma
    dv = (2 * (np.abs(xc) * e4).sum((0, 2, 3)) + (e4 * e4).sum((0, 2, 3))) / (n - 1)
    dv64 = 2 * (n + 4) * 2.0 ** -53 * (x4 * x4).sum((0, 2, 3)) / (n - 1)
    dsd = sd - np.sqrt(np.maximum(var - dv - dv64, 0.0)) + (2 * U + 2.0 ** -52) * sd
    return m, dm * SECOND_ORDER, sd, dsd * SECOND_ORDER


def cum_laplace(x, frames_before=0, carried=None, dt=np.float64, mut=None):
    """Every row of x [T][R][I] divided, frame by frame, by the mean of what the row has seen so far:
    cum[t] = carried + sum_{t' <= t} sum_i x[t'][r][i];  y = x / (cum[t] / (I (frames_before + t + 1)) + EPS).  Returns (y, tol, cum[T-1], bound of cum[T-1]).
    x and `carried` are exact inputs.  A frame's sum is an fp32 sum of I terms: gamma(I - 1) sum_i |x| in any order; the running sum
    adds one rounding per frame on the partial result: |dcum[t]| <= sum_{t' <= t} (gamma(I - 1) sum_i |x[t']| + u |cum[t']|).
    The divisor I (frames_before + t + 1) converts to fp32 with at most 1u, the mean's division and + EPS round once each, the final
    division ends the formula (the last rounding: 2u):  |dy| <= |y| (|dcum| / (I n |den|) + 5u)."""
    x = np.asarray(x, dt)
    T, R, I = x.shape
    s = x.sum(-1, dtype=dt)
    c0 = np.zeros(R, dt) if carried is None else np.asarray(carried, dt)
    cum = c0[None] + np.cumsum(s, 0, dtype=dt)
    cnt = frames_before + np.arange(T) + (0 if mut == "div_t" else 1)
    n = (I * np.maximum(cnt, 1)).astype(dt)[:, None]
    den = cum / n + dt(EPS)
    y = x / den[:, :, None]
    if dt != np.float64 or mut is not None:
        return y, None, cum[-1], None
    dcum = np.cumsum(gamma(max(I - 1, 1)) * np.abs(x).sum(-1) * (I > 1) + U * np.abs(cum), 0)
    tol = np.abs(y) * (dcum / (n * np.abs(den)) + 5 * U)[:, :, None]
    return y, tol * SECOND_ORDER, cum[-1], dcum[-1] * SECOND_ORDER


# ----------------------------------------------------------------------------------------------------------------------
# deep filter, history shift, x . W^T + b
# ----------------------------------------------------------------------------------------------------------------------
def deepfilter(ri, S, groups, dt=np.float64, mut=None):
    """groups: [(proj [T][B*N][2 fc df S], N, fc, df)], laid end to end from bin 0; bins not covered are copied.
    Y[b][s][f][t] = sum_{d < df} X[b][f][t - (df-1) + d] C[d], C[d] = proj[t][b N + k][((0 fc + fci) df + d) S + s] + i proj[..][((1 fc + fci) df + d) S + s],
    X = 0 before frame 0.  Returns (enh [B][S][F][T][2], mag [B][S][F][T], tol_ri, tol_mag, first uncovered bin).

    Bound per component: 2 df products and 2 df additions in any order, with or without contraction:
      |dY_re| <= gamma(2 df + 2) sum_d (|xr||cr| + |xi||ci|),  |dY_im| <= gamma(2 df + 2) sum_d (|xr||ci| + |xi||cr|).
    Magnitude (see mag_tol): | |Y~| - |Y| | <= |dY_re| + |dY_im|, plus fast_abs2's own A_ABS u."""
    ri = np.asarray(ri, dt)
    B, F, T, _ = ri.shape
    enh = np.zeros((B, S, F, T, 2), dt)
    tol = np.zeros((B, S, F, T, 2))
    lo = 0
    for proj, N, fc, df in groups:
        proj = np.asarray(proj, dt)
        if mut == "speaker_outer":
            c = proj.reshape(T, B, N, S, 2, fc, df).transpose(0, 1, 2, 4, 5, 6, 3)
        else:
            c = proj.reshape(T, B, N, 2, fc, df, S)
        if mut == "swap_reim":
            c = c[:, :, :, ::-1]
        if mut == "taps_desc":
            c = c[:, :, :, :, :, ::-1]
        c = c.transpose(1, 6, 3, 2, 4, 5, 0).reshape(B, S, 2, N * fc, df, T)  # [B][S][c][bin][d][t]
        X = ri[:, lo:lo + N * fc]  # [B][bins][T][2]
        yr, yi = np.zeros((B, S, N * fc, T), dt), np.zeros((B, S, N * fc, T), dt)
        ar, ai = np.zeros((B, S, N * fc, T)), np.zeros((B, S, N * fc, T))
        for d in range(df):
            sh = df - 1 - d
            xs = np.zeros_like(X)
            if sh < T:
                xs[:, :, sh:] = X[:, :, :T - sh]
            if mut == "hist_nonzero" and sh:
                xs[:, :, :min(sh, T)] = X[:, :, :1]
            xr, xi = xs[:, None, :, :, 0], xs[:, None, :, :, 1]
            cr, ci = c[:, :, 0, :, d], c[:, :, 1, :, d]
            yr += xr * cr - xi * ci
            yi += xr * ci + xi * cr
            ar += np.abs(xr * cr) + np.abs(xi * ci)
            ai += np.abs(xr * ci) + np.abs(xi * cr)
        enh[:, :, lo:lo + N * fc, :, 0], enh[:, :, lo:lo + N * fc, :, 1] = yr, yi
        tol[:, :, lo:lo + N * fc, :, 0], tol[:, :, lo:lo + N * fc, :, 1] = gamma(2 * df + 2) * ar, gamma(2 * df + 2) * ai
        lo += N * fc
    p0 = lo + 1 if mut == "pass_late" else lo
    enh[:, :, p0:] = ri[:, None, p0:]
    mag, tm = mag_tol(enh, tol)
    return enh, mag, tol, tm, lo


def mag_tol(enh, tol):
    """|Y| and its bound.  fast_abs2 costs A_ABS u (counted in a_mag's docstring).  The triangle inequality carries the components' errors:
    |d|Y|| <= |dY_re| + |dY_im|.  |dM| <= (dY_re + dY_im) (1 + 3u) + 3u |Y| + 2^-60: below the documented domain (|Y| < 2^-60, include/sfsn.h) the squares may underflow and the
    result may be anything between 0 and |Y|."""
    mag = np.hypot(enh[..., 0], enh[..., 1])
    dy = tol[..., 0] + tol[..., 1]
    return mag, (dy * (1 + A_ABS * U) + A_ABS * U * np.abs(mag.astype(np.float64)) + 2.0 ** -60) * SECOND_ORDER


def hist_shift(hist, inp, D, hop):
    """hist [rows][D + hop][2], inp [rows][hop][2]: frames [hop, hop + D) move to [0, D), the new frames follow."""
    return np.concatenate([hist[:, hop:hop + D], inp], 1)


def linear(x, w, b, dt=np.float64):
    """z = x . W^T + b.  K products and K additions (an fmaf chain rounds less), then + b:
    |dz| <= gamma(K + 2) (sum_k |x||w| + |b|)."""
    x, w = np.asarray(x, dt), np.asarray(w, dt)
    z = x @ w.T
    a = np.abs(np.asarray(x, np.float64)) @ np.abs(np.asarray(w, np.float64)).T
    if b is not None:
        z = z + np.asarray(b, dt)
        a = a + np.abs(np.asarray(b, np.float64))
    return z, gamma(x.shape[1] + 2) * a


# ----------------------------------------------------------------------------------------------------------------------
# sfsn_deepfilter's host-side dispatch, restated (the case table must reach both kernels for every reason)
# ----------------------------------------------------------------------------------------------------------------------
DF_MAX_PASSES = 48


def df_dispatch(groups, S, aligned=True):
    """groups [(N, fc, df)] -> ("pass", passes per group) or ("generic", reason in {"P%4", "align", "passes", "tile"})."""
    per, max_up, max_x, npass = [], 0, 0, 0
    for N, fc, df in groups:
        P = 2 * fc * df * S
        if P % 4 or P > 2048:
            return "generic", "P%4"
        if not aligned:
            return "generic", "align"
        umax = min(max(192 // P, 1), 255)
        np_ = -(-N // umax)
        Uu = -(-N // np_)
        cnt = 0
        for k0 in range(0, N, Uu):
            if npass >= DF_MAX_PASSES or k0 > 255:
                return "generic", "passes"
            nu = min(N - k0, Uu)
            npass += 1
            cnt += 1
            max_up = max(max_up, nu * P)
            max_x = max(max_x, nu * fc * (32 + df - 1) * 2)
        per.append(cnt)
    if ((((32 * (max_up + 1) + 3) & ~3) + max_x) * 4) > 48 * 1024:
        return "generic", "tile"
    return "pass", per


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def make_inputs(seed, B, F, T, FB, near_const=False):
    """Spectrum [B][F][T][2] and full-band columns [T][B][FB] (None when FB = 0), fp32, inside |X| in {0} U [2^-60, 2^60]:
    magnitudes over 1e-6 .. 1e3; frame T // 2 digital silence (T >= 2); frame T // 2 + 1 loud and constant (T >= 50: with fewer
    frames the rows it makes constant, whose LayerNorm is ill-conditioned by construction, would be more than 2 % of a tensor);
    clip 1 silent throughout (B >= 2); clip 2 a single non-zero bin (B >= 3); clip 3, when asked for and B >= 4, nearly constant
    (sd / mean about 1e-4, small enough in level that the standard deviation's bound stays informative);
    full-band columns with exact +0.0 / -0.0 and, in the silent clip, all zero."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-6.0, 3.0, (B, F, T, 1))
    ri = (rng.standard_normal((B, F, T, 2)) * scale).astype(np.float32)
    tiny = np.abs(ri) < 2.0 ** -60  # (a normal deviate this small has probability ~1e-12: keep the domain exact all the same)
    ri[tiny] = 0.0
    if T >= 2:
        ri[:, :, T // 2] = 0.0
    if T >= 50:
        ri[:, :, T // 2 + 1] = (7.25, 0.0)
    fb = None
    if FB:
        fb = rng.standard_normal((T, B, FB)).astype(np.float32)
        z = rng.random((T, B, FB))
        fb[z < 0.05] = -0.0
        fb[(z >= 0.05) & (z < 0.10)] = 0.0
        if T >= 2:
            fb[T // 2] = 0.0
            fb[1] = -0.0
    if B >= 2:
        ri[1] = 0.0
        if FB:
            fb[:, 1] = 0.0
    if B >= 3:
        ri[2] = 0.0
        ri[2, min(5, F - 2), T // 4] = (3.0, -4.0)
        if FB:
            fb[:, 2] = 0.0
            fb[T // 4, 2, FB // 2] = -1.5
    if near_const and B >= 4:
        # magnitudes c (1 + 1e-4 g): |X|^0.5 of level ~0.05, the full-band columns at the same level
        lev = 2.5e-3 * (1.0 + 2e-4 * rng.standard_normal((F, T)))
        ph = rng.uniform(0, 2 * np.pi, (F, T))
        ri[3] = np.stack([lev * np.cos(ph), lev * np.sin(ph)], -1).astype(np.float32)
        if FB:
            fb[:, 3] = (0.05 * (1.0 + 1e-4 * rng.standard_normal((T, FB)))).astype(np.float32)
    return ri, fb


def make_cum_input(seed, T, R, I):
    """Rows for the cumulative norm: non-negative features over six decades (sfsn_features' magnitudes), row 0 silent for its first frames,
    a frame of silence in the middle."""
    rng = np.random.default_rng(seed)
    x = (np.abs(rng.standard_normal((T, R, I))) * 10.0 ** rng.uniform(-3.0, 3.0, (T, R, 1))).astype(np.float32)
    x[:max(T // 4, 1) if T > 1 else 0, 0] = 0.0
    if T > 4:
        x[T // 2] = 0.0
    return x


def make_df_case(seed, B, F, T, S, groups):
    """Spectrum over 1e-6 .. 1e3 with a silent frame, and coefficient rows of unit scale with exact zeros."""
    rng = np.random.default_rng(seed)
    ri = (rng.standard_normal((B, F, T, 2)) * 10.0 ** rng.uniform(-6.0, 3.0, (B, F, T, 1))).astype(np.float32)
    if T > 2:
        ri[:, :, T // 2] = 0.0
    projs = []
    for N, fc, df in groups:
        p = rng.standard_normal((T, B * N, 2 * fc * df * S)).astype(np.float32)
        p[rng.random(p.shape) < 0.02] = 0.0
        projs.append(p)
    return ri, projs


# ----------------------------------------------------------------------------------------------------------------------
# case tables
# ----------------------------------------------------------------------------------------------------------------------
M_GROUPS = [(0, 8, 4, 15, 4, 0), (32, 3, 32, 15, 32, 0), (128, 2, 64, 15, 64, 0)]  # baseline_m: I = 38 / 94 / 158
WSJ0_GROUPS = [(0, 8, 2, 7, 2, 0), (16, 3, 16, 7, 16, 0), (64, 2, 32, 7, 32, 0)]   # wsj0: I = 18 / 46 / 78
# full-band neighbours with ctr_fb != ctr; the last group's last unit reflects at the top edge (lo + n ctr == nf = 256, nbr > 0)
FBN_GROUPS = [(0, 8, 4, 15, 2, 1), (32, 3, 32, 15, 16, 7), (192, 2, 32, 7, 64, 7)]
# I = 1, 3, 65, 129, 255, 256; 40 units; a single unit that spans to the top edge: eight groups in one call
WIDTH_GROUPS = [(5, 3, 1, 0, 0, 0), (0, 4, 1, 1, 0, 0), (0, 1, 33, 16, 0, 0), (40, 3, 65, 32, 0, 0), (0, 2, 61, 33, 64, 32),
                (0, 2, 64, 64, 64, 0), (0, 40, 2, 3, 2, 0), (96, 1, 160, 40, 7, 1)]

# (name, B, F, T, FB, groups, t0, nt, fdrc)
FEATURE_CASES = [
    ("baseline_m_window", 5, 257, 90, 64, M_GROUPS, 37, 41, 0.5),
    ("wsj0_b1", 1, 129, 33, 32, WSJ0_GROUPS, 0, 33, 0.5),
    ("fb_neighbours_fb48", 2, 257, 31, 48, FBN_GROUPS, 0, 31, 0.5),
    ("widths_fb128_pow03", 2, 257, 33, 128, WIDTH_GROUPS, 0, 33, 0.3),
    ("f33_t1_pow1", 1, 33, 1, 32, [(0, 8, 4, 3, 4, 1)], 0, 1, 1.0),
    ("last_frame_fb64", 2, 129, 31, 64, WSJ0_GROUPS[:2], 30, 1, 0.5),
    ("fullband_input_no_fb", 3, 257, 90, 0, [(0, 1, 64, 0, 0, 0)], 89, 1, 0.5),
    ("four_groups_fb32", 2, 129, 33, 32, WSJ0_GROUPS + [(0, 1, 32, 0, 0, 0)], 0, 33, 0.5),
    ("five_groups", 2, 257, 33, 64, M_GROUPS + [(0, 1, 64, 0, 0, 0), (5, 3, 1, 0, 0, 0)], 0, 33, 0.5),
    ("six_groups", 2, 257, 31, 64, FBN_GROUPS + M_GROUPS, 0, 31, 0.5),
    ("seven_groups_last_frame", 2, 257, 31, 128, WIDTH_GROUPS[:7], 30, 1, 0.5),
]  # (1, 2, 3, 4, 5, 6, 7 and 8 groups in one call)

NOFB = (0, 1, 64, 0, 0, 0)  # the full-band model's own input: a group without a full-band part
# (name, B, F, T, FB, groups, fdrc); T = 1 is run for the Laplace mean only (sfsn_gaussian_stats asks for T >= 2)
STATS_CASES = [
    ("m_t63", 5, 257, 63, 64, M_GROUPS + [NOFB], 0.5),
    ("wsj0_t2", 5, 129, 2, 32, WSJ0_GROUPS + [NOFB], 0.5),
    ("wsj0_t1", 3, 129, 1, 32, WSJ0_GROUPS + [NOFB], 0.5),
    ("fbn_t64", 2, 257, 64, 48, FBN_GROUPS + [NOFB], 0.5),
    ("widths_t65_pow03", 4, 257, 65, 128, WIDTH_GROUPS, 0.3),
    ("wsj0_t1000", 5, 129, 1000, 32, WSJ0_GROUPS + [NOFB], 0.5),
    ("odd_rows_t9", 1, 33, 9, 33, [(0, 8, 4, 3, 4, 1), (0, 1, 32, 0, 0, 0)], 0.5),  # B (F - 1 + FB) = 65 rows of scratch: odd
]

# (T, R, I, pieces)
CUM_CASES = [(1, 1, 1, [1]), (2, 63, 38, [1, 1]), (63, 64, 158, [5, 1, 40, 17]), (65, 65, 256, [64, 1]), (700, 130, 38, [3, 250, 447]),
             (65, 130, 1, [33, 32])]

# (name, B, F, T, S, [(N, fc, df)], t0, nt, coefficient tensors offset by 4 bytes)
DF_CASES = [
    ("pass_baseline_m", 5, 257, 33, 1, [(8, 4, 5), (3, 32, 3), (2, 64, 1)], 0, 33, False),   # groups split into 2 / 3 / 2 passes
    ("pass_one_per_group", 1, 129, 77, 2, [(3, 8, 2), (2, 16, 1), (1, 32, 1)], 19, 32, False),  # history before t0, bins left over
    ("generic_p6_s3", 1, 33, 9, 3, [(5, 1, 3), (4, 3, 1)], 0, 9, False),                      # P = 18: not a multiple of 4
    ("generic_p6_s1", 5, 33, 40, 1, [(5, 1, 3), (4, 3, 1)], 31, 9, False),                    # P = 6
    ("generic_offset", 1, 257, 33, 1, [(8, 4, 5), (3, 32, 3), (2, 64, 1)], 32, 1, True),
    ("generic_tile_48k", 1, 129, 12, 1, [(2, 64, 5)], 0, 12, False),                          # covers every bin but Nyquist
    ("generic_49_passes", 1, 257, 20, 1, [(49, 4, 16)], 0, 20, False),
    ("df_longer_than_t", 1, 33, 5, 2, [(4, 2, 8)], 0, 5, False),
    ("f2_all_covered", 5, 2, 9, 1, [(2, 1, 2)], 8, 1, False),
    ("f2_nyquist_only", 1, 2, 9, 2, [(1, 1, 2)], 0, 9, False),
]

HIST_ROWS = [1, 255, 256, 257, 771]
INPROJ_M, INPROJ_K, INPROJ_N = [1, 63, 200], [1, 193, 257, 320], [16, 272, 544]


def feature_reference(ri, fb, FB, groups, fdrc, norm, params, B, dt=np.float64, mut=None, mag_scale=None):
    """Rows of every group of a call under one normalisation.  params[i]: layernorm (w, b, eps); laplace (mu, dmu); gaussian
    (mu, dmu, sd, dsd).  Returns [(y, tol)] (tol None for fp32 / mutants).  mag_scale: a factor on the EXACT magnitudes before they are rounded to fp32 (the perturbed
    fp32 run of the host test: |factor - 1| <= (a_mag - 1) u and the rounding's 1u use the whole allowance)."""
    m64 = magnitude(ri, fdrc)
    mag = magnitude(ri, fdrc, dt) if mag_scale is None else (m64 * mag_scale).astype(dt)
    out = []
    gm = mut if mut in ("edge_repeat", "fb_noreflect", "fb_nomod", "k_ctr") else None
    for geo, pr in zip(groups, params):
        x = gather(mag, None if fb is None else fb.astype(dt), FB, geo, gm)
        e = gather_err(m64, FB, geo, fdrc)
        if norm == "none":
            # the magnitude part is a_mag u relative, the full-band part a copy (bound 0: the kernel test also compares its bit patterns)
            out.append((x, e * SECOND_ORDER))
        elif norm == "layernorm":
            out.append(layer_norm(x, e, pr[0], pr[1], pr[2], dt, mut if mut in ("unbiased", "eps_outside") else None))
        elif norm == "laplace":
            out.append(laplace_rows(x, e, pr[0], pr[1], B, dt))
        else:
            out.append(gaussian_rows(x, e, pr[0], pr[1], pr[2], pr[3], B, dt))
    if dt != np.float64 or mut is not None:
        out = [(y, None) for y, _ in out]
    return out


def make_norm_params(seed, groups, B, norm):
    """Direct-test parameters: random LayerNorm weights (a third of the biases exactly zero), random per-clip (mu, sd) with no error."""
    rng = np.random.default_rng(seed)
    out = []
    for geo in groups:
        I = sum(widths(geo))
        if norm == "layernorm":
            lb = (rng.standard_normal(I) * 0.1).astype(np.float32)
            lb[rng.random(I) < 0.3] = 0.0
            out.append((rng.uniform(0.5, 1.5, I).astype(np.float32), lb, 1e-5))
        elif norm == "laplace":
            out.append((rng.uniform(0.5, 2.0, B).astype(np.float32), np.zeros(B)))
        elif norm == "gaussian":
            out.append((rng.uniform(0.5, 2.0, B).astype(np.float32), np.zeros(B), rng.uniform(0.5, 2.0, B).astype(np.float32), np.zeros(B)))
        else:
            out.append(())
    return out


def worst(y, ref, tol):
    """max |y - ref| / tol with 0 / 0 = 0 and anything / 0 = inf; NaN anywhere is inf."""
    err = np.abs(np.asarray(y, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / tol)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def vacuous_share(tol, ref):
    """Share of elements whose tolerance exceeds 1e-4 (1 + |ref|): the whole-module tests' rule."""
    return float(np.mean(tol > 1e-4 * (1 + np.abs(ref))))


def stats_reference(ri, fb, FB, groups, fdrc, B, gauss=True):
    """Per group: dict(x, e, mu, dmu[, m, dm, sd, dsd]): the Laplace mean and the Gaussian statistics of the gathered tensor with their bounds."""
    m64 = magnitude(ri, fdrc)
    out = []
    for geo in groups:
        x = gather(m64, None if fb is None else fb.astype(np.float64), FB, geo)
        e = gather_err(m64, FB, geo, fdrc)
        d = dict(x=x, e=e)
        d["mu"], d["dmu"] = laplace_mean(x, e, B)
        if gauss:
            d["m"], d["dm"], d["sd"], d["dsd"] = gaussian_stats(x, e, B)
        out.append(d)
    return out


def stats_fp32(ri, fb, FB, groups, fdrc, B, mag_scale=None, gauss=True):
    """The statistics as an fp32 implementation with fp64 accumulators forms them (the oracle's arithmetic: fp32 magnitudes, sums in
    double, results rounded to fp32)."""
    mag = magnitude(ri, fdrc, np.float32) if mag_scale is None else (magnitude(ri, fdrc) * mag_scale).astype(np.float32)
    out = []
    for geo in groups:
        x = gather(mag, fb, FB, geo).astype(np.float64)
        d = {}
        T, R, I = x.shape
        x4 = x.reshape(T, B, R // B, I)
        d["mu"] = x4.mean((0, 2, 3)).astype(np.float32)
        if gauss:
            d["m"] = d["mu"]
            d["sd"] = x4.std((0, 2, 3), ddof=1).astype(np.float32)
        out.append(d)
    return out
