"""Reference, bounds, inputs and mutants for the TRAINING-mode layer calls of csrc/sfsn_train.hip: sfsn_gsn_train_step_fwd / _bwd,
sfsn_gsn_train_seq_fwd / _bwd and sfsn_gsn_train_seq_fwd_multi / _bwd_multi.

A helper module like frontback.py / scanref.py (not a conftest); numpy only.  Five parts:

* `fwd_step`, `bwd_step`, `running`: ONE time step of the cell in fp64, written from the formulae at the head of csrc/sfsn_train.hip
  (the reference's neuron, NEURON:132-153, with nn.BatchNorm1d in training mode inside the cell and the triangle surrogate).  The same
  functions with `dt=np.float32` are the "kernel form": every operation rounded to fp32 in the kernels' association, the two products in
  k order (`order="k"`: the step entries' fma chain) or in the 4-way interleave of the matrix instruction's k split (`order="mfma4"`),
  the row reductions per row block of `rpb` rows merged as the kernels merge them.  Used by the host test only.
* `fwd_bound`, `bwd_bound`, `running_bound`: the fp64 step together with a per-element bound on what an fp32 evaluation of the same
  step may differ by.  TEACHER-FORCED: a step's inputs are what the device itself carried into that step (its own spikes, membrane,
  saved tensors, d_z and dL/dc), taken as exact -- so a bound never has to follow a spike flip along the chain and every step is a
  short straight-line computation.  The derivations are in the docstrings.  Units: U = 2^-24 per rounding, gamma(n) for n chained
  roundings, first order times SECOND_ORDER; division and square root are one rounding each (the library is built with
  -fhip-fp32-correctly-rounded-divide-sqrt -ffp-contract=off).  No constant is fitted to what a kernel or an emulation returns.
* `CASES`, `BWD_CASES`, `GEOMETRIES`: seeded inputs that leave the mild regime, each planting its property in named neuron columns and
  leaving the other columns as the random control.
* `MUTANTS`: deliberately wrong variants of the fp64 step (and one of the kernel form) that the bounds must reject -- all but `spike_gt`,
  whose membranes are the reference's bit for bit: only the spike rule at u == 0 (an asserted spike, bound 0) can reject it.
* `sim_fwd`, `sim_bwd`, `free_chain`, `judge_fwd`, `judge_bwd`: a free-running kernel-form chain (the host test's stand-in for the device),
  a free-running fp64 chain, and the comparison of a chain's per-step tensors with the teacher-forced reference.

Domain: finite inputs, |pre-activation| <= 128, no denormal inputs posed; results below the normal range carry TINY.
"""
import zlib

import numpy as np

U = 2.0 ** -24
SECOND_ORDER = 1.001
EXPF_ULP = 2  # ASSUMED: no accuracy table of the device expf ships with the ROCm tree; a kernel outside it is a finding, not a constant to widen
TINY = 2.0 ** -126  # results below the normal range are not posed: a flushed or overflowed tail of the sigmoid is off by at most this
C_RED = 8  # roundings a row reduction takes beyond one per row: see fwd_bound
CAP = 0.02  # largest share of a step's spikes the reference alone may leave unasserted (hopref.py's figure)
F32, F64 = np.float32, np.float64


def gamma(n):
    return n * U / (1.0 - n * U)


def _fma(a, b, c):
    """fp32 fma through fp64: the product of two fp32 numbers is exact in fp64."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


# ----------------------------------------------------------------------------------------------------------------------
# the two products
# ----------------------------------------------------------------------------------------------------------------------
def product(a, w, dt=F64, order="k"):
    """a [R][K] . w [N][K]^T -> [R][N].  fp64: a BLAS product.  fp32: one fma chain in k order ("k"), or the matrix pipe's split
    ("mfma4": v_mfma_f32_16x16x4_f32 takes k = 16 s + 4 q + e for q = 0..3 in one instruction; the four products are summed and
    added to the accumulator with one rounding here -- the instruction's internal order is not documented, the bound allows any)."""
    if dt is F64:
        return np.asarray(a, F64) @ np.asarray(w, F64).T
    a, w = np.asarray(a, F32), np.asarray(w, F32)
    R, K = a.shape
    acc = np.zeros((R, w.shape[0]), F32)
    if order == "k":
        for k in range(K):
            acc = _fma(a[:, k, None], w[None, :, k], acc)
        return acc
    assert order == "mfma4" and K % 16 == 0
    for s in range(K // 16):
        for e in range(4):
            ks = 16 * s + 4 * np.arange(4) + e
            pr = a[:, ks].astype(F64)[:, None, :] * w[:, ks].astype(F64)[None, :, :]
            acc = (acc.astype(F64) + ((pr[..., 0] + pr[..., 1]) + (pr[..., 2] + pr[..., 3]))).astype(F32)
    return acc


def _product_bound(a, w):
    """gamma(number of non-zero terms) . sum |terms|: any summation order of an fp32 product with exact or singly rounded products."""
    a, w = np.asarray(a, F64), np.asarray(w, F64)
    nnz = (a != 0).astype(F64) @ (w != 0).astype(F64).T
    return gamma(nnz) * (np.abs(a) @ np.abs(w).T)


# ----------------------------------------------------------------------------------------------------------------------
# row reductions as the kernels make them (kernel form only)
# ----------------------------------------------------------------------------------------------------------------------
def _block_sum(v, w=None):
    """The workgroup's reduction over its rows: thread (rsub, j) adds rows rsub, rsub + 16, ... in order (v, or fma(v, w, .)), then
    the 16 partial sums are added in order (reduce16)."""
    part = np.zeros((16, v.shape[1]), F32)
    for i in range(v.shape[0]):
        part[i % 16] = (part[i % 16] + v[i]) if w is None else _fma(v[i], w[i], part[i % 16])
    s = np.zeros(v.shape[1], F32)
    for i in range(16):
        s = s + part[i]
    return s


def _blocks(R, rpb):
    rpb = R if rpb is None else rpb
    return [(lo, min(lo + rpb, R)) for lo in range(0, R, rpb)]


# ----------------------------------------------------------------------------------------------------------------------
# forward step
# ----------------------------------------------------------------------------------------------------------------------
def fwd_step(z, bias, w_hh, h_prev, c_prev, bn_w, bn_b, eps, shared, dt=F64, order="k", rpb=None, mut=None):
    """One forward step.  z [R][G H], bias [2 H], w_hh [G H][H] (G = 1 shared, 2 separate gates), h_prev / c_prev [R][H] (h_prev is taken
    as != 0), bn_w / bn_b [H] or None (no BatchNorm: u = c').  Returns dict f, g (= pre_g), cy (= c'), mean, var (biased), invstd, xhat,
    u, spikes.  `eps` is the fp32 number the kernel is handed."""
    H = w_hh.shape[1]
    G = 1 if shared else 2
    one = dt(1.0)
    z, bias, w_hh, c_prev = (np.asarray(v, dt) for v in (z, bias, w_hh, c_prev))
    R = z.shape[0]
    h = np.asarray(h_prev, dt) if mut == "h_value" else (np.asarray(h_prev) != 0).astype(dt)
    rec = product(h, w_hh, dt, order)
    bg = bias[:H] if mut == "bias_f_for_g" else bias[H:2 * H]
    with np.errstate(over="ignore", under="ignore"):
        pre_f = (z[:, :H] + bias[:H]) + rec[:, :H]
        pre_g = (z[:, (G - 1) * H:] + bg) + rec[:, (G - 1) * H:]
        f = one / (one + np.exp(-pre_f))
        cy = f * c_prev + (one - f) * pre_g
    out = dict(f=f, g=pre_g, cy=cy)
    if bn_w is None:
        out.update(u=cy, spikes=(cy > 0 if mut == "spike_gt" else cy >= 0).astype(dt), xhat=None, invstd=None, mean=None, var=None)
        return out
    bn_w, bn_b, eps = np.asarray(bn_w, dt), np.asarray(bn_b, dt), dt(F32(eps))
    if dt is F64:
        mean = cy.mean(0)
        var = ((cy - mean) ** 2).mean(0)
    elif mut == "var_e2":  # sum of squares minus square of the mean
        mean = _block_sum(cy) / dt(R)
        var = _block_sum(cy, cy) / dt(R) - mean * mean
        var = np.maximum(var, dt(0))
    else:  # per row block (count, mean, sum of squared deviations), merged pairwise in block order
        cnt, mean, m2 = dt(0), np.zeros(H, dt), np.zeros(H, dt)
        for lo, hi in _blocks(R, rpb):
            nb = dt(hi - lo)
            mb = _block_sum(cy[lo:hi]) / nb
            d = cy[lo:hi] - mb
            qb = _block_sum(d, d)
            if len(_blocks(R, rpb)) == 1:
                mean, m2 = mb, qb
                break
            tot, delta = cnt + nb, mb - mean
            mean = mean + delta * (nb / tot)
            m2 = m2 + qb + delta * delta * (cnt * nb / tot)
            cnt = tot
        var = m2 / dt(R)
    vn = var * dt(R) / dt(max(R - 1, 1)) if mut == "unbiased_norm" else var
    with np.errstate(divide="ignore"):
        invstd = one / (np.sqrt(vn) + eps) if mut == "eps_outside" else one / np.sqrt(vn + eps)
    xhat = (cy - mean) * invstd
    u = xhat * bn_w + bn_b
    out.update(mean=mean, var=var, invstd=invstd, xhat=xhat, u=u, spikes=(u > 0 if mut == "spike_gt" else u >= 0).astype(dt))
    return out


def running(rm, rv, mean, var, R, mom, dt=F64, mut=None):
    """Running statistics after one step.  mom >= 0: (1 - m) old + m new.  mom < 0: the cumulative form, factor 1 / (-mom) (the count of
    steps INCLUDING this one).  The running variance takes the unbiased estimate var R / (R - 1)."""
    rm, rv, mean, var = (np.asarray(v, dt) for v in (rm, rv, mean, var))
    m = dt(F32(mom)) if mom >= 0 else dt(1.0) / dt(-mom)
    unb = var if (mut == "biased_running" or R <= 1) else var * (dt(R) / dt(R - 1))
    a, b = (m, dt(1.0) - m) if mut == "momentum_swapped" else (dt(1.0) - m, m)
    return a * rm + b * mean, a * rv + b * unb


def fwd_bound(z, bias, w_hh, h_prev, c_prev, bn_w, bn_b, eps, shared):
    """(ref, bnd): the fp64 step and per-element bounds on f, g, u, xhat, invstd, mean, var for an fp32 evaluation on the same inputs.

    With e(x) the bound of x, |x| its fp64 magnitude and one U per rounding (first order; all times SECOND_ORDER, plus TINY):
      rec    : gamma(nnz) sum|h w|                                     any order; nnz = non-zero terms (h is 0 / 1)
      zb = z + b : U |zb| ;  pre = zb + rec : e(zb) + e(rec) + U |pre|  (g IS pre_g)
      E = exp(-pre_f): relative e(pre_f) + 2 EXPF_ULP U                 (1 ulp = 2 U relative, as scanref.py counts it)
      D = 1 + E : E rel(E) + U D ;  f = 1 / D : f (e(D) / D + U)  + TINY (E overflows or vanishes beyond |pre| ~ 88: f is 0 or 1
                                                                          on the device, e^-|pre| or 1 - e^-|pre| in fp64)
      a = f c : |c| e(f) + U |a| ;  o = 1 - f : e(f) + U |o| ;  b = o g : |g| e(o) + |o| e(g) + U |b| ;  c' = a + b : e(a) + e(b) + U |c'|
      mean   : mean_r e(c') + gamma(R + C_RED) max_r |c'|   =: mean_r e(c') + delta
               a sum of n numbers in ANY order is off by at most gamma(n - 1) sum |x|, the division by the count adds one rounding; a
               merge of row-block means (mean += (mb - mean) (nb / tot)) takes 4 roundings per block on magnitudes <= max |c'| and
               passes earlier errors on with a factor <= 1: gamma(rows of the largest block + 4 blocks).  The kernels give every
               row block but the last at least 16 rows and use at most 16 blocks, so rows + 4 blocks <= R + 7 (two blocks of 16
               and 1 rows: 16 + 8 = 17 + 7); one more for the final division of the variance: C_RED = 8.
      var    : (2 / R) sum_r |c' - mean| e(c')                            the inputs' errors
               + gamma(R + C_RED) (sd + delta)^2                          squares (d - m)^2 accumulated by fma, any order, the merge, / R
               + 4 delta sd + 5 delta^2                                    deviations taken from a rounded (block) mean: a block's sum
               of squares about m instead of its mean adds n (m - mean)^2 <= n delta^2; a merge term w (delta_b +- 2 delta)^2 is off
               by w (4 delta |delta_b| + 4 delta^2), and sum_b w_b |delta_b| <= sqrt(R) sqrt(R var) (Cauchy-Schwarz, sum w_b <= R).
               sd = sqrt(var).  This is what makes a large mean against a small spread expensive, rightly: see the `offset` case.
      s = var + eps : e(var) + U s ;  invstd = 1 / sqrt(s) : invstd (e(s) / (2 s) + 2 U)
      d = c' - mean : e(c') + e(mean) + U |d| ;  xhat = d invstd : |d| e(invstd) + invstd e(d) + U |xhat|
      u = xhat gamma + beta : |gamma| e(xhat) + U |xhat gamma| + U |u|    (no contraction: two roundings);  no BatchNorm: u = c'."""
    ref = fwd_step(z, bias, w_hh, h_prev, c_prev, bn_w, bn_b, eps, shared)
    H = w_hh.shape[1]
    G = 1 if shared else 2
    z, bias, w_hh, c = (np.asarray(v, F64) for v in (z, bias, w_hh, c_prev))
    R = z.shape[0]
    h = (np.asarray(h_prev) != 0).astype(F64)
    e_rec = _product_bound(h, w_hh)
    zbf, zbg = z[:, :H] + bias[:H], z[:, (G - 1) * H:] + bias[H:]
    pre_f = zbf + product(h, w_hh)[:, :H]
    e_pf = U * np.abs(zbf) + e_rec[:, :H] + U * np.abs(pre_f)
    e_g = U * np.abs(zbg) + e_rec[:, (G - 1) * H:] + U * np.abs(ref["g"])
    f, g = ref["f"], ref["g"]
    with np.errstate(over="ignore"):
        E = np.exp(-pre_f)
    D = 1.0 + E
    # (E / D = 1 - f, also where E overflows)
    e_f = f * ((1.0 - f) * (e_pf + 2 * EXPF_ULP * U) + 2 * U) + TINY
    a, o = f * c, 1.0 - f
    e_a = np.abs(c) * e_f + U * np.abs(a)
    e_o = e_f + U * np.abs(o)
    b = o * g
    e_b = np.abs(g) * e_o + np.abs(o) * e_g + U * np.abs(b)
    e_cy = e_a + e_b + U * np.abs(ref["cy"]) + TINY
    S = SECOND_ORDER
    bnd = dict(f=S * e_f, g=S * e_g + TINY, cy=S * e_cy)
    if bn_w is None:
        bnd["u"] = S * e_cy
        return ref, bnd
    cy, mean, var, invstd, xhat = ref["cy"], ref["mean"], ref["var"], ref["invstd"], ref["xhat"]
    bn_w = np.asarray(bn_w, F64)
    delta = gamma(R + C_RED) * np.abs(cy).max(0)
    e_mean = e_cy.mean(0) + delta
    sd = np.sqrt(var)
    e_var = (2.0 / R) * (np.abs(cy - mean) * e_cy).sum(0) + gamma(R + C_RED) * (sd + delta) ** 2 + 4 * delta * sd + 5 * delta ** 2 + TINY
    s = var + F64(F32(eps))
    e_inv = invstd * ((e_var + U * s) / (2 * s) + 2 * U)
    d = cy - mean
    e_d = e_cy + e_mean + U * np.abs(d)
    e_x = np.abs(d) * e_inv + invstd * e_d + U * np.abs(xhat) + TINY
    e_u = np.abs(bn_w) * e_x + U * np.abs(xhat * bn_w) + U * np.abs(ref["u"])
    bnd.update(mean=S * e_mean, var=S * e_var, invstd=S * e_inv, xhat=S * e_x, u=S * e_u)
    return ref, bnd


def running_bound(rm, rv, mean, var, e_mean, e_var, R, mom):
    """(new_rm, new_rv, e_rm, e_rv).  new = (1 - m) old + m x: o = 1 - m one rounding, two products, one sum; the cumulative factor
    1 / n one more rounding on m; x carries its own bound (the unbiased factor R / (R - 1): one division, one product):
      e = 2 U |(1 - m) old| + U |m| |old| + 2 U |m x| + |m| e(x) + U |new|      (the U |m| |old| term: the rounded m inside 1 - m)."""
    new_rm, new_rv = running(rm, rv, mean, var, R, mom)
    m = F64(F32(mom)) if mom >= 0 else 1.0 / -mom
    fac = R / (R - 1.0) if R > 1 else 1.0
    unb, e_unb = np.asarray(var, F64) * fac, (np.asarray(e_var, F64) + 2 * U * np.abs(var)) * fac

    def one(old, x, e_x, new):
        old, x = np.asarray(old, F64), np.asarray(x, F64)
        return SECOND_ORDER * (2 * U * np.abs((1 - m) * old) + U * abs(m) * np.abs(old) + 2 * U * np.abs(m * x) + abs(m) * e_x + U * np.abs(new)) + TINY

    return new_rm, new_rv, one(rm, mean, e_mean, new_rm), one(rv, unb, e_unb, new_rv)


# ----------------------------------------------------------------------------------------------------------------------
# backward step
# ----------------------------------------------------------------------------------------------------------------------
def bwd_step(dz_next, w_hh, dh_up, dc_next, u, xhat, f, g, c_prev, invstd, bn_w, shared, dt=F64, order="k", rpb=None, mut=None):
    """One backward step.  dz_next [R][G H] or None (d_z, or d_gates with separate gate weights, of step t + 1: dL/dh_t gets
    dz_next . W_hh), dh_up [R][H], dc_next [R][H] or None (dL/dc carried out of step t + 1), the forward's saved u / xhat / f / g /
    invstd of step t, c_prev (the membrane before the step) and bn_w (None: no BatchNorm).  Returns dict d_gates [R][2 H] (d pre_f | d
    pre_g), d_z [R][H] (shared gates: their sum; else None), dc_prev, k1 (= the step's part of d_bn_b), k2 (d_bn_w)."""
    u, f, g, c_prev, dh_up = (np.asarray(v, dt) for v in (u, f, g, c_prev, dh_up))
    R, H = u.shape
    one = dt(1.0)
    dh = dh_up
    if dz_next is not None:
        dh = dh + product(np.asarray(dz_next, dt), np.asarray(w_hh, dt).T, dt, order)
    au = np.abs(u)
    if mut == "tri_noclamp":
        tri = one - au
    elif mut == "tri_width2":
        tri = np.maximum(dt(0), one - au / dt(2))
    else:
        tri = np.maximum(dt(0), one - au)
    du = dh * tri
    if dc_next is not None:
        du = du + np.asarray(dc_next, dt)
    k1 = k2 = None
    if bn_w is None:
        dcy = du
    else:
        xhat, invstd, bn_w = (np.asarray(v, dt) for v in (xhat, invstd, bn_w))
        if dt is F64:
            k1, k2 = du.sum(0), (du * xhat).sum(0)
        else:
            k1, k2 = np.zeros(H, dt), np.zeros(H, dt)
            bl = _blocks(R, rpb)
            for lo, hi in bl:
                p1, p2 = _block_sum(du[lo:hi]), _block_sum(du[lo:hi], xhat[lo:hi])
                k1, k2 = (p1, p2) if len(bl) == 1 else (k1 + p1, k2 + p2)
        scale = bn_w * invstd / dt(R - 1 if mut == "scale_r1" else R)
        t1 = dt(R) * du
        t2 = t1 if mut == "no_sum_du" else t1 - k1
        dcy = scale * (t2 if mut == "no_xhat_term" else t2 - xhat * k2)
    cg = (g - c_prev) if mut == "cg_sign" else (c_prev - g)
    df = dcy * cg
    dpf = df * f * (one - f)
    dpg = dcy * (one - f)
    dc_prev = dcy if mut == "dc_no_f" else dcy * f
    d_z = (dpf if mut == "dz_dpf_only" else dpf + dpg) if shared else None
    return dict(d_gates=np.concatenate([dpf, dpg], 1), d_z=d_z, dc_prev=dc_prev, k1=k1, k2=k2)


def bwd_bound(dz_next, w_hh, dh_up, dc_next, u, xhat, f, g, c_prev, invstd, bn_w, shared):
    """(ref, bnd) for d_gates, d_z, dc_prev, k1, k2.  All inputs are exact (the device's own tensors).  First order, one U per rounding:
      rec    : gamma(nnz) sum |dz w|  (any order) ;  dh = up + rec : e(rec) + U |dh|
      tri = max(0, 1 - |u|) : U tri                                       (one rounding; rounding is monotone, so the clamp keeps its side)
      du = dh tri (+ dc) : tri e(dh) + |dh| e(tri) + U |dh tri| (+ U |du|)
      k1 = sum_r du : sum_r e(du) + gamma(R + C_RED) sum_r |du| ;  k2 = sum_r du xhat : sum_r |xhat| e(du) + gamma(R + C_RED) sum_r |du xhat|
               (row sums in any order and blocking: gamma(R - 1), the fma's one rounding per row is inside; C_RED as in fwd_bound)
      scale = gamma invstd / R : 2 U |scale|
      inner = R du - k1 - xhat k2, bounded by the magnitudes of its TERMS (it cancels): t1 = R du : R e(du) + U |t1| ;
               t2 = t1 - k1 : e(t1) + e(k1) + U |t2| ;  t3 = xhat k2 : |xhat| e(k2) + U |t3| ;  inner = t2 - t3 : e(t2) + e(t3) + U |inner|
      dc' = scale inner : |inner| e(scale) + |scale| e(inner) + U |dc'|     (no BatchNorm: dc' = du)
      cg = c_prev - g : U |cg| ;  df = dc' cg : |cg| e(dc') + |dc'| e(cg) + U |df| ;  o = 1 - f : U |o|
      dpf = (df f) o : |f o| e(df) + 3 U |dpf| ;  dpg = dc' o : |o| e(dc') + 2 U |dpg| ;  dc_prev = dc' f : |f| e(dc') + U |dc_prev|
      d_z = dpf + dpg : e(dpf) + e(dpg) + U |d_z|."""
    ref = bwd_step(dz_next, w_hh, dh_up, dc_next, u, xhat, f, g, c_prev, invstd, bn_w, shared)
    u, f, g, c_prev, dh_up = (np.asarray(v, F64) for v in (u, f, g, c_prev, dh_up))
    R, H = u.shape
    dh, e_dh = dh_up, np.zeros_like(u)
    if dz_next is not None:
        dzn, wt = np.asarray(dz_next, F64), np.asarray(w_hh, F64).T
        dh = dh_up + dzn @ wt.T
        e_dh = _product_bound(dzn, wt) + U * np.abs(dh)
    tri = np.maximum(0.0, 1.0 - np.abs(u))
    du = dh * tri
    e_du = tri * e_dh + np.abs(dh) * U * tri + U * np.abs(du)
    if dc_next is not None:
        du = du + np.asarray(dc_next, F64)
        e_du = e_du + U * np.abs(du)
    e_du = e_du + TINY
    S = SECOND_ORDER
    bnd = {}
    if bn_w is None:
        dcy, e_dcy = du, e_du
    else:
        xhat, invstd, bn_w = (np.asarray(v, F64) for v in (xhat, invstd, bn_w))
        k1, k2 = ref["k1"], ref["k2"]
        e_k1 = e_du.sum(0) + gamma(R + C_RED) * np.abs(du).sum(0)
        e_k2 = (np.abs(xhat) * e_du).sum(0) + gamma(R + C_RED) * np.abs(du * xhat).sum(0)
        scale = bn_w * invstd / R
        t1 = R * du
        t2, t3 = t1 - k1, xhat * k2
        inner = t2 - t3
        e_inner = R * e_du + U * np.abs(t1) + e_k1 + U * np.abs(t2) + np.abs(xhat) * e_k2 + U * np.abs(t3) + U * np.abs(inner)
        dcy = scale * inner
        e_dcy = np.abs(inner) * 2 * U * np.abs(scale) + np.abs(scale) * e_inner + U * np.abs(dcy) + TINY
        bnd.update(k1=S * e_k1 + TINY, k2=S * e_k2 + TINY)
    cg = c_prev - g
    df = dcy * cg
    e_df = np.abs(cg) * e_dcy + np.abs(dcy) * U * np.abs(cg) + U * np.abs(df)
    o = 1.0 - f
    dpf, dpg, dcp = df * f * o, dcy * o, dcy * f
    e_dpf = np.abs(f * o) * e_df + 3 * U * np.abs(dpf) + TINY
    e_dpg = np.abs(o) * e_dcy + 2 * U * np.abs(dpg) + TINY
    bnd["d_gates"] = S * np.concatenate([e_dpf, e_dpg], 1)
    bnd["dc_prev"] = S * (np.abs(f) * e_dcy + U * np.abs(dcp)) + TINY
    if shared:
        bnd["d_z"] = S * (e_dpf + e_dpg + U * np.abs(dpf + dpg)) + TINY
    return ref, bnd


# ----------------------------------------------------------------------------------------------------------------------
# mutants
# ----------------------------------------------------------------------------------------------------------------------
MUTANTS = {  # name: (where, what)
    "unbiased_norm": ("fwd", "unbiased variance inside the normalisation"),
    "biased_running": ("running", "biased running variance"),
    "eps_outside": ("fwd", "eps outside the square root"),
    "momentum_swapped": ("running", "momentum weights swapped"),
    "spike_gt": ("fwd", "spike > instead of >="),
    "bias_f_for_g": ("fwd", "cell-gate bias taken from bias[:H]"),
    "h_value": ("fwd", "h_prev used as a value instead of != 0"),
    "var_e2": ("fwd32", "variance as E[x^2] - mean^2 in the fp32 kernel form"),
    "tri_noclamp": ("bwd", "the triangle without its clamp"),
    "tri_width2": ("bwd", "a triangle of half-width 2"),
    "no_sum_du": ("bwd", "the BatchNorm backward without its sum du term"),
    "no_xhat_term": ("bwd", "the BatchNorm backward without its xhat sum(du xhat) term"),
    "dc_no_f": ("bwd", "dc_prev without the factor f"),
    "cg_sign": ("bwd", "the sign of (c_prev - g)"),
    "dz_dpf_only": ("bwd", "the shared d_z as dpf alone"),
    "scale_r1": ("bwd", "1 / (R - 1) in scale"),
}


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
def _base(rng, H, R, T, shared):
    """The random control every case starts from (fp32 values): bn_w in +-[0.5, 1.5], bn_b in +-0.3."""
    GH = H if shared else 2 * H
    sgn = lambda n: rng.choice([-1.0, 1.0], n)
    return dict(
        H=H, R=R, T=T, shared=shared,
        z=rng.standard_normal((T, R, GH)).astype(F32), bias=(0.5 * rng.standard_normal(2 * H)).astype(F32),
        w_hh=(rng.standard_normal((GH, H)) / np.sqrt(H)).astype(F32),
        bn_w=(sgn(H) * rng.uniform(0.5, 1.5, H)).astype(F32), bn_b=rng.uniform(-0.3, 0.3, H).astype(F32),
        eps=1e-5, momentum=0.1, n0=0, stats=True,
        rm0=(0.1 * rng.standard_normal(H)).astype(F32), rv0=rng.uniform(0.5, 1.5, H).astype(F32),
        h0=None, c0=None, dh_up=rng.standard_normal((T, R, H)).astype(F32), planted={}, holds=None)


def _isolate(p, cols):
    """The recurrent product of the planted neurons is zero: their pre-activations are z + bias alone."""
    H = p["H"]
    for c in cols:
        p["w_hh"][c] = 0
        if not p["shared"]:
            p["w_hh"][H + c] = 0


def _gcol(p, c):
    return c if p["shared"] else p["H"] + c


def case_control(rng, H, R, T, shared):
    return _base(rng, H, R, T, shared)


def case_tails(rng, H, R, T, shared):
    """Forget-gate bias of +-20, +-40, +-95 (fp32 exp overflows / underflows at 95): f is 0 or 1 on the device, e^-|x| away in fp64."""
    p = _base(rng, H, R, T, shared)
    vals = [20.0, -20.0, 40.0, -40.0, 95.0, -95.0]
    p["bias"][:6] = vals
    p["bn_b"][:6] = [0.25, -0.25, 0.25, -0.25, 0.25, -0.25]
    p["planted"] = dict(zip(("p20", "m20", "p40", "m40", "p95", "m95"), range(6)))

    def holds(st):  # st: a step's fp64 dict
        f = st["f"][:, :6]
        return bool((f[:, 0::2] > 1 - 1e-6).all() and (f[:, 1::2] < 1e-6).all())
    p["holds"] = holds
    return p


def case_constant(rng, H, R, T, shared):
    """Columns whose pre-normalisation membrane is the same in all rows at every step: var = 0, xhat = 0, u = bn_b = +-0.25."""
    p = _base(rng, H, R, T, shared)
    cols = [1, 2]
    _isolate(p, cols)
    for c in cols:
        p["z"][:, :, c] = p["z"][:, :1, c]
        p["z"][:, :, _gcol(p, c)] = p["z"][:, :1, _gcol(p, c)]
    p["bn_b"][1], p["bn_b"][2] = 0.25, -0.25
    p["planted"] = dict(const_p=1, const_m=2)
    p["holds"] = lambda st: bool((np.ptp(st["cy"][:, cols], axis=0) <= 4 * np.finfo(F64).eps * np.abs(st["cy"][:, cols]).max(0)).all())
    return p


def _pin_forget(p, c, zg):
    """Column c forgets everything (pre_f = -20: f = 2e-9), so its membrane is the cell gate's pre-activation zg [T][R] at every step.
    Shared gates add the same product z to both gates; the two biases differ, so z carries zg and the forget gate's bias takes it back."""
    H = p["H"]
    _isolate(p, [c])
    if p["shared"]:
        m = float(np.round(zg.mean()))
        p["z"][:, :, c] = zg.astype(F32)
        p["bias"][c], p["bias"][H + c] = -20.0 - m, 0.0
    else:
        p["z"][:, :, c] = 0
        p["z"][:, :, H + c] = zg.astype(F32)
        p["bias"][c], p["bias"][H + c] = -20.0, 0.0


def case_var_eps(rng, H, R, T, shared):
    """A column whose spread over the rows is about sqrt(eps): var ~ eps, the normalisation divides by sqrt(2 eps)."""
    p = _base(rng, H, R, T, shared)
    c = 3
    _pin_forget(p, c, 0.3 + np.sqrt(1e-5) * rng.standard_normal((T, R)))
    p["planted"] = dict(var_eps=c)
    p["holds"] = lambda st: bool(1e-5 / 4 < st["var"][c] < 4e-5) if R >= 16 else bool(st["var"][c] < 4e-5)
    return p


def case_offset(rng, H, R, T, shared):
    """A column of mean 3000 and spread 1: a sum-of-squares-minus-square-of-mean variance fails here."""
    p = _base(rng, H, R, T, shared)
    c = 4
    _pin_forget(p, c, 3000.0 + rng.standard_normal((T, R)))
    p["planted"] = dict(offset=c)
    p["holds"] = lambda st: bool(abs(st["mean"][c]) > 2900 and (R < 16 or 0.1 < st["var"][c] < 10))
    return p


def case_bn_scales(rng, H, R, T, shared):
    """bn_w in {0, 0, -1, 8, 2^-10}: with bn_w = 0 the membrane is bn_b exactly -- 0 (the spike must be 1: >=) and -0.25."""
    p = _base(rng, H, R, T, shared)
    p["bn_w"][5:10] = [0.0, 0.0, -1.0, 8.0, 2.0 ** -10]
    p["bn_b"][5], p["bn_b"][6] = 0.0, -0.25
    p["planted"] = dict(w0_b0=5, w0_bm=6, wm1=7, w8=8, wtiny=9)
    p["holds"] = lambda st: bool((st["u"][:, 5] == 0).all() and (st["u"][:, 6] == -0.25).all())
    return p


def _momenta(momentum, n0=0, eps=1e-5, stats=True):
    def case(rng, H, R, T, shared):
        p = _base(rng, H, R, T, shared)
        p.update(momentum=momentum, n0=n0, eps=eps, stats=stats)
        return p
    return case


def case_state(rng, H, R, T, shared):
    """A chunk start: h0 holds 0, 1, 0.5, -2 and -0.0 (anything != 0 is a spike, -0.0 is none), with its c0."""
    p = _base(rng, H, R, T, shared)
    p["h0"] = rng.choice(np.array([0.0, 1.0, 0.5, -2.0, -0.0], F32), (R, H)).astype(F32)
    p["c0"] = rng.standard_normal((R, H)).astype(F32)
    return p


def case_no_bn(rng, H, R, T, shared):
    p = _base(rng, H, R, T, shared)
    p.update(bn_w=None, bn_b=None, stats=False)
    return p


CASES = {
    "control": case_control, "tails": case_tails, "constant": case_constant, "var_eps": case_var_eps, "offset": case_offset,
    "bn_scales": case_bn_scales, "momenta_0": _momenta(0.0), "momenta_1": _momenta(1.0, eps=1e-3), "momenta_cum0": _momenta(None, 0),
    "momenta_cum7": _momenta(None, 7, eps=1e-3), "momenta_nostats": _momenta(0.1, stats=False), "state": case_state, "no_bn": case_no_bn,
}


def make_case(name, H, R, T, shared):
    """Seeded by (name, geometry): the same inputs on the host and on the device."""
    rng = np.random.default_rng(zlib.crc32(f"{name}/{H}/{R}/{T}/{int(shared)}".encode()))
    p = CASES[name](rng, H, R, T, shared)
    p["name"] = name
    return p


def mom_arg(p, t):
    """What a ONE-frame call of frame t is handed as `momentum` (the whole-sequence call: t = 0)."""
    return float(p["momentum"]) if p["momentum"] is not None else float(-(p["n0"] + t + 1))


U_EDGES = np.array([0.0, -0.0, 1.0, -1.0, 1 - 2.0 ** -24, -(1 - 2.0 ** -24), 1 + 2.0 ** -23, -(1 + 2.0 ** -23), 3.0, -3.0], F32)
F_EDGES = np.array([0.0, 1.0, 2.0 ** -30, 1 - 2.0 ** -24], F32)


def bwd_case(name, H, R, T, shared, use_bn=True):
    """Backward-only inputs: synthetic saved tensors (neither the kernels nor the reference need them to be consistent).  Returns
    (p, fwd) with fwd the dict of [T]-leading "saved" tensors u, xhat, f, g, invstd."""
    rng = np.random.default_rng(zlib.crc32(f"bwd/{name}/{H}/{R}/{T}/{int(shared)}".encode()))
    p = _base(rng, H, R, T, shared)
    p["name"] = "bwd_" + name
    if not use_bn:
        p.update(bn_w=None, bn_b=None, stats=False)
    fwd = dict(u=rng.standard_normal((T, R, H)).astype(F32), xhat=rng.standard_normal((T, R, H)).astype(F32),
               f=rng.random((T, R, H)).astype(F32), g=rng.standard_normal((T, R, H)).astype(F32),
               invstd=rng.uniform(0.5, 300.0, (T, H)).astype(F32))
    if name == "u_edges":  # the kinks of the triangle, in the first 8 columns
        fwd["u"][:, :, :8] = rng.choice(U_EDGES, (T, R, 8))
    elif name == "f_edges":
        fwd["f"][:, :, :8] = rng.choice(F_EDGES, (T, R, 8))
    elif name == "xhat_zero":
        fwd["xhat"][:, :, :4] = 0
    elif name == "all":
        fwd["u"][:, :, :8] = rng.choice(U_EDGES, (T, R, 8))
        fwd["f"][:, :, 4:12] = rng.choice(F_EDGES, (T, R, 8))
        fwd["xhat"][:, :, 10:14] = 0
    else:
        raise KeyError(name)
    if not use_bn:
        fwd["xhat"] = fwd["invstd"] = None
    return p, fwd


BWD_CASES = ("u_edges", "f_edges", "xhat_zero", "all")

# (H, R, shared): the row blocking of each, from train_geometry (target 160 workgroups: rb0 = 160 / (H / 16) row blocks asked for, rows
# per block = max(16, ceil(R / rb0)) rounded up to 16, RB = ceil(R / rpb)):
#   H = 16, 32, 48: rb0 = 160, 80, 53 -> rpb = 16 for every R <= 64: R = 2 -> one block of 2 rows (unbiased factor 2); 16 -> one full
#   block; 17 -> 16 + 1; 33 -> 16 + 16 + 1; 64 -> four full blocks.
#   H = 224 separate: rb0 = 11, ceil(130 / 11) = 12 -> rpb = 16, RB = 9, last block 2 rows.
#   H = 320 shared, R = 64: rb0 = 8, rpb = 16, RB = 4.
#   H = 320 shared, R = 513: rb0 = 8, ceil(513 / 8) = 65 -> rpb = 80 (> 64: each thread's fifth row takes the direct-load path), RB = 7,
#   last block 33 rows; backward LDS (3 . 80 . 16 + 16 . 36 + 324 . 96) . 4 = 142080 bytes <= 150 KiB, so no further split.  512 rows
#   still give 64 per block: 513 is the smallest R.
SMALL_GEOMETRIES = [(H, R, sh) for H in (16, 32, 48) for R in (2, 16, 17, 33, 64) for sh in (True, False)]
LARGE_GEOMETRIES = [(224, 130, False), (320, 64, True), (320, 513, True)]
GEOMETRIES = SMALL_GEOMETRIES + LARGE_GEOMETRIES
TS = (1, 2, 7)


def blocking(R, H, shared):
    """train_geometry restated (target 160): (row blocks, rows per block)."""
    G = 1 if shared else 2
    rb = max(1, 160 // (H // 16))
    while True:
        per = (max(16, -(-R // rb)) + 15) & ~15
        if (3 * per * 16 + 16 * 36 + (G * H + 4) * (16 + per)) * 4 <= 150 * 1024 or rb >= 16:
            return -(-R // per), per
        rb += 1


# ----------------------------------------------------------------------------------------------------------------------
# chains and their comparison
# ----------------------------------------------------------------------------------------------------------------------
def _zeros_state(p):
    R, H = p["R"], p["H"]
    h = p["h0"] if p["h0"] is not None else np.zeros((R, H), F32)
    c = p["c0"] if p["c0"] is not None else np.zeros((R, H), F32)
    return h, c


def sim_fwd(p, order="mfma4", rpb=None, dt=F32, mut=None):
    """A free-running chain of kernel-form steps (dt = F64: the fp64 chain): what a device returns -- [T]-leading spikes, u, xhat, f, g,
    invstd, and the running statistics after every step (rm, rv: [T][H])."""
    T, use_bn = p["T"], p["bn_w"] is not None
    h, c = _zeros_state(p)
    out = {k: [] for k in ("spikes", "u", "xhat", "f", "g", "invstd", "rm", "rv", "cy", "mean", "var")}
    rm, rv = (p["rm0"].astype(dt), p["rv0"].astype(dt)) if p["stats"] else (None, None)
    for t in range(T):
        st = fwd_step(p["z"][t], p["bias"], p["w_hh"], h, c, p["bn_w"], p["bn_b"], p["eps"], p["shared"], dt, order, rpb, mut)
        if use_bn and p["stats"]:
            rm, rv = running(rm, rv, st["mean"], st["var"], p["R"], mom_arg(p, t), dt)
        for k in ("spikes", "u", "xhat", "f", "g", "invstd", "cy", "mean", "var"):
            out[k].append(st[k])
        out["rm"].append(rm)
        out["rv"].append(rv)
        h, c = st["spikes"], st["u"]
    return {k: (np.stack(v) if v[0] is not None else None) for k, v in out.items()}


def free_chain(p):
    return sim_fwd(p, dt=F64)


def sim_bwd(p, fwd, order="mfma4", rpb=None, dt=F32):
    """Kernel-form backward chain over saved tensors `fwd`: d_gates, d_z, dc (dL/dc carried out of every step), and d_bn_w / d_bn_b
    after every step (dbw, dbb: [T][H], accumulated from step T - 1 down)."""
    T, R, H, sh, use_bn = p["T"], p["R"], p["H"], p["shared"], p["bn_w"] is not None
    out = dict(d_gates=np.zeros((T, R, 2 * H), dt), d_z=np.zeros((T, R, H), dt) if sh else None, dc=np.zeros((T, R, H), dt),
               dbw=np.zeros((T, H), dt) if use_bn else None, dbb=np.zeros((T, H), dt) if use_bn else None)
    dzn = dcn = None
    accw, accb = np.zeros(H, dt), np.zeros(H, dt)
    c0 = p["c0"] if p["c0"] is not None else np.zeros((R, H), F32)
    for t in range(T - 1, -1, -1):
        st = bwd_step(dzn, p["w_hh"], p["dh_up"][t], dcn, fwd["u"][t], fwd["xhat"][t] if use_bn else None, fwd["f"][t], fwd["g"][t],
                      fwd["u"][t - 1] if t else c0, fwd["invstd"][t] if use_bn else None, p["bn_w"], sh, dt, order, rpb)
        out["d_gates"][t], out["dc"][t] = st["d_gates"], st["dc_prev"]
        if sh:
            out["d_z"][t] = st["d_z"]
        if use_bn:
            accw, accb = accw + st["k2"], accb + st["k1"]
            out["dbw"][t], out["dbb"][t] = accw, accb
        dzn, dcn = (st["d_z"] if sh else st["d_gates"]), st["dc_prev"]
    return out


class Worst(dict):
    """Largest error / bound per output.  Anything that is not a number counts as infinitely far: a NaN or an infinity in what is
    judged (an element a kernel did not write, inf / inf in a tail) gives the ratio inf, and `see` returns what it stores, so that
    a caller's `> 1` fails on it."""

    def see(self, key, err, bnd):
        err = np.asarray(err, F64)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / bnd)
        r = np.where(np.isfinite(r), r, np.inf)
        r = float(np.max(r)) if np.size(r) else 0.0
        self[key] = max(self.get(key, 0.0), r)
        return r

    def line(self):
        return "  ".join(f"{k} {v:.3g}" for k, v in sorted(self.items()))


def asserted_mask(u_ref, e_u):
    """Where the reference decides the spike: beyond the bound, or where the bound is zero (bn_w = 0: the membrane is bn_b exactly)."""
    return (np.abs(u_ref) > e_u) | (e_u == 0)


def judge_fwd(p, dev, worst, mut=None, running_too=True):
    """Every step of a chain `dev` (sim_fwd's layout) against the teacher-forced fp64 step on dev's own carried state.  Returns a list of
    failure strings (empty: all within bounds, spikes as ruled) and adds error / bound figures to `worst`; worst['unasserted'] is the
    largest share of a step's spikes that the reference left open."""
    T, R, use_bn = p["T"], p["R"], p["bn_w"] is not None
    fails = []
    h, c = _zeros_state(p)
    rm, rv = (p["rm0"], p["rv0"]) if p["stats"] else (None, None)
    fm = mut if mut is not None and MUTANTS[mut][0] == "fwd" else None
    rmut = mut if mut is not None and MUTANTS[mut][0] == "running" else None
    for t in range(T):
        args = (p["z"][t], p["bias"], p["w_hh"], h, c, p["bn_w"], p["bn_b"], p["eps"], p["shared"])
        ref, bnd = fwd_bound(*args)
        if fm:
            ref = fwd_step(*args, mut=fm)
        for k in ("f", "g", "u") + (("xhat", "invstd") if use_bn else ()):
            if worst.see(k, np.abs(dev[k][t].astype(F64) - ref[k]), bnd[k]) > 1:
                fails.append(f"{p['name']} t={t} {k}")
        su = dev["u"][t]
        if not np.array_equal(dev["spikes"][t], (su >= 0).astype(su.dtype)):
            fails.append(f"{p['name']} t={t} spikes != (u >= 0)")
        m = asserted_mask(ref["u"], bnd["u"])
        if not np.array_equal(dev["spikes"][t][m] != 0, ref["spikes"][m] != 0):
            fails.append(f"{p['name']} t={t} spikes (asserted)")
        worst["unasserted"] = max(worst.get("unasserted", 0.0), 1.0 - float(m.mean()))
        if 1.0 - m.mean() > CAP:
            fails.append(f"{p['name']} t={t} unasserted share {1.0 - m.mean():.4f} > {CAP}")
        if use_bn and p["stats"] and running_too:
            if rmut:
                nrm, nrv = running(rm, rv, ref["mean"], ref["var"], R, mom_arg(p, t), mut=rmut)
                _, _, erm, erv = running_bound(rm, rv, ref["mean"], ref["var"], bnd["mean"], bnd["var"], R, mom_arg(p, t))
            else:
                nrm, nrv, erm, erv = running_bound(rm, rv, ref["mean"], ref["var"], bnd["mean"], bnd["var"], R, mom_arg(p, t))
            for k, new, e in (("rm", nrm, erm), ("rv", nrv, erv)):
                if worst.see({"rm": "running_mean", "rv": "running_var"}[k], np.abs(dev[k][t].astype(F64) - new), e) > 1:
                    fails.append(f"{p['name']} t={t} {k}")
            rm, rv = dev["rm"][t], dev["rv"][t]
        h, c = dev["spikes"][t], dev["u"][t]
    return fails


def judge_bwd(p, fwd, dev, worst, mut=None):
    """Every step of a backward chain `dev` (sim_bwd's layout) against the teacher-forced fp64 step: the saved tensors `fwd`, dev's own
    d_z (d_gates with separate gates) of step t + 1 and its own dL/dc carried out of step t + 1 as exact inputs."""
    T, R, H, sh, use_bn = p["T"], p["R"], p["H"], p["shared"], p["bn_w"] is not None
    fails = []
    c0 = p["c0"] if p["c0"] is not None else np.zeros((R, H), F32)
    for t in range(T - 1, -1, -1):
        last = t == T - 1
        args = (None if last else (dev["d_z"] if sh else dev["d_gates"])[t + 1], p["w_hh"], p["dh_up"][t], None if last else dev["dc"][t + 1],
                fwd["u"][t], fwd["xhat"][t] if use_bn else None, fwd["f"][t], fwd["g"][t], fwd["u"][t - 1] if t else c0,
                fwd["invstd"][t] if use_bn else None, p["bn_w"], sh)
        ref, bnd = bwd_bound(*args)
        if mut:
            ref = bwd_step(*args, mut=mut)
        pairs = [("d_gates", dev["d_gates"][t], ref["d_gates"], bnd["d_gates"]), ("dc_prev", dev["dc"][t], ref["dc_prev"], bnd["dc_prev"])]
        if sh:
            pairs.append(("d_z", dev["d_z"][t], ref["d_z"], bnd["d_z"]))
        if use_bn:  # the step's increment on what the device had accumulated before it: one more rounding
            for k, key, inc in (("dbw", "k2", "d_bn_w"), ("dbb", "k1", "d_bn_b")):
                before = np.zeros(H) if last else dev[k][t + 1].astype(F64)
                new = before + ref[key]
                pairs.append((inc, dev[k][t], new, bnd[key] + SECOND_ORDER * U * np.abs(new)))
        for k, d, r, e in pairs:
            if worst.see(k, np.abs(d.astype(F64) - r), e) > 1:
                fails.append(f"{p['name']} t={t} {k}")
    return fails
