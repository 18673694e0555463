"""Reference, tolerance and inputs for the GSN SCANS themselves at their arithmetic edges: sfsn_gsn_layer_scan (every kernel it selects),
sfsn_gsn_layer_scan_w16 / _split / _fused / _fused_x and sfsn_gsn_stack_scan / _x.

A helper module like frontback.py (not a conftest); numpy only.  Four parts:

* `quantise`: sfsn_w3_pack_bits restated on integers (the weights the device holds: weight quantisation is not part of the error; the
  spike products are exact -- an integer sum times a power-of-two dq), and `layer`: an fp64 GSN layer in eval mode with the semantics
  of include/sfsn.h ("GSN layer scan"), for the four forms of the input term: a given zin ("zin"), s_in . Wq_ih^T + bias_f ("spike":
  the fused scans, stack layers >= 1, the streaming hops' layers >= 1), x . W_ih^T + bias_f through the bf16 split ("x": fused-x, stack
  layer 0) and the same product in plain fp32, any order ("x32": the streaming hops' layer 0); shared and separate gate weights.
  test_scanref_host.py pins it to Oracle("f64").gsn_layer.
* the bound: a per-element tolerance on the post-BatchNorm membrane of every step, evaluated from fp64 reference quantities with
  u = 2^-24 and propagated along the chain.  Its derivation is in `layer`'s docstring.  No constant is fitted to what a kernel (or an
  emulation) returns.  Source of the hardware figures: neither the micro-architecture guide nor the HIP programming guide this project
  was written against states an accuracy for v_exp_f32 / v_rcp_f32 (they give issue costs only), so EXP2_ULP = RCP_ULP = 1 is the kernel
  comment's figure (sfsn_scan_dev.h, "the hardware exp2 / rcp (~1 ulp each)"); 1 ulp = 2u relative, as in frontback.py.
  EVERY fp32 rounding counts RND = 2u, the unit frontback.py gives the last rounding of a result, for the reason it gives there: a
  correctly rounded operation can use all of a 1u allowance, and the host test asks a correctly rounded fp32 evaluation to stay at
  <= 0.5.  Here that applies to every rounding and not only the last: a step's membrane passes through five roundings of its own size
  (the fma of pre_f, the gate's addition, the lerp's difference or products, its sum, the BatchNorm fma) that can all sit near 1u at
  once -- an fp32 evaluation with correctly rounded operations reaches up to 0.86 of a 1u-per-rounding count on this case table (the
  host test prints that figure beside the 2u one).  The unit is thus set by the host criterion and the emulation, not by first-order
  analysis alone: a strict count is half of every rounding term.  The terms that are NOT plain
  roundings keep their own figures: EXP2_ULP, RCP_ULP, the bf16 split's dropped products, the floor, and the
  propagated e_{t-1}.  Every bound is multiplied by SECOND_ORDER for the dropped O(u^2) terms.
* `compare`: the causal rule of parity.py with the derived bound in place of the fixed TAU.
* `fp32_kernel_form` / `fp32_reference_form`: fp32 numpy emulations of the two evaluation orders of the lerp (fma through fp64), with
  `mut` selecting a deliberately wrong variant -- used by the host test only -- and the seeded case table CASES.

Domain: |pre| <= 128, finite inputs, no denormals posed (a forget gate below 2^-126 may come out as 0: the bound carries that floor).
"""
import zlib

import numpy as np

U = 2.0 ** -24
QMAX = 127 * 65536 + 127 * 256 + 127  # 8355711, sfsn_pack.cpp: the largest |q| of three balanced base-256 digits
Q16MAX = 32639
SECOND_ORDER = 1.001
EXP2_ULP = 1  # sfsn_scan_dev.h's comment (no guide figure exists): a kernel outside it is a finding, not a constant to widen
RCP_ULP = 1
RND = 2 * U  # one fp32 rounding, counted as 1 ulp (see the module docstring)
TINY = 2.0 ** -126  # results below the normal range are not posed: a flushed or overflowed tail of the sigmoid is off by at most this
F32 = np.float32
LOG2E = F32(1.44269504088896341)  # the kernels' literal


# ----------------------------------------------------------------------------------------------------------------------
# weights as the device holds them
# ----------------------------------------------------------------------------------------------------------------------
def quantise(w, bits=24):
    """sfsn_w3_pack_bits on integers: fp32 [N][K] -> (q int64 [N][K], dq float64 [N]), W~ = q dq.  The row scale is the smallest power of
    two 2^e with amax 2^(23 - e) <= QMAX; q = rint(w 2^(23 - e)) (nearest even); bits = 16: q = 256 clip(rint(w 2^(15 - e)), +-32639)."""
    w = np.asarray(w, np.float64)
    amax = np.abs(w).max(1)
    m, ex = np.frexp(amax)  # amax = m 2^ex, m in [0.5, 1):  m 2^(ex + 23 - e) <= QMAX  <=>  e >= ex + (m > QMAX 2^-23)
    e = np.where(amax > 0, ex + (m > QMAX * 2.0 ** -23), 0).astype(np.int64)
    assert (e[amax > 0] - 23 >= -126).all() and (e <= 100).all(), "dq must stay a normal fp32 number"
    if bits == 16:
        q = 256 * np.clip(np.rint(np.ldexp(w, (15 - e)[:, None])), -Q16MAX, Q16MAX).astype(np.int64)
    else:
        q = np.rint(np.ldexp(w, (23 - e)[:, None])).astype(np.int64)
    return q, np.ldexp(1.0, e - 23)


def digits(q):
    """Balanced base-256 digits (d0, d1, d2), each in [-128, 127], of q = d2 65536 + d1 256 + d0."""
    q = np.asarray(q, np.int64)
    d0 = ((q + 128) & 255) - 128
    q1 = (q - d0) >> 8
    d1 = ((q1 + 128) & 255) - 128
    return d0, d1, (q1 - d1) >> 8


def dequantise(w, bits=24):
    q, dq = quantise(w, bits)
    return (q * dq[:, None]).astype(F32)  # exact: |q| < 2^23


def _isum(h01, q):
    """Exact integer sums h . q^T (0/1 times |q| < 2^23, at most 320 terms: exact in fp64, which has a BLAS)."""
    return np.rint(h01.astype(np.float64) @ q.T.astype(np.float64)).astype(np.int64)


def _bf16(x):
    b = np.ascontiguousarray(x, F32).view(np.uint32)
    return ((b + (((b >> 16) & 1) + 0x7FFF)) & np.uint32(0xFFFF0000)).view(F32)


def _fma(a, b, c):
    """fp32 fma through fp64: the product of two fp32 numbers is exact in fp64."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


# ----------------------------------------------------------------------------------------------------------------------
# the layer: fp64 reference with its bound, and the fp32 emulations
# ----------------------------------------------------------------------------------------------------------------------
def _input_term(p, mode, mut, quant, rnd):
    """(z [T][R][G H], its error bound or None, largest |integer sum| of the input product)."""
    H, kind, bias = p["H"], p["kind"], p["bias"]
    f64 = mode == "f64"
    if mut == "no_db" and not p["shared"] and kind != "zin":  # separate gates: the cell gate's product takes the forget gate's bias
        bias = np.concatenate([bias[:H], bias[:H]])
    if kind == "zin":
        z = p["zin"].astype(np.float64 if f64 else F32)
        ez, smax = np.zeros(z.shape), 0
    elif kind == "spike":
        s = p["s_in"][:, :, :H].astype(np.float64)
        GH = p["W_ih"].shape[0]  # H (shared gates) or 2H (separate: the cell gate's rows follow the forget gate's)
        if quant:
            q, dq = quantise(p["W_ih"], p.get("bits", 24))
            if mut == "drop_d0":
                q = q - digits(q)[0]
            S = np.rint(s @ q.T.astype(np.float64)).astype(np.int64)
            if mut == "wrap31":
                S = ((S + 2 ** 30) % 2 ** 31) - 2 ** 30
            smax = int(np.abs(S).max())
            if f64:
                z = S * dq + bias[:GH].astype(np.float64)
                ez = rnd * np.abs(S * dq) * (np.abs(S) >= 2 ** 24) + rnd * np.abs(z)
            else:
                z, ez = _fma(S.astype(F32), dq.astype(F32), bias[:GH]), None
        else:
            z, ez, smax = s @ p["W_ih"].astype(np.float64).T + bias[:GH].astype(np.float64), None, 0
    elif kind == "x32":
        x, w = p["x"], p["W_ih"]
        K, GH = x.shape[-1], w.shape[0]
        smax = 0
        if f64:
            z = x.astype(np.float64) @ w.astype(np.float64).T + bias[:GH].astype(np.float64)
            a = np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)).T + np.abs(bias[:GH].astype(np.float64))
            ez = rnd * (K + 1) * a
        elif mode == "kernel":  # sfsn_hop.hip: chunks of 16 columns dealt to four accumulators, ((a0 + a1) + (a2 + a3)) + b
            acc = [np.zeros(x.shape[:2] + (GH,), F32) for _ in range(4)]
            for k in range(K):
                acc[(k // 16) & 3] = _fma(x[:, :, k, None], w[None, None, :, k], acc[(k // 16) & 3])
            z, ez = (((acc[0] + acc[1]) + (acc[2] + acc[3])) + bias[:GH]).astype(F32), None
        else:  # fbh_input_role: one fmaf chain in k order, then the bias
            acc = np.zeros(x.shape[:2] + (GH,), F32)
            for k in range(K):
                acc = _fma(x[:, :, k, None], w[None, None, :, k], acc)
            z, ez = (acc + bias[:GH]).astype(F32), None
    else:
        assert kind == "x", kind
        x, w = p["x"], p["W_ih"]
        K = x.shape[-1]
        smax = 0
        if f64:
            z = x.astype(np.float64) @ w.astype(np.float64).T + bias[:H].astype(np.float64)
            a = np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)).T + np.abs(bias[:H].astype(np.float64))
            ez = (rnd * ((K + 2) * (1 + 2.0 ** -7) + 5 * K * 2.0 ** -7 * 1.01) + 2.0 ** -23 * (1 + 2.0 ** -8)) * a
        else:  # the bf16 three-way split: six leading piece products, fp32 accumulation
            x1 = _bf16(x); x2 = _bf16(x - x1); x3 = _bf16(x - x1 - x2)
            w1 = _bf16(w); w2 = _bf16(w - w1); w3 = _bf16(w - w1 - w2)
            acc = np.zeros(x.shape[:2] + (H,), F32)
            for a_, b_ in ((x3, w1), (x2, w2), (x1, w3), (x2, w1), (x1, w2), (x1, w1)):
                acc = acc + (a_ @ b_.T).astype(F32)
            z, ez = (acc + bias[:H]).astype(F32), None
    if mut == "bf16_in":
        z = _bf16(z)
    return z, ez, smax


def _run(p, mode="f64", mut=None, quant=True, rnd=RND):
    H, R, T, shared = p["H"], p["R"], p["T"], p["shared"]
    f64 = mode == "f64"
    dt = np.float64 if f64 else F32
    bias, alpha, beta = p["bias"].astype(dt), p["alpha"].astype(dt), p["beta"].astype(dt)
    if quant:
        q, dq = quantise(p["W_hh"], p.get("bits", 24))
        if mut == "drop_d0":
            q = q - digits(q)[0]
    else:
        assert f64
        whh = p["W_hh"].astype(np.float64)
    z, ez, smax = _input_term(p, mode, mut, quant, rnd)
    if mut == "abs_alpha":
        alpha = np.abs(alpha)
    db = bias[H:] - bias[:H]  # (fp32 modes: one fp32 subtraction, as the kernels form it)
    if mut == "no_db":
        db = np.zeros_like(db)
    h, c = p["h0"] > 0.5, p["c0"].astype(dt)
    ec = np.zeros((R, H))
    spk, ys, tols = np.zeros((T, R, H), bool), np.zeros((T, R, H), dt), np.zeros((T, R, H))
    one = dt(1)
    for t in range(T):
        if quant:
            S = _isum(h, q)
            if mut == "wrap31":
                S = ((S + 2 ** 30) % 2 ** 31) - 2 ** 30
            smax = max(smax, int(np.abs(S).max()))
        if f64:
            rec = S * dq if quant else h.astype(np.float64) @ whh.T
            pre = z[t] + rec
            e_pre = rnd * np.abs(pre) + (ez[t] if ez is not None else 0.0)
            if quant:
                e_pre = e_pre + rnd * np.abs(rec) * (np.abs(S) >= 2 ** 24)
            pf, epf = pre[:, :H], e_pre[:, :H]
            if shared:
                pg = pf + db
                eg = epf + rnd * np.abs(db) + rnd * np.abs(pg)
            else:
                pg, eg = pre[:, H:], e_pre[:, H:]
            with np.errstate(over="ignore"):
                f = 1.0 / (1.0 + np.exp(-pf))
            m = f * c + (1.0 - f) * pg
            y = m * alpha + beta
            df = f * ((1.0 - f) * (2 * rnd * np.abs(pf) + epf + 2 * U * EXP2_ULP) + rnd + 2 * U * RCP_ULP) + TINY
            d = np.abs(c - pg)
            em = df * d + f * ec + (1.0 - f) * eg + rnd * (np.maximum(f * d, f * np.abs(c) + 2 * (1.0 - f) * np.abs(pg)) + np.abs(m))
            tol = (np.abs(alpha) * em + rnd * np.abs(y)) * SECOND_ORDER
            tols[t], ec = tol, tol
        else:
            pre = _fma(S.astype(F32), dq.astype(F32), z[t])
            pf = pre[:, :H]
            pg = (pf + db).astype(F32) if shared else pre[:, H:]
            with np.errstate(over="ignore"):
                f = one / (one + np.exp2(pf * -LOG2E))
            m = _fma(f, c - pg, pg) if mode == "kernel" else f * c + (one - f) * pg
            y = _fma(m, alpha, beta)
        s = y > 0 if mut == "gt" else y >= 0
        spk[t], ys[t] = s, y
        h, c = s, y
    return dict(spk=spk, y=ys, tol=tols if f64 else None, smax=smax)


def layer(p, quant=True, rnd=RND):
    """The fp64 reference of one layer call on case `p` and the bound of its post-BatchNorm membranes: dict(spk [T][R][H] bool,
    y [T][R][H] fp64, tol [T][R][H], smax: the largest |integer sum| met).  quant = False takes the weights as given (the oracle pin).
    rnd: what one fp32 rounding counts; the tests use RND = 2u, and the host test prints what a strict 1u count (rnd = U) would leave.

    Per step and neuron (sfsn.h): pre_f = z + S dq (S = sum of the spiking columns' integers), pre_g = pre_f + (b_g - b_f) or its own
    product, f = 1 / (1 + exp(-pre_f)), m = f c + (1 - f) pre_g, y = m alpha + beta, spike = (y >= 0), carry (spike, y).

    Bound (first order in u; below "u" per fp32 rounding stands for RND = 2u, see the module docstring):
      input term      "zin": exact.  "spike": z = fma(float(S_in), dq, b): the conversion rounds when |S_in| >= 2^24 (u |S_in dq|; dq is a
                      power of two, the product is exact) and the fma once: e_z = u |S_in dq| [|S_in| >= 2^24] + u |z|.
                      "x": the three-way bf16 split keeps six of nine piece products, each exact in fp32, and drops x2 w3 + x3 w2 +
                      x3 w3 <= 2^-23 (1 + 2^-8) |x||w| (|x2| <= 2^-8 |x|, |x3| <= 2^-16 |x|).  The kernels keep two accumulators
                      (sfsn_kernels.hip, "layer-0 input product on the bf16 matrix cores"): the K leading products x1 w1 in one -- K
                      additions on partial sums <= (1 + 2^-7) sum |x||w| --, the 5 K small ones in the other -- partial sums <= 2^-7 1.01
                      sum |x||w| --, then (hi + lo) + b, two more: u [(K + 2)(1 + 2^-7) + 5 K 2^-7 1.01] (sum |x||w| + |b|), frontback.linear's
                      gamma(K + 2) with the second accumulator counted (an addition inside the matrix core counts like any other).
                      "x32" (the streaming hops' layer 0): a plain fp32 product in an order this bound does not know.  K products and the
                      bias are K + 1 terms; summing them in ANY order is K additions, so no term passes through more than K of them,
                      and a product that is rounded on its own (not fused) adds one: at most K + 1 roundings on any term, each
                      relative to a partial sum <= sum |x||w| + |b|: e_z = (K + 1) u (sum |x||w| + |b|).  The two paths it must cover
                      stay inside it.  sfsn_hop.hip: chunk c of 16 columns goes to accumulator c mod 4 inside mfma_f32_16x16x4f32 (the
                      order and fusing of the four products of one instruction are the matrix core's own), then ((a0 + a1) + (a2 +
                      a3)) + b: a term sees its product, at most 16 ceil(K / 64) additions in its accumulator (the
                      padding columns add zeros, exactly), two that combine the four and the bias's: 1 + 16 ceil(K / 64) + 3 <= K + 1
                      from K = 19 on (the smallest K a model here has is 38).  sfsn_fullband_hop.hip's fbh_input_role: one fmaf chain in k order from
                      zero, then + b: term k passes through K - k fused roundings and the bias addition, at most K + 1.
      pre_f           e_pre = e_z + u |S dq| [|S| >= 2^24] (the recombination's one rounding) + u |pre_f| (the fma).
      pre_g           shared: e_g = e_pre + u |b_g - b_f| (the fp32 difference) + u |pre_g| (the addition); separate: as pre_f.
      sigmoid         a = pre_f * (-log2 e): the literal and the product round (2u |a|); E = exp2(a) is off by ln 2 times the argument's
                      error -- relative 2u |pre_f| + e_pre -- plus EXP2_ULP ulp; 1 + E rounds (1u), the reciprocal RCP_ULP ulp; with
                      df / f = (1 - f) dE / E + ...:  |df| <= f [(1 - f)(2u |pre_f| + e_pre + 2u EXP2_ULP) + (1 + 2 RCP_ULP) u] + 2^-126
                      (the floor: exp2 overflows below pre_f ~ -88.7 and the reciprocal of a huge number may be flushed: f comes out
                      as 0 where it is below 2^-126).  Above pre_f ~ 17, 1 + E rounds to 1 and f to 1: inside the 1u of the addition.
      lerp            both orders.  fma(f, c - g, g): the difference rounds (u f |c - g|) and the fma (u |m|); f c + (1 - f) g: u f |c| +
                      2u (1 - f) |g| + u |m|; the larger of the two is taken.  Inputs: |df| |c - g| + f e_c + (1 - f) e_g.
      BatchNorm       tol = |alpha| e_m + u |y|, and e_c of the next step is this tol:
                      e_t = |alpha| f e_{t-1} + the step's own terms."""
    return _run(p, "f64", None, quant, rnd)


def fp32_kernel_form(p, mut=None):
    """fp32 emulation of the kernels' order: rec = float(S) (exact sum, one rounding), pre = fma(rec, dq, z), f = 1 / (1 + exp2(-log2e pre)),
    m = fma(f, c - g, g), y = fma(m, alpha, beta).  exp2 and the division are numpy's (correctly rounded division)."""
    return _run(p, "kernel", mut)


def fp32_reference_form(p, mut=None):
    """The same with the reference's lerp, four separately rounded operations: m = f c + (1 - f) g."""
    return _run(p, "reference", mut)


MUTANTS = ["gt", "no_db", "wrap31", "abs_alpha", "bf16_in", "drop_d0"]  # (no_db with separate gates: the cell gate takes the forget gate's bias)


# ----------------------------------------------------------------------------------------------------------------------
# comparison
# ----------------------------------------------------------------------------------------------------------------------
def worst(y, ref, tol):
    """max |y - ref| / tol with 0 / 0 = 0 and anything / 0 = inf; NaN anywhere is inf."""
    err = np.abs(np.asarray(y, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / tol)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


class Result:
    def __init__(self, ok, why, unasserted, ratio, t_valid):
        self.ok, self.why, self.unasserted, self.ratio, self.t_valid = ok, why, unasserted, ratio, t_valid

    def __repr__(self):
        return f"Result(ok={self.ok}, why={self.why!r}, unasserted={self.unasserted:.4f}, ratio={self.ratio:.3f})"


def compare(spk, ref, y=None, t_up=None):
    """The causal rule of parity.py with the derived bound.  spk [T][R][H] (0 / 1), ref = layer(...)'s dict, y the membranes if the
    entry point has them, t_up [R] the frames of each row whose INPUT agreed (a stack's layer >= 1: t_valid of the layer below).
      * a spike is asserted wherever |y_ref| > tol -- or tol == 0: a membrane that is exact in every evaluation order (the `threshold`
        case's zeros) is decidable by construction;
      * a row's first disagreement is accepted only on neurons that are not asserted; after that frame the row is not asserted;
      * membranes are asserted within tol up to and including that frame (its state going in was still the reference's).
    Returns Result(ok, why, unasserted: the share of (t, r, j) not asserted, ratio: worst membrane error / tol, t_valid [R])."""
    rs, ry, tol = ref["spk"], ref["y"], ref["tol"]
    T, R, H = rs.shape
    spk = np.asarray(spk) > 0.5
    assert spk.shape == rs.shape, (spk.shape, rs.shape)
    dec = (np.abs(ry) > tol) | (tol == 0)
    diff = spk != rs
    anyd = diff.any(-1)
    first = np.where(anyd.any(0), anyd.argmax(0), T)
    t_up = np.full(R, T) if t_up is None else np.asarray(t_up)
    tt = np.arange(T)[:, None]
    live = (tt <= first[None]) & (tt < t_up[None])
    asserted = dec & live[:, :, None]
    bad = diff & asserted
    ok, why = True, ""
    if bad.any():
        t, r, j = (int(v[0]) for v in np.nonzero(bad))
        ok, why = False, f"wrong spike at t={t} row={r} neuron={j}: reference membrane {ry[t, r, j]:.6g}, tolerance {tol[t, r, j]:.3g} ({int(bad.sum())} in all)"
    ratio = 0.0
    if y is not None:
        ratio = worst(np.asarray(y)[live], ry[live], tol[live])
        if ratio > 1.0 and ok:
            ok, why = False, f"membrane error {ratio:.3g} x the tolerance"
    return Result(ok, why, float(1.0 - asserted.mean()), ratio, np.minimum(first, t_up))


def final_ratio(cT, ref, t_valid):
    """Worst error / tol of the final membrane state on the rows that never diverged."""
    T = ref["y"].shape[0]
    rows = np.asarray(t_valid) >= T
    return worst(np.asarray(cT)[rows], ref["y"][T - 1][rows], ref["tol"][T - 1][rows])


def prefix(ref, T, R):
    """The reference of the first T frames of the first R rows (rows are independent, the recurrence is causal)."""
    return dict(spk=ref["spk"][:T, :R], y=ref["y"][:T, :R], tol=ref["tol"][:T, :R], smax=ref["smax"])


def crop(p, T, R):
    """Case p cut to its first T frames and R rows."""
    o = dict(p, T=T, R=R, h0=p["h0"][:R], c0=p["c0"][:R])
    for k in ("zin", "s_in", "x"):
        if k in p:
            o[k] = np.ascontiguousarray(p[k][:T, :R])
    return o


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
def _base(rng, H, R, T, shared, kind, I, p_in=0.25):
    """Today's mild distribution: refweights._cell's weights and BatchNorm statistics, standard-normal inputs."""
    G = 1 if shared else 2
    s = 1.0 / np.sqrt(H)
    p = dict(H=H, R=R, T=T, shared=shared, kind=kind, bits=24)
    p["W_hh"] = rng.uniform(-s, s, (G * H, H)).astype(F32)
    p["bias"] = rng.uniform(-s, s, 2 * H).astype(F32)
    w, b = rng.normal(1.0, 0.2, H), rng.normal(0.0, 0.3, H)
    rm, rv = rng.normal(0.0, 0.5, H), rng.uniform(0.3, 1.5, H)
    p["alpha"] = (w / np.sqrt(rv + 1e-5)).astype(F32)
    p["beta"] = (b - rm * p["alpha"]).astype(F32)
    p["h0"] = (rng.random((R, H)) > 0.5).astype(F32)
    p["c0"] = rng.standard_normal((R, H)).astype(F32)
    if kind == "zin":
        xin, wi = rng.standard_normal((T, R, I)), rng.uniform(-s, s, (G * H, I))
        p["zin"] = (xin @ wi.T + p["bias"][:G * H]).astype(F32)
    elif kind == "spike":
        p["s_in"] = (rng.random((T, R, H)) < p_in).astype(np.int8)
        p["W_ih"] = rng.uniform(-s, s, (G * H, H)).astype(F32)
    elif kind == "x32":
        p["x"] = rng.standard_normal((T, R, I)).astype(F32)
        p["W_ih"] = rng.uniform(-s, s, (G * H, I)).astype(F32)
    else:
        assert shared and kind == "x"
        p["x"] = rng.standard_normal((T, R, I)).astype(F32)
        p["W_ih"] = rng.uniform(-s, s, (H, I)).astype(F32)
    return p


def _pin_input(p, cols, value):
    """Neurons `cols`: the forget gate's input term becomes exactly `value` ([len(cols)] or scalar) at every frame and row; the cell
    gate's keeps its bias difference (shared) / becomes `value` too (separate)."""
    H, cols = p["H"], np.asarray(cols)
    value = np.broadcast_to(np.asarray(value, F32), cols.shape)
    if p["kind"] == "zin":
        p["zin"][:, :, cols] = value
        if not p["shared"]:
            p["zin"][:, :, H + cols] = value
    else:
        d = p["bias"][H + cols] - p["bias"][cols] if p["shared"] else 0.0
        p["W_ih"][cols] = 0
        if not p["shared"]:
            p["W_ih"][H + cols] = 0
        p["bias"][cols] = value
        p["bias"][H + cols] = value + d


def _control(rng, H, R, T, shared, kind, I, bits):
    return _base(rng, H, R, T, shared, kind, I)


def _sat_rows(N, K, bits, shift):
    """Every entry of row n at sign_n qmax dq_n: all digits +-127 (24 bits) / +-32639 256 (16 bits); dq_n 2^-23 = 2^(shift + n % 7)."""
    n = np.arange(N)
    top = QMAX if bits == 24 else Q16MAX * 256
    row = np.where(n % 2 == 0, 1.0, -1.0) * top * 2.0 ** -23 * 2.0 ** (shift + n % 7)
    return np.repeat(row[:, None], K, 1).astype(F32)


def _saturated(rng, H, R, T, shared, kind, I, bits):
    p = _base(rng, H, R, T, shared, kind, I)
    G = 1 if shared else 2
    p["W_hh"] = _sat_rows(G * H, H, bits, -8)  # |rec| <= K 0.9961 / 4 < 80 for K = 320
    p["h0"] = np.ones((R, H), F32)
    p["alpha"] = rng.uniform(0.5, 1.5, H).astype(F32)
    p["beta"] = np.full(H, 200.0, F32)  # m >= min(c, g) >= -(80 + 40 + 5): y >= 200 - 1.5 125 > 0: every neuron fires at every frame
    if kind == "spike":
        p["s_in"] = np.ones((T, R, H), np.int8)
        p["W_ih"] = _sat_rows(G * H, H, bits, -9)  # half the recurrent scale: |pre| < 120
    return p


def _digit_extremes(rng, H, R, T, shared, kind, I, bits):
    p = _base(rng, H, R, T, shared, kind, I, p_in=0.5)

    def corner(N, K):
        c = np.array([-128, -1, 0, 127])
        q = np.zeros((N, K), np.int64)
        todo = np.ones((N, K), bool)
        while todo.any():  # rejection: |q| <= QMAX
            d = c[rng.integers(0, 4, (3,) + q.shape)]
            cand = d[2] * 65536 + d[1] * 256 + d[0]
            take = todo & (np.abs(cand) <= QMAX)
            q[take] = cand[take]
            todo &= ~take
        q[:, 0] = 127 * 65536 + c[rng.integers(0, 4, N)] * 256 + c[rng.integers(0, 4, N)]  # pins the row scale: |q| > QMAX / 2
        return (q * 2.0 ** -28).astype(F32)  # dq = 2^-28: values up to 2^-5

    p["W_hh"] = corner((1 if shared else 2) * H, H)
    if kind == "spike":
        p["W_ih"] = corner((1 if shared else 2) * H, H)
    return p


def _tails(rng, H, R, T, shared, kind, I, bits):
    p = _base(rng, H, R, T, shared, kind, I)
    p["c0"] = rng.uniform(-5, 5, (R, H)).astype(F32)
    if kind == "zin":
        p["zin"][:, :, :H] = rng.uniform(-120, 120, (T, R, H))
        if not shared:
            p["zin"][:, :, H:] = rng.uniform(-100, 100, (T, R, H))
    else:
        _pin_input(p, np.arange(H), 0.0)  # keeps the bias difference ...
        w = p["W_ih"]
        s = 1.0 / np.sqrt(H)
        p["W_ih"] = rng.uniform(-s, s, w.shape).astype(F32)  # ... and the product
        bf = rng.uniform(-115, 115, H).astype(F32)
        p["bias"][H:] = p["bias"][H:] + bf if shared else rng.uniform(-100, 100, H).astype(F32)  # (separate: a cell gate of its own)
        p["bias"][:H] = bf
    return p


def _scaled_rows(rng, N, K, zero_row):
    """Row maxima from 2^-100 to 2^6; rows above 2^-2 keep two entries, above 2^3 one (|product| <= 64); one all-zero row."""
    e = np.round(np.linspace(-100, 6, N)).astype(np.int64)
    rng.shuffle(e)
    w = rng.uniform(-1, 1, (N, K))
    for n in np.nonzero(e > -2)[0]:
        keep = rng.choice(K, 1 if e[n] > 3 else 2, replace=False)
        row = np.zeros(K)
        row[keep] = w[n, keep]
        w[n] = row
    k0 = np.abs(w).argmax(1)
    w[np.arange(N), k0] = rng.uniform(0.5, 1.0, N) * np.where(rng.random(N) < 0.5, -1.0, 1.0)  # the row maximum in (2^(e-1), 2^e]
    w = np.where(np.abs(w) > np.abs(w[np.arange(N), k0])[:, None], 0.0, w) * 2.0 ** e[:, None]
    w[zero_row] = 0
    return w.astype(F32)


def _row_scales(rng, H, R, T, shared, kind, I, bits):
    p = _base(rng, H, R, T, shared, kind, I)
    p["W_hh"] = _scaled_rows(rng, (1 if shared else 2) * H, H, 5)
    if kind == "spike":
        p["W_ih"] = _scaled_rows(rng, (1 if shared else 2) * H, H, 7)
    return p


def _row_scales_zero(rng, H, R, T, shared, kind, I, bits):
    p = _base(rng, H, R, T, shared, kind, I)
    p["W_hh"] = np.zeros_like(p["W_hh"])
    if kind == "spike":
        p["W_ih"] = np.zeros_like(p["W_ih"])
    return p


def threshold_groups(H):
    """Neuron indices of the three groups of `threshold` (spread over the 16-neuron tiles): exact zeros, tiny shift, -0.0 shift."""
    idx = (np.arange(20) * 11 + 3) % H
    assert len(set(idx.tolist())) == 20
    return idx[:8], idx[8:16], idx[16:]


def _threshold(rng, H, R, T, shared, kind, I, bits):
    """Exact zeros: zero recurrent row(s), zero input term, equal gate biases, c0 = +-0.0, shift +0.0, scale of either sign: f = 1/2,
    m = fma(1/2, +-0, 0) = 0, y = +-0 in every order and at every frame: spikes.  Tiny shift: the same with shift +-1e-30 and a positive
    scale: y_0 = shift exactly, later frames carry c = O(1e-30) of the shift's sign (y_t = shift (1 + alpha f + ...)): spike iff the
    shift is positive, decidable at u 1e-30.  -0.0 shift: y = +-0: spikes."""
    p = _base(rng, H, R, T, shared, kind, I)
    g1, g2, g3 = threshold_groups(H)
    allg = np.concatenate([g1, g2, g3])
    p["W_hh"][allg] = 0
    if not shared:
        p["W_hh"][H + allg] = 0
    p["bias"][allg] = 0
    p["bias"][H + allg] = 0
    _pin_input(p, allg, 0.0)
    sign = np.where((np.arange(R)[:, None] + np.arange(len(allg))[None, :]) % 2 == 0, 0.0, -0.0).astype(F32)
    p["c0"][:, allg] = sign
    p["beta"][g1] = 0.0
    p["alpha"][g1[::2]] = -np.abs(p["alpha"][g1[::2]])
    p["beta"][g2] = np.where(np.arange(len(g2)) % 2 == 0, 1.0, -1.0).astype(F32) * F32(1e-30)
    p["alpha"][g2] = np.abs(p["alpha"][g2])
    p["beta"][g3] = -0.0
    p["alpha"][g3[::2]] = -np.abs(p["alpha"][g3[::2]])
    return p


def _bn_signs(rng, H, R, T, shared, kind, I, bits):
    p = _base(rng, H, R, T, shared, kind, I)
    j = np.arange(H)
    p["alpha"][j % 3 == 0] *= -1
    p["alpha"][j % 29 == 4] = 0.0  # membrane = shift
    p["alpha"][j % 31 == 7] = 8.0
    return p


CASES = dict(control=_control, saturated=_saturated, digit_extremes=_digit_extremes, tails=_tails, row_scales=_row_scales,
             row_scales_zero=_row_scales_zero, threshold=_threshold, bn_signs=_bn_signs)

T_MAX, R_MAX = 9, 48  # every shape the tests use is a prefix / a row subset of this one


def make_case(name, H, shared, kind, I=38, bits=24, R=R_MAX, T=T_MAX, salt=None):
    """Case `name` for (H, R, T, gate sharing, kind of input term, I of the real-valued product, weight bits), seeded by all of them
    (and by `salt`, where cells of one geometry in one model want parameters of their own).
    Weights are returned as the device holds them (quantised to `bits`), so packing them again is the identity."""
    seed = zlib.crc32(repr((name, H, bool(shared), kind, I, bits, R, T) + (() if salt is None else (salt,))).encode())
    p = CASES[name](np.random.default_rng(seed), H, R, T, bool(shared), kind, I, bits)
    p["bits"], p["name"] = bits, name
    p["W_hh"] = dequantise(p["W_hh"], bits)
    if kind == "spike":
        p["W_ih"] = dequantise(p["W_ih"], bits)
    return p


def next_layer(p, ref, name, bits=24):
    """The case of a stack's layer 1 above layer-0 case `p`: case `name`'s "spike" parameters fed with the reference's layer-0 spikes."""
    q = make_case(name, p["H"], True, "spike", bits=bits, R=p["R"], T=p["T"])
    if name != "saturated":  # (its all-ones input IS what a saturated layer 0 emits: checked by the host test)
        q["s_in"] = ref["spk"].astype(np.int8)
    return q


# the geometries test_scan_edges.py runs (test_scanref_host.py checks the bound and the case table on every one): (H, shared, kind, I, bits)
GRID = ([(H, True, "zin", 38, 24) for H in (64, 160, 224, 256, 320)] + [(H, False, "zin", 38, 24) for H in (128, 224, 320)]
        + [(H, True, "zin", 38, 16) for H in (160, 224)] + [(H, True, "spike", 38, 24) for H in (224, 256, 320)]
        + [(H, True, "x", I, 24) for H in (224, 256) for I in (38, 64)])

# the (H, shared, kind, I) of every GSN cell the streaming-hop tests plant a case in (tests/hopref.py, test_hop_edges*.py): layer 0 is
# "x32" with the model's input width, the layers above are "spike"; test_scanref_host.py runs the same checks on them as on GRID
HOP_GRID = ([(H, True, "x32", I) for H, I in ((48, 64), (32, 38), (32, 94), (320, 64), (224, 158), (256, 64), (64, 38), (268, 257), (20, 257))]
            + [(H, False, "x32", I) for H, I in ((48, 64), (32, 94), (320, 64), (224, 38))]
            + [(H, True, "spike", 38) for H in (48, 32, 64, 268, 20)] + [(H, False, "spike", 38) for H in (48, 32, 224, 320)])
