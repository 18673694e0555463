"""Reference, tolerances and cases for the recipe loss on rows of different lengths (sfsn_recipe_loss_ragged; the `lengths=` of
spiking_fullsubnet_amd.loss) and for its time-domain L1 term (the REVERB recipe's F.l1_loss).

A helper module like lossref.py, which it imports (not a conftest).  The fp64 reference is a COMPOSITION: lossref.reference on every
row alone, on est[r, :L_r] and tgt[r, :L_r], plus the time term below.  A row's terms are the row's own; a batch term is the mean of
the row terms with every row weighted equally; the gradient and its bound are each row's own divided by `rows`; past a row's end the
gradient and its bound are zero.  Nothing here is fitted to what a kernel returns: every bound is lossref's, or derived in a
docstring below with lossref's conventions (u = 2^-24, gamma(n), every fp32 operation 1u, the last rounding of a result 2u,
first-order analyses times SECOND_ORDER).

Dividing a row's gradient bound by `rows` is exact reasoning, not an approximation: the row's share of d total / d est is the
gradient of the row alone under the weights c / rows, and every term of lossref's gradient bound is linear in the weights (the
coefficients c / N are rounded once whatever their value).

`dt=np.float32` evaluates the same composition in fp32 numpy (the "implementation" the host test uses to show that the bounds are
attainable before a GPU is involved) and `mut` selects a deliberately wrong semantics (the host test shows that each is rejected).
"""
import numpy as np

import lossref
from lossref import SECOND_ORDER, U, gamma

FREQ, MAG, SDR, TIME = 1, 2, 4, 8
TERMS = ("freq", "mag", "sisnr", "time")
# (c_freq, c_mag, c_sdr, c_time), flags.  intel_ndns: the trainer's loss without its constant; the time term is computed (flag set)
# with weight 0, so that all four values are checked under these weights too.  REVERB: freq + mag + l1, no SI-SNR.
INTEL = ((1.0, 1.0, -0.001, 0.0), FREQ | MAG | SDR | TIME)
REVERB = ((1.0, 1.0, 0.0, 1.0), FREQ | MAG | TIME)

# (name, shape, seed, row made equal to the target or None, one length per clip)
CASES = (
    ("r4_edges", (4, 5000), 10, None, (5000, 1025, 4096, 4097)),   # the minimum clip; 512 | L; 512 | L - 1 (a frame on the right mirror point)
    ("r3_chunks", (3, 16390), 11, None, (8192, 8193, 16390)),      # the 8192-sample row-sum chunk boundary; whole chunks past a clip's end
    ("r4_odd", (4, 3001), 12, None, (3001, 2600, 1537, 1536)),     # odd row stride (unaligned rows)
    ("r2x2", (2, 2, 2600), 13, None, (2600, 1100)),                # 3-D view, one length for both rows of a clip
    ("r3_eq", (3, 3000), 14, 1, (3000, 2000, 1500)),               # est == tgt on a short row: every sign 0, SI-SNR at the eps floor, time 0
    ("r5", (5, 5120), 15, None, (2048, 1025, 3333, 2047, 5120)),   # a row count that is no power of two
)
NAMES = tuple(c[0] for c in CASES)
MUTATIONS = ("zero_padded", "reflect_padded_end", "frames_padded", "length_weighted", "frame_weighted", "grad_no_rows", "grad_tail",
             "time_padded_stride")


def row_lengths(shape, lengths):
    """One length per row: all rows of a clip (an element of the leading dimension) share the clip's."""
    return np.repeat(np.asarray(lengths, np.int64), int(np.prod(shape[1:-1])))


def time_mae(e, t, dt=np.float64):
    """F.l1_loss of one row: (value, d value / d e [L], value bound, gradient bound [L]); the bounds are None unless dt is fp64.

    value = sum |e - t| / L and d value / d e_i = sgn(e_i - t_i) / L, sgn(0) = 0 (ATen's convention).

    Bound of an fp32 evaluation.  d_i = fl(e_i - t_i) is off by at most u |d_i| and |.| is exact; the sum of L terms passes an element
    through at most lossref.sum_depth(L) roundings; the division by L and the last rounding of the result add 2u:
        |d value| <= gamma(sum_depth(L) + 1) mean|e - t| + 2u value          (mean|e - t| IS the value)
    The difference of two fp32 numbers is zero only if they are equal and has the sign of the exact difference otherwise (gradual
    underflow), so sgn(fl(e_i - t_i)) is exact: the time term has NO ambiguous kinks.  The gradient is a coefficient times that sign;
    the coefficient takes at most three roundings (the product rows L, the division, the product by the weight; formed in fp64 and
    rounded once it takes one):
        |d grad_i| <= 3u |grad_i|
    The additions onto a sample's gradient are charged where the gradients are combined (reference below)."""
    e, t = np.asarray(e, dt), np.asarray(t, dt)
    L = e.shape[-1]
    d = e - t
    value = np.abs(d).sum(dtype=dt) / dt(L)
    grad = (np.sign(d) / dt(L)).astype(dt)
    if dt != np.float64:
        return value, grad, None, None
    vtol = (gamma(lossref.sum_depth(L) + 1) * value + 2 * U * value) * SECOND_ORDER
    return value, grad, vtol, 3 * U * np.abs(grad)


def _spectral_means(e, t, src):
    """freq and mag of one row whose frames read the samples src [T][2048] of e, t (fp64): the means over 1025 T terms."""
    w = lossref.window()
    E, Tt = np.fft.rfft(e[src] * w, axis=-1), np.fft.rfft(t[src] * w, axis=-1)
    n = E.size
    return (np.abs(E.real - Tt.real).sum() + np.abs(E.imag - Tt.imag).sum()) / n, np.abs(np.abs(E) - np.abs(Tt)).sum() / n


def reference(est, tgt, lengths, weights, flags, dt=np.float64, mut=None):
    """The ragged recipe loss of est, tgt [..., Lp] with one length per clip, as a dict: the batch terms freq, mag, sisnr, time (0 for
    a term whose flag is clear), total = ((c_freq freq + c_mag mag) + c_sdr sisnr) + c_time time, row_terms [rows][4], grad of est's
    shape (zero at and beyond a row's end); with dt = fp64 and mut = None also the bounds `tol` (per batch value), `row_tol`
    [rows][4], `grad_tol` (zero past a row's end: the tail is exact) and the per-row ambiguity counts `rows_ambiguity`
    (n_ambiguous, n_structural, n_terms of lossref.reference on the row alone).

    Bounds.  Row terms: lossref's and time_mae's on the row alone.  A batch value is the mean of `rows` row terms: the mean of the row
    bounds, plus the roundings of a sum of `rows` terms and the division relative to the mean magnitude, gamma(rows + 1) mean|term_r|,
    plus the last rounding 2u |value| -- the way lossref composes sisnr_tol.  total: four products and three additions,
    sum |c| tol + 5u sum |c term|.  Gradient of row r: (lossref's bound with the row's weights + |c_time| time_mae's) / rows, plus
    2u |grad| for the addition of the time term and the last rounding."""
    est, tgt = np.asarray(est), np.asarray(tgt)
    Lp = est.shape[-1]
    e2, t2 = est.reshape(-1, Lp), tgt.reshape(-1, Lp)
    rows = e2.shape[0]
    lens = row_lengths(est.shape, lengths)
    on = [bool(flags & b) for b in (FREQ, MAG, SDR, TIME)]
    c = [dt(w) if o else dt(0.0) for w, o in zip(weights, on)]
    exact = dt == np.float64 and mut is None
    row_terms, row_tol = np.zeros((rows, 4), dt), np.zeros((rows, 4))
    grad, grad_tol = np.zeros((rows, Lp), dt), np.zeros((rows, Lp))
    ambiguity = []
    Tp = 1 + Lp // lossref.HOP
    for r in range(rows):
        L = int(lens[r])
        if mut == "zero_padded":  # the loss of the zero-padded row
            e, t = (np.where(np.arange(Lp) < L, x[r], 0).astype(np.float32)[None] for x in (e2, t2))
            L = Lp
        else:
            e, t = e2[r:r + 1, :L], t2[r:r + 1, :L]
        ref = lossref.reference(e, t, weights=tuple(float(x) for x in c[:3]), dt=dt)
        tv, tg, ttol, tgtol = time_mae(e[0], t[0], dt)
        vals = [ref["freq"], ref["mag"], ref["sisnr"], tv]
        if mut == "reflect_padded_end":  # the row's own frames, the right margin mirrored about the PADDED end (it reads the zeros)
            ez, tz = (np.where(np.arange(Lp) < L, x[r], 0).astype(np.float64) for x in (e2, t2))
            vals[0], vals[1] = _spectral_means(ez, tz, lossref.pad_index(Lp)[lossref.frame_index(Lp)][:1 + L // lossref.HOP])
        if mut == "frames_padded":  # the means divide by the padded frame count
            vals[0], vals[1] = vals[0] * (1 + L // lossref.HOP) / Tp, vals[1] * (1 + L // lossref.HOP) / Tp
        if mut == "time_padded_stride":  # the time mean over the padded stride
            vals[3] = vals[3] * L / Lp
        row_terms[r] = [v if o else 0 for v, o in zip(vals, on)]
        grad[r, :L] = (ref["grad"][0] + c[3] * tg) / dt(rows)
        if exact:
            row_tol[r] = [tl if o else 0.0 for tl, o in zip((ref["tol"]["freq"], ref["tol"]["mag"], ref["tol"]["sisnr"], ttol), on)]
            grad_tol[r, :L] = (ref["grad_tol"][0] + abs(c[3]) * tgtol) / rows + 2 * U * np.abs(grad[r, :L])
            ambiguity.append((ref["n_ambiguous"], ref["n_structural"], ref["n_terms"]))
    if mut == "grad_no_rows":
        grad *= rows
    if mut == "grad_tail":  # the smallest thing a kernel could leave past a clip's end
        grad[np.arange(Lp)[None, :] >= lens[:, None]] = np.finfo(np.float32).tiny
    wts = {"length_weighted": lens / lens.sum(), "frame_weighted": (1 + lens // lossref.HOP) / (1 + lens // lossref.HOP).sum()}.get(
        mut, np.full(rows, 1.0 / rows))
    if mut in ("length_weighted", "frame_weighted"):
        batch = (row_terms * wts[:, None]).sum(0)
    else:
        batch = row_terms.sum(0, dtype=dt) / dt(rows)
    out = dict(zip(TERMS, batch))
    out["total"] = ((c[0] * batch[0] + c[1] * batch[1]) + c[2] * batch[2]) + c[3] * batch[3]
    out.update(row_terms=row_terms, grad=grad.reshape(est.shape), rows=rows, lens=lens)
    if not exact:
        return out
    tol = {k: row_tol[:, i].mean() + gamma(rows + 1) * np.abs(row_terms[:, i]).mean() + 2 * U * abs(batch[i]) for i, k in enumerate(TERMS)}
    tol["total"] = (sum(abs(c[i]) * tol[k] for i, k in enumerate(TERMS))
                    + 5 * U * sum(abs(c[i] * batch[i]) for i in range(4))) * SECOND_ORDER
    out.update(tol=tol, row_tol=row_tol, grad_tol=grad_tol.reshape(est.shape), rows_ambiguity=ambiguity)
    return out


def outside(got, ref):
    """Names of the results of `got` (freq / mag / sisnr / time / total, row_terms [rows][4], grad) that lie outside the bounds of the
    fp64 reference `ref`, with the share of its bound each one uses.  NaN counts as outside; where a bound is zero (a term whose flag
    is clear, the gradient past a row's end, est == tgt in the time term) only the exact value is inside."""
    def share(g, r, tol):
        with np.errstate(all="ignore"):
            d = np.abs(np.asarray(g, np.float64) - r)
            s = np.where(tol > 0, d / np.where(tol > 0, tol, 1.0), np.where(d == 0, 0.0, np.inf))
        return float(np.max(np.where(np.isnan(s), np.inf, s)))

    bad, used = [], {}
    for k in TERMS + ("total",):
        used[k] = share(got[k], ref[k], ref["tol"][k])
    used["row_terms"] = share(got["row_terms"], ref["row_terms"], ref["row_tol"])
    used["grad"] = share(got["grad"], ref["grad"], ref["grad_tol"])
    bad = [k for k, v in used.items() if not v <= 1.0]
    return bad, used


_cache = {}


def case(name, which=INTEL):
    """(est, tgt, lengths, fp64 reference under the weights and flags `which`) of a case; computed once, shared, never modified.  The
    inputs are lossref.make_inputs' on the whole padded shape."""
    key = (name, which)
    if key not in _cache:
        _, shape, seed, eq, lengths = next(c for c in CASES if c[0] == name)
        if name not in _cache:
            _cache[name] = lossref.make_inputs(shape, seed, eq)
        e, t = _cache[name]
        _cache[key] = (e, t, lengths, reference(e, t, lengths, *which))
    return _cache[key]
