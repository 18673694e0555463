"""Reference, tolerances and inputs for scoring ragged batches (sfsn_pit_sdr_ragged; PITWrapper(..., lengths=), PITWrapper.per_clip,
metric.SISDR): the permutation-invariant SI-SDR loss with per-clip lengths, and audiozen.metric.SISDR of the matched rows.

A helper module like pitref.py (not a conftest).  Four parts:

* the case table and its seeded generator (pitref.make_inputs' formula with explicit arguments; the padding is whatever the caller puts
  there -- `padded` fills it with NaN);
* the COMPOSITION that is the yardstick: tests/pitref.py's fp64 `reference()` on each clip alone, est[b:b+1, :, :L_b].  A clip's pair,
  loss_p, perm and reordered[:L_b] are that reference's; the batch loss is the mean of the clips' losses (every clip weighted equally);
  the PIT gradient of clip b is that reference's grad divided by B, with grad_tol divided by B (the bound is linear in the weight); the
  pairwise gradient is grad_pw with cot[b:b+1]; reordered and both gradients are zero from L_b on;
* an fp64 POINTWISE restatement of audiozen.metric.SISDR (metric.py:67-101) and its bound (`sisdr_rows`), pinned to the reference's own
  fp32 values by tests/golden/sisdr_metric.npz (tests/golden/make_golden_sisdr.py);
* `mut`: deliberately wrong variants of the composition, each of which test_pit_ragged_host.py shows to be rejected.
"""
import numpy as np

import pitref
from lossref import LOG_ULP, SECOND_ORDER, U, gamma, sum_depth

U64 = pitref.U64
K10 = pitref.K10
EPS32 = 2.0 ** -23  # torch.finfo(torch.float32).eps: the metric's eps
MUTATIONS = ("mean_over_lmax", "length_weighted_loss", "grad_over_B", "grad_tail", "sisdr_pit_eps")

# (name, B, S, Lmax, seed, mix, dc, lengths): the kernel's chunk is 2048 samples, the last workgroup solves 16 clips at a time
CASES = (
    ("r3s2", 3, 2, 1000, 100, 0.0, 0.0, (1000, 33, 999)),
    ("r2s3_odd", 2, 3, 4097, 101, 0.2, 0.03, (4097, 2049)),           # odd row stride: unaligned rows; 3 chunks beside 2
    ("r5s4", 5, 4, 777, 102, 0.2, 0.0, (777, 5, 6, 776, 400)),        # all 24 permutations on 5 samples
    ("r3s2_chunks", 3, 2, 6150, 103, 0.0, 0.03, (2048, 4096, 6150)),  # lengths on chunk boundaries; whole workgroups past a clip's end
    ("r3s1", 3, 1, 5000, 104, 0.0, 0.03, (5000, 2047, 2)),            # one source; the shortest legal clip
    ("r17s2", 17, 2, 300, 105, 0.1, 0.0, tuple(300 - 7 * b for b in range(17))),  # a second pass of the 16-clip batch
)


def case(name):
    return next(c for c in CASES if c[0] == name)


def lengths(name):
    return list(case(name)[7])


def make_inputs(name):
    """(est, ref) fp32 numpy [B, S, Lmax] of a case, every sample generated (the clips are the leading L_b samples of their rows):
    ref = 0.1 randn, a seeded permutation sigma_b per clip, est[b, i] = 0.7 ref[b, sigma_b[i]] + mix sum_k ref[b, k] + 0.05 randn + dc."""
    import torch
    _, B, S, L, seed, mix, dc, _ = case(name)
    g = torch.Generator().manual_seed(seed)
    ref = 0.1 * torch.randn(B, S, L, generator=g)
    sigma = torch.stack([torch.randperm(S, generator=g) for _ in range(B)])
    est = 0.7 * torch.stack([ref[b, sigma[b]] for b in range(B)]) + mix * ref.sum(1, keepdim=True) + 0.05 * torch.randn(B, S, L, generator=g) + dc
    return est.numpy().copy(), ref.numpy().copy()


def padded(x, lens, fill=np.nan):
    """A copy of x [B, S, Lmax] with everything from L_b on replaced by `fill`."""
    out = np.array(x, copy=True)
    for b, n in enumerate(lens):
        out[b, :, n:] = fill
    return out


def cotangent(name):
    """The seeded [B, S, S] fp32 cotangent of the pairwise mode."""
    _, B, S, L, seed, *_ = case(name)
    return np.random.default_rng(1000 + seed).standard_normal((B, S, S)).astype(np.float32)


def sisdr_rows(est, tgt, dt=np.float64, mut=None):
    """audiozen.metric.SISDR per row of est, tgt [..., L] (reduce_mean=False), evaluated pointwise: (val, tol), tol None unless dt is
    fp64 and mut is None.

    a = est - mean(est), s = tgt - mean(tgt) (always), eps = 2^-23, dot = <s, a>, n = |s|^2, ne = n + eps,
    proj_k = (dot s_k + eps) / ne, noise = a - proj, P = sum proj^2, N = sum noise^2, arg = (P + eps) / (N + eps) + eps,
    val = 10 log10(arg).

    Bound of an fp32 evaluation, counted like pitref's pair_tol (u = 2^-24, d = sum_depth(L) + 1: a sum and the operation feeding it):
      means     da_k = d u mean|e| + u |a_k|, ds_k likewise
      dot       ddot = sum(|s| da + |a| ds) + d u sum|a s|;  dn = 2 sum |s| ds + d u n;  dne = dn + u ne
      proj      the numerator num_k = dot s_k + eps: dnum_k = |s_k| ddot + |dot| ds_k + u |dot s_k| + u |num_k| (eps itself is exact);
                dproj_k = dnum_k / ne + |proj_k| (dne / ne + u);  dnoise_k = da_k + dproj_k + u |noise_k|
      P         dP = sum(2 |proj| dproj + dproj^2) + d u P + c64 2^-53 alpha^2 sum r^2;  dPe = dP + u (P + eps)
      N         dN = sum(2 |noise| dnoise + dnoise^2) + d u N                                        (pointwise evaluation)
                     + c64 2^-53 (sum e^2 + 2 |alpha| sum|e r| + alpha^2 sum r^2)                      (the kernel's sum identity)
                The kernel forms N = sum a^2 - 2 dot^2 / ne + (dot^2 n + L eps^2) / ne^2 from fp64 sums of the RAW samples e, r
                (alpha = dot / ne): every sum carries at most 8 + 6 + 2 + ceil(L / 2048) fp64 additions per element and the identity
                twelve more operations, c64 in all; relative to N that is the cancellation factor |e|^2 / |noise|^2 times 2^-53 (the
                raw |e|^2 holds the DC the centring removes, which is why the raw sums are charged).  dNe = dN + u (N + eps)
      ratio     dratio = ratio (dPe / (P + eps) + dNe / (N + eps) + u);  darg = dratio + u arg
      val       (10 / ln 10) darg / arg + (2 LOG_ULP + 2) u |val|, times SECOND_ORDER.
    The eps terms: eps = 2^-23 is a power of two and enters by four additions and one product per sample, each charged above; its
    contribution L eps^2 / ne^2 to P is exact in the identity to within the fp64 roundings of c64.

    mut = "sisdr_pit_eps": PairwiseNegSDR's placement of the same eps (proj = dot s / ne, P / (N + eps) + eps)."""
    e, t = np.asarray(est, dt), np.asarray(tgt, dt)
    L = e.shape[-1]
    eps = dt(EPS32)
    s_ = lambda x: x.sum(-1, keepdims=True)
    a, s = e - e.mean(-1, keepdims=True), t - t.mean(-1, keepdims=True)
    with np.errstate(all="ignore"):
        dot, n = s_(s * a), s_(s * s)
        ne = n + eps
        if mut == "sisdr_pit_eps":
            proj = dot * s / ne
            noise = a - proj
            P, N = s_(proj * proj), s_(noise * noise)
            arg = P / (N + eps) + eps
            return (dt(10.0) * np.log10(arg))[..., 0], None
        num = dot * s + eps
        proj = num / ne
        noise = a - proj
        P, N = s_(proj * proj), s_(noise * noise)
        Pe, Ne = P + eps, N + eps
        ratio = Pe / Ne
        arg = ratio + eps
        val = dt(10.0) * np.log10(arg)
    if dt != np.float64 or mut is not None:
        return val[..., 0], None
    d = sum_depth(L) + 1
    c64 = 8 + 6 + 2 + (L + 2047) // 2048 + 12
    with np.errstate(all="ignore"):
        alpha = dot / ne
        da = d * U * np.abs(e).mean(-1, keepdims=True) + U * np.abs(a)
        ds = d * U * np.abs(t).mean(-1, keepdims=True) + U * np.abs(s)
        ddot = s_(np.abs(s) * da + np.abs(a) * ds) + d * U * s_(np.abs(a * s))
        dn = 2 * s_(np.abs(s) * ds) + d * U * n
        dne = dn + U * ne
        dnum = np.abs(s) * ddot + np.abs(dot) * ds + U * np.abs(dot * s) + U * np.abs(num)
        dproj = dnum / ne + np.abs(proj) * (dne / ne + U)
        dnoise = da + dproj + U * np.abs(noise)
        dP = s_(2 * np.abs(proj) * dproj + dproj * dproj) + d * U * P + c64 * U64 * alpha * alpha * s_(t * t)
        dN = s_(2 * np.abs(noise) * dnoise + dnoise * dnoise) + d * U * N \
            + c64 * U64 * (s_(e * e) + 2 * np.abs(alpha) * s_(np.abs(e * t)) + alpha * alpha * s_(t * t))
        dPe, dNe = dP + U * Pe, dN + U * Ne
        dratio = ratio * (dPe / Pe + dNe / Ne + U)
        darg = dratio + U * arg
        tol = (K10 * darg / arg + (2 * LOG_ULP + 2) * U * np.abs(val)) * SECOND_ORDER
    return val[..., 0], tol[..., 0]


def sisdr_mean(val, tol):
    """The reduce_mean=True value of rows `val` and its bound: the mean of the rows' bounds, a sum of n fp32 terms and a division
    (gamma(n + 1) of the mean magnitude) and the last rounding."""
    m = float(np.mean(val))
    return m, float(np.mean(tol) + gamma(val.size + 1) * np.abs(val).mean() + 2 * U * abs(m))


def reference(est, ref, lens, zero_mean=True, eps=pitref.EPS, cot=None, mut=None):
    """The composition over the clips alone, est[b:b+1, :, :L_b] (nothing from L_b on is read).  A dict of pair [B,S,S], loss_p [B,S!],
    perm, clip_loss [B], loss, reordered and grad [B,S,Lmax] (zero from L_b on), si_sdr [B,S] (reference j against est[perm[j]]) and,
    with `cot`, grad_pw; with mut = None also pair_tol, loss_p_tol, clip_loss_tol, loss_tol, grad_tol, si_sdr_tol and grad_pw_tol.

    clip_loss_tol is the clip's loss_p_tol of the chosen permutation plus 2u |clip_loss| (its fp32 rounding); loss_tol is pitref's:
    the mean of the chosen loss_p_tol + gamma(B + 1) mean|clip_loss| + 2u |loss|."""
    est, ref = np.asarray(est), np.asarray(ref)
    B, S, Lmax = est.shape
    assert len(lens) == B
    if mut == "mean_over_lmax":  # the padded batch through the equal-length formulas: means and sums over Lmax of the zero-padded clip
        full = pitref.reference(padded(est, lens, 0.0), padded(ref, lens, 0.0), zero_mean, eps, cot=cot, mut="composed")
        clips = [{k: (v[b:b + 1] if isinstance(v, np.ndarray) and v.ndim else v) for k, v in full.items()} for b in range(B)]
        for b, c in enumerate(clips):  # (the weight of its gradient is already 1 / (B S))
            c["grad"] = c["grad"] * B
    else:
        clips = [pitref.reference(est[b:b + 1, :, :n], ref[b:b + 1, :, :n], zero_mean, eps, cot=None if cot is None else cot[b:b + 1],
                                  mut=None if mut is None else "composed") for b, n in enumerate(lens)]
    out = dict(B=B, S=S, L=Lmax, lens=list(lens))
    out["pair"] = np.concatenate([c["pair"] for c in clips])
    out["loss_p"] = np.concatenate([c["loss_p"] for c in clips])
    out["perm"] = np.concatenate([c["perm"] for c in clips])
    best = np.argmin(out["loss_p"], axis=1)
    out["clip_loss"] = out["loss_p"][np.arange(B), best]
    if mut == "length_weighted_loss":
        out["loss"] = float(np.sum(out["clip_loss"] * np.asarray(lens, np.float64)) / np.sum(lens))
    else:
        out["loss"] = float(out["clip_loss"].mean())
    scale = S / B if mut == "grad_over_B" else 1.0 / B  # a clip alone weighs its pairs 1 / S; the batch's weight is 1 / (B S)

    def rows(key, weight=1.0, tail=0.0):
        full = np.full((B, S, Lmax), tail, np.float64)
        for b, n in enumerate(lens):
            full[b, :, :n] = weight * clips[b][key][0, :, :n]
        return full

    out["grad"] = rows("grad", scale, 1e-3 if mut == "grad_tail" else 0.0)
    out["reordered"] = np.zeros((B, S, Lmax), np.float32)
    for b, n in enumerate(lens):
        out["reordered"][b, :, :n] = est[b, out["perm"][b], :n]
    if cot is not None:
        out["grad_pw"] = rows("grad_pw")
    vals, tols = [], []
    for b, n in enumerate(lens):
        v, t = sisdr_rows(est[b, out["perm"][b], :n], ref[b, :, :n], mut=mut if mut == "sisdr_pit_eps" else None)
        vals.append(v)
        tols.append(t)
    out["si_sdr"] = np.stack(vals)
    if mut is not None:
        return out
    out["pair_tol"] = np.concatenate([c["pair_tol"] for c in clips])
    out["loss_p_tol"] = np.concatenate([c["loss_p_tol"] for c in clips])
    chosen_tol = out["loss_p_tol"][np.arange(B), best]
    out["clip_loss_tol"] = chosen_tol + 2 * U * np.abs(out["clip_loss"])
    out["loss_tol"] = float(chosen_tol.mean() + gamma(B + 1) * np.abs(out["clip_loss"]).mean() + 2 * U * abs(out["loss"]))
    out["grad_tol"] = rows("grad_tol", 1.0 / B)
    if cot is not None:
        out["grad_pw_tol"] = rows("grad_pw_tol")
    out["si_sdr_tol"] = np.stack(tols)
    return out


KEYS = (("pair", "pair_tol"), ("clip_loss", "clip_loss_tol"), ("loss", "loss_tol"), ("grad", "grad_tol"), ("grad_pw", "grad_pw_tol"),
        ("si_sdr", "si_sdr_tol"))


def outside(got, ref):
    """Names of the results of `got` outside the bounds of the composition `ref`, with the share of the bound each one uses.  NaN counts
    as outside; where the bound is zero (the tails) the value must be exactly zero; perm and reordered must be equal."""
    bad, used = [], {}
    for k, tol in KEYS:
        if got.get(k) is None or k not in ref:
            continue
        g, r, t = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64), np.asarray(ref[tol], np.float64)
        with np.errstate(all="ignore"):
            diff = np.abs(g - r)
            rr = np.where(t > 0, diff / np.where(t > 0, t, 1.0), np.where(diff == 0, 0.0, np.inf))
        used[k] = float(np.max(np.where(np.isnan(rr), np.inf, rr)))
        if not used[k] <= 1.0:
            bad.append(k)
    if got.get("perm") is not None and not np.array_equal(np.asarray(got["perm"], np.int64), ref["perm"]):
        bad.append("perm")
    if got.get("reordered") is not None and not np.array_equal(np.asarray(got["reordered"], np.float32).view(np.uint32), ref["reordered"].view(np.uint32)):
        bad.append("reordered")
    return bad, used
