"""Reference, tolerance, dispatch and inputs for the time-parallel PRODUCTS at their arithmetic edges: sfsn_input_proj_f32 (its three
kernels), sfsn_spike_proj (both kernels), their _multi entries and the z of sfsn_features_proj.

A helper module like scanref.py (not a conftest); numpy only.  Every constant is scanref's (U, RND, SECOND_ORDER, QMAX): none is fitted
to what a kernel or an emulation returns.  Five parts:

* the dispatch of sfsn_kernels.hip restated: `form` (sfsn_input_proj_f32 -> "bf3" / "f32mfma" / "plain"), `multi_ok`, `spike_form`
  ("fast" / "generic"), `grid` (how many workgroups share the 64-row tiles) and `deal_blocks` (the _multi entries' block ranges).  A
  shape the entry refuses is "unsupported" (K > 192 for the real-valued product, more than 3 column tiles per wave, K > 320 for spikes).
* `real_reference`: z = x . w^T + b in fp64 with a = |x| . |w|^T + |b| and the per-element bound of scanref.layer's docstring: kind "x"
  for the bf16 three-way split, kind "x32" for the two fp32 kernels (any order of the sum) -- with K replaced by n[m][j] = the number of
  k with x[m][k] != 0 and w[j][k] != 0.  Why that is still a bound: a term with x_k = 0 or w_k = 0 has every piece (bf16 split of
  zero) and every piece product exactly zero, and adding an exact zero to a partial sum rounds nothing, inside the matrix core or
  outside it; so only the n non-zero terms pass through roundings, and only they have dropped piece products.  For a one-hot row
  n = 1 and the bound collapses to a few roundings of ONE product -- a lost piece product (2^-17 |x||w| and more) is far outside it.
      "x"    tol = [RND ((n + 2)(1 + 2^-7) + 5 n 2^-7 1.01) + 2^-23 (1 + 2^-8)] a SECOND_ORDER
      "x32"  tol = RND (n + 1) a SECOND_ORDER
  RND = 2u counts one fp32 rounding as in scanref (its module docstring says why); the host test shows that the fp32 emulations and a
  correctly rounded k-ordered fp32 chain stay at or below 1, and prints the worst ratio.
* `spike_reference`: S = s . q^T on integers with scanref.quantise, y = S dq + b.  The kernels' recombination (sfsn_scan_dev.h,
  recombine3) is fma(float(a2), 65536, float(a1 256 + a0)): |a1 256 + a0| < 2^24 and |a2| < 2^16 are exact conversions, so it is
  the exact integer S rounded ONCE to fp32 -- no rounding at all where |S| < 2^24.  dq is a power of two, so rec dq is exact and
  y = fl(fl(S) dq + b) whether or not the compiler contracts the multiply-add.  Hence: where |S| < 2^24 the output is fl(S dq + b)
  BIT FOR BIT (`want`, formed as fp32(S dq) + b in fp32: one correctly rounded addition of two exact operands) whatever the
  recombination does with larger sums (`exact` marks these); elsewhere it holds under scanref's "spike" bound, which carries the
  recombination's rounding: tol = [RND |S dq| + RND |y|] SECOND_ORDER.  Because this recombination IS one round-to-nearest of the
  exact S, `want` (fp32(S dq) rounds S the same way) is the kernels' bit pattern for every |S|: the tests assert it everywhere
  (`every`) and the bound besides, which would still hold a recombination that rounded twice.
* fp32 emulations with `mut=` (host test only): `emulate_bf3` (scanref._input_term's "x" branch made k-step-wise: six piece
  products per 32 columns, `hi` takes x1 w1, `lo` the five small ones, (hi + lo) + b), `emulate_f32` (one fma chain in k order,
  then + b -- correctly rounded operations), `emulate_spike`; `lay_out` places a result in a NaN-filled [rows][ld] buffer the way
  the kernels' epilogue does and `check` is the ONE comparison both test files use: every element of the buffer is asserted -- the
  M x N results against the reference, everything else (gap columns, rows after M) must still be NaN.
* seeded cases.  Domain of the real-valued product: every x, w, b is zero or has a magnitude in [2^-60, 2^60] and every non-zero
  product |x_k w_k| lies in [2^-80, 2^80]: the smallest piece product (2^-46 |x_k w_k|) is then a normal fp32 number and no partial sum
  overflows.  Denormals and overflow are NOT posed (`in_domain` asserts this for every case).  Spike rows hold 0 / 1 in columns
  0 .. K-1 and zeros in the padding columns K .. pad64(K)-1, which is how the scans leave the rows they write into a zeroed buffer
  (include/sfsn.h: "s int8 0/1 [M][pad64(K)] as written by the scan").
"""
import zlib

import numpy as np

import scanref as sr

U, RND, SECOND_ORDER, F32 = sr.U, sr.RND, sr.SECOND_ORDER, sr.F32
LDS_MAX = 150 * 1024  # sfsn_kernels.hip: the fast kernels' LDS budget
BF3_INSTANCES = [(1, 2), (1, 3), (1, 5), (1, 6), (2, 2), (2, 3), (2, 5), (3, 2), (3, 3)]  # (TPW, KSB): IPB_CASE
BF3_MULTI_INSTANCES = [(1, 2), (1, 3), (1, 5), (1, 6), (2, 2), (2, 3), (2, 5)]              # IPM_CASE
F32_GRID_CAP = 512   # input_proj_fast_kernel's grid cap (the bf3 and spike kernels are capped by the CU count)


# ----------------------------------------------------------------------------------------------------------------------
# dispatch, restated from sfsn_kernels.hip
# ----------------------------------------------------------------------------------------------------------------------
def pick_tiling(N):
    """(TPW: column tiles per wave, NWN: waves across the columns) of N output columns."""
    NT = (N + 15) // 16
    TPW = (NT + 7) // 8
    return TPW, (NT + TPW - 1) // TPW


def ksb(K):
    """32-column k-steps the bf3 kernel is compiled for."""
    return 2 if K <= 64 else (3 if K <= 96 else (5 if K <= 160 else 6))


def form(M, K, N, ld, x_ptr_offset=0):
    """The kernel sfsn_input_proj_f32 runs for z [M][ld] = x [M][K] . w [N][K]^T with x `x_ptr_offset` bytes behind a 16-byte boundary:
    "bf3" (input_proj_bf3_kernel), "f32mfma" (input_proj_fast_kernel), "plain" (input_proj_kernel), "unsupported", "invalid".
    TPW = 2, KSB = 6 satisfies TPW KSB <= 12 but is not instantiated: it falls through to the fp32 kernels."""
    if M <= 0 or K <= 0 or N <= 0 or ld < N:
        return "invalid"
    TPW, _ = pick_tiling(N)
    KC = (K + 15) // 16
    if TPW > 3 or KC > 12:
        return "unsupported"
    KSB = ksb(K)
    blds = 3 * 64 * (KSB * 32 + 8) * 2 + 64 * (N + 4) * 4
    rows = N % 4 == 0 and ld % 4 == 0 and M >= 64
    if K % 2 == 0 and K <= 192 and rows and TPW * KSB <= 12 and blds <= LDS_MAX and x_ptr_offset % 8 == 0 and (TPW, KSB) in BF3_INSTANCES:
        return "bf3"
    KCB = 3 if KC <= 3 else (6 if KC <= 6 else (10 if KC <= 10 else 12))
    flds = (2 * 64 * (KCB * 16 + 4) + 64 * (N + 4)) * 4
    return "f32mfma" if rows and flds <= LDS_MAX else "plain"


def multi_ok(M, K, N, ld, x_ptr_offset=0):
    """Whether sfsn_input_proj_f32_multi takes the job (only what the single entry runs on its bf3 kernel, at most two column tiles)."""
    return form(M, K, N, ld, x_ptr_offset) == "bf3" and (pick_tiling(N)[0], ksb(K)) in BF3_MULTI_INSTANCES


def spike_form(M, K, N, ld, y_ptr_offset=0):
    """sfsn_spike_proj's kernel: "fast" (spike_proj_fast_kernel: whole rows through LDS) or "generic" (spike_proj_kernel)."""
    if M <= 0 or K <= 0 or N <= 0 or ld < N or y_ptr_offset % 4:
        return "invalid"
    TPW, _ = pick_tiling(N)
    KS = (K + 63) // 64
    if TPW > 3 or KS > 5:
        return "unsupported"
    lds = 2 * 64 * (KS * 64 + 16) + 64 * (N + 4) * 4
    return "fast" if N % 4 == 0 and ld % 4 == 0 and M >= 64 and lds <= LDS_MAX and y_ptr_offset % 16 == 0 else "generic"


def spike_multi_ok(M, K, N, ld):
    return spike_form(M, K, N, ld) == "fast" and pick_tiling(N)[0] <= 2


def grid(kind, M, N, n_cu):
    """Workgroups that share the ceil(M / 64) tiles of a single launch of kernel `kind` ("bf3", "f32mfma", "fast"); a workgroup takes a
    second tile (the prefetch / park path) exactly when this is smaller than the number of tiles."""
    ns = (M + 63) // 64
    cap = dict(bf3=n_cu, f32mfma=F32_GRID_CAP, fast=n_cu * (2 if pick_tiling(N)[0] == 1 else 1))[kind]
    return min(ns, cap)


def deal_blocks(weights, ns, total):
    """deal_blocks: `total` workgroups in proportion to the jobs' bytes, at least one and at most ns[i] each."""
    s = float(sum(weights))
    return [min(max(int(total * w / s + 0.5), 1), n) for w, n in zip(weights, ns)]


def inproj_multi_blocks(shapes, n_cu):
    """Block counts of sfsn_input_proj_f32_multi for jobs [(M, K, N)]."""
    ns = [(M + 63) // 64 for M, K, N in shapes]
    return deal_blocks([n * (64.0 * K * 4 + 64.0 * N * 4) for n, (M, K, N) in zip(ns, shapes)], ns, n_cu), ns


def spike_multi_blocks(shapes, n_cu):
    """Block counts of sfsn_spike_proj_multi for jobs [(M, K, N)]."""
    ns = [(M + 63) // 64 for M, K, N in shapes]
    return deal_blocks([n * (64.0 * ((K + 63) // 64) * 64 + 64.0 * N * 4) for n, (M, K, N) in zip(ns, shapes)], ns, n_cu), ns


# ----------------------------------------------------------------------------------------------------------------------
# references and bounds
# ----------------------------------------------------------------------------------------------------------------------
def real_reference(x, w, b, kind):
    """(z fp64 [M][N], tol [M][N]) of z = x . w^T + b; kind "bf3" (scanref's "x" bound) or "f32" (its "x32" bound), K replaced by the
    number of non-zero terms of each (row, column): see the module docstring."""
    x64, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
    z = x64 @ w64.T
    a = np.abs(x64) @ np.abs(w64).T
    n = np.rint((x64 != 0).astype(np.float64) @ (w64 != 0).astype(np.float64).T)
    if b is not None:
        z = z + np.asarray(b, np.float64)
        a = a + np.abs(np.asarray(b, np.float64))
    if kind == "bf3":
        tol = (RND * ((n + 2) * (1 + 2.0 ** -7) + 5 * n * 2.0 ** -7 * 1.01) + 2.0 ** -23 * (1 + 2.0 ** -8)) * a
    else:
        assert kind == "f32", kind
        tol = RND * (n + 1) * a
    return z, tol * SECOND_ORDER


def pad64(K):
    return (K + 63) // 64 * 64


def spike_reference(s, w, b, bits=24):
    """dict(y fp64 [M][N], tol, exact: |S| < 2^24, want fp32: the bit pattern where exact, smax) of y = dq (s . q^T) + b with
    (q, dq) = scanref.quantise(w, bits); s [M][>= K] holds 0 / 1 (padding columns are not read)."""
    K = w.shape[1]
    q, dq = sr.quantise(w, bits)
    S = sr._isum(np.asarray(s)[:, :K], q)
    p = S * dq  # exact in fp64: |S| < 2^33, dq a power of two
    b64 = np.zeros(len(w)) if b is None else np.asarray(b, np.float64)
    y = p + b64
    exact = np.abs(S) < 2 ** 24
    want = (p.astype(F32) + b64.astype(F32)).astype(F32)  # where exact: fp32(S dq) is S dq, the addition rounds once
    tol = (RND * np.abs(p) + RND * np.abs(y)) * SECOND_ORDER
    return dict(y=y, tol=tol, exact=exact, every=np.ones_like(exact), want=want, smax=int(np.abs(S).max()))


# ----------------------------------------------------------------------------------------------------------------------
# fp32 emulations and their deliberately wrong variants (host test only)
# ----------------------------------------------------------------------------------------------------------------------
PIECE_MUTANTS = ["drop_x1w1", "drop_x1w2", "drop_x2w1", "drop_x1w3", "drop_x2w2", "drop_x3w1"]
ROW_MUTANTS = ["last_row_repeat", "stale_tile"]
REAL_MUTANTS = PIECE_MUTANTS + ["trunc_split", "no_bias", "zero_last_kstep"] + ROW_MUTANTS + ["pitch_n"]
SPIKE_MUTANTS = ["drop_d0", "wrap31"] + ROW_MUTANTS[1:] + ["pitch_n"]


def _trunc16(x):
    return (np.ascontiguousarray(x, F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def _rows(a, mut, nblk):
    """The row mutants on the left operand: the last row repeats the last row of the tile before it / a row of a workgroup's second
    tile (m >= 64 nblk) takes the operand of row m - 64 nblk, what a prefetch that was never parked would leave behind."""
    M = len(a)
    if mut == "last_row_repeat" and (M - 1) // 64 >= 1:
        a = a.copy()
        a[M - 1] = a[64 * ((M - 1) // 64) - 1]
    elif mut == "stale_tile" and M > 64 * nblk:
        a = a.copy()
        a[64 * nblk:] = a[:M - 64 * nblk]
    return a


def emulate_bf3(x, w, b, mut=None, nblk=1):
    """input_proj_bf3_body in fp32 numpy: per 32-column k-step the six piece products (a k-step's 32-term sum is formed in fp64 and
    rounded once: the matrix core's own order is not known, the products are exact), `hi` += x1 w1, `lo` += x1 w3, x2 w2, x3 w1,
    x1 w2, x2 w1 in the kernel's order, z = (hi + lo) + b."""
    x = _rows(np.ascontiguousarray(x, F32), mut, nblk)
    w = np.ascontiguousarray(w, F32)
    K = x.shape[1]
    if mut == "zero_last_kstep" and K % 32:
        x = x.copy()
        x[:, K - K % 32:] = 0
    cut = _trunc16 if mut == "trunc_split" else sr._bf16
    xs, ws = [cut(x)], [cut(w)]
    xs.append(cut(x - xs[0])); xs.append(cut(x - xs[0] - xs[1]))
    ws.append(cut(w - ws[0])); ws.append(cut(w - ws[0] - ws[1]))
    hi = np.zeros((len(x), len(w)), F32)
    lo = np.zeros_like(hi)
    for k0 in range(0, K, 32):
        for (i, j) in ((0, 2), (0, 0), (1, 1), (2, 0), (0, 1), (1, 0)):  # (x piece, w piece): IPB_STEP's order
            if mut == f"drop_x{i + 1}w{j + 1}":
                continue
            blk = (xs[i][:, k0:k0 + 32].astype(np.float64) @ ws[j][:, k0:k0 + 32].astype(np.float64).T).astype(F32)
            if (i, j) == (0, 0):
                hi = (hi + blk).astype(F32)
            else:
                lo = (lo + blk).astype(F32)
    z = (hi + lo).astype(F32)
    return z if b is None or mut == "no_bias" else (z + np.asarray(b, F32)).astype(F32)


def emulate_f32(x, w, b, mut=None, nblk=1):
    """The fp32 kernels' sum with correctly rounded operations: one fma chain in k order from zero, then + b."""
    x = _rows(np.ascontiguousarray(x, F32), mut, nblk)
    w = np.ascontiguousarray(w, F32)
    acc = np.zeros((len(x), len(w)), F32)
    for k in range(x.shape[1]):
        acc = sr._fma(x[:, k, None], w[None, :, k], acc)
    return acc if b is None or mut == "no_bias" else (acc + np.asarray(b, F32)).astype(F32)


def emulate_spike(s, w, b, bits=24, mut=None, nblk=1):
    """spike_proj: fp32(exact integer sum) (recombine3's one rounding) times dq plus the bias in one fma."""
    s = _rows(np.asarray(s), mut, nblk)
    q, dq = sr.quantise(w, bits)
    if mut == "drop_d0":
        q = q - sr.digits(q)[0]
    S = sr._isum(s[:, :w.shape[1]], q)
    if mut == "wrap31":
        S = ((S + 2 ** 30) % 2 ** 31) - 2 ** 30
    return sr._fma(S.astype(F32), dq.astype(F32)[None, :], np.zeros(len(w), F32) if b is None else np.asarray(b, F32))


def lay_out(z, rows, ld, mut=None):
    """z [M][N] in a NaN-filled [rows][ld] buffer; mut "pitch_n": row m starts at m N instead of m ld."""
    M, N = z.shape
    buf = np.full(rows * ld, np.nan, F32)
    if mut == "pitch_n":
        buf[:M * N] = z.ravel()
        return buf.reshape(rows, ld)
    buf = buf.reshape(rows, ld)
    buf[:M, :N] = z
    return buf


def check(buf, M, N, ref, tol, exact=None, want=None):
    """Every element of buf [rows][ld]: (ok, why, worst error / tolerance).  Columns N.. of every row and the rows M.. must still be
    NaN; the M x N results must lie within tol of ref -- and, where `exact`, equal `want` as fp32 numbers."""
    buf = np.asarray(buf)
    got = buf[:M, :N]
    if not (np.isnan(buf[:M, N:]).all() and np.isnan(buf[M:]).all()):
        return False, "a canary behind the columns or the rows was overwritten", float("inf")
    if np.isnan(got).any():
        m, n = (int(v[0]) for v in np.nonzero(np.isnan(got)))
        return False, f"row {m} column {n} was not written (or is NaN)", float("inf")
    ratio = sr.worst(got, ref, tol)
    if exact is not None and not np.array_equal(got[exact], want[exact]):
        m, n = (int(v[0]) for v in np.nonzero(exact & (got != want)))
        return False, f"row {m} column {n}: {got[m, n]!r} is not the exact {want[m, n]!r} ({int((exact & (got != want)).sum())} in all)", ratio
    if not ratio <= 1.0:
        err = np.abs(got.astype(np.float64) - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            m, n = np.unravel_index(np.argmax(np.where(err == 0, 0.0, err / tol)), err.shape)
        return False, f"row {m} column {n}: {got[m, n]!r} against {ref[m, n]!r}, {ratio:.3g} x the tolerance", ratio
    return True, "", ratio


# ----------------------------------------------------------------------------------------------------------------------
# cases of the real-valued product
# ----------------------------------------------------------------------------------------------------------------------
def _sig(v, bits):
    """v rounded to `bits` significant bits."""
    m, e = np.frexp(np.asarray(v, np.float64))
    return np.ldexp(np.rint(np.ldexp(m, bits)), e - bits)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _per_tile(seed, M, K, draw):
    """x [M][K] drawn 64 rows at a time, every tile from a generator of its own: a workgroup that computed a tile from another
    tile's rows cannot be right by symmetry."""
    return np.concatenate([draw(np.random.default_rng((seed, t)), min(64, M - 64 * t), K) for t in range((M + 63) // 64)])


def _control(rng, seed, M, K, N):
    x = _per_tile(seed, M, K, lambda g, m, k: g.standard_normal((m, k)))
    return x, rng.uniform(-0.1, 0.1, (N, K)), rng.standard_normal(N)


def _one_hot(xbits, wbits, edge=False):
    def make(rng, seed, M, K, N):
        """Row m: one non-zero at k = m mod K (M >= K rows probe every k, the partial k-step and K - 1 included; every 16-row block probes 16
        consecutive k).  Exponents over the domain with |x w| in [2^-78, 2^80); mantissas of `xbits` / `wbits` significant bits.  Every
        other column tile has no bias, so that a = |x||w| there.
        edge: mantissas 1 + 2^-7 - j 2^-23 (w: with some of the next three bits set, so that the last rounding varies), whose pieces are
        the largest a TRUNCATING split can leave (x2 = 2^-7 - 2^-15): its dropped products reach 2^-21 |x||w| = 7.9u of the 8.1u this
        bound allows one product, and with the last rounding on the same side they are outside it -- where round-to-nearest keeps
        them under the bound's 2^-23 (1 + 2^-8)."""
        m = np.arange(M)
        ex = rng.integers(-60, 60, M)  # mantissas are in [1, 2]: |x| in [2^-60, 2^60]
        if edge:
            mx = 1 + 2.0 ** -7 - rng.integers(1, 17, M) * 2.0 ** -23
            mw = 1 + rng.integers(0, 8, (N, K)) * 2.0 ** -7 + 2.0 ** -7 - rng.integers(1, 65, (N, K)) * 2.0 ** -23
        else:
            mx = _sig(rng.uniform(1.0, 2.0, M), xbits)
            mw = _sig(rng.uniform(1.0, 2.0, (N, K)), wbits)
        x = np.zeros((M, K))
        x[m, m % K] = np.where(rng.random(M) < 0.5, -1.0, 1.0) * np.ldexp(mx, ex)
        ew = rng.integers(-18, 19, (N, K))  # |e_x + e_w| <= 78, |e_w| <= 18: w, and x w, stay in the domain
        w = np.where(rng.random((N, K)) < 0.5, -1.0, 1.0) * np.ldexp(mw, ew)
        b = rng.standard_normal(N) * 2.0 ** rng.integers(-20, 21, N)
        b[(np.arange(N) // 16) % 2 == 1] = 0.0
        return x, w, (None if edge else b)
    return make


def _dynamic(rng, seed, M, K, N):
    x = rng.standard_normal((M, K)) * np.where(rng.random((M, K)) < 0.5, 1e4, 1e-4)
    w = rng.uniform(-0.1, 0.1, (N, K)) * np.where(rng.random((N, K)) < 0.5, 1e4, 1e-4)
    return x, w, rng.standard_normal(N)


def _row_scales(rng, seed, M, K, N):
    """scanref._scaled_rows (row maxima over 106 binades, one all-zero row) moved into the domain: times 2^40 (maxima 2^-60 .. 2^46),
    entries under 2^-60 set to zero, x in +-[2^-8, 2^4]."""
    w = sr._scaled_rows(rng, N, K, 7 % N).astype(np.float64) * 2.0 ** 40
    w[np.abs(w) < 2.0 ** -60] = 0
    x = np.where(rng.random((M, K)) < 0.5, -1.0, 1.0) * np.exp2(rng.uniform(-8, 4, (M, K)))
    return x, w, rng.standard_normal(N) * 2.0 ** rng.integers(-40, 41, N)


def _cancel(rng, seed, M, K, N):
    """The second half of the columns repeats the first with w negated and scaled by 1 + 2^-12: z = -2^-12 (half the sum) + b with
    sum |x||w| 2^13 times larger; a tiny bias."""
    h = K // 2
    x, w = np.zeros((M, K)), np.zeros((N, K))
    x[:, :h] = rng.standard_normal((M, h))
    w[:, :h] = rng.uniform(0.02, 0.1, (N, h)) * np.where(rng.random((N, h)) < 0.5, -1.0, 1.0)
    x[:, h:2 * h] = x[:, :h]
    w[:, h:2 * h] = -w[:, :h].astype(F32).astype(np.float64) * (1 + 2.0 ** -12)
    return x, w, rng.standard_normal(N) * 1e-6


def _no_bias(rng, seed, M, K, N):
    x, w, _ = _control(rng, seed + 1, M, K, N)
    return x, w, None


REAL_CASES = dict(control=_control, one_hot_x8=_one_hot(8, 24), one_hot_w8=_one_hot(24, 8), one_hot_16=_one_hot(16, 16),
                  one_hot_edge=_one_hot(24, 24, True), dynamic=_dynamic, row_scales=_row_scales, cancel=_cancel, no_bias=_no_bias)
REAL_QUICK = ["control", "one_hot_x8", "one_hot_w8", "one_hot_16", "one_hot_edge"]  # the cases run at every shape


def real_case(name, M, K, N):
    """dict(x [M][K], w [N][K], b [N] or None) fp32 of case `name`, seeded by the name and (K, N): rows are drawn in order, so the case of
    a smaller M is NOT a prefix -- every shape has inputs of its own."""
    seed = _seed(name, M, K, N)
    x, w, b = REAL_CASES[name](np.random.default_rng(seed), seed, M, K, N)
    return dict(name=name, x=np.ascontiguousarray(x, F32), w=np.ascontiguousarray(w, F32), b=None if b is None else np.ascontiguousarray(b, F32))


def in_domain(c):
    """Zero or [2^-60, 2^60] for every input, [2^-80, 2^80] for every non-zero product."""
    for v in (c["x"], c["w"]) + (() if c["b"] is None else (c["b"],)):
        a = np.abs(v[v != 0].astype(np.float64))
        if not (np.isfinite(v).all() and (a.size == 0 or (a.min() >= 2.0 ** -60 and a.max() <= 2.0 ** 60))):
            return False
    ax, aw = np.abs(c["x"].astype(np.float64)), np.abs(c["w"].astype(np.float64))
    for k in range(ax.shape[1]):  # the extreme products of column k are products of the column's extreme non-zero entries
        xs, ws = ax[:, k][ax[:, k] > 0], aw[:, k][aw[:, k] > 0]
        if xs.size and ws.size and not (xs.min() * ws.min() >= 2.0 ** -80 and xs.max() * ws.max() <= 2.0 ** 80):
            return False
    return True


# ----------------------------------------------------------------------------------------------------------------------
# cases of the spike product
# ----------------------------------------------------------------------------------------------------------------------
def _spike_rows(rng, M, K):
    """Rows in turn: all zero, all one, then random rows of density 0.1, 0.5, 0.9 (five kinds in every 16-row block); the padding columns
    K .. pad64(K) - 1 are zero."""
    s = np.zeros((M, pad64(K)), np.int8)
    dens = np.array([0.0, 1.0, 0.1, 0.5, 0.9])[np.arange(M) % 5]
    s[:, :K] = rng.random((M, K)) < dens[:, None]
    return s


def _sp_control(rng, M, K, N, bits):
    return rng.uniform(-1, 1, (N, K)) / np.sqrt(K), rng.standard_normal(N)


def _sp_saturated(rng, M, K, N, bits):
    return sr._sat_rows(N, K, bits, -9), rng.standard_normal(N)  # |y| <= 320 2^-3: every digit at its extreme, |S| up to 320 QMAX > 2^31


def _sp_digit_extremes(rng, M, K, N, bits):
    H = max(N, K)
    return sr._digit_extremes(rng, H, 1, 1, True, "spike", 38, bits)["W_ih"][:N, :K], None  # (column 0 pins every row's scale: the cut keeps the digits)


def _sp_row_scales(rng, M, K, N, bits):
    return sr._scaled_rows(rng, N, K, 3 % N), rng.standard_normal(N) * 2.0 ** rng.integers(-30, 7, N)


SPIKE_CASES = dict(control=_sp_control, saturated=_sp_saturated, digit_extremes=_sp_digit_extremes, row_scales=_sp_row_scales)


def spike_case(name, M, K, N, bits=24):
    """dict(s int8 [M][pad64(K)], w fp32 [N][K] as given to the packing, b [N] or None, bits)."""
    rng = np.random.default_rng(_seed("spike", name, M, K, N, bits))
    w, b = SPIKE_CASES[name](rng, M, K, N, bits)
    return dict(name=name, s=_spike_rows(rng, M, K), w=np.ascontiguousarray(w, F32), b=None if b is None else np.ascontiguousarray(b, F32), bits=bits)


# ----------------------------------------------------------------------------------------------------------------------
# the shapes test_product_edges.py runs (test_prodref_host.py checks that they reach every compiled form)
# ----------------------------------------------------------------------------------------------------------------------
REAL_N = [64, 224, 320]
REAL_K = [38, 64, 94, 96, 158, 160, 162, 192] + [39, 193]  # even widths on both sides of every k-step threshold; odd K; K = 193 (more than 12 chunks of 16: refused)
REAL_M = [64, 65, 209]
SMALLEST = dict(bf3=(65, 38, 64), f32mfma=(65, 39, 64), plain=(33, 38, 64))  # (M, K, N) at which every case runs
PLAIN_N = (65, 38, 62)  # N % 4 != 0
# (N, K) that reach input_proj_fast_kernel<TPW, KCB> beyond <., 3>: KCB = 6, 10, 12 at one column tile per wave, 6 and 10 at two, 6 at
# three (the wider ones exceed its LDS budget and run the plain kernel)
F32MFMA_NK = [(64, 95), (64, 159), (64, 191), (224, 95), (224, 159), (320, 95)]
SPIKE_K = [48, 64, 224, 268, 320]
SPIKE_N = [6, 40, 64, 192, 320]
