"""fp64 reference of the 3:1 decimator and the 1:3 interpolator (include/sfsn.h, csrc/sfsn_resample_dev.h), the per-element error
bound of their fp32 sums, the quantiser, and an fp32 emulation of the stated summation order.  numpy only.

The reference is the plain float64 sum with the float32 taps AS GIVEN (not the float64 design they were rounded from):

    down   y[m] = sum_{k < 96} h[k] x[3 m + 2 - k]                 x[n < 0] = the carried samples, zero at the start
    up     z[3 m + p] = sum_{j < 32} g[p][j] y[m - j]              g[p][j] = fl32(3 h64[3 j + p])

The bound of a K-term fp32 sum in any order with fused or unfused products (Higham, Accuracy and Stability, section 3.1):
``|fl(sum) - sum| <= gamma_K sum_k |h[k]| |x[.]|``, ``gamma_K = K u / (1 - K u)``, ``u = 2**-24``; K = 96 down, K = 32 up.
float64's own error on the same sum is 2**-29 of that and is ignored.
"""
import numpy as np

U = 2.0 ** -24
N_TAPS, N_PHASE = 96, 32
DEC_KEEP, INT_KEEP = 93, 31


def gamma(K: int) -> float:
    return K * U / (1.0 - K * U)


def design64():
    """The float64 design: sinc((k - 47.5) / 3) / 3 * kaiser(96, 8), divided by its sum."""
    k = np.arange(N_TAPS, dtype=np.float64)
    h = np.sinc((k - 47.5) / 3.0) / 3.0 * np.kaiser(N_TAPS, 8.0)
    return h / h.sum()


def taps():
    """``(h float32 [96], g float32 [3, 32])`` as the library takes them."""
    h = design64()
    return h.astype(np.float32), np.stack([3.0 * h[p::3] for p in range(3)]).astype(np.float32)


def response_db(h, freqs_hz, rate=48000.0):
    """Magnitude response of taps ``h`` at ``freqs_hz`` in dB (float64)."""
    h = np.asarray(h, dtype=np.float64)
    w = 2.0 * np.pi * np.asarray(freqs_hz, dtype=np.float64) / rate
    H = np.exp(-1j * np.outer(w, np.arange(len(h)))) @ h
    return 20.0 * np.log10(np.maximum(np.abs(H), 1e-300))


def _history(x, state, keep):
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    st = np.zeros((B, keep)) if state is None else np.asarray(state, dtype=np.float64)[:, :keep]
    return np.concatenate([st, x], axis=1)


def down3(x, h, state=None):
    """``x`` [B, 3 n] (already float: int16 * 2**-15 is exact) -> ``(y float64 [B, n], bound [B, n], new state [B, 96] float64)``."""
    h = np.asarray(h, dtype=np.float64)
    full = _history(x, state, DEC_KEEP)  # full[:, 93 + n] = x[n]
    n = x.shape[1] // 3
    idx = DEC_KEEP + 3 * np.arange(n)[:, None] + 2 - np.arange(N_TAPS)[None, :]  # [n, 96]
    win = full[:, idx]                                                        # [B, n, 96]
    y = win @ h
    bound = gamma(N_TAPS) * (np.abs(win) @ np.abs(h))
    new = np.zeros((x.shape[0], 96))
    new[:, :DEC_KEEP] = full[:, -DEC_KEEP:]
    return y, bound, new


def up3(y, g, state=None):
    """``y`` [R, n] -> ``(z float64 [R, 3 n], bound [R, 3 n], new state [R, 32] float64)``."""
    g = np.asarray(g, dtype=np.float64)
    full = _history(y, state, INT_KEEP)  # full[:, 31 + m] = y[m]
    n = np.asarray(y).shape[1]
    idx = INT_KEEP + np.arange(n)[:, None] - np.arange(N_PHASE)[None, :]  # [n, 32]
    win = full[:, idx]                                                   # [R, n, 32]
    z = np.stack([win @ g[p] for p in range(3)], axis=-1).reshape(full.shape[0], 3 * n)
    bound = gamma(N_PHASE) * np.stack([np.abs(win) @ np.abs(g[p]) for p in range(3)], axis=-1).reshape(full.shape[0], 3 * n)
    new = np.zeros((full.shape[0], 32))
    new[:, :INT_KEEP] = full[:, -INT_KEEP:]
    return z, bound, new


def quantise(v):
    """``clamp(rint(v * 32768), -32768, 32767)`` as int16, ties to even, NaN -> 0 (``v`` float32)."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(v * np.float32(32768.0))
    r = np.where(np.isnan(r), np.float32(0.0), r)
    return np.clip(r, -32768.0, 32767.0).astype(np.int16)


def _fma32(a, b, c):
    """fl32(a b + c) for float32 arrays: the product of two float32 is exact in float64 (48 bits), and the float64 sum with a float32
    is rounded once more to float32 -- double rounding can differ from a fused fp32 operation only when the float64 sum lies within
    2**-53 relative of a float32 tie, which the emulation accepts (it is checked against the BOUND, not for bits)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def down3_f32(x, h, state=None):
    """The stated order in float32: one accumulator from 0, fma, ascending k."""
    full = _history(x, state, DEC_KEEP).astype(np.float32)
    n = np.asarray(x).shape[1] // 3
    acc = np.zeros((full.shape[0], n), dtype=np.float32)
    base = DEC_KEEP + 3 * np.arange(n) + 2
    for k in range(N_TAPS):
        acc = _fma32(np.broadcast_to(np.float32(h[k]), acc.shape), full[:, base - k], acc)
    return acc


def up3_f32(y, g, state=None):
    full = _history(y, state, INT_KEEP).astype(np.float32)
    n = np.asarray(y).shape[1]
    out = np.zeros((full.shape[0], n, 3), dtype=np.float32)
    base = INT_KEEP + np.arange(n)
    for p in range(3):
        acc = np.zeros((full.shape[0], n), dtype=np.float32)
        for j in range(N_PHASE):
            acc = _fma32(np.broadcast_to(np.float32(g[p][j]), acc.shape), full[:, base - j], acc)
        out[:, :, p] = acc
    return out.reshape(full.shape[0], 3 * n)


# ---- the inputs of the kernel tests (tests/test_resample_kernels.py) and of the host tests --------------------------------------------
def signals(B: int, n: int, seed: int = 0):
    """``{name: float32 or int16 [B, n]}``: an impulse at each of the three phases, a step, +-full-scale alternation as int16, noise."""
    rng = np.random.default_rng(seed)
    out = {}
    for p in range(3):
        x = np.zeros((B, n), dtype=np.float32)
        if n > p:
            x[:, p] = 1.0
        if n > p + 3 * 7:
            x[-1, p + 3 * 7] = -0.5
        out[f"impulse{p}"] = x
    out["step"] = np.ones((B, n), dtype=np.float32)
    alt = np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)
    out["fullscale_s16"] = np.broadcast_to(alt, (B, n)).copy()
    out["noise"] = rng.standard_normal((B, n)).astype(np.float32)
    out["noise_s16"] = rng.integers(-32768, 32768, size=(B, n)).astype(np.int16)
    return out


def as_float(x):
    """int16 -> float32 * 2**-15 (exact); float32 as it is."""
    x = np.asarray(x)
    return x.astype(np.float32) * np.float32(2.0 ** -15) if x.dtype == np.int16 else x.astype(np.float32)
