"""``sfsn_resample_down3`` / ``sfsn_resample_up3`` (spectral.resample_down3 / resample_up3) against the float64 reference of
tests/resampleref.py under ITS bound -- ``gamma_K sum |h| |x|`` per element, K = 96 down and 32 up; no tolerance is chosen here.  The
int16 way out is compared with the quantiser of the kernel's own float result (exact) and with the reference wherever the bound leaves
the rounding no choice.  Chunked calls with the carried state equal the one-shot call with ``torch.equal``."""
import ctypes

import numpy as np
import pytest
import torch

import resampleref as rr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LENGTHS = (1, 31, 32, 33, 128, 129)  # outputs (down) / inputs (up): either side of the carried 31 and of one call's 128


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def inside(got, ref, bound, what):
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err - bound).max())
    print(f"{what}: max err {err.max():.3e}, max bound {bound.max():.3e}")
    assert np.all(err <= bound), f"{what}: {worst:.3e} over the bound"


def saturating(B, n):
    """Model-rate samples of +-(32767 / 32768) in the sign pattern of phase 0's taps: the interpolator's output reaches sum |g| > 1."""
    _, g = rr.taps()
    pat = np.sign(g[0][::-1]).astype(np.float32) * np.float32(32767.0 / 32768.0)
    return np.broadcast_to(np.resize(pat, n), (B, n)).copy()


@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("n", LENGTHS)
def test_down3_against_the_reference(B, n):
    from spiking_fullsubnet_amd import spectral
    h, _ = rr.taps()
    rng = np.random.default_rng(100 * B + n)
    for name, x in rr.signals(B, 3 * n, seed=n).items():
        st = rng.standard_normal((B, 96)).astype(np.float32)
        st[:, 93:] = 0.0
        y_ref, bound, st_ref = rr.down3(rr.as_float(x), h, st)
        state = dev(st)
        y, state_out = spectral.resample_down3(dev(x), state)
        assert state_out is state and y.dtype == torch.float32 and tuple(y.shape) == (B, n)
        inside(y.cpu().numpy(), y_ref, bound, f"down {name} B={B} n={n}")
        assert np.array_equal(state.cpu().numpy().astype(np.float64), st_ref), name  # the carried samples are copies: exact
        y0, s0 = spectral.resample_down3(dev(x))  # state=None equals a zero state
        y1, s1 = spectral.resample_down3(dev(x), torch.zeros((B, 96), device=DEV))
        assert torch.equal(y0, y1) and torch.equal(s0, s1)


@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("n", LENGTHS)
def test_up3_against_the_reference(B, n):
    from spiking_fullsubnet_amd import spectral
    _, g = rr.taps()
    rng = np.random.default_rng(200 * B + n)
    sigs = {k: rr.as_float(v) for k, v in rr.signals(B, n, seed=n).items()}
    sigs["saturating"] = saturating(B, n)
    for name, yin in sigs.items():
        st = rng.standard_normal((B, 32)).astype(np.float32) * (0.0 if name == "saturating" else 1.0)
        st[:, 31:] = 0.0
        z_ref, bound, st_ref = rr.up3(yin, g, st)
        state = dev(st)
        z, _ = spectral.resample_up3(dev(yin), state)
        assert z.dtype == torch.float32 and tuple(z.shape) == (B, 3 * n)
        zf = z.cpu().numpy()
        inside(zf, z_ref, bound, f"up {name} B={B} n={n}")
        assert np.array_equal(state.cpu().numpy().astype(np.float64), st_ref), name
        q, _ = spectral.resample_up3(dev(yin), dev(st), sample_format="s16")
        assert q.dtype == torch.int16
        qn = q.cpu().numpy()
        assert np.array_equal(qn, rr.quantise(zf)), name  # Q of the float result, exactly
        # and against the reference: the quantiser is monotone, so Q(ref - bound) <= q <= Q(ref + bound) (float64 ends, exact scale)
        lo = np.clip(np.rint((z_ref - bound) * 32768.0), -32768, 32767)
        hi = np.clip(np.rint((z_ref + bound) * 32768.0), -32768, 32767)
        assert np.all((lo <= qn) & (qn <= hi)), name
        z0, s0 = spectral.resample_up3(dev(yin))
        z1, s1 = spectral.resample_up3(dev(yin), torch.zeros((B, 32), device=DEV))
        assert torch.equal(z0, z1) and torch.equal(s0, s1)
    if n >= 32:  # the way out saturates: sum |g| > 1
        q, _ = spectral.resample_up3(dev(saturating(B, n)), sample_format="s16")
        qn = q.cpu().numpy()
        assert qn.max() == 32767 and qn.min() == -32768
        assert float(np.abs(rr.up3(saturating(B, n), g)[0]).max()) > 1.5


@pytest.mark.parametrize("chunks", ([128, 128, 128], [1, 40, 87]), ids=["128x3", "1-40-87"])
def test_chunked_calls_equal_the_one_shot_call(chunks):
    from spiking_fullsubnet_amd import spectral
    n, B = sum(chunks), 3
    for name in ("noise", "noise_s16"):
        x = dev(rr.signals(B, 3 * n, seed=77)[name])
        y, s_end = spectral.resample_down3(x)
        st, parts, a = None, [], 0
        for c in chunks:
            yp, st = spectral.resample_down3(x[:, 3 * a:3 * (a + c)], st)  # (a strided view of the rows)
            parts.append(yp)
            a += c
        assert torch.equal(torch.cat(parts, dim=1), y) and torch.equal(st, s_end), name
        for fmt in ("f32", "s16"):
            z, u_end = spectral.resample_up3(y, sample_format=fmt)
            st, parts, a = None, [], 0
            for c in chunks:
                zp, st = spectral.resample_up3(y[:, a:a + c], st, sample_format=fmt)
                parts.append(zp)
                a += c
            assert torch.equal(torch.cat(parts, dim=1), z) and torch.equal(st, u_end), (name, fmt)


def test_row_stride_gap_and_sentinels():
    from spiking_fullsubnet_amd import _lib, spectral
    L = _lib.lib()
    B, n, gap = 3, 33, 7
    h, g = spectral.resample_taps(DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    # down: rows of 3 n samples inside rows of 3 n + gap, the gap NaN; the output between two sentinel rows
    x = torch.full((B, 3 * n + gap), float("nan"), device=DEV)
    x[:, :3 * n] = dev(rr.signals(B, 3 * n, seed=5)["noise"])
    out = torch.full((B + 2, n), 12345.0, device=DEV)
    rc = L.sfsn_resample_down3(x.data_ptr(), _lib.SAMPLE_F32, B, n, 3 * n + gap, h.data_ptr(), None, out[1:].data_ptr(), st)
    assert rc == 0
    y_ref, _ = spectral.resample_down3(x[:, :3 * n].contiguous())
    assert torch.equal(out[1:B + 1], y_ref) and bool((out[0] == 12345.0).all()) and bool((out[-1] == 12345.0).all())
    assert not bool(torch.isnan(out).any())
    # up: int16 rows of 3 n samples inside rows of 3 n + gap; the gap and the rows around keep their sentinel
    z = torch.full((B + 2, 3 * n + gap), 1234, dtype=torch.int16, device=DEV)
    rc = L.sfsn_resample_up3(y_ref.data_ptr(), B, n, g.data_ptr(), None, z[1:].data_ptr(), _lib.SAMPLE_S16, 3 * n + gap, st)
    assert rc == 0
    z_ref, _ = spectral.resample_up3(y_ref, sample_format="s16")
    assert torch.equal(z[1:B + 1, :3 * n], z_ref)
    assert bool((z[1:B + 1, 3 * n:] == 1234).all()) and bool((z[0] == 1234).all()) and bool((z[-1] == 1234).all())
    zv = torch.full((B, 3 * n + gap), 1234, dtype=torch.int16, device=DEV)  # the wrapper's out= with strided rows
    spectral.resample_up3(y_ref, sample_format="s16", out=zv[:, :3 * n])
    assert torch.equal(zv[:, :3 * n], z_ref) and bool((zv[:, 3 * n:] == 1234).all())
