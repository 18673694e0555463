"""The ragged-batch kernels (csrc/sfsn_ragged.hip), export by export, against the EXISTING export called on each clip alone:
bit for bit (``torch.equal``), no tolerance -- a ragged kernel performs its sibling's operations on the same values in the same
order and only skips the terms a clip does not have.  STFT and inverse STFT are also held to the fp64 oracle at the tolerance
tests/test_hip_parity.py uses for their siblings (3e-6 x max|ref|).

Clip table (tests/raggedref.py), hop 128: lengths 200 ... 16600 samples = 2, 16, 17, 19, 33, 65, 130 frames -- either side of
the 16-frame FFT tile and its 3-frame halo, either side of the 64-lane stride of the row sums, some no multiple of the hop."""
import ctypes

import numpy as np
import pytest
import torch

import raggedref as rr
import refweights as rw
from oracle import model as omodel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LENS, FRAMES = rr.CLIP_LENGTHS, rr.CLIP_FRAMES
B, LMAX, TMAX = len(LENS), max(LENS), max(FRAMES)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _real(x):
    return torch.view_as_real(x) if x.is_complex() else x


@pytest.fixture(scope="module")
def hip():
    from spiking_fullsubnet_amd import _lib
    return _lib.lib()


def _junk_spectrum(seed):
    rng = np.random.default_rng(seed)  # arbitrary, not STFT-consistent, non-zero imaginary DC / Nyquist parts, junk past every end
    return (rng.standard_normal((B, 257, TMAX)) + 1j * rng.standard_normal((B, 257, TMAX))).astype(np.complex64)


# ---- STFT -----------------------------------------------------------------------------------------------------------------------
def test_stft_ragged_equals_each_clip_alone():
    from spiking_fullsubnet_amd import spectral
    waves = rr.clip_waves(5)
    junk = torch.from_numpy(rr.pad_batch(waves, junk_seed=6)).to(DEV)  # non-zero junk beyond every clip's end
    assert all(bool((junk[b, L:] != 0).all()) for b, L in enumerate(LENS))
    X = spectral.stft_ragged(junk, 512, 128, _i32(LENS))
    assert tuple(X.shape) == (B, 257, TMAX)
    for b, (L, T) in enumerate(zip(LENS, FRAMES)):
        alone = spectral.stft(junk[b:b + 1, :L].contiguous(), 512, 128)
        assert torch.equal(_real(X[b, :, :T]), _real(alone[0])), b
    # frames t >= T_b: the transform of what remains of the clip, then of zeros = the equal-length kernel on the zero-padded batch
    zero = torch.from_numpy(rr.pad_batch(waves)).to(DEV)
    assert torch.equal(_real(X), _real(spectral.stft(zero, 512, 128)))
    tail = X[0, :, 4:]
    assert not bool(_real(tail).any())  # clip 0 (200 samples): frames from 4 on see nothing of it
    ref = omodel.stft(rr.pad_batch(waves))
    np.testing.assert_allclose(X.cpu().numpy(), ref, atol=3e-6 * np.abs(ref).max(), rtol=0)


# ---- inverse STFT ---------------------------------------------------------------------------------------------------------------
def test_istft_ragged_equals_each_clip_alone():
    from spiking_fullsubnet_amd import spectral
    Z = _junk_spectrum(7)
    Zd = torch.from_numpy(Z).to(DEV)
    y = spectral.istft_ragged(Zd, 512, 128, LMAX, _i32(FRAMES), _i32(LENS))
    assert tuple(y.shape) == (B, LMAX)
    for b, (L, T) in enumerate(zip(LENS, FRAMES)):
        alone = spectral.istft(Zd[b:b + 1, :, :T].contiguous(), 512, 128, length=L)
        assert torch.equal(y[b, :L], alone[0]), b
        assert not bool(y[b, L:].any()), b  # exactly 0 beyond the clip
    ref = rr.istft_ref(Z, FRAMES, LENS)
    np.testing.assert_allclose(y.cpu().numpy(), ref, atol=3e-6 * np.abs(ref).max(), rtol=0)
    # not vacuous: without the lengths the junk frames reach every shorter clip's last samples
    plain = spectral.istft(Zd, 512, 128, length=LMAX)
    assert all(not torch.equal(plain[b, :L], y[b, :L]) for b, L in enumerate(LENS[:-1]))


def test_istft_ragged_with_full_lengths_is_the_equal_length_kernel():
    from spiking_fullsubnet_amd import spectral
    Zd = torch.from_numpy(_junk_spectrum(8)).to(DEV)
    for length in (LMAX, (TMAX - 1) * 128, 16 * 128 - 256 + 1):  # the last: one sample into the second tile
        y = spectral.istft_ragged(Zd, 512, 128, length, _i32([TMAX] * B), _i32([length] * B))
        assert torch.equal(y, spectral.istft(Zd, 512, 128, length=length)), length


# ---- utterance statistics ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frozen_engine():
    import spiking_fullsubnet_amd as pkg
    kw = rw.FROZEN_TINY
    m = pkg.Separator(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in rw.frozen_state_dict(kw, 3).items()}, strict=True)
    return m.eval().to(DEV).engine()


@pytest.mark.parametrize("gaussian", [False, True], ids=["laplace", "gaussian"])
@pytest.mark.parametrize("with_fb", [False, True], ids=["fullband", "subband+fb_tbf"])
def test_statistics_ragged_equal_each_clip_alone(hip, frozen_engine, gaussian, with_fb):
    from spiking_fullsubnet_amd._lib import check
    eng, spec = frozen_engine, frozen_engine.spec
    F, FB = 257, spec.fb_proj if with_fb else 0
    groups = eng._feature_groups("sb", None, None) if with_fb else eng._feature_groups("fb", [None], None)
    ng = spec.n_groups if with_fb else 1
    stft = torch.from_numpy(_junk_spectrum(9)).to(DEV)
    fb = torch.rand((TMAX, B, spec.fb_proj), generator=torch.Generator().manual_seed(10)).to(DEV) if with_fb else None

    def run(ri, fb_, nb, T, frames):
        mu, sd = torch.full((ng, nb), float("nan"), device=DEV), torch.full((ng, nb), float("nan"), device=DEV)
        scratch = torch.empty(((5 if gaussian else 1) * nb * (F - 1 + FB) + 2,), device=DEV)
        head = (_p(ri), _p(fb_), nb, F, T, FB, spec.fdrc, groups, ng)
        if frames is None and gaussian:
            check(hip.sfsn_gaussian_stats(*head, _p(mu), _p(sd), _p(scratch), None), "gaussian_stats")
        elif frames is None:
            check(hip.sfsn_laplace_means(*head, _p(mu), _p(scratch), None), "laplace_means")
        elif gaussian:
            check(hip.sfsn_gaussian_stats_ragged(*head, _p(frames), _p(mu), _p(sd), _p(scratch), None), "gaussian_stats_ragged")
        else:
            check(hip.sfsn_laplace_means_ragged(*head, _p(frames), _p(mu), _p(scratch), None), "laplace_means_ragged")
        torch.cuda.synchronize()
        return mu, sd

    mu, sd = run(torch.view_as_real(stft), fb, B, TMAX, _i32(FRAMES))
    for b, T in enumerate(FRAMES):
        one = torch.view_as_real(stft[b:b + 1, :, :T].contiguous())
        mu1, sd1 = run(one, None if fb is None else fb[:T, b:b + 1].contiguous(), 1, T, None)
        assert torch.equal(mu[:, b], mu1[:, 0]), b
        if gaussian:
            assert torch.equal(sd[:, b], sd1[:, 0]), b
    # not vacuous: the equal-length call on the padded batch gives other means for every shorter clip
    mu_pad, _ = run(torch.view_as_real(stft), fb, B, TMAX, None)
    assert bool((mu_pad[:, :-1] != mu[:, :-1]).all()) and torch.equal(mu_pad[:, -1], mu[:, -1])


# ---- per-clip spike counts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rpc", [1, 3])
def test_spike_count_rows_ragged(hip, rpc):
    from spiking_fullsubnet_amd._lib import RowCount, check
    HP = 64
    g = torch.Generator().manual_seed(11 + rpc)
    tens = [(torch.rand((TMAX, B * rpc, HP), generator=g) < p).to(torch.int8).to(DEV) for p in (0.3, 0.05)]
    frames = _i32(FRAMES)

    def ragged(t0, nt, counts):
        arr = (RowCount * len(tens))()
        for i, t in enumerate(tens):
            arr[i].spikes_i8, arr[i].T, arr[i].R, arr[i].HP, arr[i].rows_per_clip = t.data_ptr(), TMAX, B * rpc, HP, rpc
            arr[i].counts = counts.data_ptr() + 8 * i * B
        check(hip.sfsn_spike_count_rows_ragged(arr, len(tens), t0, nt, _p(frames), B, None), "spike_count_rows_ragged")

    def alone(t, b, t0, nt):
        """the existing export on clip b alone, window cut at the clip's end (an empty window is not a call: 0)"""
        T = FRAMES[b]
        nt = min(nt, T - t0)
        if nt <= 0:
            return 0
        one = t[:T, b * rpc:(b + 1) * rpc].contiguous()
        cnt = torch.zeros((1,), dtype=torch.int64, device=DEV)
        arr = (RowCount * 1)()
        arr[0].spikes_i8, arr[0].T, arr[0].R, arr[0].HP, arr[0].rows_per_clip, arr[0].counts = one.data_ptr(), T, rpc, HP, rpc, cnt.data_ptr()
        check(hip.sfsn_spike_count_rows(arr, 1, t0, nt, None), "spike_count_rows")
        return int(cnt.item())

    # windows that start before, straddle and lie beyond the clips' ends (2, 16, 17, 19, 33, 65, 130 frames)
    for t0, nt in ((0, TMAX), (0, 10), (15, 10), (1, 1), (17, 47), (64, 2), (70, 60)):
        counts = torch.zeros((len(tens), B), dtype=torch.int64, device=DEV)
        ragged(t0, nt, counts)
        torch.cuda.synchronize()
        for i, t in enumerate(tens):
            want = [alone(t, b, t0, nt) for b in range(B)]
            direct = [int(t[t0:min(t0 + nt, FRAMES[b]), b * rpc:(b + 1) * rpc].sum()) for b in range(B)]
            assert counts[i].tolist() == want == direct, (t0, nt, i)
    # counts are accumulated: two windows that tile the clip add up to the whole
    counts = torch.full((len(tens), B), 7, dtype=torch.int64, device=DEV)
    ragged(0, 20, counts)
    ragged(20, TMAX - 20, counts)
    torch.cuda.synchronize()
    for i, t in enumerate(tens):
        assert counts[i].tolist() == [7 + int(t[:FRAMES[b], b * rpc:(b + 1) * rpc].sum()) for b in range(B)]


# ---- zeroing the frames past each clip's end ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,width", [(70, 2), (257, 1), (3, 5)])
def test_zero_tail_frames(hip, rows, width):
    from spiking_fullsubnet_amd._lib import check
    x = (torch.rand((B, rows, TMAX, width), generator=torch.Generator().manual_seed(rows)) + 1.0).to(DEV)
    want = x * (torch.arange(TMAX, device=DEV)[None, :] < _i32(FRAMES)[:, None])[:, None, :, None]
    check(hip.sfsn_zero_tail_frames(_p(x), B, rows, TMAX, width, _p(_i32(FRAMES)), None), "zero_tail_frames")
    torch.cuda.synchronize()
    assert torch.equal(x, want)
    assert bool((x[-1] >= 1.0).all()) and not bool(x[0, :, 2:].any())  # the longest clip is untouched, the shortest keeps 2 frames
