"""features_kernel with a lane per (frame, unit) row for the LayerNorm statistics and a wave per frame for the stores, against the
two implementations that keep a wave per row and the DPP wave reductions: sfsn_features_proj with rows-only jobs (w = NULL) where
it takes the shape, the wave-per-row body of features_kernel itself (SFSN_FEAT_ROWS=wave) where it refuses it.  Bit for bit, the
NaN canaries of rows outside [t0, t0 + nt) included."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def hip():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    assert L.sfsn_device_count() >= 1
    return L


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# (name, B, F, T, FB, [(lo, n_units, ctr, nbr, ctr_fb, nbr_fb)], t0, nt); nt = None: the whole sequence
M_GROUPS = [(0, 8, 4, 15, 4, 0), (32, 3, 32, 15, 32, 0), (128, 2, 64, 15, 64, 0)]       # baseline_m: I = 38 / 94 / 158
WSJ0_GROUPS = [(0, 8, 2, 7, 2, 0), (16, 3, 16, 7, 16, 0), (64, 2, 32, 7, 32, 0)]        # LIVE_WSJ0: I = 18 / 46 / 78
CASES = [
    ("baseline_m", 2, 257, 70, 64, M_GROUPS, 0, None),
    ("wsj0", 2, 129, 70, 32, WSJ0_GROUPS, 0, None),
    ("baseline_m_t0_ragged", 3, 257, 90, 64, M_GROUPS, 37, 41),
    ("wsj0_b1_t33", 1, 129, 33, 32, WSJ0_GROUPS, 0, None),
    ("baseline_m_b1_t31", 1, 257, 31, 64, M_GROUPS, 0, None),
    ("baseline_m_nt1", 2, 257, 50, 64, M_GROUPS, 45, 1),
    ("fullband_group_I64", 2, 257, 40, 0, [(0, 1, 64, 0, 0, 0)], 3, 35),
    ("I256_two_units", 2, 257, 40, 64, [(0, 2, 64, 64, 64, 0)], 0, None),
    ("I64_exactly_no_fb", 2, 257, 45, 0, [(0, 4, 32, 16, 0, 0)], 5, 38),
    ("I65_one_unit_and_I129_odd_units", 2, 257, 40, 64, [(0, 1, 33, 16, 0, 0), (40, 3, 65, 32, 0, 0)], 0, None),
    ("I65_with_fb_odd_units", 2, 257, 35, 64, [(0, 5, 31, 15, 4, 0), (160, 7, 8, 20, 16, 1)], 2, 33),
    ("many_small_units", 2, 257, 40, 64, [(0, 40, 2, 3, 2, 0), (80, 17, 4, 3, 0, 0)], 0, None),
    ("fb_48_columns", 2, 257, 40, 48, [(0, 8, 4, 15, 4, 0), (128, 2, 64, 15, 64, 0)], 7, 30),
]


def _inputs(rng, B, F, T, FB):
    """Spectrum with magnitudes over 1e-6 .. 1e3 and one frame of digital silence; full-band columns with exact -0.0f / +0.0f."""
    scale = 10.0 ** rng.uniform(-6.0, 3.0, (B, F, T, 1))
    ri = (rng.standard_normal((B, F, T, 2)) * scale).astype(np.float32)
    tz = T // 2
    ri[:, :, tz, :] = 0.0
    fbp = None
    if FB:
        fbp = rng.standard_normal((T, B, FB)).astype(np.float32)
        fbp[tz] = 0.0
        z = rng.random((T, B, FB))
        fbp[z < 0.05] = -0.0
        fbp[(z >= 0.05) & (z < 0.10)] = 0.0
        fbp[1, :, :] = -0.0  # a frame whose full-band part is all negative zeros
    return ri, fbp


def _run(hip, monkeypatch, rng, B, F, T, FB, groups, norm, t0, nt):
    """x per group from sfsn_features and from the reference that takes the shape; returns (xa, xb, which reference)."""
    from spiking_fullsubnet_amd import _lib
    from spiking_fullsubnet_amd._lib import FeatProjJob, FeatureGroup, check
    ri_np, fb_np = _inputs(rng, B, F, T, FB)
    ri, fbp = _t(ri_np), (None if fb_np is None else _t(fb_np))
    n = len(groups)
    fg, fw, jobs, keep, xs = (FeatureGroup * n)(), (FeatureGroup * n)(), (FeatProjJob * n)(), [], ([], [], [])
    for i, (lo, nu, ctr, nbr, cfb, nfb) in enumerate(groups):
        I = ctr + 2 * nbr + (cfb + 2 * nfb if cfb else 0)
        ts = []
        if norm == _lib.NORM_LAYERNORM:
            lb = rng.standard_normal(I).astype(np.float32) * 0.1
            lb[rng.random(I) < 0.3] = 0.0
            ts = [_t(rng.uniform(0.5, 1.5, I).astype(np.float32)), _t(lb)]
        elif norm == _lib.NORM_LAPLACE:
            ts = [_t(rng.uniform(0.5, 2.0, B).astype(np.float32))]
        elif norm == _lib.NORM_GAUSSIAN:
            ts = [_t(rng.uniform(0.5, 2.0, B).astype(np.float32)), _t(rng.uniform(0.5, 2.0, B).astype(np.float32))]
        keep.append(ts)
        for g, store in ((fg[i], xs[0]), (fw[i], xs[1]), (jobs[i].feat, xs[2])):
            g.lo, g.n_units, g.ctr, g.nbr, g.ctr_fb, g.nbr_fb, g.norm, g.ln_eps = lo, nu, ctr, nbr, cfb, nfb, norm, 1e-5
            if norm == _lib.NORM_LAYERNORM:
                g.ln_w, g.ln_b = ts[0].data_ptr(), ts[1].data_ptr()
            elif norm == _lib.NORM_LAPLACE:
                g.mu = ts[0].data_ptr()
            elif norm == _lib.NORM_GAUSSIAN:
                g.mu, g.ln_w = ts[0].data_ptr(), ts[1].data_ptr()
            x = torch.full((T, B * nu, I), float("nan"), device=DEV)
            g.x = x.data_ptr()
            store.append(x)
    monkeypatch.delenv("SFSN_FEAT_ROWS", raising=False)
    check(hip.sfsn_features(_p(ri), _p(fbp), B, F, T, FB, 0.5, fg, n, t0, nt, None), "sfsn_features")
    rc = hip.sfsn_features_proj(_p(ri), _p(fbp), B, F, T, FB, 0.5, jobs, n, t0, nt, None, 0, None)
    torch.cuda.synchronize()
    if rc == 0:
        return xs[0], xs[2], "featproj"
    assert rc == _lib.SFSN_EUNSUPPORTED, rc
    monkeypatch.setenv("SFSN_FEAT_ROWS", "wave")
    check(hip.sfsn_features(_p(ri), _p(fbp), B, F, T, FB, 0.5, fw, n, t0, nt, None), "sfsn_features (wave per row)")
    torch.cuda.synchronize()
    monkeypatch.delenv("SFSN_FEAT_ROWS", raising=False)
    return xs[0], xs[1], "wave"


@pytest.mark.parametrize("norm", ["layernorm", "laplace", "gaussian", "none"])
def test_lane_per_row_features_equal_the_wave_per_row_references(hip, monkeypatch, norm):
    """Every case is compared with one of the two references; baseline_m's and WSJ0's geometry must be taken by sfsn_features_proj
    (an implementation in another file), the shapes it refuses go to the wave-per-row body."""
    from spiking_fullsubnet_amd import _lib
    nm = dict(layernorm=_lib.NORM_LAYERNORM, laplace=_lib.NORM_LAPLACE, gaussian=_lib.NORM_GAUSSIAN, none=_lib.NORM_NONE)[norm]
    rng = np.random.default_rng(2024)
    how = {}
    for name, B, F, T, FB, groups, t0, nt in CASES:
        nt = T if nt is None else nt
        xa, xb, ref = _run(hip, monkeypatch, rng, B, F, T, FB, groups, nm, t0, nt)
        how[name] = ref
        for gi, (a, b) in enumerate(zip(xa, xb)):
            assert bool(torch.isnan(a[:t0]).all()) and bool(torch.isnan(a[t0 + nt:]).all()), (name, norm, gi)
            assert not bool(torch.isnan(a[t0:t0 + nt]).any()), (name, norm, gi)
            assert _same(a, b), (name, norm, gi, ref)
    print(how)
    assert len(how) == len(CASES)
    assert how["baseline_m"] == "featproj" and how["wsj0"] == "featproj", how


def test_wave_per_row_switch_is_read_on_every_call(hip, monkeypatch):
    """SFSN_FEAT_ROWS=wave selects the reference body for that call only; both bodies fill the same rows."""
    from spiking_fullsubnet_amd import _lib
    rng = np.random.default_rng(7)
    xa, xb, ref = _run(hip, monkeypatch, rng, 2, 257, 40, 64, [(0, 2, 64, 64, 64, 0)], _lib.NORM_LAYERNORM, 0, 40)
    assert ref == "wave" and _same(xa[0], xb[0])
