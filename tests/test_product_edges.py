"""The time-parallel products through the C ABI against the fp64 references of tests/prodref.py, under its derived per-element bounds:
sfsn_input_proj_f32 on every compiled form (the nine bf3 instances, the fp32-MFMA kernel, the plain kernel), sfsn_spike_proj on both
kernels, both _multi entries and the z of sfsn_features_proj.  Every output starts as NaN canaries: the gap columns of a pitch
ld > N, the rows after M and the floats behind the buffer must still hold them.  The wrap shapes have more 64-row tiles than the
launch has workgroups, so that workgroups take a second tile through the prefetch / park path, and a partial last tile.  Every test
prints its worst error / tolerance per form; the criterion is <= 1 (profiles/product_edges.md records a run)."""
import ctypes

import numpy as np
import pytest
import torch

import frontback as fbk
import prodref as pr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 64  # canary floats behind every output buffer


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _at(a, off):
    """`a` on the device, `off` bytes (a multiple of 4) behind a 256-byte boundary; keep the returned tensor alive."""
    if a is None:
        return None
    buf = torch.zeros(a.size + 64, dtype=torch.float32, device=DEV)
    v = buf[off // 4:off // 4 + a.size].view(*a.shape)
    v.copy_(_t(a))
    assert buf.data_ptr() % 256 == 0 and v.data_ptr() % 256 == off
    return v


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _canary(rows, ld, off=0):
    """A NaN-filled [rows][ld] output with PAD more NaNs behind it, `off` bytes behind a 256-byte boundary: (view, whole buffer)."""
    buf = torch.full((off // 4 + rows * ld + PAD,), float("nan"), device=DEV)
    assert buf.data_ptr() % 256 == 0
    return buf[off // 4:off // 4 + rows * ld].view(rows, ld), buf


@pytest.fixture(scope="module")
def hip():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    assert L.sfsn_device_count() >= 1
    return L


@pytest.fixture(scope="module")
def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Worst(dict):
    """Worst error / tolerance per form, and every failure of a test (all are printed before the test fails)."""

    def __init__(self):
        super().__init__()
        self.fails = []

    def note(self, key, ok, why, ratio, *info):
        self[key] = max(self.get(key, 0.0), ratio)
        if not ok:
            self.fails.append((key,) + info + (why,))
            print("FAILED:", key, info, why)

    def done(self, what):
        print(f"{what} worst error/tolerance: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(self.items())))
        assert not self.fails, (len(self.fails), self.fails[:8])


# ----------------------------------------------------------------------------------------------------------------------
# sfsn_input_proj_f32
# ----------------------------------------------------------------------------------------------------------------------
def _input_proj(hip, c, ld, x_off=0, w_off=0):
    """One call on case c: (rc, buffer [M + 2][ld] as numpy, the floats behind it still NaN)."""
    M, K = c["x"].shape
    N = len(c["w"])
    x, w, b = _at(c["x"], x_off), _at(c["w"], w_off), (None if c["b"] is None else _t(c["b"]))
    z, zb = _canary(M + 2, ld)
    rc = hip.sfsn_input_proj_f32(_p(x), _p(w), _p(b), _p(z), M, K, N, ld, None)
    torch.cuda.synchronize()
    return rc, z.cpu().numpy(), bool(torch.isnan(zb[-PAD:]).all())


def _check_input_proj(hip, w, name, M, K, N, ld, x_off=0, w_off=0, want_form=None):
    from spiking_fullsubnet_amd import _lib
    f = pr.form(M, K, N, ld, x_off)
    assert want_form is None or f == want_form, (f, want_form, M, K, N, ld, x_off)
    c = pr.real_case(name, M, K, N)
    rc, buf, tail = _input_proj(hip, c, ld, x_off, w_off)
    if f == "unsupported":
        assert rc == _lib.SFSN_EUNSUPPORTED and np.isnan(buf).all() and tail, (rc, M, K, N)  # a refused call writes nothing
        return f
    assert rc == 0 and tail, (rc, tail, M, K, N, ld)
    z, tol = pr.real_reference(c["x"], c["w"], c["b"], "bf3" if f == "bf3" else "f32")
    key = f if f != "bf3" else f"bf3{(pr.pick_tiling(N)[0], pr.ksb(K))}"
    w.note(key, *pr.check(buf, M, N, z, tol), name, M, K, N, ld, x_off, w_off)
    return f


@pytest.mark.parametrize("N", pr.REAL_N)
def test_input_proj_every_compiled_form(hip, N):
    """The N x K x M grid of prodref: every bf3 instance where prodref.form says bf3 (N = 64 / 224 / 320 is 1 / 2 / 3 column tiles per wave, K
    selects 2, 3, 5 or 6 k-steps), the fp32 kernels elsewhere (odd K, TPW KSB > 12, the uninstantiated (2, 6)); K = 193 is refused.
    M = 64 with ld = N, M = 65 with ld = N + 4, M = 209 (three full tiles and 17 rows) with ld = N + 8."""
    w, forms = Worst(), set()
    for K in pr.REAL_K:
        for M, ld in zip(pr.REAL_M, (N, N + 4, N + 8)):
            for name in pr.REAL_QUICK:
                forms.add(_check_input_proj(hip, w, name, M, K, N, ld))
    assert "bf3" in forms and "unsupported" in forms and ("f32mfma" in forms or "plain" in forms), forms
    w.done(f"sfsn_input_proj_f32 N={N}")


def test_input_proj_fp32_mfma_instances(hip):
    """The shape list above reaches input_proj_fast_kernel only at K = 39 (three chunks of 16): its wider instances through odd K."""
    w = Worst()
    for N, K in pr.F32MFMA_NK:
        for M, ld in ((65, N + 4), (209, N + 8)):
            for name in pr.REAL_QUICK:
                _check_input_proj(hip, w, name, M, K, N, ld, want_form="f32mfma")
    w.done("sfsn_input_proj_f32, fp32-MFMA instances")


def test_input_proj_all_cases_at_the_smallest_shape_of_each_form(hip):
    """Every case at (65, 38, 64) bf3, (65, 39, 64) fp32-MFMA, (33, 38, 64) and (65, 38, 62) plain, with both pitches; then the
    pointer alignments: x 8 bytes behind a 16-byte boundary stays on the bf3 kernel (its loads are 8 bytes wide), x 4 bytes behind
    one takes the fp32-MFMA kernel, w 4 bytes behind one (the dispatch does not look at w; the bf3 kernel loads it as dword-aligned
    16-byte vectors) on every form."""
    w = Worst()
    shapes = [(f,) + s for f, s in pr.SMALLEST.items()] + [("plain",) + pr.PLAIN_N]
    for f, M, K, N in shapes:
        for name in pr.REAL_CASES:
            for ld in (N + 4, N + 8) if N % 4 == 0 else (N + 2, N + 6):  # (N = 62: both pitches a multiple of 4, the plain kernel's vector stores)
                _check_input_proj(hip, w, name, M, K, N, ld, want_form=f)
            _check_input_proj(hip, w, name, M, K, N, ld, w_off=4, want_form=f)
    M, K, N = pr.SMALLEST["bf3"]
    for name in pr.REAL_CASES:
        _check_input_proj(hip, w, name, M, K, N, N + 4, x_off=8, want_form="bf3")
        _check_input_proj(hip, w, name, M, K, N, N + 4, x_off=8, w_off=4, want_form="bf3")
        _check_input_proj(hip, w, name, M, K, N, N + 4, x_off=4, want_form="f32mfma")
        _check_input_proj(hip, w, name, M, 192, N, N + 4, w_off=4, want_form="bf3")  # every k-step whole: all weights through the 16-byte loads
    w.done("sfsn_input_proj_f32, smallest shapes and alignments")


def test_input_proj_second_tile_of_a_workgroup(hip, n_cu):
    """M = 64 (n_cu + 3) + 5: the bf3 launch has n_cu workgroups, so workgroups 0 .. 3 take a second tile (fetch(nxt) / park()) and the
    last tile has five rows.  The fp32-MFMA launch is capped at 512 workgroups, not at the CU count: it is run at that M and at
    M = 64 (512 + 3) + 5, where it wraps.  one_hot (row m is told from row m - 64 nblk by its column) and control (a generator
    per tile)."""
    w = Worst()
    M = 64 * (n_cu + 3) + 5
    assert pr.grid("bf3", M, 64, n_cu) < (M + 63) // 64
    M2 = 64 * (pr.F32_GRID_CAP + 3) + 5
    assert pr.grid("f32mfma", M2, 64, n_cu) < (M2 + 63) // 64
    for name in pr.REAL_QUICK:
        _check_input_proj(hip, w, name, M, 38, 64, 68, want_form="bf3")
        _check_input_proj(hip, w, name, M, 39, 64, 68, want_form="f32mfma")
    for name in ("one_hot_w8", "control"):
        _check_input_proj(hip, w, name, M, 94, 224, 224, want_form="bf3")   # two column tiles per wave, three k-steps
        _check_input_proj(hip, w, name, M2, 39, 64, 68, want_form="f32mfma")
    w.done(f"sfsn_input_proj_f32, {n_cu} CUs, M = {M} / {M2}")


# ----------------------------------------------------------------------------------------------------------------------
# sfsn_spike_proj
# ----------------------------------------------------------------------------------------------------------------------
def _spike_tensors(c):
    from spiking_fullsubnet_amd.engine import pack_w3
    pk, dq = pack_w3(c["w"], c["bits"])
    return [_t(c["s"]), _t(pk), _t(dq), None if c["b"] is None else _t(c["b"])]


def _check_spike_proj(hip, w, name, M, K, N, ld, bits=24, y_off=0, want_form=None):
    f = pr.spike_form(M, K, N, ld, y_off)
    assert f in ("fast", "generic") and (want_form is None or f == want_form), (f, want_form, M, K, N, ld, y_off)
    c = pr.spike_case(name, M, K, N, bits)
    ts = _spike_tensors(c)
    y, yb = _canary(M + 2, ld, y_off)
    rc = hip.sfsn_spike_proj(_p(ts[0]), _p(ts[1]), _p(ts[2]), _p(ts[3]), _p(y), M, K, N, ld, None)
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.isnan(yb[-PAD:]).all()) and bool(torch.isnan(yb[:y_off // 4]).all()), (rc, name, M, K, N, ld)
    ref = pr.spike_reference(c["s"], c["w"], c["b"], bits)
    w.note(f, *pr.check(y.cpu().numpy(), M, N, ref["y"], ref["tol"], ref["every"], ref["want"]), name, M, K, N, ld, bits, y_off)
    return f, ref


@pytest.mark.parametrize("K", pr.SPIKE_K)
def test_spike_proj_both_kernels(hip, K):
    """The K x N grid of prodref (K = 268 is padded to 320 columns): M = 209 with ld = N + 4 and M = 65 with ld = N on the fast kernel where
    N % 4 == 0 (the generic one for N = 6), M = 47 with ld = N + 8 on the generic kernel; saturated rows, corner digits, row scales
    with a zero row and the mild control, spike rows all zero / all one / random; weights of 24 and of 16 bits."""
    w, forms, big = Worst(), set(), 0
    for N in pr.SPIKE_N:
        for M, ld in ((209, N + 4), (65, N), (47, N + 8)):
            for name, bits in [(n, b) for n in pr.SPIKE_CASES for b in (24, 16)]:
                f, ref = _check_spike_proj(hip, w, name, M, K, N, ld, bits)
                forms.add(f)
                big += int((~ref["exact"]).sum())
    assert forms == {"fast", "generic"} and big > 0
    w.done(f"sfsn_spike_proj K={K} ({big} results with |S| >= 2^24)")


def test_spike_proj_output_4_bytes_behind_a_16_byte_boundary(hip):
    """The fast kernel's row stores need 16 bytes: such a y takes the generic kernel's scalar stores, and the floats in front of it
    stay untouched."""
    w = Worst()
    for name in pr.SPIKE_CASES:
        for off in (4, 8, 12):
            _check_spike_proj(hip, w, name, 209, 224, 64, 68, y_off=off, want_form="generic")
        _check_spike_proj(hip, w, name, 209, 224, 64, 68, want_form="fast")
    w.done("sfsn_spike_proj, y offset")


def test_spike_proj_second_tile_of_a_workgroup(hip, n_cu):
    """One column tile per wave: 2 n_cu workgroups, M = 64 (2 n_cu + 3) + 5; two per wave: n_cu workgroups, M = 64 (n_cu + 3) + 5."""
    w = Worst()
    M1, M2 = 64 * (2 * n_cu + 3) + 5, 64 * (n_cu + 3) + 5
    assert pr.pick_tiling(64)[0] == 1 and pr.grid("fast", M1, 64, n_cu) < (M1 + 63) // 64
    assert pr.pick_tiling(192)[0] == 2 and pr.grid("fast", M2, 192, n_cu) < (M2 + 63) // 64
    for name in ("control", "saturated"):
        _check_spike_proj(hip, w, name, M1, 64, 64, 68, want_form="fast")
        _check_spike_proj(hip, w, name, M2, 224, 192, 196, want_form="fast")
    w.done(f"sfsn_spike_proj, {n_cu} CUs, M = {M1} / {M2}")


# ----------------------------------------------------------------------------------------------------------------------
# the _multi entries
# ----------------------------------------------------------------------------------------------------------------------
def test_input_proj_multi_jobs_of_different_tilings_in_one_launch(hip, n_cu):
    """Four jobs on four bf3 instances, (1, 2), (2, 3), (1, 6), (2, 5); the block ranges of deal_blocks (restated) leave the first and
    the last job fewer workgroups than tiles, so their workgroups loop inside a block range.  Bit for bit the single launches
    (held to the reference by the tests above); the first and the last job also directly against fp64."""
    from spiking_fullsubnet_amd._lib import InProjJob
    shapes = [(64 * 300 + 5, 38, 64), (209, 94, 224), (130, 192, 64), (64 * 200 + 7, 158, 224)]
    names = ["one_hot_w8", "control", "one_hot_16", "control"]
    assert [(pr.pick_tiling(N)[0], pr.ksb(K)) for M, K, N in shapes] == [(1, 2), (2, 3), (1, 6), (2, 5)]
    nb, ns = pr.inproj_multi_blocks(shapes, n_cu)
    assert nb[0] < ns[0] and nb[3] < ns[3] and all(1 <= b <= n for b, n in zip(nb, ns)), (nb, ns)
    jobs, keep, outs, w = (InProjJob * 4)(), [], [], Worst()
    for j, (M, K, N), name in zip(jobs, shapes, names):
        ld = N + 4
        assert pr.multi_ok(M, K, N, ld)
        c = pr.real_case(name, M, K, N)
        ts = [_t(c["x"]), _t(c["w"]), None if c["b"] is None else _t(c["b"])]
        (z1, b1), (z2, b2) = _canary(M + 2, ld), _canary(M + 2, ld)
        assert hip.sfsn_input_proj_f32(_p(ts[0]), _p(ts[1]), _p(ts[2]), _p(z1), M, K, N, ld, None) == 0
        j.x, j.w, j.bias, j.z, j.M, j.K, j.N, j.ldz = ts[0].data_ptr(), ts[1].data_ptr(), None if ts[2] is None else ts[2].data_ptr(), z2.data_ptr(), M, K, N, ld
        keep.append(ts)
        outs.append((c, b1, b2, z2))
    assert hip.sfsn_input_proj_f32_multi(jobs, 4, None) == 0
    torch.cuda.synchronize()
    for i, ((c, b1, b2, z2), (M, K, N)) in enumerate(zip(outs, shapes)):
        assert torch.equal(b1.view(torch.int32), b2.view(torch.int32)), (i, "the multi launch differs from the single launch")
        if i in (0, 3):
            z, tol = pr.real_reference(c["x"], c["w"], c["b"], "bf3")
            w.note(f"job{i}", *pr.check(z2.cpu().numpy(), M, N, z, tol), M, K, N)
    w.done(f"sfsn_input_proj_f32_multi, blocks {nb} for {ns} tiles,")


def test_spike_proj_multi_jobs_of_different_tilings_in_one_launch(hip, n_cu):
    """Four jobs of K = 224 with one and two column tiles per wave; the two large jobs get fewer workgroups than tiles."""
    from spiking_fullsubnet_amd._lib import ProjJob
    K = 224
    shapes = [(64 * 300 + 5, K, 40), (64 * 150 + 9, K, 192), (209, K, 64), (64, K, 128)]
    names = ["saturated", "control", "digit_extremes", "row_scales"]
    assert [pr.pick_tiling(N)[0] for M, K, N in shapes] == [1, 2, 1, 1]
    nb, ns = pr.spike_multi_blocks(shapes, n_cu)
    assert nb[0] < ns[0] and nb[1] < ns[1] and all(1 <= b <= n for b, n in zip(nb, ns)), (nb, ns)
    jobs, keep, outs, w = (ProjJob * 4)(), [], [], Worst()
    for j, (M, K, N), name in zip(jobs, shapes, names):
        ld = N + 4
        assert pr.spike_multi_ok(M, K, N, ld)
        c = pr.spike_case(name, M, K, N)
        ts = _spike_tensors(c)
        (y1, b1), (y2, b2) = _canary(M + 2, ld), _canary(M + 2, ld)
        assert hip.sfsn_spike_proj(_p(ts[0]), _p(ts[1]), _p(ts[2]), _p(ts[3]), _p(y1), M, K, N, ld, None) == 0
        j.s, j.w_packed, j.w_dq, j.bias, j.y = ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), None if ts[3] is None else ts[3].data_ptr(), y2.data_ptr()
        j.M, j.K, j.N, j.ldy = M, K, N, ld
        keep.append(ts)
        outs.append((c, b1, b2, y2))
    assert hip.sfsn_spike_proj_multi(jobs, 4, None) == 0
    torch.cuda.synchronize()
    for i, ((c, b1, b2, y2), (M, K, N)) in enumerate(zip(outs, shapes)):
        assert torch.equal(b1.view(torch.int32), b2.view(torch.int32)), (i, "the multi launch differs from the single launch")
        if i in (0, 1):
            ref = pr.spike_reference(c["s"], c["w"], c["b"])
            w.note(f"job{i}", *pr.check(y2.cpu().numpy(), M, N, ref["y"], ref["tol"], ref["every"], ref["want"]), M, K, N)
    w.done(f"sfsn_spike_proj_multi, blocks {nb} for {ns} tiles,")


# ----------------------------------------------------------------------------------------------------------------------
# sfsn_features_proj with weights
# ----------------------------------------------------------------------------------------------------------------------
def test_features_proj_z_against_fp64_on_its_own_rows(hip):
    """One baseline_m chunk (three sub-band groups, I = 38 / 94 / 158, H = 224, LayerNorm, frames [3, 18) of 20): the rows it writes
    are inside frontback's bound of the fp64 features, and its z is the bf3 product of exactly those rows -- the fp64 product of the
    rows the device wrote, under prodref's "x" bound -- with the pitch gap and the floats behind z untouched."""
    from spiking_fullsubnet_amd._lib import FeatProjJob, NORM_LAYERNORM
    B, F, T, FB, t0, nt, H = 5, 257, 20, 64, 3, 15, 224
    groups = fbk.M_GROUPS
    ri_np, fb_np = fbk.make_inputs(5, B, F, T, FB)
    params = fbk.make_norm_params(7, groups, B, "layernorm")
    refs = fbk.feature_reference(ri_np, fb_np, FB, groups, 0.5, "layernorm", params, B)
    rng = np.random.default_rng(11)
    ri, fb = _t(ri_np), _t(fb_np)
    jobs, keep, outs, w = (FeatProjJob * 3)(), [], [], Worst()
    for j, geo, prm in zip(jobs, groups, params):
        I, R = sum(fbk.widths(geo)), B * geo[1]
        x, xb = _canary(T * R, I)
        z, zb = _canary(nt * R + 2, H + 4)
        wt = rng.uniform(-0.1, 0.1, (H, I)).astype(np.float32)
        bias = rng.standard_normal(H).astype(np.float32)
        ts = [_t(prm[0]), _t(prm[1]), _t(wt), _t(bias)]
        g = j.feat
        g.lo, g.n_units, g.ctr, g.nbr, g.ctr_fb, g.nbr_fb = geo
        g.norm, g.ln_eps, g.ln_w, g.ln_b, g.x = NORM_LAYERNORM, prm[2], ts[0].data_ptr(), ts[1].data_ptr(), x.data_ptr()
        j.w, j.bias, j.z, j.H, j.ldz = ts[2].data_ptr(), ts[3].data_ptr(), z.data_ptr(), H, H + 4
        keep.append(ts)
        outs.append((x, xb, z, zb, wt, bias, I, R))
    rc = hip.sfsn_features_proj(_p(ri), _p(fb), B, F, T, FB, 0.5, jobs, 3, t0, nt, None, 0, None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    for (x, xb, z, zb, wt, bias, I, R), (y, tol), geo in zip(outs, refs, groups):
        assert bool(torch.isnan(xb[-PAD:]).all()) and bool(torch.isnan(zb[-PAD:]).all()), geo
        rows = x.cpu().numpy().reshape(T, R, I)
        assert np.isnan(rows[:t0]).all() and np.isnan(rows[t0 + nt:]).all(), geo
        own = rows[t0:t0 + nt]
        r = fbk.worst(own, y[t0:t0 + nt], tol[t0:t0 + nt])
        w.note(f"rows I={I}", r <= 1.0, "feature rows outside frontback's bound", r, geo)
        own = np.ascontiguousarray(own.reshape(nt * R, I))
        zr, zt = pr.real_reference(own, wt, bias, "bf3")
        w.note(f"z I={I}", *pr.check(z.cpu().numpy(), nt * R, H, zr, zt), geo)
    w.done("sfsn_features_proj")
