"""The 16-row IO-wave scans after the compute waves' step was trimmed (sfsn_scan3j_dev.h: two steps per loop trip with the state
buffer's parity as an immediate, a carried ring slot, the digit planes recombined in two shift-adds, the input product's last k-step
as one 32-wide matrix instruction): bit for bit round 2's body (SFSN_FUSED_V2=1, read by the library on every call) through the C ABI,
for both output sets -- with the fp32 spike tensor, and counts only."""
import numpy as np
import pytest

from test_hip_parity import _run_fused, _run_fused_x, make_layer

pytestmark = pytest.mark.gpu

NAMES = ("fp32 spikes", "int8 spikes", "h", "c", "count")


@pytest.fixture(scope="module")
def hip():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    assert L.sfsn_device_count() >= 1
    return L


def _same(new, old, tag):
    for a, b, nm in zip(new, old, NAMES):
        if a is None or b is None:
            assert a is None and b is None, f"{tag}: {nm}"
        else:
            np.testing.assert_array_equal(a, b, err_msg=f"{tag}: {nm}")


def _both(run, monkeypatch, *args, **kw):
    """(trimmed body, round 2's body) x (with fp32 spikes, counts only) of one case."""
    new = (run(*args, **kw), run(*args, want_f32=False, **kw))
    monkeypatch.setenv("SFSN_FUSED_V2", "1")
    old = (run(*args, **kw), run(*args, want_f32=False, **kw))
    monkeypatch.delenv("SFSN_FUSED_V2")
    return new, old


def _check(new, old, tag):
    _same(new[0], old[0], tag + " with fp32 spikes")
    _same(new[1], old[1], tag + " counts only")
    assert new[1][0] is None and new[1][4] == int(old[0][0].sum()), f"{tag}: the count is not the number of spikes written"
    np.testing.assert_array_equal(new[1][1], new[0][1], err_msg=f"{tag}: int8 spikes of the two output sets")


def _fused_case(rng, H, R, T, p=0.25):
    sd, alpha, beta, _ = make_layer(rng, H, H, True, True)
    HP = (H + 63) // 64 * 64
    s_in = np.zeros((T, R, HP), np.int8)
    s_in[:, :, :H] = rng.random((T, R, H)) < p
    h0 = (rng.random((R, H)) > 0.5).astype(np.float32)
    c0 = rng.standard_normal((R, H)).astype(np.float32)
    return sd, alpha, beta, s_in, h0, c0


TS = (1, 2, 15, 16, 33)  # odd / even against the two-step trip, the prologue alone (T < the ring's lead of 6), more than two wraps of 7 slots


@pytest.mark.parametrize("R", [5, 16, 37])  # a ragged block with duplicated rows past R, one full block, three blocks with a ragged last
@pytest.mark.parametrize("H", [224, 160, 192, 144])  # KS 4 + tail step, KS 3 + tail step, KS 3 without, KS 3 + tail step of 16 live columns
def test_fused_scan_equals_round_2_body(hip, H, R, monkeypatch):
    rng = np.random.default_rng(1000 * H + R)
    sd, alpha, beta, s_in, h0, c0 = _fused_case(rng, H, R, max(TS))
    seen = False
    for T in TS:
        new, old = _both(lambda *a, **k: _run_fused(hip, *a, **k), monkeypatch, s_in[:T], sd, alpha, beta, h0, c0)
        _check(new, old, f"H={H} R={R} T={T}")
        assert not new[0][1][:, :, H:].any()
        seen = seen or bool(new[0][1].any())
    assert seen


@pytest.mark.parametrize("H", [224, 192])
def test_fused_scan_state_carry_and_two_segments(hip, H, monkeypatch):
    rng = np.random.default_rng(77 + H)
    R = 37
    sd, alpha, beta, s_in, h0, c0 = _fused_case(rng, H, R, 15)
    for f32 in (True, False):
        one = _run_fused(hip, s_in, sd, alpha, beta, h0, c0, want_f32=f32)
        a = _run_fused(hip, s_in[:7], sd, alpha, beta, h0, c0, want_f32=f32)
        b = _run_fused(hip, s_in[7:], sd, alpha, beta, a[2], a[3], want_f32=f32)
        tag = f"H={H} T=7 then T=8, fp32 spikes {f32}"
        if f32:
            np.testing.assert_array_equal(np.concatenate([a[0], b[0]]), one[0], err_msg=tag)
        else:
            assert a[4] + b[4] == one[4], tag
        np.testing.assert_array_equal(np.concatenate([a[1], b[1]]), one[1], err_msg=tag)
        np.testing.assert_array_equal(b[2], one[2], err_msg=tag)
        np.testing.assert_array_equal(b[3], one[3], err_msg=tag)
    new, old = _both(lambda *a, **k: _run_fused(hip, *a, **k), monkeypatch, s_in, sd, alpha, beta, h0, c0, segs_split=21)
    _check(new, old, f"H={H} two segments")
    _same(new[0][:4], _run_fused(hip, s_in, sd, alpha, beta, h0, c0)[:4], f"H={H} two segments against one")


def test_fused_scan_does_not_read_the_padding_columns_of_its_input(hip, monkeypatch):
    """H = 224: columns 224 .. 255 of spikes_in met zero weight digits in the full last k-step and are not read by the 32-wide one."""
    rng = np.random.default_rng(5)
    sd, alpha, beta, s_in, h0, c0 = _fused_case(rng, 224, 21, 16)
    dirty = s_in.copy()
    dirty[:, :, 224:] = rng.integers(1, 128, size=dirty[:, :, 224:].shape)
    new, old = _both(lambda *a, **k: _run_fused(hip, *a, **k), monkeypatch, dirty, sd, alpha, beta, h0, c0)
    _check(new, old, "dirty padding")
    clean = _run_fused(hip, s_in, sd, alpha, beta, h0, c0)
    _same(new[0][:4], clean[:4], "dirty padding against zero padding")


def test_fused_scan_tail_step_takes_the_right_half_of_the_fragment(hip, monkeypatch):
    """Input spikes in columns 192 .. 223 only: all of the input term comes from the 32-wide k-step."""
    rng = np.random.default_rng(6)
    sd, alpha, beta, s_in, h0, c0 = _fused_case(rng, 224, 21, 16, p=0.5)
    s_in[:, :, :192] = 0
    assert s_in[:, :, 192:224].any()
    new, old = _both(lambda *a, **k: _run_fused(hip, *a, **k), monkeypatch, s_in, sd, alpha, beta, h0, c0)
    _check(new, old, "tail columns only")
    none = _run_fused(hip, np.zeros_like(s_in), sd, alpha, beta, h0, c0)
    assert (none[1] != new[0][1]).any(), "the case cannot tell the tail columns from no input at all"


TSX = (1, 2, 15, 33)


@pytest.mark.parametrize("R", [16, 48])
@pytest.mark.parametrize("H", [224, 192])
@pytest.mark.parametrize("I", [6, 38, 64])  # one 32-wide k-chunk, two, two full ones
def test_fused_x_scan_equals_round_2_body(hip, I, H, R, monkeypatch):
    rng = np.random.default_rng(100000 * I + 100 * H + R)
    sd, alpha, beta, _ = make_layer(rng, I, H, True, True)
    x = rng.standard_normal((max(TSX), R, I)).astype(np.float32)
    h0 = (rng.random((R, H)) > 0.5).astype(np.float32)
    c0 = rng.standard_normal((R, H)).astype(np.float32)
    seen = False
    for T in TSX:
        new, old = _both(lambda *a, **k: _run_fused_x(hip, *a, **k), monkeypatch, x[:T], sd, alpha, beta, h0, c0)
        _check(new, old, f"I={I} H={H} R={R} T={T}")
        seen = seen or bool(new[0][1].any())
    assert seen


@pytest.mark.parametrize("H", [224, 192])
def test_fused_x_scan_state_carry(hip, H):
    rng = np.random.default_rng(99 + H)
    I, R = 38, 48
    sd, alpha, beta, _ = make_layer(rng, I, H, True, True)
    x = rng.standard_normal((15, R, I)).astype(np.float32)
    h0 = (rng.random((R, H)) > 0.5).astype(np.float32)
    c0 = rng.standard_normal((R, H)).astype(np.float32)
    for f32 in (True, False):
        one = _run_fused_x(hip, x, sd, alpha, beta, h0, c0, want_f32=f32)
        a = _run_fused_x(hip, x[:7], sd, alpha, beta, h0, c0, want_f32=f32)
        b = _run_fused_x(hip, x[7:], sd, alpha, beta, a[2], a[3], want_f32=f32)
        tag = f"H={H} T=7 then T=8, fp32 spikes {f32}"
        if f32:
            np.testing.assert_array_equal(np.concatenate([a[0], b[0]]), one[0], err_msg=tag)
        else:
            assert a[4] + b[4] == one[4], tag
        np.testing.assert_array_equal(np.concatenate([a[1], b[1]]), one[1], err_msg=tag)
        np.testing.assert_array_equal(b[2], one[2], err_msg=tag)
        np.testing.assert_array_equal(b[3], one[3], err_msg=tag)
