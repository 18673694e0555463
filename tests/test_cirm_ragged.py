"""Ragged batches of the cIRM-GSN model on the device: the length-aware projection + deep filter
(``sfsn_fullband_proj_deepfilter_ragged``) against ``sfsn_fullband_proj_deepfilter`` on a contiguous copy of every clip alone, then
``FullbandEngine.forward_stft(frames=)`` and ``Model.forward_ragged`` against the same model run on every clip alone.  Everything is
compared bit for bit; the one tolerance is that of tests/test_ragged_forward.py for the ATen edges of 256-point frames."""
import ctypes

import numpy as np
import pytest
import torch

import frontback as fbk

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -7.25  # what the outputs hold before a call: must survive wherever the call may not write
NAN_BYTE = np.int8(-128)  # the byte 0x80 in the spike padding: a value no spike has, -128 in every sum it would reach


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _lib():
    from spiking_fullsubnet_amd import _lib as L
    return L


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------
def make_case(seed, B, F, T, S, df, H, bias):
    """Spectrum from frontback.make_df_case (1e-6 .. 1e3, a silent frame), spikes at rate 0.3, projection weights of scale 0.1."""
    from spiking_fullsubnet_amd.engine import pack_w3
    from spiking_fullsubnet_amd.fullband_engine import permute_proj
    ri, _ = fbk.make_df_case(seed, B, F, T, S, [])
    rng = np.random.default_rng(seed + 1000)
    P, HP8 = 2 * df * S * F, (H + 63) // 64 * 64
    s8 = np.zeros((T, B, HP8), np.int8)
    s8[:, :, :H] = rng.random((T, B, H)) < 0.3
    w = (rng.standard_normal((P, H)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(P) * 0.1).astype(np.float32) if bias else None
    wp, bp = permute_proj(w, b, F, df, S, H)
    pk, dq = pack_w3(wp)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return dict(B=B, F=F, T=T, S=S, df=df, H=H, P=P, ri=ri, s8=s8, pk=dev(pk), dq=dev(dq), bp=dev(bp))


def run(c, ri, s8, B, T, act, want_mag, t0, nt, frames=None):
    """One launch on sentinel-filled outputs -> (enh, mag or None, proj) as numpy.  frames None: the existing entry."""
    lib = _lib().lib()
    S, F, P = c["S"], c["F"], c["P"]
    ri_d, s8_d = torch.from_numpy(np.ascontiguousarray(ri)).to(DEV), torch.from_numpy(np.ascontiguousarray(s8)).to(DEV)
    enh = torch.full((B, S, F, T, 2), SENTINEL, device=DEV)
    mag = torch.full((B, S, F, T), SENTINEL, device=DEV) if want_mag else None
    proj = torch.full((T, B, P), SENTINEL, device=DEV)
    args = (_p(ri_d), _p(s8_d), c["H"], _p(c["pk"]), _p(c["dq"]), _p(c["bp"]), act, B, F, T, S, c["df"], _p(proj), _p(enh), _p(mag), t0, nt)
    if frames is None:
        rc = lib.sfsn_fullband_proj_deepfilter(*args, None)
    else:
        fr = torch.tensor(frames, dtype=torch.int32, device=DEV)
        rc = lib.sfsn_fullband_proj_deepfilter_ragged(*args, _p(fr), None)
    assert rc == 0, lib.sfsn_strerror(rc)
    torch.cuda.synchronize()
    return enh.cpu().numpy(), None if mag is None else mag.cpu().numpy(), proj.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_ragged(c, frames, act, want_mag, t0=0, nt=None):
    """The contract of include/sfsn.h's ragged section for one call; NaN (spectrum) and 0x80 (spikes) at every frame >= T_b."""
    B, T = c["B"], c["T"]
    nt = T - t0 if nt is None else nt
    t1 = t0 + nt
    Tb = [min(max(f, 0), T) for f in frames]
    ri, s8 = c["ri"].copy(), c["s8"].copy()
    for b in range(B):
        ri[b, :, Tb[b]:] = np.nan
        s8[Tb[b]:, b] = NAN_BYTE
    enh, mag, proj = run(c, ri, s8, B, T, act, want_mag, t0, nt, frames)
    outs = [("enh_ri", enh)] + ([("enh_mag", mag)] if want_mag else [])
    for b in range(B):
        te = min(t1, Tb[b])  # clip b's own frames of the window: [t0, te)
        tz = max(t0, Tb[b])  # written as zero: [tz, t1)
        if te > t0:
            e1, m1, p1 = run(c, c["ri"][b:b + 1, :, :Tb[b]], c["s8"][:Tb[b], b:b + 1], 1, Tb[b], act, want_mag, t0, te - t0)
            assert np.array_equal(bits(enh[b, ..., t0:te, :]), bits(e1[0, ..., t0:te, :])), f"enh_ri of clip {b} (T_b = {Tb[b]})"
            if want_mag:
                assert np.array_equal(bits(mag[b, ..., t0:te]), bits(m1[0, ..., t0:te])), f"enh_mag of clip {b} (T_b = {Tb[b]})"
            assert np.array_equal(bits(proj[t0:te, b]), bits(p1[t0:te, 0])), f"proj of clip {b} (T_b = {Tb[b]})"
        for name, x in outs:
            x = np.moveaxis(x[b], 2, 0)  # frames first
            assert not bits(x[tz:t1]).any(), f"{name} of clip {b}: not exactly +0 on frames [{tz}, {t1})"  # (-0 and NaN have bits set)
            assert (x[:t0] == SENTINEL).all() and (x[t1:] == SENTINEL).all(), f"{name} of clip {b}: touched outside [{t0}, {t1})"
        assert (proj[tz:t1, b] == SENTINEL).all(), f"proj of clip {b} was written past the clip's end"
        assert (proj[:t0, b] == SENTINEL).all() and (proj[t1:, b] == SENTINEL).all(), f"proj of clip {b}: touched outside [{t0}, {t1})"


FR8 = [35, 1, 16, 17, 15, 2, 0, 99]  # full, one frame, a tile boundary and either side of it, shorter than df - 1, clamped from both sides
# (name, B, F, S, df, H, act, bias, enh_mag, clip_frames): T = 35 = two full tiles and three frames
KERNEL_CASES = [
    ("b8_f257_s1_df3_h272_none", 8, 257, 1, 3, 272, 0, True, True, FR8),
    ("b8_f129_s1_df5_h272_tanh", 8, 129, 1, 5, 272, 1, True, True, FR8),         # clips of 1 and 2 frames under df - 1 = 4
    ("b5_f129_s2_df5_h48_sigmoid_nobias", 5, 129, 2, 5, 48, 2, False, False, [35, 3, 17, 0, 99]),  # B = 5: the last workgroup has idle waves
    ("b5_f257_s2_df3_h48_relu", 5, 257, 2, 3, 48, 3, True, False, [1, 35, 16, 2, 20]),
    ("b8_f129_s1_df1_h48_nobias", 8, 129, 1, 1, 48, 0, False, True, FR8),
]


@pytest.mark.parametrize("case", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_kernel_equals_each_clip_alone(case):
    name, B, F, S, df, H, act, bias, want_mag, frames = case
    if B == 5:  # 255 or 135 work items: the last workgroup of four waves has idle ones
        assert (B * 3 * ((F + 15) // 16)) % 4 != 0
    c = make_case(len(name) + 7 * B + df, B, F, 35, S, df, H, bias)
    check_ragged(c, frames, act, want_mag)


def test_kernel_window():
    """t0 = 16, nt = 9: a clip that ends before the window (and one that ends where it starts), one inside it, one at its last frame, one
    where it ends, one after it."""
    c = make_case(41, 6, 257, 35, 1, 3, 272, True)
    check_ragged(c, [10, 16, 20, 24, 25, 35], 0, True, t0=16, nt=9)
    c2 = make_case(42, 3, 129, 35, 2, 5, 48, False)
    check_ragged(c2, [10, 20, 35], 1, False, t0=16, nt=9)


@pytest.mark.parametrize("B,F,S,df,H,act,bias,want_mag", [(5, 257, 1, 3, 272, 0, True, True), (5, 129, 2, 5, 48, 1, False, False)])
def test_kernel_full_lengths_equal_the_existing_entry(B, F, S, df, H, act, bias, want_mag):
    c = make_case(50 + F, B, F, 35, S, df, H, bias)
    for t0, nt in ((0, 35), (16, 9)):
        got = run(c, c["ri"], c["s8"], B, 35, act, want_mag, t0, nt, [35] * B)
        ref = run(c, c["ri"], c["s8"], B, 35, act, want_mag, t0, nt)
        for g, r, what in zip(got, ref, ("enh_ri", "enh_mag", "proj")):
            assert (g is None) == (r is None)
            if g is not None:
                assert np.array_equal(bits(g), bits(r)), f"{what} differs from sfsn_fullband_proj_deepfilter on the batch (t0 = {t0})"


# ---- engine and module --------------------------------------------------------------------------------------------------------------
TINY = dict(n_fft=512, hop_length=128, win_length=512, fdrc=0.5, input_size=257, hidden_size=20, num_layers=3, proj_size=257,
            output_activate_function=False, df_order=3, use_pre_layer_norm_fb=True, bn=True, shared_weights=True, sequence_model="GSN",
            num_spks=1)  # tests/golden/cirm_tiny.npz's configuration
TINY256 = dict(TINY, n_fft=256, hop_length=64, win_length=256, input_size=129, proj_size=129, num_spks=2)
CONFIGS = dict(one_spk=TINY, two_spk=dict(TINY, num_spks=2), unshared=dict(TINY, shared_weights=False), two_spk_256=TINY256)


def tiny_model(kw, seed=11):
    """The configuration under a seed, BatchNorm statistics and LayerNorm parameters moved away from the identity."""
    from spiking_fullsubnet_amd.modeling_cirm_gsn import Model
    torch.manual_seed(seed)
    m = Model(**kw)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.weight.copy_(1.0 + 0.3 * torch.rand(mod.num_features, generator=g))
                mod.bias.copy_(0.2 * torch.randn(mod.num_features, generator=g))
                mod.running_mean.copy_(0.1 * torch.randn(mod.num_features, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(mod.num_features, generator=g))
            if isinstance(mod, torch.nn.LayerNorm):
                mod.weight.copy_(1.0 + 0.2 * torch.randn(mod.normalized_shape, generator=g))
                mod.bias.copy_(0.1 * torch.randn(mod.normalized_shape, generator=g))
    return m.eval().to(DEV)


def real(x):
    return torch.view_as_real(x) if x.is_complex() else x


def same(a, b, what):
    a, b = real(a), real(b)
    assert a.shape == b.shape, (what, tuple(a.shape), tuple(b.shape))
    if not torch.equal(a, b):
        d = (a.double() - b.double()).abs()
        raise AssertionError(f"{what}: {int((a != b).sum())} of {a.numel()} elements differ, max |diff| {float(d.max()):.3g}")


def same_layers(got, want, what):
    """Two all_layers lists of one clip: tensors bit for bit, summaries by count and shape, meta tensors by shape, None as None."""
    from spiking_fullsubnet_amd.engine import SpikeSummary
    assert len(got) == len(want), what
    for i, (x, y) in enumerate(zip(got, want)):
        if x is None or y is None:
            assert x is None and y is None, f"{what}[{i}]"
        elif isinstance(y, SpikeSummary):
            assert type(x) is SpikeSummary and x.shape == y.shape and int(x.count) == int(y.count), f"{what}[{i}]: {x} {int(x.count)} != {y} {int(y.count)}"
        elif y.device.type == "meta":
            assert x.device.type == "meta" and x.shape == y.shape, f"{what}[{i}]"
        else:
            same(x, y, f"{what}[{i}]")


class Case:
    """One configuration: the model and four clips -- 1 sample, less than one hop, exactly 17 hops, Lmax (23 hops: 24 frames, more
    than one 16-frame tile) -- in a batch whose padding holds junk and NaN."""

    def __init__(self, name):
        from spiking_fullsubnet_amd import ragged
        self.kw = CONFIGS[name]
        self.model = tiny_model(self.kw)
        self.hop = hop = self.kw["hop_length"]
        self.lens = [1, hop - 28, 17 * hop, 23 * hop]
        self.frames = ragged.frames_of(self.lens, hop)
        assert self.frames == [1, 1, 18, 24]
        rng = np.random.default_rng(5)
        self.lmax = max(self.lens)
        clean = np.zeros((4, self.lmax), np.float32)
        junk = (rng.standard_normal((4, self.lmax)) * 3.0).astype(np.float32)
        junk[:, ::7] = np.nan
        for b, L in enumerate(self.lens):
            clean[b, :L] = junk[b, :L] = (rng.standard_normal(L) * 0.1 * (1.0, 0.45, 1.8, 0.8)[b]).astype(np.float32)
        self.batch, self.zero_batch = torch.from_numpy(junk).to(DEV), torch.from_numpy(clean).to(DEV)

    def clip(self, b):
        return self.batch[b:b + 1, :self.lens[b]].contiguous()


_cases = {}


def get_case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


@pytest.mark.parametrize("name", ["one_spk", "two_spk", "unshared"])
def test_forward_stft_frames_equals_each_clip_alone(name):
    from spiking_fullsubnet_amd import ragged
    c = get_case(name)
    m, frames = c.model, c.frames
    eng = m.engine()
    stft = m._stft(c.zero_batch)
    T = stft.shape[-1]
    for kw in (dict(want_layers=True), dict(want_counts=True), dict(want_layers=True, want_counts=True), dict()):
        eng.launches.clear()
        res = m.forward_stft(stft, frames=frames, **kw)
        assert eng.launches.get("projdf_ragged") == 1 and "projdf" not in eng.launches, eng.launches
        assert eng.launches.get("stack", 0) == (0 if name == "unshared" else 1) and (eng.launches.get("layer_scan", 0) > 0) == (name == "unshared")
        spiked = False
        for b, Tb in enumerate(frames):
            one = m.forward_stft(stft[b:b + 1, :, :Tb].contiguous(), **kw)
            same(res["enh_stft"][b, ..., :Tb], one["enh_stft"][0], f"{kw}: enh_stft of clip {b}")
            assert not bool(real(res["enh_stft"][b, ..., Tb:]).any()), f"{kw}: enh_stft of clip {b} is not zero beyond its {Tb} frames"
            if c.kw["num_spks"] == 1:
                same(res["enh_mag"][b, ..., :Tb], one["enh_mag"][0], f"{kw}: enh_mag of clip {b}")
                assert not bool(res["enh_mag"][b, ..., Tb:].any()), f"{kw}: enh_mag of clip {b} is not zero beyond its {Tb} frames"
            else:
                assert res["enh_mag"] is None
            if "want_counts" in kw:
                assert torch.equal(res["clip_counts"][:, b], one["clip_counts"][:, 0]), f"{kw}: clip_counts of clip {b}"
                spiked = spiked or bool(one["clip_counts"].sum() > 0)
            if kw:
                fb, sb = ragged.clip_layers(res["all_layers"], [], b, frames)
                assert sb == []
                same_layers(fb, one["all_layers"], f"{kw}: all_layers of clip {b}")
            else:
                assert res["all_layers"] is None
            if "want_layers" in kw:
                assert not bool(res["all_layers"][-1][Tb:, b].any()), f"{kw}: proj of clip {b} is not zero beyond its {Tb} frames"
        assert spiked or "want_counts" not in kw, "no clip spiked: the counts compare nothing"
        if "want_counts" in kw and "want_layers" not in kw:
            assert all(isinstance(s, ragged.ClipSpikeSummary) and s.rows_per_clip == 1 for s in res["all_layers"][1:-1])
    eng.launches.clear()
    m.forward_stft(stft)
    assert eng.launches.get("projdf") == 1 and "projdf_ragged" not in eng.launches, eng.launches  # without frames: as before
    dev = ragged.upload(frames, DEV)
    a = eng.forward_stft(stft, frames=frames, frames_dev=dev)
    b_ = eng.forward_stft(stft, frames=frames)
    same(a["enh_stft"], b_["enh_stft"], "frames_dev given / uploaded")
    with pytest.raises(ValueError, match=rf"frames\[1\] = {T + 1}: clip 1"):
        m.forward_stft(stft, frames=[1, T + 1, 3, 4])
    with pytest.raises(ValueError, match=r"frames\[2\] = 0: clip 2"):
        m.forward_stft(stft, frames=[1, 1, 0, 4])


def _ragged_and_alone(c, mode):
    m = c.model
    m.layer_outputs = mode
    try:
        out = m.forward_ragged(c.batch, c.lens)
        alone = [m(c.clip(b)) for b in range(4)]
    finally:
        m.layer_outputs = "tensors"
    return out, alone


@pytest.mark.parametrize("name", ["one_spk", "unshared"])
def test_forward_ragged_one_speaker(name):
    c = get_case(name)
    (y, mag), alone = _ragged_and_alone(c, "tensors")
    assert c.model._device_fft(c.batch)
    assert tuple(y.shape) == (4, c.lmax) and tuple(mag.shape) == (4, 257, max(c.frames))
    for b, (L, Tb) in enumerate(zip(c.lens, c.frames)):
        y1, mag1 = alone[b]
        same(y[b, :L], y1[0], f"enh_y of clip {b}")
        assert not bool(y[b, L:].any()), f"enh_y of clip {b} is not zero beyond its {L} samples"
        same(mag[b, :, :Tb], mag1[0], f"enh_mag of clip {b}")
        assert not bool(mag[b, :, Tb:].any()), f"enh_mag of clip {b} is not zero beyond its {Tb} frames"


@pytest.mark.parametrize("mode", ["tensors", "counts", "none"])
def test_forward_ragged_two_speakers(mode):
    from spiking_fullsubnet_amd import metric, ragged
    c = get_case("two_spk")
    (y, rest), alone = _ragged_and_alone(c, mode)
    assert tuple(y.shape) == (4, 2, c.lmax) and isinstance(rest, list) and len(rest) == 1 and len(rest[0]) == c.kw["num_layers"] + 2
    for b, L in enumerate(c.lens):
        y1, rest1 = alone[b]
        same(y[b, :, :L], y1[0], f"{mode}: enh_y of clip {b}")
        assert not bool(y[b, :, L:].any()), f"{mode}: enh_y of clip {b} is not zero beyond its {L} samples"
        fb = ragged.clip_layers(rest[0], [], b, c.lens, hop=c.hop)[0]
        same_layers(fb, rest1[0], f"{mode}: layers of clip {b}")
        if mode != "none":
            assert metric.compute_synops(fb, [], shared_weights=True) == metric.compute_synops(rest1[0], [], shared_weights=True)
            assert metric.compute_neuronops(fb, []) == metric.compute_neuronops(rest1[0], [])
    if mode == "counts":
        assert sum(int(s.count) for s in rest[0][1:-1]) > 0, "nothing spiked: the SynOPs compare nothing"


def test_forward_ragged_256_point_frames_take_the_aten_edges():
    """The tolerance of tests/test_ragged_forward.py for this edge (torch.stft on the batch against torch.stft on the clip)."""
    c = get_case("two_spk_256")
    m = c.model
    assert not m._device_fft(c.batch)
    (y, rest), alone = _ragged_and_alone(c, "tensors")
    assert tuple(y.shape) == (4, 2, c.lmax)
    for b, L in enumerate(c.lens):
        ref = alone[b][0][0].cpu().numpy()
        got = y[b, :, :L].cpu().numpy()
        print(f"clip {b} (L = {L}): max |diff| {np.abs(got - ref).max():.3g}, peak {np.abs(ref).max():.3g}")
        np.testing.assert_allclose(got, ref, atol=3e-6 * np.abs(ref).max(), rtol=0)
        assert not bool(y[b, :, L:].any())


def test_two_speakers_score_per_clip_as_each_clip_alone():
    """forward_ragged -> PITWrapper.per_clip(lengths=) against the clip's own forward -> per_clip: the two bit contracts compose.
    (The scorer takes clips of two samples or more -- pit.device_lengths -- so the one-sample clip is forwarded but not scored.)"""
    from spiking_fullsubnet_amd.pit import PairwiseNegSDR, PITWrapper
    c = get_case("two_spk")
    (y, _), alone = _ragged_and_alone(c, "none")
    rng = np.random.default_rng(8)
    ref = torch.from_numpy((rng.standard_normal((4, 2, c.lmax)) * 0.1).astype(np.float32)).to(DEV)
    pit = PITWrapper(PairwiseNegSDR())
    keep = [b for b, L in enumerate(c.lens) if L >= 2]
    assert keep == [1, 2, 3]
    got = pit.per_clip(y[keep].contiguous(), ref[keep].contiguous(), [c.lens[b] for b in keep])
    for i, b in enumerate(keep):
        L = c.lens[b]
        one = pit.per_clip(alone[b][0], ref[b:b + 1, :, :L].contiguous())
        assert torch.equal(got.perm[i], one.perm[0]), f"perm of clip {b}"
        assert torch.equal(got.loss[i:i + 1].view(torch.int32), one.loss.view(torch.int32)), f"loss of clip {b}: {float(got.loss[i])} != {float(one.loss[0])}"


def test_refusals():
    from spiking_fullsubnet_amd.modeling_cirm_gsn import Model
    c = get_case("one_spk")
    m = c.model
    with pytest.raises(ValueError, match="CPU int tensor"):
        m.forward_ragged(c.zero_batch, torch.tensor(c.lens, device=DEV))
    with pytest.raises(RuntimeError, match="HIP device"):
        m.forward_ragged(c.zero_batch.cpu(), c.lens)
    with pytest.raises(ValueError, match=r"lengths\[0\] = 0: clip 0"):
        m.forward_ragged(c.zero_batch, [0, 1, 2, 3])
    with pytest.raises(ValueError, match=rf"lengths\[3\] = {c.lmax + 1}: clip 3"):
        m.forward_ragged(c.zero_batch, [1, 1, 2, c.lmax + 1])
    with pytest.raises(RuntimeError, match="requires grad"):
        m.forward_ragged(c.zero_batch.clone().requires_grad_(True), c.lens)
    m.train()
    try:
        with pytest.raises(RuntimeError, match="training mode"):
            m.forward_ragged(c.zero_batch, c.lens)
    finally:
        m.eval()
    lstm = Model(**dict(TINY, sequence_model="LSTM", output_activate_function="tanh")).eval().to(DEV)
    with pytest.raises(NotImplementedError, match="LSTM"):
        lstm.forward_ragged(c.zero_batch, c.lens)
    with pytest.raises(NotImplementedError, match="LSTM"):
        lstm.forward_stft(m._stft(c.zero_batch), frames=c.frames)
