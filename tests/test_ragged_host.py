"""Ragged batches (clips of different lengths in one padded batch), host side -- no GPU needed: the C ABI's new exports and their
argument checks (hipcc cross-compiles the library), the length logic of ``spiking_fullsubnet_amd.ragged``, and the fp64 references
of tests/raggedref.py pinned to the CPU oracle's clip-alone results on the clip table the GPU tests use."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import raggedref as rr
import refweights as rw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = ("sfsn_stft_ragged", "sfsn_istft_ragged", "sfsn_laplace_means_ragged", "sfsn_gaussian_stats_ragged",
          "sfsn_spike_count_rows_ragged", "sfsn_zero_tail_frames")
_P, _I, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


@pytest.fixture(scope="module")
def L():
    from spiking_fullsubnet_amd import _lib
    _lib.build()
    return _lib.lib()


# ---- exports, prototypes, ABI ---------------------------------------------------------------------------------------------------
def test_exports_and_prototypes(L):
    from spiking_fullsubnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "sfsn.h")).read()
    feat, rowc = ctypes.POINTER(_lib.FeatureGroup), ctypes.POINTER(_lib.RowCount)
    want = dict(
        sfsn_stft_ragged=[_P, _I, _I, _I, _I, _P, _P, _I, _P, _P],
        sfsn_istft_ragged=[_P, _I, _I, _I, _I, _P, _P, _I, _P, _P, _P],
        sfsn_laplace_means_ragged=[_P, _P, _I, _I, _I, _I, _F, feat, _I, _P, _P, _P, _P],
        sfsn_gaussian_stats_ragged=[_P, _P, _I, _I, _I, _I, _F, feat, _I, _P, _P, _P, _P, _P],
        sfsn_spike_count_rows_ragged=[rowc, _I, _I, _I, _P, _I, _P],
        sfsn_zero_tail_frames=[_P, _I, _I, _I, _I, _P, _P])
    assert set(want) == set(RAGGED)
    for name, argtypes in want.items():
        assert name in _lib.EXPORTS and hasattr(L, name), name
        fn = getattr(L, name)
        assert fn.restype is _I and list(fn.argtypes) == argtypes, name
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl, f"{name} is not declared in sfsn.h"
        assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == len(argtypes), name


def test_abi_version_is_still_21(L):
    from spiking_fullsubnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "sfsn.h")).read()
    assert re.search(r"#define\s+SFSN_ABI_VERSION\s+21\b", header)
    assert _lib.ABI_VERSION == 21 and L.sfsn_abi_version() == 21


def test_ragged_unit_is_built_and_hashed():
    from spiking_fullsubnet_amd import _lib
    assert any(s.endswith("sfsn_ragged.hip") for s in _lib._sources())
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert re.search(r"^OBJS\s*:=.*\bsfsn_ragged\.o\b", mk, re.M) and re.search(r"^SRCS\s*:=.*\bsfsn_ragged\.hip\b", mk, re.M)


# ---- argument checks: answered before any launch (without a GPU a launch would answer SFSN_EHIP) ----------------------------------
class _Args:
    """Valid arguments of every ragged export over dummy host buffers (never dereferenced: each case below is refused first)."""

    def __init__(self):
        from spiking_fullsubnet_amd import _lib
        self.buf = (ctypes.c_char * 4096)()
        p = ctypes.addressof(self.buf)
        p += (-p) % 16
        self.p = p
        self.groups = (_lib.FeatureGroup * 1)()
        g = self.groups[0]
        g.lo, g.n_units, g.ctr, g.nbr, g.ctr_fb, g.nbr_fb = 0, 1, 64, 0, 0, 0
        self.rows = (_lib.RowCount * 1)()
        r = self.rows[0]
        r.spikes_i8, r.T, r.R, r.HP, r.rows_per_clip, r.counts = p, 8, 6, 64, 3, p

    def calls(self, B=2, n_fft=512, null=None):
        """name -> (function arguments), with clip count B, frame size n_fft, and the pointer argument number `null` of each call
        (counting pointers only) replaced by NULL."""
        p = self.p
        spec = dict(
            sfsn_stft_ragged=[p, B, 1024, n_fft, 128, p, p, 9, p, None],
            sfsn_istft_ragged=[p, B, 9, n_fft, 128, p, p, 1024, p, p, None],
            sfsn_laplace_means_ragged=[p, None, B, 257, 9, 0, 0.5, self.groups, 1, p, p, p, None],
            sfsn_gaussian_stats_ragged=[p, None, B, 257, 9, 0, 0.5, self.groups, 1, p, p, p, p, None],
            sfsn_spike_count_rows_ragged=[self.rows, 1, 0, 8, p, B, None],
            sfsn_zero_tail_frames=[p, B, 5, 9, 2, p, None])
        if null is None:
            return spec
        out = {}
        for name, args in spec.items():
            ptrs = [i for i, a in enumerate(args[:-1]) if a == p or a is self.groups or a is self.rows]
            if null < len(ptrs):
                a = list(args)
                a[ptrs[null]] = None
                out[name] = a
        return out


def test_null_pointers_are_refused(L):
    from spiking_fullsubnet_amd import _lib
    args, seen = _Args(), {n: 0 for n in RAGGED}
    for k in range(8):
        for name, a in args.calls(null=k).items():
            assert getattr(L, name)(*a) == _lib.SFSN_EINVAL, (name, k)
            seen[name] += 1
    # every required pointer of every export was tried: 4 / 5 / 4 (+ groups) / 5 (+ groups) / 2 / 2
    assert seen == dict(sfsn_stft_ragged=4, sfsn_istft_ragged=5, sfsn_laplace_means_ragged=5, sfsn_gaussian_stats_ragged=6,
                        sfsn_spike_count_rows_ragged=2, sfsn_zero_tail_frames=2)


@pytest.mark.parametrize("B", [0, -3])
def test_no_clips_is_refused(L, B):
    from spiking_fullsubnet_amd import _lib
    for name, a in _Args().calls(B=B).items():
        assert getattr(L, name)(*a) == _lib.SFSN_EINVAL, name


def test_other_frame_sizes_are_unsupported(L):
    from spiking_fullsubnet_amd import _lib
    calls = _Args().calls(n_fft=256)
    for name in ("sfsn_stft_ragged", "sfsn_istft_ragged"):
        assert getattr(L, name)(*calls[name]) == _lib.SFSN_EUNSUPPORTED, name


def test_sibling_conditions_still_hold(L):
    from spiking_fullsubnet_amd import _lib
    a = _Args()
    c = a.calls()
    c["sfsn_stft_ragged"][7] = 8  # T != 1 + L / hop
    assert L.sfsn_stft_ragged(*c["sfsn_stft_ragged"]) == _lib.SFSN_EINVAL
    c["sfsn_istft_ragged"][7] = 8 * 128 + 257  # longer than the frames cover
    assert L.sfsn_istft_ragged(*c["sfsn_istft_ragged"]) == _lib.SFSN_EINVAL
    c["sfsn_gaussian_stats_ragged"][4] = 1  # one frame: no unbiased deviation
    assert L.sfsn_gaussian_stats_ragged(*c["sfsn_gaussian_stats_ragged"]) == _lib.SFSN_EINVAL
    c["sfsn_spike_count_rows_ragged"][3] = 9  # t0 + nt > T
    assert L.sfsn_spike_count_rows_ragged(*c["sfsn_spike_count_rows_ragged"]) == _lib.SFSN_EINVAL
    c = a.calls(B=3)  # R = 6 rows at 3 rows per clip are 2 clips
    assert L.sfsn_spike_count_rows_ragged(*c["sfsn_spike_count_rows_ragged"]) == _lib.SFSN_EINVAL
    c = a.calls()
    c["sfsn_zero_tail_frames"][4] = 0
    assert L.sfsn_zero_tail_frames(*c["sfsn_zero_tail_frames"]) == _lib.SFSN_EINVAL


# ---- host-side length logic -----------------------------------------------------------------------------------------------------
def test_frame_counts():
    from spiking_fullsubnet_amd import ragged
    assert tuple(ragged.frames_of(rr.CLIP_LENGTHS, rr.HOP)) == rr.CLIP_FRAMES
    assert ragged.frames_of([1, 127, 128, 129], 128) == [1, 1, 2, 2] and ragged.frames_of([63, 64], 64) == [1, 2]
    assert ragged.check_lengths(torch.tensor([5, 300]), 2, 300, 128) == [5, 300]
    assert ragged.check_frames((1, 9), 2, 9) == [1, 9]


@pytest.mark.parametrize("lengths,msg", [
    ([200, 0, 300], r"lengths\[1\] = 0"), ([200, 301, 300], r"lengths\[1\] = 301"), ([-1, 10, 20], r"lengths\[0\] = -1"),
    ([200, 300], "one length per clip"), ([1, 2, 3, 4], "one length per clip"), ([200.5, 3, 4], "not an integer")])
def test_bad_lengths_name_the_clip(lengths, msg):
    from spiking_fullsubnet_amd import ragged
    with pytest.raises(ValueError, match=msg):
        ragged.check_lengths(lengths, 3, 300, 128)


def test_gaussian_norm_needs_two_frames():
    from spiking_fullsubnet_amd import ragged
    assert ragged.check_lengths([127, 128], 2, 128, 128) == [127, 128]
    assert ragged.check_lengths([128, 128], 2, 128, 128, gaussian=True) == [128, 128]
    with pytest.raises(ValueError, match=r"lengths\[1\] = 127.*one hop"):
        ragged.check_lengths([128, 127], 2, 128, 128, gaussian=True)
    with pytest.raises(ValueError, match=r"frames\[0\] = 1"):
        ragged.check_frames([1, 2], 2, 2, gaussian=True)
    for bad, msg in (([0, 2], r"frames\[0\] = 0"), ([2, 3], r"frames\[1\] = 3"), ([2], "one frame count per clip")):
        with pytest.raises(ValueError, match=msg):
            ragged.check_frames(bad, 2, 2)
    with pytest.raises(ValueError, match="1-D integer tensor"):
        ragged.check_frames(torch.tensor([1.0, 2.0]), 2, 2)


# ---- clip_layers ----------------------------------------------------------------------------------------------------------------
def _layers(T, B, units, H=(6, 4)):
    g = torch.Generator().manual_seed(5)
    mk = lambda R, C: torch.rand((T, R, C), generator=g)
    fb_all = [mk(B, 8), mk(B, H[0]), mk(B, H[0]), mk(B, 8)]
    sb_all = [[mk(B * n, 5), mk(B * n, H[1]), mk(B * n, H[1]), mk(B * n, 3)] for n in units]
    return fb_all, sb_all


def test_clip_layers_tensors():
    from spiking_fullsubnet_amd import ragged
    frames, units = [2, 7, 4], (3, 1)
    fb_all, sb_all = _layers(7, 3, units)
    for b, Tb in enumerate(frames):
        fb, sb = ragged.clip_layers(fb_all, sb_all, b, frames)
        assert [tuple(x.shape) for x in fb] == [(Tb, 1, 8), (Tb, 1, 6), (Tb, 1, 6), (Tb, 1, 8)]
        assert all(torch.equal(x, full[:Tb, b:b + 1]) for x, full in zip(fb, fb_all))
        for g, n in enumerate(units):
            assert all(torch.equal(x, full[:Tb, b * n:(b + 1) * n]) for x, full in zip(sb[g], sb_all[g]))
    # lengths in samples with hop=: the same views
    fb, sb = ragged.clip_layers(fb_all, sb_all, 0, [300, 800, 520], hop=128)  # 3, 7, 5 frames
    assert fb[1].shape[0] == 3 and sb[1][2].shape == (3, 1, 4)
    # None entries (layer_outputs="none") stay None
    fb, _ = ragged.clip_layers([fb_all[0], None, None, fb_all[3]], sb_all, 1, frames)
    assert fb[1] is None and fb[2] is None and fb[0].shape == (7, 1, 8)
    with pytest.raises(IndexError):
        ragged.clip_layers(fb_all, sb_all, 3, frames)
    with pytest.raises(ValueError):
        ragged.clip_layers(fb_all, sb_all, 1, [2, 8, 4])  # more frames than the batch has


def test_clip_layers_counts():
    from spiking_fullsubnet_amd import metric, ragged
    from spiking_fullsubnet_amd.engine import SpikeSummary
    frames, units, T, B = [2, 7, 4], (3, 1), 7, 3
    fb_all, sb_all = _layers(T, B, units)

    def summarise(outs, n):
        out = list(outs)
        for i in (1, 2):
            spk = (outs[i] > 0.6).float()
            counts = torch.tensor([int(spk[:frames[b], b * n:(b + 1) * n].sum()) for b in range(B)], dtype=torch.int64)
            out[i] = ragged.ClipSpikeSummary(counts, spk.shape, frames)
            outs[i] = spk
        return out

    fb_c = summarise(fb_all, 1)
    sb_c = [summarise(outs, n) for outs, n in zip(sb_all, units)]
    for b, Tb in enumerate(frames):
        fb_t, sb_t = ragged.clip_layers(fb_all, sb_all, b, frames)
        fb, sb = ragged.clip_layers(fb_c, sb_c, b, frames)
        assert isinstance(fb[1], SpikeSummary) and not isinstance(fb[1], ragged.ClipSpikeSummary)
        assert fb[1].shape == (Tb, 1, 6) and sb[0][2].shape == (Tb, 3, 4)
        assert int(fb[2].count) == int(fb_t[2].sum()) and int(sb[0][1].count) == int(sb_t[0][1].sum())
        assert metric.compute_synops(fb, sb) == metric.compute_synops(fb_t, sb_t)
        assert metric.compute_neuronops(fb, sb) == metric.compute_neuronops(fb_t, sb_t)
    # as a whole: the batch's valid part
    whole = fb_c[1]
    assert int(whole.count) == sum(int(fb_all[1][:Tb, b].sum()) for b, Tb in enumerate(frames)) and whole.numel() == sum(frames) * 6
    with pytest.raises(ValueError, match="counted with frames"):
        ragged.clip_layers(fb_c, sb_c, 0, [2, 7, 5])
    with pytest.raises(ValueError, match="no per-clip counts"):
        ragged.clip_layers([fb_all[0], SpikeSummary(torch.tensor(3), (T, B, 6)), None, fb_all[3]], sb_c, 0, frames)


# ---- the fp64 references, pinned to the oracle's clip-alone results on the clip table ----------------------------------------
def test_istft_reference_equals_the_oracle_on_each_clip_alone():
    from oracle import model as omodel
    rng = np.random.default_rng(17)
    B, T = len(rr.CLIP_LENGTHS), max(rr.CLIP_FRAMES)
    spec = (rng.standard_normal((B, 257, T)) + 1j * rng.standard_normal((B, 257, T))).astype(np.complex64)  # junk past every end too
    got = rr.istft_ref(spec, rr.CLIP_FRAMES, rr.CLIP_LENGTHS)
    assert got.shape == (B, max(rr.CLIP_LENGTHS))
    for b, (Tb, Lb) in enumerate(zip(rr.CLIP_FRAMES, rr.CLIP_LENGTHS)):
        alone = omodel.istft(spec[b:b + 1, :, :Tb], length=Lb)[0]
        assert np.array_equal(got[b, :Lb], alone), b
        assert not got[b, Lb:].any(), b
    # a padded batch without lengths is NOT that: the frames past a clip's end are overlap-added into its last n_fft/2 samples
    plain = omodel.istft(spec, length=max(rr.CLIP_LENGTHS))
    for b, Lb in enumerate(rr.CLIP_LENGTHS[:-1]):
        assert np.abs(plain[b, :Lb] - got[b, :Lb]).max() > 0.01, b  # (samples are O(0.05): no rounding effect)


@pytest.mark.parametrize("gaussian", [False, True], ids=["laplace", "gaussian"])
def test_statistics_reference_equals_the_oracle_on_each_clip_alone(gaussian):
    from oracle import Oracle
    from oracle import model as omodel
    o = Oracle("f64")
    kw = rw.FROZEN_TINY
    spec = omodel.spec_from_frozen_kwargs(kw)
    waves = rr.clip_waves(3, gains=(1.0, 0.45, 1.8))
    stft = omodel.stft(rr.pad_batch(waves))
    B, T = len(waves), stft.shape[-1]
    mag = o.front_mag(stft, kw["fdrc"])
    fb_tbf = np.abs(np.random.default_rng(23).standard_normal((T, B, spec["fb_proj"])))  # stands for the full-band output
    cut = spec["cutoffs"]
    groups = [o.gather_fullband(mag, spec["fb_in"])] + [
        o.gather_group(mag, fb_tbf, cut[g], cut[g + 1], spec["ctr"][g], spec["nbr"][g], spec["ctr_fb"][g], spec["nbr_fb"][g])
        for g in range(len(spec["ctr"]))]
    for gi, x in enumerate(groups):
        N = x.shape[1] // B
        ref = rr.stats_ref(x, rr.CLIP_FRAMES, gaussian)
        mu = ref[0] if gaussian else ref
        unmasked = rr.stats_ref(x, [T] * B, gaussian)
        for b, Tb in enumerate(rr.CLIP_FRAMES):
            alone = np.ascontiguousarray(x[:Tb, b * N:(b + 1) * N])
            if gaussian:
                m, sd, work = np.empty(1), np.empty(1), alone.copy()
                o._fn("gaussian_norm", [_P, _I, _I, _I, _I, _P, _P])(work.ctypes.data, Tb, 1, N, x.shape[2], m.ctypes.data, sd.ctypes.data)
                assert np.isclose(m[0], mu[b], rtol=1e-12, atol=0), (gi, b)
                assert np.isclose(sd[0], ref[1][b], rtol=1e-9, atol=0), (gi, b)
            else:
                _, m = o.laplace_norm(alone, 1)
                assert np.isclose(m[0], mu[b], rtol=1e-12, atol=0), (gi, b)
        # a padded batch without lengths is NOT that: the mean runs over the padding as well
        short = [b for b, Tb in enumerate(rr.CLIP_FRAMES) if Tb < T]
        plain_mu = unmasked[0] if gaussian else unmasked
        assert all(abs(plain_mu[b] - mu[b]) > 1e-3 * abs(mu[b]) for b in short), gi


def test_a_padded_batch_without_lengths_is_wrong_on_the_oracle():
    """The figures the feature answers (seed 3, the clip table, zero padding, CPU oracle in fp32)."""
    live = rr.padded_vs_alone(rw.LIVE_TINY)
    # causal model: what the network computes on a clip's own frames is the clip alone, bit for bit ...
    assert live["spikes_equal"] and live["enh_equal"]
    # ... but the inverse STFT overlap-adds the frames past the end: the last n_fft/2 samples are off (0.028 on a 0.05-rms signal)
    assert live["wave_err_body"] == 0.0 and 0.01 < live["wave_err"] < 0.06
    assert live["synops_rel"] > 0.005  # SynOPs as a mean over the padded tensors (1.2 % here)
    frozen = rr.padded_vs_alone(rw.FROZEN_TINY)
    # offline norm: the per-clip mean runs over the padding, all of it differs
    assert not frozen["spikes_equal"] and not frozen["enh_equal"] and frozen["wave_err_body"] > 0.01
