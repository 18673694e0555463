"""CPU checks of scoring ragged batches before a GPU is involved: the new export and its refusals (answered before any launch), the
Python layer's length checks, and tests/pitraggedref.py itself -- every reference value and bound of its table is finite and no clip
is ambiguous, the composition over full-length clips equals pitref.reference on the batch, every mutant of the composition is
rejected by at least one case, and the fp64 restatement of audiozen.metric.SISDR lies within its derived bound of the reference's own
fp32 values (tests/golden/sisdr_metric.npz, made by tests/golden/make_golden_sisdr.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pitraggedref as prr
import pitref
from spiking_fullsubnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c[0] for c in prr.CASES]
ZM = [True, False]
_refs = {}


def _case(name, zm):
    """(est, ref, cotangent, lengths, composition) of a case, computed once and shared (never modified)."""
    if (name, zm) not in _refs:
        e, t = prr.make_inputs(name)
        w = prr.cotangent(name)
        lens = prr.lengths(name)
        _refs[name, zm] = (e, t, w, lens, prr.reference(e, t, lens, zm, cot=w))
    return _refs[name, zm]


def test_export_exists_with_its_prototype_and_the_abi_is_still_21():
    _lib.build()
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "sfsn.h")).read()
    proto = re.search(r"int sfsn_pit_sdr_ragged\((.*?)\);", header, re.S).group(1)
    proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    assert [" ".join(a.split()) for a in proto.split(",")] == [
        "const float* est", "const float* ref", "int clips", "int sources", "int n_samples", "const int32_t* clip_len", "int zero_mean",
        "float eps", "const float* pair_cot", "float* pair", "int32_t* perm", "float* clip_loss", "float* loss", "float* grad_est",
        "float* reordered", "float* si_sdr", "void* scratch", "void* stream"]
    assert "sfsn_pit_sdr_ragged" in _lib.EXPORTS and hasattr(L, "sfsn_pit_sdr_ragged")
    assert L.sfsn_pit_sdr_ragged.argtypes == [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_float] + \
        [ctypes.c_void_p] * 10
    assert L.sfsn_pit_sdr_ragged.restype == ctypes.c_int
    assert L.sfsn_abi_version() == _lib.ABI_VERSION == 21
    assert int(re.search(r"#define SFSN_ABI_VERSION (\d+)", header).group(1)) == 21


def test_argument_refusals_are_answered_before_any_launch():
    """None of these reaches a launch (the pointers are never dereferenced on the host), so they answer on a box without a GPU."""
    L = _lib.lib()
    p = 0x10000  # a 16-byte aligned address that is never read

    def call(est=p, ref=p, clips=2, sources=2, n=1000, clip_len=p, zm=1, eps=1e-8, cot=None, pair=p, perm=p, clip_loss=p, loss=p, grad=p,
             reordered=p, si_sdr=p, scratch=p):
        return L.sfsn_pit_sdr_ragged(est, ref, clips, sources, n, clip_len, zm, eps, cot, pair, perm, clip_loss, loss, grad, reordered, si_sdr,
                                     scratch, None)

    pw = dict(cot=p, perm=None, loss=None, reordered=None, clip_loss=None, si_sdr=None)  # a well-formed pairwise-mode call
    einval = [dict(clip_len=None), dict(est=None), dict(ref=None), dict(pair=None), dict(scratch=None), dict(perm=None), dict(loss=None),
              dict(pw, clip_len=None), dict(pw, scratch=None),
              dict(pw, clip_loss=p), dict(pw, si_sdr=p), dict(pw, clip_loss=p, si_sdr=p), dict(pw, perm=p), dict(pw, loss=p), dict(pw, reordered=p),
              dict(est=p + 4), dict(ref=p + 8), dict(clip_len=p + 4), dict(pair=p + 4), dict(perm=p + 4), dict(clip_loss=p + 4), dict(loss=p + 12),
              dict(grad=p + 4), dict(reordered=p + 8), dict(si_sdr=p + 4), dict(scratch=p + 8), dict(pw, cot=p + 4),
              dict(clips=0), dict(sources=0), dict(n=1), dict(n=0), dict(eps=-1e-8), dict(eps=float("nan")), dict(eps=float("inf"))]
    for kw in einval:
        assert call(**kw) == _lib.SFSN_EINVAL, kw
    for kw in (dict(sources=5), dict(pw, sources=5), dict(clips=64, sources=4, n=1 << 23)):
        assert call(**kw) == _lib.SFSN_EUNSUPPORTED, kw
    with pytest.raises(ValueError, match="invalid argument"):
        _lib.check(call(clip_len=None), "sfsn_pit_sdr_ragged")
    with pytest.raises(NotImplementedError):
        _lib.check(call(sources=5))


@pytest.mark.parametrize("zm", ZM)
def test_every_reference_value_and_bound_is_finite_and_no_clip_is_ambiguous(zm):
    smallest = {}
    for name in NAMES:
        e, t, w, lens, ref = _case(name, zm)
        for k, tol in prr.KEYS:
            assert np.all(np.isfinite(ref[k])) and np.all(np.isfinite(ref[tol])), (name, k)
        for b, n in enumerate(lens):
            assert np.all(ref["grad_tol"][b, :, :n] > 0) and np.all(ref["grad_tol"][b, :, n:] == 0)
            assert np.all(ref["reordered"][b, :, n:] == 0) and np.all(ref["grad"][b, :, n:] == 0)
            amb, gap = pitref.ambiguous_clips(name, dict(B=1, loss_p=ref["loss_p"][b:b + 1], loss_p_tol=ref["loss_p_tol"][b:b + 1]))
            assert amb == [], (name, b)
            if gap is not None:
                smallest[name] = min(gap, smallest.get(name, np.inf))
        assert ref["si_sdr_tol"].max() <= 0.02 and ref["loss_tol"] <= 0.01  # not vacuous (dB)
    print(zm, smallest)
    assert min(smallest.values()) > 0.02  # (the issue's figure: 0.0275 dB on r5s4, at least 11 dB elsewhere)
    _, _, _, _, ref = _case("r5s4", zm)
    assert sum(p.tolist() != [0, 1, 2, 3] for p in ref["perm"]) >= 4  # the 24-permutation case really leaves the identity


@pytest.mark.parametrize("zm", ZM)
@pytest.mark.parametrize("name", [c[0] for c in pitref.CASES])
def test_composition_over_full_length_clips_equals_the_batch_reference(name, zm):
    """With every L_b = L the composition over the clips alone IS pitref.reference on the batch: the per-clip quantities bit for bit,
    the batch loss and the gradient to a few fp64 roundings (the mean over clips and the 1 / B are applied in another order)."""
    e, t = pitref.make_inputs(name)
    w = pitref.cotangent(name)
    B, S, L = e.shape
    whole = pitref.reference(e, t, zm, cot=w)
    comp = prr.reference(e, t, [L] * B, zm, cot=w)
    for k in ("pair", "loss_p", "perm", "reordered", "pair_tol", "loss_p_tol", "grad_pw", "grad_pw_tol"):
        assert np.array_equal(comp[k], whole[k]), k
    assert np.array_equal(comp["clip_loss"], whole["loss_p"].min(1))
    assert abs(comp["loss"] - whole["loss"]) <= 4 * pitref.U64 * abs(whole["loss"])
    assert abs(comp["loss_tol"] - whole["loss_tol"]) <= 1e-12 * whole["loss_tol"]
    assert np.all(np.abs(comp["grad"] - whole["grad"]) <= 8 * pitref.U64 * np.abs(whole["grad"]))
    assert np.all(np.abs(comp["grad_tol"] - whole["grad_tol"]) <= 1e-9 * whole["grad_tol"])


@pytest.mark.parametrize("mut", prr.MUTATIONS)
def test_every_mutant_of_the_composition_is_rejected(mut):
    rejected = {}
    for name in NAMES:
        for zm in ZM:
            e, t, w, lens, ref = _case(name, zm)
            bad, used = prr.outside(prr.reference(e, t, lens, zm, cot=w, mut=mut), ref)
            if bad:
                rejected[name, zm] = (bad, {k: used[k] for k in bad if k in used})
    print(mut, rejected)
    assert rejected, mut
    names = lambda key: {k for k, v in rejected.items() if key in v[0]}
    if mut == "mean_over_lmax":  # every case tells the clip's own mean from the mean over the padded row (without zero_mean there is none)
        assert names("pair") == {(n, True) for n in NAMES} == set(rejected)
        assert min(v[1]["pair"] for v in rejected.values()) >= 100
    if mut == "length_weighted_loss":
        assert names("loss") == {(n, zm) for n in NAMES for zm in ZM}
        assert min(v[1]["loss"] for v in rejected.values()) >= 100
    if mut == "grad_over_B":  # (one source: 1 / B is 1 / (B S))
        assert names("grad") == {(n, zm) for n in NAMES for zm in ZM if n != "r3s1"}
    if mut == "grad_tail":
        assert names("grad") == {(n, zm) for n in NAMES for zm in ZM}
    if mut == "sisdr_pit_eps":
        assert all(v[0] == ["si_sdr"] for v in rejected.values())


def test_sisdr_restatement_lies_within_its_bound_of_the_reference():
    """tests/golden/sisdr_metric.npz holds audiozen.metric.SISDR's own fp32 values for every clip of the table alone (rows as generated).
    The derivation of pitraggedref.sisdr_rows needed no widening: the reference's evaluation uses at most 2 % of it."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "sisdr_metric.npz"))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "sisdr_metric.npz")) < 64 * 1024 and str(gold["torch_version"])
    worst = 0.0
    for name in NAMES:
        e, t = prr.make_inputs(name)
        assert np.array_equal(gold[f"{name}.checksum"], [np.abs(e).sum(dtype=np.float64), np.abs(t).sum(dtype=np.float64)])
        for b, n in enumerate(prr.lengths(name)):
            val, tol = prr.sisdr_rows(e[b, :, :n], t[b, :, :n])
            assert np.all(np.isfinite(val)) and np.all(np.isfinite(tol)) and np.all(tol > 0)
            used = np.abs(gold[f"{name}.rows"][b].astype(np.float64) - val) / tol
            m, mtol = prr.sisdr_mean(val, tol)
            used_mean = abs(float(gold[f"{name}.mean"][b]) - m) / mtol
            worst = max(worst, used.max(), used_mean)
            assert used.max() <= 1.0 and used_mean <= 1.0, (name, b, used, used_mean)
            v32, _ = prr.sisdr_rows(e[b, :, :n], t[b, :, :n], dt=np.float32)  # an fp32 numpy evaluation of the restatement as well
            assert np.all(np.abs(v32.astype(np.float64) - val) <= 0.5 * tol), (name, b)
    print("largest share of the bound the reference uses:", worst)


def test_sisdr_restatement_is_scale_invariant_and_exact_on_a_known_pair():
    """a = 2 s + n with n orthogonal to s and |s|^2 = |n|^2 (eps aside): proj = 2 s, SI-SDR = 10 log10(4) dB; scaling a changes nothing."""
    s = np.array([1.0, -1.0, 1.0, -1.0]) * 0.5
    n = np.array([1.0, 1.0, -1.0, -1.0]) * 0.5
    for scale in (1.0, 37.0):
        val, tol = prr.sisdr_rows(scale * (2 * s + n)[None], s[None])
        assert abs(val[0] - 10 * np.log10(4.0 * scale ** 2 / scale ** 2)) < 1e-5 and tol[0] < 1e-3


def test_length_checks_name_the_clip():
    from spiking_fullsubnet_amd import pit
    ok = pit.device_lengths(None, 3, 100, "cpu")
    assert ok is None
    for bad, msg in (([50, 60], r"one length per clip \(3\), got 2"), ([50, 60, 70, 80], r"one length per clip \(3\), got 4"),
                     ([50, 1, 70], r"lengths\[1\] = 1: clip 1 must have between 2 and 100"),
                     ([50, 60, 101], r"lengths\[2\] = 101: clip 2 must have between 2 and 100"),
                     ([0, 60, 70], r"lengths\[0\] = 0: clip 0"), ([50, -3, 70], r"lengths\[1\] = -3: clip 1"),
                     (torch.tensor([50.0, 60.0, 70.0]), "1-D integer tensor"), (torch.tensor([[50, 60, 70]]), "1-D integer tensor"),
                     ([50, 60.5, 70], r"lengths\[1\] = 60.5 is not an integer"), ([50, True, 70], r"lengths\[1\] = True is not an integer")):
        with pytest.raises(ValueError, match=msg):
            pit.device_lengths(bad, 3, 100, "cpu")

    class OnDevice(torch.Tensor):  # a CPU tensor that says it is on the device: reaches the checks of a device tensor
        is_cuda = True

    dev = lambda x: x.as_subclass(OnDevice)
    for bad in (torch.tensor([50, 60, 70]), torch.tensor([50.0, 60.0, 70.0]), torch.tensor([50, 60], dtype=torch.int32),
                torch.tensor([[50, 60, 70]], dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"a device tensor must be int32 of shape \[3\]"):
            pit.device_lengths(dev(bad), 3, 100, "cpu")
    trusted = dev(torch.tensor([50, 1, 700], dtype=torch.int32))  # a device tensor is trusted: no host read of its values
    assert pit.device_lengths(trusted, 3, 100, "cpu").data_ptr() == trusted.data_ptr()
    # through the entry points: the checks run before any kernel call; unknown keywords are still refused
    wrapper = pit.PITWrapper(pit.PairwiseNegSDR())
    e, t = dev(torch.zeros(3, 2, 100)), dev(torch.zeros(3, 2, 100))
    for fn in (wrapper, wrapper.full, wrapper.per_clip, wrapper.loss_func):
        with pytest.raises(ValueError, match=r"lengths\[1\] = 1: clip 1"):
            fn(e, t, lengths=[50, 1, 70])
        with pytest.raises(ValueError, match="one length per clip"):
            fn(e, t, lengths=[50, 70])
    with pytest.raises(NotImplementedError, match="keyword"):
        wrapper(e, t, lengths=[50, 60, 70], foo=1)
    with pytest.raises(NotImplementedError, match="CPU"):
        wrapper.per_clip(torch.zeros(3, 2, 100), torch.zeros(3, 2, 100), lengths=[50, 60, 70])


def test_metric_sisdr_refusals():
    import spiking_fullsubnet_amd as pkg
    from spiking_fullsubnet_amd import metric, pit
    assert pkg.SISDR is metric.SISDR and pkg.PerClip is pit.PerClip and pit.PerClip._fields == ("loss", "perm", "pair", "reordered", "si_sdr")
    m = metric.SISDR()
    with pytest.raises(NotImplementedError, match="CPU"):
        m(torch.zeros(100), torch.zeros(100))
    with pytest.raises(NotImplementedError, match="torch tensors"):
        m(np.zeros(100, np.float32), np.zeros(100, np.float32))
    with pytest.raises(TypeError, match=r"\[L\], \[S, L\] or \[B, S, L\]"):
        m(torch.zeros(2, 100), torch.zeros(2, 99))
    with pytest.raises(TypeError, match=r"\[L\], \[S, L\] or \[B, S, L\]"):
        m(torch.zeros(1, 1, 2, 100), torch.zeros(1, 1, 2, 100))

    class OnDevice(torch.Tensor):
        is_cuda = True

    dev = lambda x: x.as_subclass(OnDevice)
    with pytest.raises(NotImplementedError, match="float32"):
        m(dev(torch.zeros(2, 100).double()), dev(torch.zeros(2, 100).double()))
    with pytest.raises(ValueError, match=r"lengths\[0\] = 101: clip 0"):
        m(dev(torch.zeros(2, 100)), dev(torch.zeros(2, 100)), lengths=101)
    with pytest.raises(ValueError, match=r"one length per clip \(3\), got 2"):
        m(dev(torch.zeros(3, 2, 100)), dev(torch.zeros(3, 2, 100)), lengths=[100, 50])
