"""CPU checks of the recipe loss before a GPU is involved: the new exports and their refusals (answered before any launch), the
Python surface's refusals, and tests/lossref.py itself -- the fp64 restatement equals the reference's own results (the fixture made by
tests/golden/make_golden_loss.py) within its bounds, an fp32 evaluation of the same formulas uses at most half of every bound (so the
bounds are attainable), every mutant is rejected by at least one case (so the bounds bite), and the ambiguity cap holds."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lossref
from spiking_fullsubnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_refs = {}


def _case(name):
    """(est, tgt, fp64 reference) of a case, computed once and shared (never modified)."""
    if name not in _refs:
        _, shape, seed, eq = next(c for c in lossref.CASES if c[0] == name)
        e, t = lossref.make_inputs(shape, seed, eq)
        _refs[name] = (e, t, lossref.reference(e, t))
    return _refs[name]


NAMES = [c[0] for c in lossref.CASES]


def test_exports_exist_with_their_prototypes_and_the_abi_is_still_21():
    _lib.build()
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "sfsn.h")).read()
    assert re.search(r"size_t sfsn_recipe_loss_scratch_bytes\(int rows, int n_samples\);", header)
    proto = re.search(r"int sfsn_recipe_loss\((.*?)\);", header, re.S).group(1)
    proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    assert [" ".join(a.split()) for a in proto.split(",")] == [
        "const float* est", "const float* tgt", "int rows", "int n_samples", "float c_freq", "float c_mag", "float c_sdr", "int flags",
        "float* terms", "float* grad_est", "void* scratch", "void* stream"]
    assert {"sfsn_recipe_loss", "sfsn_recipe_loss_scratch_bytes"} <= set(_lib.EXPORTS)
    assert L.sfsn_recipe_loss.argtypes == [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_float] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 4
    assert L.sfsn_recipe_loss.restype == ctypes.c_int and L.sfsn_recipe_loss_scratch_bytes.restype == ctypes.c_size_t
    assert L.sfsn_abi_version() == _lib.ABI_VERSION == 21
    assert int(re.search(r"#define SFSN_ABI_VERSION (\d+)", header).group(1)) == 21
    assert (_lib.LOSS_FREQ, _lib.LOSS_MAG, _lib.LOSS_SDR) == tuple(
        int(re.search(rf"#define SFSN_LOSS_{n} (\d+)", header).group(1)) for n in ("FREQ", "MAG", "SDR"))


def test_scratch_bytes_cover_the_three_regions():
    L = _lib.lib()
    rows, n = 3, 5000
    T = 1 + n // 512
    need = rows * T * 4 * 4 + rows * ((n + 8191) // 8192) * 5 * 8 + rows * T * 2048 * 4
    got = L.sfsn_recipe_loss_scratch_bytes(rows, n)
    assert need <= got <= need + 3 * 256
    assert L.sfsn_recipe_loss_scratch_bytes(0, n) == 0 and L.sfsn_recipe_loss_scratch_bytes(rows, 1024) == 0
    assert L.sfsn_recipe_loss_scratch_bytes(1, 1025) > 0
    assert L.sfsn_recipe_loss_scratch_bytes(70000, 131072) == 0


def test_argument_refusals_are_answered_before_any_launch():
    """None of these reaches a launch (the pointers are never dereferenced on the host), so they answer on a box without a GPU."""
    L = _lib.lib()
    p = 0x10000  # a 16-byte aligned address that is never read

    def call(est=p, tgt=p, rows=2, n=4096, flags=7, terms=p, grad=p, scratch=p):
        return L.sfsn_recipe_loss(est, tgt, rows, n, 1.0, 1.0, -0.001, flags, terms, grad, scratch, None)

    for kw in (dict(est=None), dict(tgt=None), dict(terms=None), dict(scratch=None), dict(est=p + 4), dict(tgt=p + 8), dict(terms=p + 4),
               dict(grad=p + 4), dict(scratch=p + 8), dict(rows=0), dict(rows=-3), dict(flags=0), dict(flags=8), dict(n=1024), dict(n=0),
               dict(n=-5)):
        assert call(**kw) == _lib.SFSN_EINVAL, kw
    assert L.sfsn_strerror(_lib.SFSN_EINVAL).decode() == "invalid argument"
    for kw in (dict(rows=70000, n=131072), dict(rows=1 << 20, n=4096), dict(rows=600, n=1 << 20)):
        assert call(**kw) == _lib.SFSN_EUNSUPPORTED, kw
    with pytest.raises(ValueError, match="invalid argument"):
        _lib.check(call(n=1024), "sfsn_recipe_loss")
    with pytest.raises(NotImplementedError):
        _lib.check(call(rows=70000, n=131072))


def test_python_refusals_name_their_limit():
    from spiking_fullsubnet_amd import loss
    import spiking_fullsubnet_amd as pkg
    assert pkg.RecipeLoss is loss.RecipeLoss
    e, t = torch.zeros(2, 4096), torch.zeros(2, 4096)
    fns = (loss.freq_MAE, loss.mag_MAE, loss.SISNRLoss(), loss.RecipeLoss())
    for fn in fns:
        with pytest.raises(NotImplementedError, match="CPU"):
            fn(e, t)
        with pytest.raises(RuntimeError, match="Dimension mismatch"):
            fn(e, t[:, :-1])
    for fn in (loss.freq_MAE, loss.mag_MAE):
        with pytest.raises(NotImplementedError, match="win=2048, stride=512"):
            fn(e, t, win=1024)
        with pytest.raises(NotImplementedError, match="win=2048, stride=512"):
            fn(e, t, stride=256)
        with pytest.raises(NotImplementedError, match="srs"):
            fn(e, t, srs=[16000, 16000], sudo_sr=16000)

    class OnDevice(torch.Tensor):  # a CPU tensor that says it is on the device: reaches the checks behind the device check
        is_cuda = True

    def dev(x):
        return x.as_subclass(OnDevice)

    for fn in fns:
        with pytest.raises(NotImplementedError, match="float32"):
            fn(dev(e.double()), dev(t.double()))
        with pytest.raises(NotImplementedError, match="float32"):
            fn(dev(e), dev(t.half()))
        with pytest.raises(NotImplementedError, match="target that requires"):
            fn(dev(e), dev(t.clone().requires_grad_(True)))
        with pytest.raises(NotImplementedError, match="longer than 1024"):
            fn(dev(e[:, :1024]), dev(t[:, :1024]))


def test_fixture_is_small_and_holds_the_golden_cases():
    path = os.path.join(ROOT, "tests", "golden", "recipe_loss.npz")
    assert os.path.getsize(path) < 512 * 1024
    gold = np.load(path)
    for name, shape, seed, eq in lossref.GOLDEN_CASES:
        e, t, _ = _case(name)
        assert np.array_equal(gold[f"{name}.est"], e) and np.array_equal(gold[f"{name}.tgt"], t)  # the generator is the fixture's


@pytest.mark.parametrize("name", [c[0] for c in lossref.GOLDEN_CASES])
def test_reference_results_lie_within_the_bounds_of_the_restatement(name):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "recipe_loss.npz"))
    e, t, ref = _case(name)
    v = gold[f"{name}.values"]
    bad, used = lossref.outside(dict(freq=v[0], mag=v[1], sisnr=v[2], total=v[3], grad=gold[f"{name}.grad"]), ref)
    print(name, used)
    assert not bad, (bad, used)


@pytest.mark.parametrize("name", NAMES)
def test_fp32_evaluation_uses_at_most_half_of_every_bound(name):
    e, t, ref = _case(name)
    bad, used = lossref.outside(lossref.reference(e, t, dt=np.float32), ref)
    print(name, used)
    assert not bad and max(used.values()) <= 0.5, used


@pytest.mark.parametrize("name", NAMES)
def test_bounds_are_not_vacuous(name):
    """Every value bound is below 0.2 % of the value (SI-SNR at the eps floor: of 30 dB), and, away from frames with an ambiguous term
    and from the eps floor, the gradient bound is a small part of the gradient's typical size: with one or two ambiguous terms per frame
    on average only samples whose four frames all have none are sharp, so a twentieth of the samples is asked for."""
    e, t, ref = _case(name)
    for k in ("freq", "mag", "sisnr", "total"):
        assert ref["tol"][k] <= 2e-3 * abs(ref[k]), (k, ref["tol"][k], ref[k])
    g, tol = np.abs(ref["grad"]).reshape(ref["rows"], -1), ref["grad_tol"].reshape(ref["rows"], -1)
    sharp = tol <= 0.05 * np.median(g)
    print(name, "sharp share", sharp.mean())
    if name in ("r2_L4096", "r2_L5000"):  # (the shorter cases have too few frames clear of the margins for a share to mean much)
        assert sharp.mean() >= 0.05, sharp.mean()


@pytest.mark.parametrize("mut", lossref.MUTATIONS)
def test_every_mutant_is_rejected(mut):
    rejected = {}
    for name in NAMES:
        e, t, ref = _case(name)
        bad, _ = lossref.outside(lossref.reference(e, t, mut=mut), ref)
        if bad:
            rejected[name] = bad
    print(mut, rejected)
    assert rejected, mut
    if mut == "no_eps":  # eps matters only at its floor
        assert "r3_L3000_eq" in rejected
    if mut in ("edge_repeat", "no_fold", "double_inner", "symmetric_hann"):  # geometry: no case with a sharp gradient check may miss it
        assert {"r2_L4096", "r2_L5000", "r2x2_L2600"} <= set(rejected), rejected


@pytest.mark.parametrize("name", NAMES)
def test_ambiguity_cap_holds(name):
    e, t, ref = _case(name)
    loose = ref["n_ambiguous"] - ref["n_structural"]
    print(name, ref["n_ambiguous"], ref["n_structural"], ref["n_terms"])
    assert 0 <= loose <= lossref.AMBIGUOUS_CAP * ref["n_terms"], (loose, ref["n_terms"])
