"""CPU checks of the permutation-invariant SI-SDR loss before a GPU is involved: the two new exports and their refusals (answered before
any launch), the Python surface's refusals and helpers, and tests/pitref.py itself -- the fp64 restatement equals the reference's own
results (the fixture made by tests/golden/make_golden_pit.py) within its bounds and picks the reference's permutations, its gradients
equal central finite differences of its loss, an fp32 evaluation of the same formulas uses at most half of every bound, every mutant
is rejected by at least one case, and no clip of the table is ambiguous."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pitref
from spiking_fullsubnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c[0] for c in pitref.CASES]
GOLDEN = [c[0] for c in pitref.GOLDEN_CASES]
ZM = [True, False]
_refs = {}


def _case(name, zm):
    """(est, ref, cotangent, fp64 reference) of a case, computed once and shared (never modified)."""
    if (name, zm) not in _refs:
        e, t = pitref.make_inputs(name)
        w = pitref.cotangent(name)
        _refs[name, zm] = (e, t, w, pitref.reference(e, t, zm, cot=w))
    return _refs[name, zm]


def test_exports_exist_with_their_prototypes_and_the_abi_is_still_21():
    _lib.build()
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "sfsn.h")).read()
    assert re.search(r"size_t sfsn_pit_sdr_scratch_bytes\(int clips, int sources, int n_samples\);", header)
    proto = re.search(r"int sfsn_pit_sdr\((.*?)\);", header, re.S).group(1)
    proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    assert [" ".join(a.split()) for a in proto.split(",")] == [
        "const float* est", "const float* ref", "int clips", "int sources", "int n_samples", "int zero_mean", "float eps",
        "const float* pair_cot", "float* pair", "int32_t* perm", "float* loss", "float* grad_est", "float* reordered", "void* scratch",
        "void* stream"]
    assert {"sfsn_pit_sdr", "sfsn_pit_sdr_scratch_bytes"} <= set(_lib.EXPORTS)
    assert L.sfsn_pit_sdr.argtypes == [ctypes.c_void_p] * 2 + [ctypes.c_int] * 4 + [ctypes.c_float] + [ctypes.c_void_p] * 8
    assert L.sfsn_pit_sdr_scratch_bytes.argtypes == [ctypes.c_int] * 3
    assert L.sfsn_pit_sdr.restype == ctypes.c_int and L.sfsn_pit_sdr_scratch_bytes.restype == ctypes.c_size_t
    assert L.sfsn_abi_version() == _lib.ABI_VERSION == 21
    assert int(re.search(r"#define SFSN_ABI_VERSION (\d+)", header).group(1)) == 21


def test_scratch_bytes_are_zero_exactly_on_refused_shapes():
    L = _lib.lib()
    p = 0x10000

    def rc(b, s, n):
        return L.sfsn_pit_sdr(p, p, b, s, n, 1, 1e-8, None, p, p, p, p, p, p, None)

    refused = [(0, 2, 100), (-1, 2, 100), (2, 0, 100), (2, -1, 100), (2, 2, 1), (2, 2, 0), (2, 2, -7), (2, 5, 100), (1, 9, 100),
               (64, 4, 1 << 23), (1 << 16, 1, 1 << 15), (2, 4, 1 << 28), (1, 2, 1 << 30)]
    for b, s, n in refused:
        assert L.sfsn_pit_sdr_scratch_bytes(b, s, n) == 0, (b, s, n)
        assert rc(b, s, n) in (_lib.SFSN_EINVAL, _lib.SFSN_EUNSUPPORTED), (b, s, n)
    for b, s, n in [(1, 1, 2), (64, 2, 32000), (5, 4, 777), (1, 1, 0x7fffffff), (1, 4, (1 << 29) - 1), (1 << 15, 1, (1 << 16) - 1)]:
        got = L.sfsn_pit_sdr_scratch_bytes(b, s, n)
        need = b * ((n + 2047) // 2048) * (s * s + 4 * s) * 8  # one fp64 partial of S^2 + 4S sums per (clip, chunk of 2048)
        assert need <= got <= need + 256, (b, s, n, got)


def test_argument_refusals_are_answered_before_any_launch():
    """None of these reaches a launch (the pointers are never dereferenced on the host), so they answer on a box without a GPU."""
    L = _lib.lib()
    p = 0x10000  # a 16-byte aligned address that is never read

    def call(est=p, ref=p, clips=2, sources=2, n=1000, zm=1, eps=1e-8, cot=None, pair=p, perm=p, loss=p, grad=p, reordered=p, scratch=p):
        return L.sfsn_pit_sdr(est, ref, clips, sources, n, zm, eps, cot, pair, perm, loss, grad, reordered, scratch, None)

    einval = [dict(est=None), dict(ref=None), dict(pair=None), dict(perm=None), dict(loss=None), dict(scratch=None),
              dict(est=p + 4), dict(ref=p + 8), dict(pair=p + 4), dict(perm=p + 4), dict(loss=p + 12), dict(grad=p + 4), dict(reordered=p + 8),
              dict(scratch=p + 8), dict(cot=p + 4, perm=None, loss=None, reordered=None),
              dict(clips=0), dict(clips=-3), dict(sources=0), dict(sources=-1), dict(n=1), dict(n=0), dict(n=-5),
              dict(eps=-1e-8), dict(eps=float("inf")), dict(eps=float("nan")), dict(eps=float("-inf")),
              dict(cot=p), dict(cot=p, perm=None), dict(cot=p, perm=None, loss=None), dict(cot=p, loss=None, reordered=None),
              dict(cot=p, perm=None, reordered=None), dict(cot=p, pair=None, perm=None, loss=None, reordered=None)]
    for kw in einval:
        assert call(**kw) == _lib.SFSN_EINVAL, kw
    for kw in (dict(sources=5), dict(sources=9), dict(clips=64, sources=4, n=1 << 23), dict(clips=1 << 16, sources=1, n=1 << 15),
               dict(sources=5, cot=p, perm=None, loss=None, reordered=None)):
        assert call(**kw) == _lib.SFSN_EUNSUPPORTED, kw
    with pytest.raises(ValueError, match="invalid argument"):
        _lib.check(call(n=1), "sfsn_pit_sdr")
    with pytest.raises(NotImplementedError):
        _lib.check(call(sources=5))


def test_python_refusals_name_their_limit():
    import spiking_fullsubnet_amd as pkg
    from spiking_fullsubnet_amd import pit
    assert pkg.PITWrapper is pit.PITWrapper and pkg.PairwiseNegSDR is pit.PairwiseNegSDR and pkg.pit is pit
    pw = pit.PairwiseNegSDR()
    assert (pw.zero_mean, pw.EPS) == (True, 1e-8) and pit.PairwiseNegSDR(zero_mean=False, EPS=1e-6).EPS == 1e-6
    wrapper = pit.PITWrapper(pw)
    assert wrapper.loss_func is pw
    e, t = torch.zeros(2, 2, 100), torch.zeros(2, 2, 100)
    fns = (pw, wrapper, wrapper.full)
    for fn in fns:
        with pytest.raises(NotImplementedError, match="CPU"):
            fn(e, t)
        for bad_e, bad_t in ((e, t[:, :, :-1]), (e[0], t[0]), (e[:, :1], t)):
            with pytest.raises(TypeError, match=r"Inputs must be of shape \[batch, n_src, time\], got"):
                fn(bad_e, bad_t)
    with pytest.raises(NotImplementedError, match="keyword"):
        wrapper(e, t, foo=1)
    for other in (lambda a, b: a, torch.nn.MSELoss(), None):
        with pytest.raises(NotImplementedError, match="PairwiseNegSDR"):
            pit.PITWrapper(other)

    class OnDevice(torch.Tensor):  # a CPU tensor that says it is on the device: reaches the checks behind the device check
        is_cuda = True

    def dev(x):
        return x.as_subclass(OnDevice)

    for fn in fns:
        with pytest.raises(NotImplementedError, match="float32"):
            fn(dev(e.double()), dev(t.double()))
        with pytest.raises(NotImplementedError, match="float32"):
            fn(dev(e), dev(t.half()))
        with pytest.raises(NotImplementedError, match="ref that requires"):
            fn(dev(e), dev(t.clone().requires_grad_(True)))
        with pytest.raises(NotImplementedError, match="at most 4 sources"):
            fn(dev(torch.zeros(1, 5, 50)), dev(torch.zeros(1, 5, 50)))


def test_torch_helpers_return_what_the_reference_returns():
    """find_best_perm and reorder_source against the fixture's pair and chosen indices, and the first-minimum rule on an exact tie."""
    from spiking_fullsubnet_amd.pit import PITWrapper
    gold = np.load(os.path.join(ROOT, "tests", "golden", "pit_loss.npz"))
    for name in GOLDEN:
        e, _, _, ref = _case(name, True)
        pair = torch.from_numpy(gold[f"{name}.zm1.pair"])
        min_loss, idx = PITWrapper.find_best_perm(pair)
        assert idx.dtype == torch.int64 and np.array_equal(idx.numpy(), gold[f"{name}.zm1.perm"])
        assert abs(float(min_loss.mean()) - float(gold[f"{name}.zm1.loss"])) <= 4 * pitref.U * max(1.0, float(pair.abs().max()))
        assert np.array_equal(PITWrapper.reorder_source(torch.from_numpy(e), idx).numpy(), ref["reordered"])
    tie = torch.tensor([[[1.0, 2.0], [1.0, 2.0]], [[3.0, 1.0], [1.0, 3.0]]])
    assert PITWrapper.find_best_perm(tie)[1].tolist() == [[0, 1], [1, 0]]
    tie3 = torch.zeros(1, 3, 3)
    assert PITWrapper.find_best_perm(tie3)[1].tolist() == [[0, 1, 2]]


def test_fixture_is_small_and_made_from_the_generator():
    path = os.path.join(ROOT, "tests", "golden", "pit_loss.npz")
    assert os.path.getsize(path) < 512 * 1024
    gold = np.load(path)
    for name in GOLDEN:
        e, t, _, _ = _case(name, True)
        assert np.array_equal(gold[f"{name}.checksum"], [np.abs(e).sum(dtype=np.float64), np.abs(t).sum(dtype=np.float64)])
        for zm in (0, 1):
            assert bool(gold[f"{name}.zm{zm}.reordered_is_gather"])
    e, _, _, _ = _case("b2s2_L9000_tie", True)
    assert np.array_equal(e[1, 1].view(np.uint32), e[1, 0].view(np.uint32))  # the tie is exact by construction
    e, t, _, _ = _case("b2s2_L3000_scaled", True)
    assert any(np.array_equal(e[0, 0], np.float32(0.5) * t[0, j]) for j in range(2))


@pytest.mark.parametrize("zm", ZM)
@pytest.mark.parametrize("name", GOLDEN)
def test_reference_results_lie_within_the_bounds_of_the_restatement(name, zm):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "pit_loss.npz"))
    e, t, w, ref = _case(name, zm)
    key, st = f"{name}.zm{int(zm)}", pitref.GOLDEN_STRIDE[name]
    assert np.array_equal(gold[f"{key}.perm"], ref["perm"])  # the reference's permutations
    if (name, 1) in pitref.EXACT_TIES:
        assert ref["perm"][1].tolist() == [0, 1]  # the first minimum on the exact tie, in the reference as well
    sub = dict(ref, grad=ref["grad"][..., ::st], grad_tol=ref["grad_tol"][..., ::st], grad_pw=ref["grad_pw"][..., ::st],
               grad_pw_tol=ref["grad_pw_tol"][..., ::st])
    bad, used = pitref.outside(dict(pair=gold[f"{key}.pair"], loss=gold[f"{key}.loss"], grad=gold[f"{key}.grad"], grad_pw=gold[f"{key}.grad_pw"]), sub)
    print(key, used)
    assert not bad, (bad, used)


@pytest.mark.parametrize("zm", ZM)
@pytest.mark.parametrize("name", NAMES)
def test_fp64_gradients_equal_central_finite_differences(name, zm):
    """A dozen seeded samples per case: (f(e + h) - f(e - h)) / 2h of the fp64 loss (PIT mode, the permutation held: the loss is smooth
    around an unambiguous clip) and of sum(w pair) (pairwise mode).  h = 1e-5: the truncation error is f''' h^2 / 6 and the rounding
    error 2^-53 |f| / h, both far below the 1e-5 relative (plus 1e-9 of the largest entry) asked for."""
    e, t, w, ref = _case(name, zm)
    rng = np.random.default_rng(7)
    B, S, L = e.shape
    h = 1e-5
    e64 = e.astype(np.float64)
    scaled = name == "b2s2_L3000_scaled"
    for _ in range(12):
        idx = (int(rng.integers(B)), int(rng.integers(S)), int(rng.integers(L)))
        if (scaled and idx[:2] == (0, 0)) or (name, idx[0]) in pitref.EXACT_TIES:
            idx = (1 - idx[0], idx[1], idx[2])  # (row (0, 0) of the scaled case sits on the eps floor, where the loss bends within h; on an exact tie the loss is the minimum of two branches: a kink)
        vals = []
        for sgn in (1.0, -1.0):
            x = e64.copy()
            x[idx] += sgn * h
            r = pitref.reference(x, t, zm, cot=w, mut="fd")  # (mut set: values only, no bounds)
            assert np.array_equal(r["perm"], ref["perm"])
            vals.append((r["loss"], float((w.astype(np.float64) * r["pair"]).sum())))
        fd_loss, fd_pw = (vals[0][0] - vals[1][0]) / (2 * h), (vals[0][1] - vals[1][1]) / (2 * h)
        assert abs(fd_loss - ref["grad"][idx]) <= 1e-5 * abs(ref["grad"][idx]) + 1e-9 * np.abs(ref["grad"]).max(), (idx, fd_loss, ref["grad"][idx])
        assert abs(fd_pw - ref["grad_pw"][idx]) <= 1e-5 * abs(ref["grad_pw"][idx]) + 1e-9 * np.abs(ref["grad_pw"]).max(), (idx, fd_pw, ref["grad_pw"][idx])


@pytest.mark.parametrize("zm", ZM)
@pytest.mark.parametrize("name", NAMES)
def test_fp32_evaluation_uses_at_most_half_of_every_bound(name, zm):
    e, t, w, ref = _case(name, zm)
    bad, used = pitref.outside(pitref.reference(e, t, zm, cot=w, dt=np.float32), ref)
    print(name, zm, used)
    assert not bad and max(used.values()) <= 0.5, (bad, used)


@pytest.mark.parametrize("zm", ZM)
@pytest.mark.parametrize("name", NAMES)
def test_bounds_are_not_vacuous(name, zm):
    """Away from the eps floor every pair bound is below 0.01 dB and the loss bound below 0.01 dB; the median gradient bound is below
    1 % of the median gradient magnitude (at the eps floor the bound of one row is, by derivation, larger than its gradient)."""
    _, _, _, ref = _case(name, zm)
    floor = name == "b2s2_L3000_scaled"
    tie = name == "b2s2_L9000_tie"  # (two identical estimates: one of them is 50 dB off its reference, |a|^2 / |noise|^2 is large)
    assert ref["pair_tol"].max() <= (0.5 if floor else 0.03 if tie else 0.01)
    assert ref["loss_tol"] <= (0.1 if floor else 0.01)
    assert np.median(ref["grad_tol"]) <= 0.02 * np.median(np.abs(ref["grad"]))
    assert np.median(ref["grad_pw_tol"]) <= 0.02 * np.median(np.abs(ref["grad_pw"]))


@pytest.mark.parametrize("mut", pitref.MUTATIONS)
def test_every_mutant_is_rejected(mut):
    rejected = {}
    for name in NAMES:
        for zm in ZM:
            e, t, w, ref = _case(name, zm)
            bad, _ = pitref.outside(pitref.reference(e, t, zm, cot=w, mut=mut), ref)
            if bad:
                rejected[name, zm] = bad
    print(mut, rejected)
    assert rejected, mut
    if mut == "last_min":  # only an exact tie tells the two rules apart
        assert set(k[0] for k in rejected) == {"b2s2_L9000_tie"} and all("perm" in v for v in rejected.values())
    if mut == "inverse_gather":  # needs a chosen permutation that is not its own inverse: three sources or more
        assert ("b5s4_L777", True) in rejected and "reordered" in rejected["b5s4_L777", True]
    if mut == "no_mean":
        assert ("b2s3_L4097", True) in rejected and not any(not zm for _, zm in rejected)
    if mut == "no_eps_tn":
        assert ("b1s2_L500_quiet", True) in rejected
    if mut == "grad_over_B":
        assert all("grad" in v for v in rejected.values()) and len(rejected) >= 10
    if mut == "swap_axes":
        assert all("pair" in v for v in rejected.values()) and len(rejected) >= 10


@pytest.mark.parametrize("zm", ZM)
def test_ambiguity_cap_is_zero_clips(zm):
    smallest = {}
    for name in NAMES:
        _, _, _, ref = _case(name, zm)
        amb, gap = pitref.ambiguous_clips(name, ref)
        smallest[name] = gap
        assert amb == [], (name, amb)
    print(zm, smallest)
    assert sum(ref_perm_non_identity("b5s4_L777", zm)) >= 4  # the 24-permutation case really leaves the identity


def ref_perm_non_identity(name, zm):
    _, _, _, ref = _case(name, zm)
    return [p.tolist() != list(range(ref["S"])) for p in ref["perm"]]
