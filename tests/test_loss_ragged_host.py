"""CPU checks of the ragged recipe loss and the REVERB loss before a GPU is involved: tests/lossraggedref.py itself -- its composition
and time term equal the reference's own REVERB numbers (the fixture made by tests/golden/make_golden_reverb_loss.py) within its
bounds, with equal lengths it equals lossref.reference on the whole batch, the ambiguity cap holds for every row of its table, an fp32
evaluation lies inside every bound (so the bounds are attainable) and every likely wrong semantics falls outside them (so they bite) --
then the host length check, the new exports and the refusals that are answered before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lossraggedref as lr
import lossref
from spiking_fullsubnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "reverb_loss.npz")


@pytest.mark.parametrize("name", [c[0] for c in lossref.GOLDEN_CASES])
def test_reverb_composition_and_time_term_match_the_reference_within_the_bounds(name):
    assert os.path.getsize(GOLD) < 512 * 1024
    gold = np.load(GOLD)
    _, shape, seed, eq = next(c for c in lossref.GOLDEN_CASES if c[0] == name)
    e, t = lossref.make_inputs(shape, seed, eq)
    ref = lr.reference(e, t, [shape[-1]] * shape[0], *lr.REVERB)
    v = gold[f"{name}.values"]  # freq, mag, time, freq + mag + time of the reference's own fp32 run
    got = dict(freq=v[0], mag=v[1], sisnr=0.0, time=v[2], total=v[3], grad=gold[f"{name}.grad"], row_terms=ref["row_terms"])
    bad, used = lr.outside(got, ref)
    print(name, used)
    assert not bad, (bad, used)
    assert ref["tol"]["time"] <= 1e-5 * ref["time"] and ref["sisnr"] == 0 and ref["tol"]["sisnr"] == 0  # sharp, and no SI-SNR in REVERB


@pytest.mark.parametrize("name", ["r2_L5000", "r2x2_L2600", "r3_L3000_eq"])
def test_equal_lengths_give_the_whole_batch_reference(name):
    """Both sides are fp64 evaluations of the same formulas that differ in the order of a few sums: 1e-12 relative is far above that
    and far below any bound."""
    _, shape, seed, eq = next(c for c in lossref.CASES if c[0] == name)
    e, t = lossref.make_inputs(shape, seed, eq)
    whole = lossref.reference(e, t)
    comp = lr.reference(e, t, [shape[-1]] * shape[0], lossref.RECIPE_WEIGHTS + (0.0,), lr.FREQ | lr.MAG | lr.SDR)
    for k in ("freq", "mag", "sisnr", "total"):
        assert abs(comp[k] - whole[k]) <= 1e-12 * abs(whole[k]), k
    assert comp["time"] == 0 and np.max(np.abs(comp["grad"] - whole["grad"])) <= 1e-12 * np.max(np.abs(whole["grad"]))
    # the time term alone: F.l1_loss and its autograd gradient, in fp64
    et, tt = torch.from_numpy(e).double().requires_grad_(True), torch.from_numpy(t).double()
    l1 = torch.nn.functional.l1_loss(et, tt)
    l1.backward()
    tm = lr.reference(e, t, [shape[-1]] * shape[0], (0.0, 0.0, 0.0, 1.0), lr.TIME)
    assert abs(tm["time"] - l1.item()) <= 1e-12 * l1.item() and tm["total"] == tm["time"]
    assert np.max(np.abs(tm["grad"] - et.grad.numpy())) <= 1e-12 * np.max(np.abs(tm["grad"]))


@pytest.mark.parametrize("name", lr.NAMES)
def test_ambiguity_cap_holds_for_every_row(name):
    _, _, _, ref = lr.case(name)
    for r, (n_amb, n_struct, n_terms) in enumerate(ref["rows_ambiguity"]):
        print(name, r, n_amb - n_struct, lossref.AMBIGUOUS_CAP * n_terms)
        assert 0 <= n_amb - n_struct <= lossref.AMBIGUOUS_CAP * n_terms, (r, n_amb, n_struct, n_terms)


@pytest.mark.parametrize("which", [lr.INTEL, lr.REVERB], ids=["intel", "reverb"])
@pytest.mark.parametrize("name", lr.NAMES)
def test_fp32_evaluation_lies_inside_every_bound(name, which):
    e, t, lengths, ref = lr.case(name, which)
    bad, used = lr.outside(lr.reference(e, t, lengths, *which, dt=np.float32), ref)
    print(name, used)
    assert not bad, (bad, used)
    lens = ref["lens"]
    assert np.all(ref["grad_tol"].reshape(len(lens), -1)[np.arange(e.shape[-1])[None, :] >= lens[:, None]] == 0)  # the tail is exact


@pytest.mark.parametrize("mut", lr.MUTATIONS)
def test_every_wrong_semantics_falls_outside_the_bounds(mut):
    """On every case of the table (each has a row shorter than the padded length), and in the result the semantics touches."""
    touched = dict(zero_padded="freq", reflect_padded_end="freq", frames_padded="freq", length_weighted="freq", frame_weighted="freq",
                   grad_no_rows="grad", grad_tail="grad", time_padded_stride="time")[mut]
    for name in lr.NAMES:
        e, t, lengths, ref = lr.case(name)
        bad, _ = lr.outside(lr.reference(e, t, lengths, *lr.INTEL, mut=mut), ref)
        print(mut, name, bad)
        assert touched in bad, (mut, name, bad)


def test_host_length_check_names_the_clip():
    from spiking_fullsubnet_amd import loss
    assert loss.check_lengths([1025, 4096], 2, 4096) == [1025, 4096]
    assert loss.check_lengths(torch.tensor([2000, 3000]), 2, 3000) == [2000, 3000]
    with pytest.raises(ValueError, match=r"one length per clip \(2\), got 3"):
        loss.check_lengths([2000, 2000, 2000], 2, 4096)
    with pytest.raises(ValueError, match=r"lengths\[1\] = 1024: clip 1 "):
        loss.check_lengths([2000, 1024], 2, 4096)
    with pytest.raises(ValueError, match=r"lengths\[0\] = 4097: clip 0 "):
        loss.check_lengths([4097, 2000], 2, 4096)
    with pytest.raises(ValueError, match=r"lengths\[1\] = 2000.5 is not an integer"):
        loss.check_lengths([2000, 2000.5], 2, 4096)
    with pytest.raises(ValueError, match=r"lengths\[0\] = True is not an integer"):
        loss.check_lengths([True, 2000], 2, 4096)
    with pytest.raises(ValueError, match="integer tensor"):
        loss.check_lengths(torch.tensor([2000.0, 2000.0]), 2, 4096)


def test_new_symbols_are_exported_without_an_abi_bump():
    import spiking_fullsubnet_amd as pkg
    from spiking_fullsubnet_amd import loss
    assert pkg.ReverbRecipeLoss is loss.ReverbRecipeLoss and "ReverbRecipeLoss" in pkg.__all__
    assert callable(loss.time_MAE) and callable(loss.check_lengths)
    assert callable(loss.RecipeLoss.per_clip) and callable(loss.ReverbRecipeLoss.per_clip)
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "sfsn.h")).read()
    assert re.search(r"size_t sfsn_recipe_loss_ragged_scratch_bytes\(int rows, int n_samples\);", header)
    proto = re.search(r"int sfsn_recipe_loss_ragged\((.*?)\);", header, re.S).group(1)
    proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    assert [" ".join(a.split()) for a in proto.split(",")] == [
        "const float* est", "const float* tgt", "int rows", "int n_samples", "const int32_t* row_len", "float c_freq", "float c_mag",
        "float c_sdr", "float c_time", "int flags", "float* terms", "float* row_terms", "float* grad_est", "void* scratch", "void* stream"]
    assert {"sfsn_recipe_loss_ragged", "sfsn_recipe_loss_ragged_scratch_bytes"} <= set(_lib.EXPORTS)
    assert L.sfsn_recipe_loss_ragged.argtypes == ([ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] + [ctypes.c_float] * 4
                                                  + [ctypes.c_int] + [ctypes.c_void_p] * 5)
    assert _lib.LOSS_TIME == int(re.search(r"#define SFSN_LOSS_TIME (\d+)", header).group(1)) == lr.TIME == 8
    assert L.sfsn_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define SFSN_ABI_VERSION (\d+)", header).group(1))


def test_scratch_bytes_and_argument_refusals_are_answered_before_any_launch():
    """None of these reaches a launch (the pointers are never dereferenced on the host), so they answer on a box without a GPU."""
    L = _lib.lib()
    rows, n = 3, 5000
    T = 1 + n // 512
    need = rows * T * 4 * 4 + rows * ((n + 8191) // 8192) * 6 * 8 + rows * 4 * 4 + rows * T * 2048 * 4
    assert need <= L.sfsn_recipe_loss_ragged_scratch_bytes(rows, n) <= need + 4 * 256
    assert L.sfsn_recipe_loss_ragged_scratch_bytes(0, n) == 0 and L.sfsn_recipe_loss_ragged_scratch_bytes(rows, 1024) == 0
    assert L.sfsn_recipe_loss_ragged_scratch_bytes(1, 1025) > 0 and L.sfsn_recipe_loss_ragged_scratch_bytes(70000, 131072) == 0
    p = 0x10000  # a 16-byte aligned address that is never read

    def call(est=p, tgt=p, rows=2, n=4096, row_len=p, flags=15, terms=p, row_terms=p, grad=p, scratch=p):
        return L.sfsn_recipe_loss_ragged(est, tgt, rows, n, row_len, 1.0, 1.0, -0.001, 1.0, flags, terms, row_terms, grad, scratch, None)

    for kw in (dict(est=None), dict(tgt=None), dict(terms=None), dict(scratch=None), dict(est=p + 4), dict(tgt=p + 8), dict(row_len=p + 4),
               dict(terms=p + 4), dict(row_terms=p + 8), dict(grad=p + 4), dict(scratch=p + 8), dict(rows=0), dict(rows=-3), dict(flags=0),
               dict(flags=16), dict(flags=-1), dict(n=1024), dict(n=0), dict(n=-5)):
        assert call(**kw) == _lib.SFSN_EINVAL, kw
    for kw in (dict(rows=70000, n=131072), dict(rows=1 << 20, n=4096), dict(rows=600, n=1 << 20)):
        assert call(**kw) == _lib.SFSN_EUNSUPPORTED, kw


def test_python_refusals_stay_with_lengths_and_the_new_entry_points():
    from spiking_fullsubnet_amd import loss
    e, t = torch.zeros(2, 4096), torch.zeros(2, 4096)
    fns = (loss.freq_MAE, loss.mag_MAE, loss.time_MAE, loss.SISNRLoss(), loss.RecipeLoss(), loss.ReverbRecipeLoss(),
           loss.RecipeLoss().per_clip, loss.ReverbRecipeLoss().per_clip)
    for fn in fns:
        with pytest.raises(NotImplementedError, match="CPU"):
            fn(e, t, lengths=[4096, 2000])
        with pytest.raises(RuntimeError, match="Dimension mismatch"):
            fn(e, t[:, :-1], lengths=[4096, 2000])

    class OnDevice(torch.Tensor):  # a CPU tensor that says it is on the device: reaches the checks behind the device check
        is_cuda = True

    for fn in fns:
        with pytest.raises(NotImplementedError, match="float32"):
            fn(e.double().as_subclass(OnDevice), t.double().as_subclass(OnDevice), lengths=[4096, 2000])
        with pytest.raises(NotImplementedError, match="longer than 1024"):
            fn(e[:, :1024].as_subclass(OnDevice), t[:, :1024].as_subclass(OnDevice), lengths=[1024, 1024])
        with pytest.raises(ValueError, match=r"lengths\[1\] = 4097: clip 1 "):  # the host check comes before any device work
            fn(e.as_subclass(OnDevice), t.as_subclass(OnDevice), lengths=[4096, 4097])
