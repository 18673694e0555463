"""The recipe loss on rows of different lengths and the REVERB loss on the device (sfsn_recipe_loss_ragged and the `lengths=` surface
of spiking_fullsubnet_amd.loss) against the fp64 composition and the derived bounds of tests/lossraggedref.py: values, row terms and
gradient for every case of its table with NaN past every clip's end, every row bit for bit against the equal-length kernel on the row
alone, row_len = NULL against lossref's whole-batch bounds, the Python surface bit for bit against the C call, determinism, and a
training step with the REVERB loss and device lengths replayed from a HIP graph."""
import ctypes

import numpy as np
import pytest
import torch

import lossraggedref as lr
import lossref
import refweights as rw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INTEL3 = (lossref.RECIPE_WEIGHTS + (0.0,), lr.FREQ | lr.MAG | lr.SDR)  # what RecipeLoss asks of the kernel


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _poisoned(name, which=lr.INTEL):
    """(est, tgt [rows, Lp] device tensors with NaN written past every row's end, row lengths int32 device tensor, lens, reference)."""
    e, t, lengths, ref = lr.case(name, which)
    Lp, lens = e.shape[-1], ref["lens"]
    tail = np.arange(Lp)[None, :] >= lens[:, None]
    e2, t2 = e.reshape(-1, Lp).copy(), t.reshape(-1, Lp).copy()  # (the shared inputs stay as they are)
    e2[tail] = t2[tail] = np.nan
    return _t(e2), _t(t2), torch.tensor(lens, dtype=torch.int32, device=DEV), lens, ref


def _c_ragged(e, t, row_len, weights, flags, want_grad=True, stream=None):
    """sfsn_recipe_loss_ragged through ctypes on [rows, Lp] device tensors -> (terms [5], row_terms [rows, 4], grad or None) numpy."""
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    rows, n = e.shape
    st = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(st):
        terms = torch.full((5,), float("nan"), device=DEV)
        row_terms = torch.full((rows, 4), float("nan"), device=DEV)
        grad = torch.full_like(e, float("nan")) if want_grad else None
        scratch = torch.empty(L.sfsn_recipe_loss_ragged_scratch_bytes(rows, n), dtype=torch.uint8, device=DEV)
        _lib.check(L.sfsn_recipe_loss_ragged(e.data_ptr(), t.data_ptr(), rows, n, row_len.data_ptr() if row_len is not None else None,
                                             *weights, flags, terms.data_ptr(), row_terms.data_ptr(),
                                             grad.data_ptr() if want_grad else None, scratch.data_ptr(), ctypes.c_void_p(st.cuda_stream)),
                   "sfsn_recipe_loss_ragged")
    st.synchronize()
    return terms.cpu().numpy(), row_terms.cpu().numpy(), (grad.cpu().numpy() if want_grad else None)


def _c_equal(e, t, weights, flags=7):
    """The existing sfsn_recipe_loss on [rows, L] device tensors -> (terms [4], grad) numpy."""
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    rows, n = e.shape
    terms, grad = torch.full((4,), float("nan"), device=DEV), torch.full_like(e, float("nan"))
    scratch = torch.empty(L.sfsn_recipe_loss_scratch_bytes(rows, n), dtype=torch.uint8, device=DEV)
    _lib.check(L.sfsn_recipe_loss(e.data_ptr(), t.data_ptr(), rows, n, *weights, flags, terms.data_ptr(), grad.data_ptr(), scratch.data_ptr(),
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "sfsn_recipe_loss")
    torch.cuda.synchronize()
    return terms.cpu().numpy(), grad.cpu().numpy()


def _as_got(terms, row_terms, grad, shape):
    return dict(freq=terms[0], mag=terms[1], sisnr=terms[2], time=terms[3], total=terms[4], row_terms=row_terms, grad=grad.reshape(shape))


@pytest.mark.parametrize("which", [lr.INTEL, lr.REVERB], ids=["intel", "reverb"])
@pytest.mark.parametrize("name", lr.NAMES)
def test_c_abi_values_row_terms_and_gradient_within_the_derived_bounds(name, which):
    e, t, row_len, lens, ref = _poisoned(name, which)
    terms, row_terms, grad = _c_ragged(e, t, row_len, *which)
    bad, used = lr.outside(_as_got(terms, row_terms, grad, ref["grad"].shape), ref)
    print(name, "share of each bound used:", used)
    assert not bad, (bad, used)
    assert not np.isnan(terms).any() and not np.isnan(row_terms).any() and not np.isnan(grad).any()
    tail = np.arange(grad.shape[1])[None, :] >= lens[:, None]
    assert np.array_equal(_bits(grad[tail]), np.zeros(int(tail.sum()), np.uint32))  # exactly +0.0f past every clip's end
    fwd, fwd_rows, none = _c_ragged(e, t, row_len, *which, want_grad=False)
    assert none is None and np.array_equal(_bits(fwd), _bits(terms)) and np.array_equal(_bits(fwd_rows), _bits(row_terms))
    # a batch term is the mean of the fp32 row terms in row order (fp64)
    acc = np.zeros(4)
    for r in range(len(lens)):
        acc += row_terms[r].astype(np.float64)
    assert np.array_equal(_bits(terms[:4]), _bits((acc / len(lens)).astype(np.float32)))


@pytest.mark.parametrize("name", lr.NAMES)
def test_every_row_forward_has_the_bits_of_the_row_alone(name):
    e, t, row_len, lens, _ = _poisoned(name)
    _, rt7, _ = _c_ragged(e, t, row_len, *INTEL3, want_grad=False)
    _, rt15, _ = _c_ragged(e, t, row_len, *lr.INTEL, want_grad=False)
    assert np.array_equal(_bits(rt7[:, :3]), _bits(rt15[:, :3])) and not rt7[:, 3].any()
    for r, L in enumerate(lens):
        er, tr = e[r:r + 1, :L].clone(), t[r:r + 1, :L].clone()  # (a copy of its own: contiguous AND 16-byte aligned)
        alone, _ = _c_equal(er, tr, lossref.RECIPE_WEIGHTS)  # the EXISTING entry on the row alone
        assert np.array_equal(_bits(rt7[r, :3]), _bits(alone[:3])), (name, r, rt7[r], alone)
        _, alone_t, _ = _c_ragged(er, tr, None, (0.0, 0.0, 0.0, 1.0), lr.TIME, want_grad=False)
        assert np.array_equal(_bits(rt15[r, 3]), _bits(alone_t[0, 3])), (name, r)


@pytest.mark.parametrize("name", ["r4_edges", "r4_odd", "r2x2"])
def test_every_row_gradient_has_the_bits_of_the_row_alone(name):
    """Four rows: the factor 1 / rows is a power of two, so the row alone with the weights c / 4 has the same coefficients exactly."""
    e, t, row_len, lens, _ = _poisoned(name)
    assert len(lens) == 4
    _, _, grad = _c_ragged(e, t, row_len, *INTEL3)
    quarter = tuple(float(np.float32(c) / np.float32(4)) for c in lossref.RECIPE_WEIGHTS)
    for r, L in enumerate(lens):
        _, alone = _c_equal(e[r:r + 1, :L].clone(), t[r:r + 1, :L].clone(), quarter)
        assert np.array_equal(_bits(grad[r, :L]), _bits(alone[0])), (name, r)


@pytest.mark.parametrize("name", [c[0] for c in lossref.CASES])
def test_null_row_len_lies_within_the_whole_batch_bounds(name):
    """lossref's value bounds admit 16 fp32 roundings on the path of a term; the equal-length kernel takes 13 and the per-row rounding
    of the ragged entry one more."""
    _, shape, seed, eq = next(c for c in lossref.CASES if c[0] == name)
    e, t = lossref.make_inputs(shape, seed, eq)
    ref = lossref.reference(e, t)
    L = shape[-1]
    terms, _, grad = _c_ragged(_t(e.reshape(-1, L)), _t(t.reshape(-1, L)), None, *INTEL3)
    bad, used = lossref.outside(dict(freq=terms[0], mag=terms[1], sisnr=terms[2], total=terms[4], grad=grad.reshape(e.shape)), ref)
    print(name, used)
    assert not bad and terms[3] == 0, (bad, used)
    if name in [c[0] for c in lossref.GOLDEN_CASES]:  # the REVERB weights, against the reference the golden file is pinned to
        rref = lr.reference(e, t, [L] * shape[0], *lr.REVERB)
        terms, row_terms, grad = _c_ragged(_t(e), _t(t), None, *lr.REVERB)
        bad, used = lr.outside(_as_got(terms, row_terms, grad, e.shape), rref)
        print(name, "reverb", used)
        assert not bad, (bad, used)


@pytest.mark.parametrize("name", lr.NAMES)
def test_python_surface_returns_the_bits_of_the_c_call(name):
    from spiking_fullsubnet_amd import loss
    e, t, lengths, ref = lr.case(name)
    Lp = e.shape[-1]
    e2, t2, row_len, lens, _ = _poisoned(name)
    est_p, tgt_p = e2.reshape(e.shape), t2.reshape(e.shape)
    dev_len = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    # RecipeLoss: host list and device tensor
    terms, row_terms, grad = _c_ragged(e2, t2, row_len, *INTEL3)
    for given in (list(lengths), torch.tensor(lengths), dev_len):
        est = est_p.clone().requires_grad_(True)
        total, parts = loss.RecipeLoss()(est, tgt_p, lengths=given)
        total.backward()
        assert sorted(parts) == ["loss", "loss_freq_mae", "loss_mag_mae", "loss_sdr", "loss_sdr_norm"] and parts["loss"] is total
        assert np.array_equal(_bits(est.grad.cpu().numpy().reshape(-1, Lp)), _bits(grad))
        f, m, s = parts["loss_freq_mae"], parts["loss_mag_mae"], parts["loss_sdr"]
        assert np.array_equal(_bits([float(f), float(m), float(s)]), _bits(terms[:3]))
        assert torch.equal(parts["loss_sdr_norm"], 0.001 * (100 - s)) and torch.equal(total.detach(), f + m + 0.001 * (100 - s))
    pc = loss.RecipeLoss().per_clip(est_p, tgt_p, dev_len)
    clip = torch.from_numpy(row_terms).to(DEV).view(len(lengths), -1, 4).mean(1)
    assert sorted(pc) == sorted(parts) and all(v.shape == (len(lengths),) and v.is_cuda and not v.requires_grad for v in pc.values())
    assert torch.equal(pc["loss_freq_mae"], clip[:, 0]) and torch.equal(pc["loss_mag_mae"], clip[:, 1]) and torch.equal(pc["loss_sdr"], clip[:, 2])
    assert torch.equal(pc["loss_sdr_norm"], 0.001 * (100 - clip[:, 2])) and torch.equal(pc["loss"], clip[:, 0] + clip[:, 1] + pc["loss_sdr_norm"])
    # ReverbRecipeLoss
    terms, row_terms, grad = _c_ragged(e2, t2, row_len, *lr.REVERB)
    est = est_p.clone().requires_grad_(True)
    total, parts = loss.ReverbRecipeLoss()(est, tgt_p, lengths=list(lengths))
    total.backward()
    assert sorted(parts) == ["loss", "loss_freq_mae", "loss_mag_mae", "loss_time_mae"] and parts["loss"] is total
    assert np.array_equal(_bits(est.grad.cpu().numpy().reshape(-1, Lp)), _bits(grad))
    got = [float(parts[k].detach()) for k in ("loss_freq_mae", "loss_mag_mae", "loss_time_mae", "loss")]
    assert np.array_equal(_bits(got), _bits(terms[[0, 1, 3, 4]]))
    assert torch.equal(total.detach(), parts["loss_freq_mae"] + parts["loss_mag_mae"] + parts["loss_time_mae"])
    pc = loss.ReverbRecipeLoss().per_clip(est_p, tgt_p, list(lengths))
    clip = torch.from_numpy(row_terms).to(DEV).view(len(lengths), -1, 4).mean(1)
    assert sorted(pc) == sorted(parts) and torch.equal(pc["loss_time_mae"], clip[:, 3]) and torch.equal(pc["loss_freq_mae"], clip[:, 0])
    assert torch.equal(pc["loss"], clip[:, 0] + clip[:, 1] + clip[:, 3]) and not pc["loss"].requires_grad
    # each single-term drop-in: the component's bits, and the C call's gradient with that flag alone
    for fn, flag, i in ((loss.freq_MAE, lr.FREQ, 0), (loss.mag_MAE, lr.MAG, 1), (loss.SISNRLoss(), lr.SDR, 2), (loss.time_MAE, lr.TIME, 3)):
        w = tuple(1.0 if flag == b else 0.0 for b in (1, 2, 4, 8))
        terms1, _, grad1 = _c_ragged(e2, t2, row_len, w, flag)
        est1 = est_p.clone().requires_grad_(True)
        v = fn(est1, tgt_p, lengths=dev_len)
        assert v.shape == () and np.array_equal(_bits(float(v.detach())), _bits(terms1[i])) and terms1[4] == terms1[i], fn
        v.backward()
        assert np.array_equal(_bits(est1.grad.cpu().numpy().reshape(-1, Lp)), _bits(grad1)), fn
        assert [terms1[j] for j in range(4) if j != i] == [0.0] * 3
    assert torch.equal(loss.SISNRLoss(return_neg=True)(est_p, tgt_p, lengths=dev_len), -loss.SISNRLoss()(est_p, tgt_p, lengths=dev_len))
    with pytest.raises(ValueError, match="int32 of shape"):
        loss.RecipeLoss()(est_p, tgt_p, lengths=dev_len.long())


def test_time_mae_without_lengths_is_a_drop_in_for_l1_loss():
    from spiking_fullsubnet_amd import loss
    e, t, lengths, _ = lr.case("r2x2")
    ref = lr.reference(e, t, [e.shape[-1]] * e.shape[0], (0.0, 0.0, 0.0, 1.0), lr.TIME)
    est = _t(e).requires_grad_(True)
    ours = loss.time_MAE(est, _t(t))
    ours.backward()
    aten = torch.nn.functional.l1_loss(_t(e), _t(t))
    print(ours.item(), aten.item(), ref["time"], ref["tol"]["time"])
    assert abs(ours.item() - ref["time"]) <= ref["tol"]["time"] and abs(aten.item() - ref["time"]) <= ref["tol"]["time"]
    assert np.all(np.abs(est.grad.cpu().numpy() - ref["grad"]) <= ref["grad_tol"])


def test_backward_scales_the_stored_gradient():
    from spiking_fullsubnet_amd import loss
    e2, t2, row_len, lens, _ = _poisoned("r4_edges")
    _, _, grad = _c_ragged(e2, t2, row_len, *lr.REVERB)
    est = e2.clone().requires_grad_(True)
    (2.5 * loss.ReverbRecipeLoss()(est, t2, lengths=row_len)[0]).backward()
    assert np.array_equal(_bits(est.grad.cpu().numpy()), _bits((np.float32(2.5) * grad).astype(np.float32)))


def test_non_contiguous_and_offset_views_are_copied_not_misread():
    from spiking_fullsubnet_amd import loss
    e2, t2, row_len, lens, _ = _poisoned("r4_odd")
    want = loss.ReverbRecipeLoss()(e2, t2, lengths=row_len)[0]
    wide_e, wide_t = torch.zeros(4, e2.shape[1] + 3, device=DEV), torch.zeros(4, e2.shape[1] + 3, device=DEV)
    wide_e[:, 3:], wide_t[:, 3:] = e2, t2
    assert torch.equal(loss.ReverbRecipeLoss()(wide_e[:, 3:], wide_t[:, 3:], lengths=row_len)[0], want)
    padded_len = torch.zeros(5, dtype=torch.int32, device=DEV)
    padded_len[1:] = row_len
    assert torch.equal(loss.ReverbRecipeLoss()(e2, t2, lengths=padded_len[1:])[0], want)  # a lengths view that is not 16-byte aligned


def test_repeated_calls_and_a_side_stream_are_bit_identical():
    e2, t2, row_len, lens, _ = _poisoned("r3_chunks")
    a = _c_ragged(e2, t2, row_len, (1.0, 1.0, -0.001, 1.0), 15)
    b = _c_ragged(e2, t2, row_len, (1.0, 1.0, -0.001, 1.0), 15)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    c = _c_ragged(e2, t2, row_len, (1.0, 1.0, -0.001, 1.0), 15, stream=side)
    for other in (b, c):
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, other))


def test_training_step_with_the_reverb_loss_and_device_lengths_replayed_from_a_hip_graph_equals_the_eager_step():
    """training.GraphedTrainStep unchanged, with loss_fn closing over a static clean tensor and a static int32 lengths tensor on the
    device (no host work inside the step, so the captured region stays a linear chain): the replayed loss and every parameter gradient
    are bit-identical to the eager step from the same state."""
    import spiking_fullsubnet_amd as pkg
    from spiking_fullsubnet_amd import training as tr
    kw = rw.LIVE_TINY
    m = pkg.SpikingFullSubNet(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in rw.live_state_dict(kw, 11).items()}, strict=True)
    m = m.to(DEV).train()
    waves = [_t(rw.synth_wave(4, 24, seed=s)) for s in (1, 2, 3)]
    shape = m(waves[0])[0].shape  # (moves the BatchNorm buffers: the state both sides start from is taken after it)
    n_out = shape[-1]
    state0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    clean = (0.5 * _t(rw.synth_wave(4, 24, seed=7)))[..., :n_out].contiguous()
    assert clean.shape == shape and n_out > 1025
    lengths = torch.tensor([n_out, 1025, (n_out + 1025) // 2, n_out - 1][:shape[0]], dtype=torch.int32, device=DEV)
    recipe = pkg.ReverbRecipeLoss()
    loss_fn = lambda out: recipe(out[0], clean, lengths=lengths)[0]

    def restore():
        with torch.no_grad():
            for k, v in m.state_dict().items():
                v.copy_(state0[k])

    eager = []
    for w in waves[1:]:
        for p in m.parameters():
            p.grad = None
        loss = loss_fn(m(w))
        loss.backward()
        eager.append((float(loss), [p.grad.clone() for p in m.parameters()]))
        del loss
    restore()
    gs = tr.GraphedTrainStep(m, waves[0], loss_fn)
    for (l_e, g_e), w in zip(eager, waves[1:]):
        l_g = gs(w)
        assert float(l_g) == l_e and np.isfinite(l_e)
        for (k, p), ge in zip(m.named_parameters(), g_e):
            assert torch.equal(p.grad, ge), f"gradient of {k} differs between the replayed and the eager step"
    assert any(float(g.abs().max()) > 0 for g in eager[0][1])
