"""The recipe loss on the device (sfsn_recipe_loss and spiking_fullsubnet_amd.loss) against the fp64 restatement and the derived bounds
of tests/lossref.py: losses and gradient for every case of its table (the gradient with the ambiguity rule), the Python drop-ins bit for
bit against the C call, determinism, the autograd plumbing, a whole training step replayed from a HIP graph, and one cross-check against
ATen's own torch.stft composite on the device."""
import ctypes

import numpy as np
import pytest
import torch

import lossref
import refweights as rw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = [c[0] for c in lossref.CASES]
_refs = {}


def _case(name):
    """(est, tgt, fp64 reference) of a case, computed once and shared (never modified)."""
    if name not in _refs:
        _, shape, seed, eq = next(c for c in lossref.CASES if c[0] == name)
        e, t = lossref.make_inputs(shape, seed, eq)
        _refs[name] = (e, t, lossref.reference(e, t))
    return _refs[name]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _c_call(e, t, weights=lossref.RECIPE_WEIGHTS, flags=7, want_grad=True, stream=None):
    """sfsn_recipe_loss through ctypes on [rows, L] device tensors -> (terms [4] numpy, grad numpy or None)."""
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    rows, n = e.shape
    st = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(st):
        terms = torch.full((4,), float("nan"), device=DEV)
        grad = torch.full_like(e, float("nan")) if want_grad else None
        scratch = torch.empty(L.sfsn_recipe_loss_scratch_bytes(rows, n), dtype=torch.uint8, device=DEV)
        _lib.check(L.sfsn_recipe_loss(e.data_ptr(), t.data_ptr(), rows, n, *weights, flags, terms.data_ptr(),
                                      grad.data_ptr() if want_grad else None, scratch.data_ptr(), ctypes.c_void_p(st.cuda_stream)),
                   "sfsn_recipe_loss")
    st.synchronize()
    return terms.cpu().numpy(), (grad.cpu().numpy() if want_grad else None)


@pytest.mark.parametrize("name", NAMES)
def test_c_abi_losses_and_gradient_within_the_derived_bounds(name):
    e, t, ref = _case(name)
    L = e.shape[-1]
    terms, grad = _c_call(_t(e.reshape(-1, L)), _t(t.reshape(-1, L)))
    got = dict(freq=terms[0], mag=terms[1], sisnr=terms[2], total=terms[3], grad=grad.reshape(e.shape))
    bad, used = lossref.outside(got, ref)
    print(name, "share of each bound used:", used)
    assert not bad, (bad, used)
    fwd, none = _c_call(_t(e.reshape(-1, L)), _t(t.reshape(-1, L)), want_grad=False)
    assert none is None and np.array_equal(fwd, terms)  # forward only: the same values


@pytest.mark.parametrize("name", NAMES)
def test_python_drop_ins_return_the_bits_of_the_c_call(name):
    from spiking_fullsubnet_amd import _lib, loss
    e, t, ref = _case(name)
    L = e.shape[-1]
    terms, grad = _c_call(_t(e.reshape(-1, L)), _t(t.reshape(-1, L)))
    est = _t(e).requires_grad_(True)
    total, parts = loss.RecipeLoss()(est, _t(t))
    total.backward()
    assert sorted(parts) == ["loss", "loss_freq_mae", "loss_mag_mae", "loss_sdr", "loss_sdr_norm"] and parts["loss"] is total
    assert est.grad.shape == est.shape and np.array_equal(est.grad.cpu().numpy().reshape(-1, L), grad)
    f, m, s = parts["loss_freq_mae"], parts["loss_mag_mae"], parts["loss_sdr"]
    assert (float(f), float(m), float(s)) == (float(terms[0]), float(terms[1]), float(terms[2]))
    assert torch.equal(parts["loss_sdr_norm"], 0.001 * (100 - s)) and torch.equal(total.detach(), f + m + 0.001 * (100 - s))
    # each single-term drop-in: the component's bits, and the C call's gradient with that flag alone
    for fn, flag, comp in ((loss.freq_MAE, _lib.LOSS_FREQ, f), (loss.mag_MAE, _lib.LOSS_MAG, m), (loss.SISNRLoss(), _lib.LOSS_SDR, s)):
        est1 = _t(e).requires_grad_(True)
        v = fn(est1, _t(t))
        assert v.shape == () and torch.equal(v.detach(), comp), fn
        v.backward()
        w = [1.0 if flag == b else 0.0 for b in (1, 2, 4)]
        terms1, grad1 = _c_call(_t(e.reshape(-1, L)), _t(t.reshape(-1, L)), weights=w, flags=flag)
        assert np.array_equal(est1.grad.cpu().numpy().reshape(-1, L), grad1)
        assert [terms1[i] for i in range(3)] == [float(comp) if flag == b else 0.0 for b in (1, 2, 4)] and terms1[3] == float(comp)
    neg = loss.SISNRLoss(return_neg=True)(_t(e), _t(t))
    assert torch.equal(neg, -s)
    with torch.no_grad():  # nothing asks for a gradient: forward only, the same values
        assert torch.equal(loss.RecipeLoss()(_t(e), _t(t))[0], total.detach())


def test_repeated_calls_and_a_side_stream_are_bit_identical():
    e, t, _ = _case("r2_L5000")
    a = _c_call(_t(e), _t(t))
    b = _c_call(_t(e), _t(t))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    c = _c_call(_t(e), _t(t), stream=side)
    for other in (b, c):
        assert np.array_equal(a[0], other[0]) and np.array_equal(a[1], other[1])


def test_backward_scales_the_stored_gradient():
    from spiking_fullsubnet_amd import loss
    e, t, _ = _case("r2_L4096")
    _, grad = _c_call(_t(e), _t(t))
    est = _t(e).requires_grad_(True)
    (2.5 * loss.RecipeLoss()(est, _t(t))[0]).backward()
    assert np.array_equal(est.grad.cpu().numpy(), (np.float32(2.5) * grad).astype(np.float32))


def test_non_contiguous_and_offset_views_are_copied_not_misread():
    from spiking_fullsubnet_amd import loss
    e, t, _ = _case("r2_L4096")
    want = loss.RecipeLoss()(_t(e), _t(t))[0]
    wide_e, wide_t = torch.zeros(2, 4096 + 3, device=DEV), torch.zeros(2, 4096 + 3, device=DEV)
    wide_e[:, 3:], wide_t[:, 3:] = _t(e), _t(t)
    assert torch.equal(loss.RecipeLoss()(wide_e[:, 3:], wide_t[:, 3:])[0], want)


def test_training_step_with_the_recipe_loss_replayed_from_a_hip_graph_equals_the_eager_step():
    """training.GraphedTrainStep unchanged, with loss_fn closing over a static clean tensor: the replayed loss and every parameter
    gradient are bit-identical to the eager step from the same state."""
    import spiking_fullsubnet_amd as pkg
    from spiking_fullsubnet_amd import training as tr
    kw = rw.LIVE_TINY
    m = pkg.SpikingFullSubNet(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in rw.live_state_dict(kw, 11).items()}, strict=True)
    m = m.to(DEV).train()
    waves = [_t(rw.synth_wave(4, 24, seed=s)) for s in (1, 2, 3)]
    n_out = m(waves[0])[0].shape[-1]  # (moves the BatchNorm buffers: the state both sides start from is taken after it)
    state0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    clean = (0.5 * _t(rw.synth_wave(4, 24, seed=7)))[..., :n_out].contiguous()
    assert clean.shape[-1] == n_out > 1024
    recipe = pkg.RecipeLoss()
    loss_fn = lambda out: recipe(out[0], clean)[0]

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


def test_cross_check_against_the_aten_composite_on_the_device():
    """The reference's three functions restated with torch.stft, on the device in fp32: both sides are fp32 evaluations of the same
    formulas, so the loss values differ by at most the sum of both sides' bounds.  A cross-check, not the yardstick."""
    e, t, ref = _case("r2_L5000")
    terms, _ = _c_call(_t(e), _t(t))
    w = torch.hann_window(2048, device=DEV)
    E = torch.stft(_t(e), n_fft=2048, hop_length=512, window=w, return_complex=True)
    T = torch.stft(_t(t), n_fft=2048, hop_length=512, window=w, return_complex=True)
    freq = (E.real - T.real).abs().mean() + (E.imag - T.imag).abs().mean()
    mag = (E.abs() - T.abs()).abs().mean()
    a, b = _t(e), _t(t)
    eps = torch.finfo(torch.float32).eps
    a, b = a - a.mean(-1, keepdim=True), b - b.mean(-1, keepdim=True)
    proj = (b * a).sum(-1, keepdim=True) * b / (b * b).sum(-1, keepdim=True)
    sisnr = (10 * torch.log10((proj ** 2).sum(-1) / (((a - proj) ** 2).sum(-1) + eps) + eps)).mean()
    for k, ours, aten in (("freq", terms[0], freq), ("mag", terms[1], mag), ("sisnr", terms[2], sisnr)):
        d = abs(float(ours) - float(aten))
        print(k, float(ours), float(aten), "difference / (2 bound):", d / (2 * ref["tol"][k]))
        assert d <= 2 * ref["tol"][k], k
