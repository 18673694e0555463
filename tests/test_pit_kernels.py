"""The permutation-invariant SI-SDR loss on the device (sfsn_pit_sdr and spiking_fullsubnet_amd.pit) against the fp64 restatement and
the derived bounds of tests/pitref.py: every case of its table with zero_mean on and off through the C ABI (PIT mode, forward only,
pairwise mode; outputs pre-filled with NaN), the Python drop-ins bit for bit against the C call, the autograd plumbing, determinism,
views, one cross-check against the ATen restatement on the device, and a whole two-speaker training step replayed from a HIP graph."""
import ctypes

import numpy as np
import pytest
import torch

import pitref
import refweights as rw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = [c[0] for c in pitref.CASES]
ZM = [True, False]
_refs = {}


def _case(name, zm):
    """(est, ref, cotangent, fp64 reference) of a case, computed once and shared (never modified)."""
    if (name, zm) not in _refs:
        e, t = pitref.make_inputs(name)
        w = pitref.cotangent(name)
        _refs[name, zm] = (e, t, w, pitref.reference(e, t, zm, cot=w))
    return _refs[name, zm]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _c_call(e, t, zm=True, eps=pitref.EPS, cot=None, want_grad=True, want_reordered=True, stream=None):
    """sfsn_pit_sdr through ctypes on [B, S, L] device tensors -> dict of numpy results (None where not asked for).  Every output is
    pre-filled with NaN (perm with -1), so an element the kernel does not write fails the comparison."""
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    B, S, n = e.shape
    st = torch.cuda.current_stream() if stream is None else stream
    pit_mode = cot is None
    with torch.cuda.stream(st):
        pair = torch.full((B, S, S), float("nan"), device=DEV)
        perm = torch.full((B, S), -1, dtype=torch.int32, device=DEV) if pit_mode else None
        loss = torch.full((1,), float("nan"), device=DEV) if pit_mode else None
        grad = torch.full_like(e, float("nan")) if want_grad else None
        reordered = torch.full_like(e, float("nan")) if pit_mode and want_reordered else None
        scratch = torch.empty(L.sfsn_pit_sdr_scratch_bytes(B, S, n), dtype=torch.uint8, device=DEV)
        ptr = lambda x: x.data_ptr() if x is not None else None
        _lib.check(L.sfsn_pit_sdr(e.data_ptr(), t.data_ptr(), B, S, n, int(zm), eps, ptr(cot), pair.data_ptr(), ptr(perm), ptr(loss),
                                  ptr(grad), ptr(reordered), scratch.data_ptr(), ctypes.c_void_p(st.cuda_stream)), "sfsn_pit_sdr")
    st.synchronize()
    host = lambda x: x.cpu().numpy() if x is not None else None
    return dict(pair=host(pair), perm=host(perm), loss=(host(loss)[0] if pit_mode else None), grad=host(grad), reordered=host(reordered))


@pytest.mark.parametrize("zm", ZM)
@pytest.mark.parametrize("name", NAMES)
def test_c_abi_pit_mode_within_the_derived_bounds(name, zm):
    e, t, w, ref = _case(name, zm)
    got = _c_call(_t(e), _t(t), zm)
    bad, used = pitref.outside(got, ref)  # pair, loss, grad within bounds; perm equal as integers; reordered bit-equal to the gather
    print(name, zm, "share of each bound used:", used, "perm", got["perm"].tolist())
    assert not bad, (bad, used)
    fwd = _c_call(_t(e), _t(t), zm, want_grad=False)  # forward only: the same bits
    assert fwd["grad"] is None
    for k in ("pair", "perm", "loss", "reordered"):
        assert np.array_equal(fwd[k], got[k]), k
    bare = _c_call(_t(e), _t(t), zm, want_grad=False, want_reordered=False)  # neither chunked output: the last workgroup alone
    for k in ("pair", "perm", "loss"):
        assert np.array_equal(bare[k], got[k]), k


@pytest.mark.parametrize("zm", ZM)
@pytest.mark.parametrize("name", NAMES)
def test_c_abi_pairwise_mode_within_the_derived_bounds(name, zm):
    e, t, w, ref = _case(name, zm)
    got = _c_call(_t(e), _t(t), zm, cot=_t(w))
    bad, used = pitref.outside(dict(pair=got["pair"], grad_pw=got["grad"]), ref)
    print(name, zm, "share of each bound used:", used)
    assert not bad, (bad, used)
    assert np.array_equal(got["pair"], _c_call(_t(e), _t(t), zm, want_grad=False)["pair"])  # the bits of PIT mode's pair
    assert np.array_equal(got["pair"], _c_call(_t(e), _t(t), zm, cot=_t(w), want_grad=False)["pair"])


@pytest.mark.parametrize("name,zm", [("b3s2_L1000", True), ("b2s3_L4097", False), ("b5s4_L777", True), ("b2s2_L9000_tie", True)])
def test_python_drop_ins_return_the_bits_of_the_c_call(name, zm):
    from spiking_fullsubnet_amd import pit
    e, t, w, ref = _case(name, zm)
    c = _c_call(_t(e), _t(t), zm)
    wrapper = pit.PITWrapper(pit.PairwiseNegSDR(zero_mean=zm))
    est = _t(e).requires_grad_(True)
    loss, reordered = wrapper(est, _t(t))
    assert loss.shape == () and float(loss) == float(c["loss"]) and np.array_equal(reordered.cpu().numpy(), c["reordered"])
    assert loss.requires_grad and not reordered.requires_grad
    loss.backward()
    assert np.array_equal(est.grad.cpu().numpy(), c["grad"])
    l2, r2, perm, pair = wrapper.full(_t(e), _t(t))  # nothing asks for a gradient: forward only, the same values
    assert torch.equal(l2, loss.detach()) and torch.equal(r2, reordered)
    assert perm.dtype == torch.int64 and np.array_equal(perm.cpu().numpy(), c["perm"]) and np.array_equal(pair.cpu().numpy(), c["pair"])
    # the torch helpers on the kernel's own pair: the same choice and the same rows
    min_loss, idx = wrapper.find_best_perm(pair)
    assert torch.equal(idx, perm) and torch.equal(wrapper.reorder_source(_t(e), idx), reordered)
    # PairwiseNegSDR alone, backpropagated through a weighted sum: a second kernel call in pairwise mode
    est2 = _t(e).requires_grad_(True)
    pw = pit.PairwiseNegSDR(zero_mean=zm)(est2, _t(t))
    assert np.array_equal(pw.detach().cpu().numpy(), c["pair"])
    (pw * _t(w)).sum().backward()
    assert np.array_equal(est2.grad.cpu().numpy(), _c_call(_t(e), _t(t), zm, cot=_t(w))["grad"])


def test_backward_scales_the_stored_gradient_and_reordered_carries_none():
    from spiking_fullsubnet_amd import pit
    e, t, _, _ = _case("b3s2_L1000", True)
    c = _c_call(_t(e), _t(t))
    wrapper = pit.PITWrapper(pit.PairwiseNegSDR())
    est = _t(e).requires_grad_(True)
    loss, reordered = wrapper(est, _t(t))
    (2.5 * loss).backward()
    assert np.array_equal(est.grad.cpu().numpy(), (np.float32(2.5) * c["grad"]).astype(np.float32))
    with pytest.raises(RuntimeError, match="does not require grad"):  # a loss built on `reordered` raises, it does not lose the gradient
        reordered.sum().backward()


def test_repeated_calls_and_a_side_stream_are_bit_identical():
    e, t, _, _ = _case("b2s2_L9000_tie", True)
    a = _c_call(_t(e), _t(t))
    b = _c_call(_t(e), _t(t))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    c = _c_call(_t(e), _t(t), stream=side)
    for other in (b, c):
        for k in ("pair", "perm", "loss", "grad", "reordered"):
            assert np.array_equal(a[k], other[k]), k


def test_non_contiguous_and_offset_views_are_copied_not_misread():
    from spiking_fullsubnet_amd import pit
    e, t, _, _ = _case("b3s2_L1000", True)
    wrapper = pit.PITWrapper(pit.PairwiseNegSDR())
    want = wrapper.full(_t(e), _t(t))
    wide_e, wide_t = torch.zeros(3, 2, 1003, device=DEV), torch.zeros(3, 2, 1003, device=DEV)
    wide_e[:, :, 3:], wide_t[:, :, 3:] = _t(e), _t(t)
    for a, b in zip(wrapper.full(wide_e[:, :, 3:], wide_t[:, :, 3:]), want):
        assert torch.equal(a, b)
    swapped_e, swapped_t = _t(e).transpose(0, 1).contiguous().transpose(0, 1), _t(t).transpose(0, 1).contiguous().transpose(0, 1)
    assert not swapped_e.is_contiguous()
    for a, b in zip(wrapper.full(swapped_e, swapped_t), want):
        assert torch.equal(a, b)
    flat = torch.zeros(3 * 2 * 1000 + 1, device=DEV)  # a base that is 4 bytes past a 16-byte boundary
    flat[1:] = _t(e).reshape(-1)
    for a, b in zip(wrapper.full(flat[1:].view(3, 2, 1000), _t(t)), want):
        assert torch.equal(a, b)


def test_cross_check_against_the_aten_restatement_on_the_device():
    """audiozen/pit.py's formulas restated in ATen, on the device in fp32: both sides are fp32 evaluations of the same formulas, so they
    differ by at most the sum of both sides' bounds.  A cross-check, not the yardstick."""
    name, zm = "b2s3_L4097", True
    e, t, _, ref = _case(name, zm)
    got = _c_call(_t(e), _t(t), zm)
    est, tgt = _t(e).requires_grad_(True), _t(t)
    a, r = est - est.mean(2, keepdim=True), tgt - tgt.mean(2, keepdim=True)
    a, r = a.unsqueeze(2), r.unsqueeze(1)
    dot = (a * r).sum(3, keepdim=True)
    proj = dot * r / ((r ** 2).sum(3, keepdim=True) + pitref.EPS)
    pair = -10 * torch.log10((proj ** 2).sum(3) / (((a - proj) ** 2).sum(3) + pitref.EPS) + pitref.EPS)
    perms = torch.tensor(pitref.all_perms(3), device=DEV)
    loss_p = pair[:, perms, torch.arange(3, device=DEV)].sum(-1) / 3
    loss = loss_p.min(1).values.mean()
    loss.backward()
    d_pair = np.abs(pair.detach().cpu().numpy() - got["pair"]) / (2 * ref["pair_tol"])
    d_grad = np.abs(est.grad.cpu().numpy() - got["grad"]) / (2 * ref["grad_tol"])
    print("difference / (2 bound): pair", d_pair.max(), "loss", abs(float(loss) - got["loss"]) / (2 * ref["loss_tol"]), "grad", d_grad.max())
    assert d_pair.max() <= 1.0 and abs(float(loss) - float(got["loss"])) <= 2 * ref["loss_tol"] and d_grad.max() <= 1.0
    assert np.array_equal(perms[loss_p.argmin(1)].cpu().numpy(), got["perm"])


def test_training_step_with_the_pit_loss_replayed_from_a_hip_graph_equals_the_eager_step():
    """training.GraphedTrainStep unchanged, with loss_fn closing over a static reference tensor: the replayed loss and every parameter
    gradient of the two-speaker model are bit-identical to the eager step from the same state."""
    import spiking_fullsubnet_amd as pkg
    from spiking_fullsubnet_amd import training as tr
    kw = rw.LIVE_TINY_2SPK
    m = pkg.SpikingFullSubNet(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in rw.live_state_dict(kw, 12).items()}, strict=True)
    m = m.to(DEV).train()
    waves = [_t(rw.synth_wave(3, 24, seed=s)) for s in (1, 2, 3)]
    B, S, n_out = m(waves[0])[0].shape  # (moves the BatchNorm buffers: the state both sides start from is taken after it; no tensor of this step is kept)
    assert (B, S) == (3, 2)
    state0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ref_static = torch.stack([0.5 * _t(rw.synth_wave(3, 24, seed=s))[..., :n_out] for s in (8, 7)], dim=1).contiguous()
    assert ref_static.shape == (B, S, n_out)
    wrapper = pkg.PITWrapper(pkg.PairwiseNegSDR())
    loss_fn = lambda out: wrapper(out[0], ref_static)[0]

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
