"""Training the cIRM-GSN model (modeling_cirm_gsn.Model in train() mode / with gradients): the two deep-filter kernels against their
fp64 reference under derived bounds, the whole model against one training step of the REFERENCE (tests/golden/cirm_*_train.npz and
cirm_tiny_evalgrad.npz, made by tests/golden/make_golden_cirm_train.py), the HIP deep filter against the torch one, the padded stack
through GSNStackTrainFn, the hand-over to the inference kernels and the graphed step."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import cirm_train_cases as cases
import frontback as fbk
from test_cirm_gsn_training_host import df_backward_reference, df_forward_reference, df_inputs
from test_training import _close, chunked_stacks  # noqa: F401  (the tolerances and the chunk settings of the live model's tests)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _model(name):
    from spiking_fullsubnet_amd.modeling_cirm_gsn import Model
    kw, seed, B, T, mode = cases.CASES[name]
    g = cases.load_fixture(GOLD, name)
    m = cases.build_model(Model, kw, seed)
    assert cases.state_checksum(m) == str(g["checksum"])
    return m.to(DEV), g, kw


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ---- 5. / 6. the kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,S,df", [(257, 1, 3), (257, 2, 3), (257, 1, 1), (257, 4, 5), (129, 2, 2)])
@pytest.mark.parametrize("T", [1, 2, 37, 130])
@pytest.mark.parametrize("B", [1, 3])
def test_deepfilter_kernels_against_the_fp64_reference(F, S, df, T, B):
    from spiking_fullsubnet_amd import _lib as L
    lib = L.lib()
    spec, coef, g = df_inputs(1000 * F + 100 * S + 10 * df + T + B, B, F, T, S, df)
    ri = torch.view_as_real(_t(spec)).contiguous()
    enh = torch.full((B, S, F, T, 2), float("nan"), device=DEV)
    assert lib.sfsn_fullband_deepfilter_fwd(_p(ri), _p(_t(coef)), B, F, T, S, df, _p(enh), None) == 0
    d_coef = torch.full((T, B, 2 * df * S * F), float("nan"), device=DEV)
    assert lib.sfsn_fullband_deepfilter_bwd(_p(ri), _p(_t(g)), B, F, T, S, df, _p(d_coef), None) == 0
    torch.cuda.synchronize()
    y, tol = df_forward_reference(spec, coef, S, df)
    w, vac = fbk.worst(enh.cpu().numpy(), y, tol), fbk.vacuous_share(tol, y)
    dref, dtol = df_backward_reference(spec, g, S, df)
    wb, vacb = fbk.worst(d_coef.cpu().numpy(), dref, dtol), fbk.vacuous_share(dtol, dref)
    print(f"deepfilter F={F} S={S} df={df} T={T} B={B}: forward worst {w:.3f} of the bound (vacuous {vac:.3g}), backward {wb:.3f} ({vacb:.3g})")
    assert w <= 1.0 and wb <= 1.0
    assert vac == 0.0 and vacb == 0.0


def test_deepfilter_kernels_check_their_arguments():
    from spiking_fullsubnet_amd import _lib as L
    lib = L.lib()
    B, F, T, S, df = 1, 257, 16, 1, 3
    ri, coef = torch.zeros((B, F, T, 2), device=DEV), torch.zeros((T, B, 2 * df * S * F), device=DEV)
    n = T * 5 * 2 * 17 * 321  # room for every refused geometry, should a check be missing
    big, big_out = torch.zeros((n,), device=DEV), torch.zeros((n,), device=DEV)
    for fn in (lib.sfsn_fullband_deepfilter_fwd, lib.sfsn_fullband_deepfilter_bwd):
        call = lambda a=_p(ri), b=_p(big), o=_p(big_out), F_=F, S_=S, df_=df, T_=T: fn(a, b, B, F_, T_, S_, df_, o, None)
        assert call() == L.SFSN_OK
        assert call(a=None) == L.SFSN_EINVAL and call(b=None) == L.SFSN_EINVAL and call(o=None) == L.SFSN_EINVAL
        assert call(T_=0) == L.SFSN_EINVAL
        assert call(a=ctypes.c_void_p(ri.data_ptr() + 4)) == L.SFSN_EINVAL  # (complex rows are read as float2)
        assert call(F_=321) == L.SFSN_EUNSUPPORTED and call(S_=5) == L.SFSN_EUNSUPPORTED and call(df_=17) == L.SFSN_EUNSUPPORTED
    torch.cuda.synchronize()


# ---- 7. / 8. one training step against the reference's ------------------------------------------------------------------------------------
def _unpack(g, key, l):
    shape = tuple(int(v) for v in g[f"spikes_shape/{l}"])
    return np.unpackbits(g[f"{key}/{l}"])[:int(np.prod(shape))].reshape(shape)


def _forward_with_layers(m, wave):
    """m(wave) and the layer list [x_norm, S1, ..., SL, proj] (returned by the model itself for several speakers only: tapped where
    the model builds it)."""
    from spiking_fullsubnet_amd import training
    seen = {}
    orig = training._cirm_sequence_model

    def tap(seq, x, tr):
        coef, layers = orig(seq, x, tr)
        seen["layers"] = layers
        return coef, layers

    training._cirm_sequence_model = tap
    try:
        out = m(wave)
    finally:
        training._cirm_sequence_model = orig
    return out, seen["layers"]


def _run_case(name):
    """One step against the fixture: outputs, loss, gradients, buffers; the causal rule of
    test_training.test_gsn_stack_training_forward_and_backward_match_the_reference where the fixture allows near-threshold membranes
    (the recipe case)."""
    from spiking_fullsubnet_amd import training
    m, g, kw = _model(name)
    S, H, L_, recipe = kw["num_spks"], kw["hidden_size"], kw["num_layers"], kw["hidden_size"] > 64
    mode = str(g["mode"])
    m.train() if mode == "train" else m.eval()
    wave = _t(g["wave"])
    if mode == "evalgrad":
        wave.requires_grad_(True)
    before = {k: b.detach().clone() for k, b in m.named_buffers()}
    out, layers = _forward_with_layers(m, wave)
    if S > 1:
        assert isinstance(out[1], list) and len(out[1]) == 1 and out[1][0] is layers
    assert len(layers) == L_ + 2
    T, B = layers[0].shape[0], layers[0].shape[1]
    rows = 4 if recipe else T
    _close(layers[0][:rows].detach().cpu().numpy(), g["x"], f"{name}: x_norm", rtol=1e-4, atol_frac=1e-5)
    flipped = False
    for l in range(L_):
        got = layers[1 + l].detach().cpu().numpy()
        ref = _unpack(g, "spikes_packed", l).astype(np.float32)
        assert got.shape == ref.shape == (T, B, H)
        d = got != ref
        if d.any() and recipe and not flipped:
            near = _unpack(g, f"near{cases.TAU:g}", l).astype(bool)
            t0 = int(np.nonzero(d.any(axis=(1, 2)))[0][0])
            assert near[t0][d[t0]].all(), f"{name} layer {l}: first disagreement at frame {t0} on a neuron outside the don't-care band"
            print(f"{name} layer {l}: exact up to frame {t0} of {T}; {int(d[t0].sum())} near-threshold flip(s) there, {int(d.sum())} in all")
            flipped = True
        elif not flipped:
            assert not d.any(), f"{name} layer {l}: {int(d.sum())} spikes differ from the reference's"
    print(f"{name}: {'a near-threshold flip was accepted' if flipped else 'every spike equals the reference'}")

    def close(a, b, nm, **tol):
        if not flipped:
            return _close(a, b, nm, **tol)
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        err = np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)
        assert err < 2e-2, f"{nm}: relative L2 error {err:.3g} after an accepted near-threshold flip"

    close(layers[-1][:rows].detach().cpu().numpy(), g["proj"], f"{name}: proj", rtol=1e-4, atol_frac=1e-5)
    enh_y = out[0]
    close(enh_y.detach().cpu().numpy(), g["enh_y"], f"{name}: enh_y", rtol=1e-3, atol_frac=1e-4)
    if S == 1:
        close(out[1].detach().cpu().numpy(), g["enh_mag"], f"{name}: enh_mag", rtol=1e-4, atol_frac=1e-5)
    loss = cases.loss_of(out, S)
    if not flipped:
        assert float(loss) == pytest.approx(float(g["loss"]), rel=1e-5)
    loss.backward()
    training.check_pending()
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        close(p.grad.cpu().numpy(), g[f"grad/{k}"], f"{name}: grad {k}")
    if mode == "evalgrad":
        close(wave.grad.cpu().numpy(), g["grad_wave"], f"{name}: grad wave")
    for k, b in m.named_buffers():
        ref = g[f"buf/{k}"]
        assert tuple(b.shape) == ref.shape, k
        if mode == "evalgrad":
            assert torch.equal(b, before[k]), f"{k} changed in eval mode"
        elif k.endswith("num_batches_tracked"):
            assert int(b) == int(ref), k
        else:
            _close(b.cpu().numpy(), ref, f"{name}: buffer {k}", rtol=1e-4 if not flipped else 1e-2, atol_frac=1e-5 if not flipped else 1e-3)
    return m, g, kw


@pytest.mark.parametrize("name", ["cirm_tiny_train", "cirm_tiny_2spk_train", "cirm_tiny_nobn_train", "cirm_tiny_unshared_train"])
def test_tiny_training_step_matches_the_reference(name):
    _run_case(name)


def test_recipe_training_step_matches_the_reference():
    _run_case("cirm_recipe_train")


# ---- 9. the HIP deep filter against deep_filter_torch in the same step ------------------------------------------------------------------
def test_hip_deep_filter_equals_the_torch_one_in_a_recipe_step():
    from spiking_fullsubnet_amd import training
    from spiking_fullsubnet_amd.modeling_cirm_gsn import Model
    kw, seed = cases.RECIPE, 5
    m = cases.build_model(Model, kw, seed).to(DEV).train()
    twin = copy.deepcopy(m)
    wave = cases.make_wave(kw, seed, 8, 40).to(DEV)
    res = []
    for mod, on in ((m, True), (twin, False)):
        old = training.TRAIN_FULLBAND_DF
        training.TRAIN_FULLBAND_DF = on
        try:
            (y, mag), layers = _forward_with_layers(mod, wave)
            loss = cases.loss_of((y, mag), 1)
            loss.backward()
            training.check_pending()
        finally:
            training.TRAIN_FULLBAND_DF = old
        res.append((y.detach(), mag.detach(), float(loss), layers))
    assert res[0][2] == pytest.approx(res[1][2], rel=1e-6)
    assert _rel(res[0][0], res[1][0]) < 1e-5 and _rel(res[0][1], res[1][1]) < 1e-5
    for l in range(1, kw["num_layers"] + 1):
        assert torch.equal(res[0][3][l], res[1][3][l]), f"layer {l}: spikes differ"
    for (k, p), (_, q) in zip(m.named_parameters(), twin.named_parameters()):
        assert _rel(p.grad, q.grad) < 1e-5, (k, _rel(p.grad, q.grad))
    for (k, a), (_, b) in zip(m.named_buffers(), twin.named_buffers()):
        assert torch.equal(a, b), k  # (the stacks ran on the same numbers: the same spikes and statistics)


# ---- 10. the padded stack through GSNStackTrainFn -----------------------------------------------------------------------------------------
def test_padded_stack_pipelined_equals_the_layer_calls(chunked_stacks):
    from spiking_fullsubnet_amd.modeling_cirm_gsn import Model
    tr = chunked_stacks
    kw, seed = dict(cases.TINY, num_spks=2), 9
    m = cases.build_model(Model, kw, seed).to(DEV).train()
    twin = copy.deepcopy(m)
    wave = cases.make_wave(kw, seed, 4, 24).to(DEV)

    def run(mod, chunks):
        old = tr.STACK_CHUNKS
        tr.STACK_CHUNKS = chunks
        try:
            y, rest = mod(wave)
            y.pow(2).mean().backward()
            tr.check_pending()
        finally:
            tr.STACK_CHUNKS = old
        return rest[0]
    n0 = tr._STACK_CALLS
    la = run(m, 3)
    assert tr._STACK_CALLS == n0 + 1
    lb = run(twin, 1)
    assert tr._STACK_CALLS == n0 + 1
    for l in range(1, kw["num_layers"] + 1):
        assert tuple(la[l].shape) == (24, 4, kw["hidden_size"]) and torch.equal(la[l], lb[l]), l
    for (k, p), (_, q) in zip(m.named_parameters(), twin.named_parameters()):
        assert _rel(p.grad, q.grad) < 1e-5, (k, _rel(p.grad, q.grad))
    for (k, a), (_, b) in zip(m.named_buffers(), twin.named_buffers()):
        assert tuple(a.shape) == tuple(b.shape)
        assert torch.equal(a, b) if k.endswith("num_batches_tracked") else _rel(a.float(), b.float()) < 1e-6, k


# ---- 11. back on the inference kernels after a step -------------------------------------------------------------------------------------
def test_eval_after_a_training_step_runs_the_kernels_with_the_new_statistics():
    from spiking_fullsubnet_amd import training
    m, g, kw = _model("cirm_tiny_train")
    wave = _t(g["wave"])
    m.eval()
    with torch.no_grad():
        y0, mag0 = m(wave)
    n0 = dict(m.engine().launches)
    m.train()
    cases.loss_of(m(wave), 1).backward()
    training.check_pending()
    m.eval()
    with torch.no_grad():
        y1, mag1 = m(wave)
    eng = m.engine()
    assert eng.launches.get("projdf", 0) == 1 and eng.launches.get("features", 0) == 1 and n0.get("projdf", 0) == 1  # (re-packed: a new engine)
    assert torch.isfinite(y1).all() and torch.isfinite(mag1).all() and not torch.equal(y0, y1) and not torch.equal(mag0, mag1)


# ---- 12. eval mode with gradients; the LSTM option ---------------------------------------------------------------------------------------
def test_eval_mode_gradients_match_the_reference():
    m, g, kw = _run_case("cirm_tiny_evalgrad")
    grads = {k: p.grad.clone() for k, p in m.named_parameters()}
    for p in m.parameters():
        p.grad = None
    m.autograd_in_eval = True
    cases.loss_of(m(_t(g["wave"])), 1).backward()
    for k, p in m.named_parameters():
        assert _rel(p.grad, grads[k]) < 1e-5, k


def test_lstm_model_trains_on_the_aten_path():
    from spiking_fullsubnet_amd.modeling_cirm_gsn import Model
    torch.manual_seed(0)
    wave = torch.randn(2, 31 * 128, device=DEV) * 0.1
    m = Model(512, 128, 512, 0.5, 257, 32, 2, 257, "tanh", 3, sequence_model="LSTM", num_spks=1).to(DEV).train()
    y, mag = m(wave)
    assert y.shape == wave.shape and mag.shape == (2, 257, 32)
    (y.pow(2).mean() + mag.mean()).backward()
    m2 = Model(512, 128, 512, 0.5, 257, 32, 2, 257, None, 2, sequence_model="LSTM", num_spks=2).to(DEV).train()
    y2, rest = m2(wave)
    assert y2.shape == (2, 2, wave.shape[1]) and rest == [[]]
    y2.pow(2).mean().backward()
    for mod in (m, m2):
        for k, p in mod.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all() and bool((p.grad != 0).any()), k


# ---- 13. the graphed step ------------------------------------------------------------------------------------------------------------------
def test_graphed_training_step_of_the_cirm_model_equals_the_eager_step(chunked_stacks):
    from spiking_fullsubnet_amd.modeling_cirm_gsn import Model
    tr = chunked_stacks
    kw, seed = cases.TINY, 13
    m = cases.build_model(Model, kw, seed).to(DEV).train()
    waves = [cases.make_wave(kw, seed + s, 4, 24).to(DEV) for s in (1, 2, 3)]
    loss_fn = lambda out: out[0].pow(2).mean() + out[1].mean()
    state0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    eager = []
    for w in waves[1:]:
        for p in m.parameters():
            p.grad = None
        loss = loss_fn(m(w))
        loss.backward()
        eager.append((float(loss), [p.grad.clone() for p in m.parameters()], {k: v.clone() for k, v in m.state_dict().items()}))
        del loss
    with torch.no_grad():
        for k, v in m.state_dict().items():
            v.copy_(state0[k])
    gs = tr.GraphedTrainStep(m, waves[0], loss_fn)
    assert gs.layer_calls_captured >= 2
    for k, v in m.state_dict().items():
        assert torch.equal(v, state0[k]), f"capturing changed {k}"
    for (l_e, g_e, st_e), w in zip(eager, waves[1:]):
        l_g = gs(w)
        assert float(l_g) == l_e
        for (k, p), ge in zip(m.named_parameters(), g_e):
            assert torch.equal(p.grad, ge), f"gradient of {k} differs between the replayed and the eager step"
        for k, v in m.state_dict().items():
            assert torch.equal(v, st_e[k]), f"{k} differs after the replayed step"
    tr.check_pending()


# ---- the eval-mode (folded) BatchNorm path of GSNLayerTrainFn, which every model shares -------------------------------------------------
@pytest.mark.parametrize("shared", [True, False])
def test_eval_mode_layer_call_returns_the_aten_batchnorm_gradients(shared):
    """GSNLayerTrainFn with eval-mode BatchNorm (the live and frozen models in eval() with gradients take it too) now returns the
    gradients of gamma and beta: against the same stack written with ATen operations (F.batch_norm on the running statistics, the
    triangle surrogate) on the device, H a multiple of 16 -- spikes equal, every gradient by test_training._close."""
    import torch.nn.functional as Fn
    import spiking_fullsubnet_amd.modeling_spiking_fullsubnet as M
    from spiking_fullsubnet_amd import training
    from test_cirm_gsn_training_host import _Spike
    torch.manual_seed(3 + shared)
    T, R, I, H, L_ = 20, 6, 10, 32, 2
    stack = M.StackedGSU(I, H, L_, shared, True).to(DEV).eval()
    for layer in stack.layers:
        bn = layer.cell.batchnorm
        bn.weight.data.uniform_(0.5, 1.5)
        bn.bias.data.uniform_(-0.3, 0.3)
        bn.running_mean.uniform_(-0.2, 0.2)
        bn.running_var.uniform_(0.5, 1.5)
    x = torch.randn(T, R, I, device=DEV)
    cot = [torch.randn(T, R, H, device=DEV) for _ in range(L_)]
    before = {k: b.clone() for k, b in stack.named_buffers()}
    xa = x.clone().requires_grad_(True)
    outs = training.gsn_stack(xa, stack, False)
    sum((o * c).sum() for o, c in zip(outs[1:], cot)).backward()
    training.check_pending()
    got = {k: p.grad.clone() for k, p in stack.named_parameters()}
    assert all(g is not None for g in got.values())
    for k, b in stack.named_buffers():
        assert torch.equal(b, before[k]), k
    stack.zero_grad()
    xb = x.clone().requires_grad_(True)
    cur, ref = xb, []
    for layer in stack.layers:
        cell, rep = layer.cell, (2 if shared else 1)
        wi, wh, bn = cell.weight_ih.repeat(rep, 1), cell.weight_hh.repeat(rep, 1), cell.batchnorm
        h = c = torch.zeros(R, H, device=DEV)
        seq = []
        for t in range(T):
            gates = cur[t] @ wi.t() + cell.bias_ih + h @ wh.t()
            f, g = torch.sigmoid(gates[:, :H]), gates[:, H:]
            c = Fn.batch_norm(f * c + (1 - f) * g, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
            h = _Spike.apply(c)
            seq.append(h)
        cur = torch.stack(seq)
        ref.append(cur)
    sum((o * c).sum() for o, c in zip(ref, cot)).backward()
    for l in range(L_):
        assert torch.equal(outs[1 + l], ref[l]), f"layer {l}: {int((outs[1 + l] != ref[l]).sum())} spikes differ"
    _close(xa.grad.cpu().numpy(), xb.grad.cpu().numpy(), "dL/dx")
    for k, p in stack.named_parameters():
        _close(got[k].cpu().numpy(), p.grad.cpu().numpy(), f"grad {k}")
