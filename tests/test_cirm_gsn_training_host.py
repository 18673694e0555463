"""cIRM-GSN training, host-side checks (no GPU): the differentiable padding of a GSN stack against fullband_engine.pad_cell and against
a plain-torch cell loop in training mode, the fp64 reference of sfsn_fullband_deepfilter_fwd / _bwd that the GPU tests use
(df_forward_reference / df_backward_reference below) against the existing references and torch autograd, and the committed training fixtures."""
import json
import os

import numpy as np
import pytest
import torch

import cirm_train_cases as cases
import frontback as fbk
from spiking_fullsubnet_amd import training
from spiking_fullsubnet_amd.fullband_engine import ceil16, pad_cell
from spiking_fullsubnet_amd.modeling_cirm_gsn import Model, deep_filter_torch
from spiking_fullsubnet_amd.modeling_spiking_fullsubnet import StackedGSU

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- the fp64 reference of the two kernels (imported by tests/test_cirm_gsn_training.py) ----------------------------------------------
def df_forward_reference(spec, coef, S, df, mut=None):
    """spec complex [B, F, T], coef [T, B, 2 df S F] (channel ((c df + d) S + s) F + f) -> (Y [B, S, F, T, 2] in fp64, the bound
    gamma(2 df + 2) sum_d (|xr cr| + |xi ci|) resp. (|xr ci| + |xi cr|) of an fp32 evaluation in any order)."""
    B, F, T = spec.shape
    c = np.asarray(coef, np.float64).reshape(T, B, 2, df, S, F).transpose(1, 2, 3, 4, 5, 0)  # [B, c, d, S, F, T]
    if mut == "swap_reim":
        c = c[:, ::-1]
    if mut == "taps_desc":
        c = c[:, :, ::-1]
    X = np.stack([spec.real, spec.imag], -1).astype(np.float64)  # [B, F, T, 2]
    y, tol = np.zeros((B, S, F, T, 2)), np.zeros((B, S, F, T, 2))
    for d in range(df):
        sh = df - 1 - d
        xs = np.zeros_like(X)
        if sh < T:
            xs[:, :, sh:] = X[:, :, :T - sh]
        if mut == "hist_nonzero" and sh:
            xs[:, :, :min(sh, T)] = X[:, :, :1]
        xr, xi = xs[:, None, :, :, 0], xs[:, None, :, :, 1]
        cr, ci = c[:, 0, d], c[:, 1, d]
        y[..., 0] += xr * cr - xi * ci
        y[..., 1] += xr * ci + xi * cr
        tol[..., 0] += np.abs(xr * cr) + np.abs(xi * ci)
        tol[..., 1] += np.abs(xr * ci) + np.abs(xi * cr)
    return y, fbk.gamma(2 * df + 2) * tol


def df_backward_reference(spec, g, S, df, mut=None):
    """spec complex [B, F, T], g [B, S, F, T, 2] -> (d_coef [T, B, 2 df S F] in fp64, the bound gamma(3) (|xr gr| + |xi gi|) resp.
    gamma(3) (|xr gi| + |xi gr|))."""
    B, F, T = spec.shape
    X = np.stack([spec.real, spec.imag], -1).astype(np.float64)
    g = np.asarray(g, np.float64)
    gr, gi = g[..., 0], g[..., 1]  # [B, S, F, T]
    out, tol = np.zeros((B, 2, df, S, F, T)), np.zeros((B, 2, df, S, F, T))
    for d in range(df):
        sh = df - 1 - d
        xs = np.zeros_like(X)
        if sh < T:
            xs[:, :, sh:] = X[:, :, :T - sh]
        if mut == "hist_nonzero" and sh:
            xs[:, :, :min(sh, T)] = X[:, :, :1]
        xr, xi = xs[:, None, :, :, 0], xs[:, None, :, :, 1]
        dd = df - 1 - d if mut == "taps_desc" else d
        re, im = xr * gr + xi * gi, xr * gi - xi * gr
        if mut == "sign_flip":
            im = xr * gi + xi * gr
        if mut == "swap_reim":
            re, im = im, re
        out[:, 0, dd], out[:, 1, dd] = re, im
        tol[:, 0, dd], tol[:, 1, dd] = np.abs(xr * gr) + np.abs(xi * gi), np.abs(xr * gi) + np.abs(xi * gr)
    to_tbp = lambda a: np.ascontiguousarray(a.transpose(5, 0, 1, 2, 3, 4)).reshape(T, B, 2 * df * S * F)
    return to_tbp(out), fbk.gamma(3) * to_tbp(tol)


def df_inputs(seed, B, F, T, S, df):
    """N(0, 0.5^2) spectrum, N(0, 1) coefficients and cotangent, all exactly representable in fp32."""
    rng = np.random.default_rng(seed)
    spec = ((rng.standard_normal((B, F, T)) + 1j * rng.standard_normal((B, F, T))) * 0.5).astype(np.complex64)
    coef = rng.standard_normal((T, B, 2 * df * S * F)).astype(np.float32)
    g = rng.standard_normal((B, S, F, T, 2)).astype(np.float32)
    return spec, coef, g


def fp32_forward(spec, coef, S, df):
    """The kernel's arithmetic restated in numpy fp32 (taps ascending, products rounded one by one)."""
    B, F, T = spec.shape
    f32 = np.float32
    c = coef.reshape(T, B, 2, df, S, F).transpose(1, 2, 3, 4, 5, 0)
    X = np.stack([spec.real, spec.imag], -1).astype(f32)
    y = np.zeros((B, S, F, T, 2), f32)
    for d in range(df):
        sh = df - 1 - d
        xs = np.zeros_like(X)
        if sh < T:
            xs[:, :, sh:] = X[:, :, :T - sh]
        xr, xi = xs[:, None, :, :, 0], xs[:, None, :, :, 1]
        y[..., 0] += (xr * c[:, 0, d]).astype(f32) - (xi * c[:, 1, d]).astype(f32)
        y[..., 1] += (xr * c[:, 1, d]).astype(f32) + (xi * c[:, 0, d]).astype(f32)
    return y


# ---- 1. the padding helper ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hp", [(20, 32), (268, 272), (32, 32)])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("bn", [True, False])
def test_pad_cell_tensors_equal_pad_cell_and_pass_the_gradient_slice(H, Hp, shared, bn):
    assert ceil16(H) == Hp == training.ceil16(H)
    g = torch.Generator().manual_seed(H + 2 * shared + bn)
    G = 1 if shared else 2
    # H = 20: a layer >= 1 (its inputs are the padded spikes of the layer below); the others: layer 0 (feature rows, never padded)
    I, in_pad = {20: (20, 32), 268: (257, 257), 32: (7, 7)}[H]
    leaf = lambda *s: torch.randn(*s, generator=g).requires_grad_(True)
    w_ih, w_hh, bias = leaf(G * H, I), leaf(G * H, H), leaf(2 * H)
    bw, bb = (leaf(H), leaf(H)) if bn else (None, None)
    wi, wh, b, a, be = training.pad_cell_tensors(w_ih, w_hh, bias, bw, bb, H, Hp, in_pad, shared)
    n = lambda t: None if t is None else t.detach().numpy()
    rwi, rwh, rb, ra, rbe = pad_cell(n(w_ih), n(w_hh), n(bias), n(bw), n(bb), H, Hp, in_pad, shared)
    assert np.array_equal(n(wi), rwi) and np.array_equal(n(wh), rwh) and np.array_equal(n(b), rb)
    if bn:
        assert np.array_equal(n(a), ra) and np.array_equal(n(be), rbe)
    else:
        assert a is None and be is None and (ra == 1).all() and (rbe == 0).all()
    if H == Hp:
        assert wi is w_ih and wh is w_hh and b is bias
        return
    outs = [wi, wh, b] + ([a, be] if bn else [])
    cots = [torch.randn(o.shape, generator=g) for o in outs]
    sum((o * c).sum() for o, c in zip(outs, cots)).backward()
    for gate in range(G):
        assert torch.equal(w_ih.grad[gate * H:(gate + 1) * H], cots[0][gate * Hp:gate * Hp + H, :I])
        assert torch.equal(w_hh.grad[gate * H:(gate + 1) * H], cots[1][gate * Hp:gate * Hp + H, :H])
    assert torch.equal(bias.grad, torch.cat([cots[2][:H], cots[2][Hp:Hp + H]]))
    if bn:
        assert torch.equal(bw.grad, cots[3][:H]) and torch.equal(bb.grad, cots[4][:H])


def test_padded_stack_shim_and_its_limits():
    torch.manual_seed(0)
    st = StackedGSU(7, 20, 2, True, True).train()
    p = training.PaddedStack(st)
    assert (p.H, p.Hp) == (20, 32) and len(p.layers) == 2
    c0, c1 = p.layers[0].cell, p.layers[1].cell
    assert tuple(c0.weight_ih.shape) == (32, 7) and tuple(c1.weight_ih.shape) == (32, 32) and tuple(c1.weight_hh.shape) == (32, 32)
    bn = c1.batchnorm
    assert bn.num_batches_tracked is st.layers[1].cell.batchnorm.num_batches_tracked
    assert (bn.running_mean[20:] == 0).all() and (bn.running_var[20:] == 1).all() and bn.momentum == 0.1 and bn.eps == 1e-5
    bn.running_mean[:] = 3.0  # what the kernels do in place; commit() hands the first H entries back
    p.commit()
    assert tuple(st.layers[1].cell.batchnorm.running_mean.shape) == (20,) and (st.layers[1].cell.batchnorm.running_mean == 3).all()
    with pytest.raises(NotImplementedError, match="register-resident"):
        training.PaddedStack(StackedGSU(7, 330, 1, True, False))


# ---- 2. a plain-torch cell loop in training mode on the padded tensors ------------------------------------------------------------------
class _Spike(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u):
        ctx.save_for_backward(u)
        return (u >= 0).to(u.dtype)

    @staticmethod
    def backward(ctx, g):
        u, = ctx.saved_tensors
        return g * (1 - u.abs()).clamp(min=0)


def _cell_loop(x, stack, stats):
    """StackedGSU.forward in training mode from the cell's formula: gates = x W_ih^T + b + h W_hh^T, f = sigmoid, c = f c + (1 - f) g,
    c = BatchNorm(c) on the batch statistics (running statistics updated in `stats`), h = spike(c)."""
    outs, cur = [], x
    for l, layer in enumerate(stack.layers):
        cell = layer.cell
        rep = 2 if cell.shared_weights else 1
        wi, wh = cell.weight_ih.repeat(rep, 1), cell.weight_hh.repeat(rep, 1)
        n = cell.weight_hh.shape[1]
        h = c = torch.zeros(x.shape[1], n, dtype=x.dtype)
        seq = []
        for t in range(x.shape[0]):
            gates = cur[t] @ wi.t() + cell.bias_ih + h @ wh.t()
            f, g = torch.sigmoid(gates[:, :n]), gates[:, n:]
            c = f * c + (1 - f) * g
            if cell.use_bn:
                bn = cell.batchnorm
                mean, var = c.mean(0), c.var(0, unbiased=False)
                with torch.no_grad():
                    stats[l][0].mul_(0.9).add_(0.1 * mean)
                    stats[l][1].mul_(0.9).add_(0.1 * c.var(0, unbiased=True))
                c = (c - mean) / torch.sqrt(var + bn.eps) * bn.weight + bn.bias
            h = _Spike.apply(c)
            seq.append(h)
        cur = torch.stack(seq)
        outs.append(cur)
    return outs


@pytest.mark.parametrize("H,shared,bn", [(20, True, True), (20, False, True), (20, True, False), (268, True, True)])
def test_cell_loop_on_padded_tensors_equals_the_unpadded_loop(H, shared, bn):
    torch.manual_seed(H + shared + 2 * bn)
    T, R, I, L = 12, 5, 9, 2
    st = StackedGSU(I, H, L, shared, bn).double().train()
    if bn:
        for layer in st.layers:
            layer.cell.batchnorm.weight.data.uniform_(0.5, 1.5)
            layer.cell.batchnorm.bias.data.uniform_(-0.3, 0.3)
    x = torch.randn(T, R, I, dtype=torch.float64)
    cot = [torch.randn(T, R, H, dtype=torch.float64) for _ in range(L)]
    stats = [[layer.cell.batchnorm.running_mean.clone(), layer.cell.batchnorm.running_var.clone()] if bn else None for layer in st.layers]
    ref = _cell_loop(x, st, stats)
    sum((o * c).sum() for o, c in zip(ref, cot)).backward()
    ref_grads = {k: p.grad.clone() for k, p in st.named_parameters()}
    st.zero_grad()
    padded = training.PaddedStack(st)
    Hp = padded.Hp
    pstats = [[layer.cell.batchnorm.running_mean, layer.cell.batchnorm.running_var] if bn else None for layer in padded.layers]
    got = _cell_loop(x, padded, pstats)
    sum((o[:, :, :H] * c).sum() for o, c in zip(got, cot)).backward()
    for l in range(L):
        assert tuple(got[l].shape) == (T, R, Hp)
        assert torch.equal(got[l][:, :, :H], ref[l]), f"layer {l}: spikes of the real neurons differ"
        assert not got[l][:, :, H:].any(), f"layer {l}: a padded neuron spiked"
        if bn:
            assert torch.allclose(pstats[l][0][:H], stats[l][0], rtol=1e-12, atol=1e-14) and torch.allclose(pstats[l][1][:H], stats[l][1], rtol=1e-12, atol=1e-14)
    for k, p in st.named_parameters():
        rel = float((p.grad - ref_grads[k]).norm() / ref_grads[k].norm())
        assert rel < 1e-5, (k, rel)


# ---- 3. the kernels' fp64 reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,S,df,T,B", [(257, 1, 3, 37, 2), (129, 2, 2, 9, 3), (33, 4, 5, 2, 1), (17, 1, 1, 5, 2)])
def test_forward_reference_equals_the_existing_references(F, S, df, T, B):
    spec, coef, _ = df_inputs(F + S + df, B, F, T, S, df)
    y, tol = df_forward_reference(spec, coef, S, df)
    ri = np.stack([spec.real, spec.imag], -1)
    perm = coef.reshape(T, B, 2, df, S, F).transpose(0, 1, 2, 5, 3, 4).reshape(T, B, 2 * F * df * S)  # test_cirm_gsn._oracle_filter's
    enh, _, tol_fb, _, lo = fbk.deepfilter(ri, S, [(perm, 1, F, df)])
    assert lo == F and np.array_equal(enh, y) and np.array_equal(tol_fb, tol)
    t = deep_filter_torch(torch.from_numpy(spec).to(torch.complex128), torch.from_numpy(coef).double().permute(1, 2, 0), df, S)
    assert np.abs(torch.view_as_real(t).numpy() - y).max() < 1e-12
    # the kernel's arithmetic in numpy fp32 lies inside the bound; each mutation of the reference is caught by it
    y32 = fp32_forward(spec, coef, S, df)
    assert fbk.worst(y32, y, tol) <= 1.0 and fbk.vacuous_share(tol, y) == 0.0
    for mut in ("taps_desc", "swap_reim", "hist_nonzero"):
        if (mut in ("taps_desc", "hist_nonzero") and df == 1) or (mut == "hist_nonzero" and T < 2):
            continue
        ym, _ = df_forward_reference(spec, coef, S, df, mut=mut)
        assert fbk.worst(ym, y, tol) > 1.0, f"mutation {mut} passes the forward bound"


@pytest.mark.parametrize("F,S,df,T,B", [(257, 1, 3, 37, 2), (129, 2, 2, 9, 3), (33, 4, 5, 2, 1), (17, 1, 1, 5, 2)])
def test_backward_reference_equals_torch_autograd(F, S, df, T, B):
    spec, coef, g = df_inputs(7 * F + S + df, B, F, T, S, df)
    d_coef, tol = df_backward_reference(spec, g, S, df)
    c = torch.from_numpy(coef).double().requires_grad_(True)
    y = torch.view_as_real(deep_filter_torch(torch.from_numpy(spec).to(torch.complex128), c.permute(1, 2, 0), df, S))
    (y * torch.from_numpy(g).double()).sum().backward()
    assert np.abs(c.grad.numpy() - d_coef).max() < 1e-12
    # (the correctly rounded result lies inside the bound, and the bound says something about every element)
    assert fbk.worst(d_coef.astype(np.float32), d_coef, tol) <= 1.0 and fbk.vacuous_share(tol, d_coef) == 0.0
    for mut in ("taps_desc", "swap_reim", "sign_flip", "hist_nonzero"):
        if (mut in ("taps_desc", "hist_nonzero") and df == 1) or (mut == "hist_nonzero" and T < 2):
            continue
        dm, _ = df_backward_reference(spec, g, S, df, mut=mut)
        assert fbk.worst(dm, d_coef, tol) > 1.0, f"mutation {mut} passes the backward bound"


# ---- 4. the committed fixtures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.CASES))
def test_training_fixture_holds_what_the_gpu_tests_read(name):
    kw, seed, B, T, mode = cases.CASES[name]
    for p in cases.shard_paths(GOLD, name):
        assert os.path.getsize(p) < (1 << 20), p
    g = cases.load_fixture(GOLD, name)
    assert json.loads(str(g["kwargs"])) == kw and int(g["seed"]) == seed and str(g["mode"]) == mode
    m = cases.build_model(Model, kw, seed)
    assert cases.state_checksum(m) == str(g["checksum"]), "the weights rebuilt from the seed are not the ones the reference ran"
    S, H, Fq, recipe = kw["num_spks"], kw["hidden_size"], kw["n_fft"] // 2 + 1, kw["hidden_size"] > 64
    L = (T - 1) * kw["hop_length"]
    assert g["wave"].shape == (B, L) and torch.equal(torch.from_numpy(g["wave"]), cases.make_wave(kw, seed, B, T))
    assert g["enh_y"].shape == ((B, L) if S == 1 else (B, S, L)) and np.isfinite(float(g["loss"]))
    if S == 1:
        assert g["enh_mag"].shape == (B, Fq, T)
    rows = 4 if recipe else T
    assert g["x"].shape == (rows, B, Fq) and g["proj"].shape == (rows, B, 2 * kw["df_order"] * S * Fq)
    for l in range(kw["num_layers"]):
        assert tuple(g[f"spikes_shape/{l}"]) == (T, B, H)
        n = T * B * H
        spikes = np.unpackbits(g[f"spikes_packed/{l}"])[:n]
        near = np.unpackbits(g[f"near{cases.TAU:g}/{l}"])[:n]
        assert 0.05 < spikes.mean() < 0.95
        assert near.mean() <= (2e-4 if recipe else 0.0), (name, l, near.mean())
    for k, p in m.named_parameters():
        assert g[f"grad/{k}"].shape == tuple(p.shape) and g[f"grad/{k}"].any(), k
    for k, b in m.named_buffers():
        assert g[f"buf/{k}"].shape == tuple(b.shape), k
        if mode == "evalgrad":
            assert np.array_equal(g[f"buf/{k}"], b.numpy()), k
    if mode == "evalgrad":
        assert g["grad_wave"].shape == (B, L) and g["grad_wave"].any()


def test_cpu_tensors_are_refused_with_the_training_message():
    m = Model(512, 128, 512, 0.5, 257, 20, 2, 257, False, 3, bn=True, shared_weights=True, sequence_model="LSTM", num_spks=1)
    with pytest.raises(NotImplementedError, match="training.*no CPU path"):
        m.train()(torch.zeros(1, 1280))
    m.eval()
    m.autograd_in_eval = True
    with pytest.raises(NotImplementedError, match="training.*no CPU path"):
        m(torch.zeros(1, 1280))
