"""tests/trainref.py on the CPU: the fp64 steps pinned to PyTorch in float64 (nn.BatchNorm1d in training mode, a triangle
autograd.Function), the fp32 kernel form inside every bound, every mutant rejected, the planted properties kept along a free-running
chain, the reference alone leaving at most 2 % of a step's spikes unasserted, and the comparison itself failing on NaN.

Fifteen of the sixteen mutants are rejected by the bounds.  The sixteenth, `spike_gt` (> for >=), leaves every membrane as the reference
has it, bit for bit, and differs only in the spike at u == 0: it is rejected by the spike rule, at the `bn_scales` column whose membrane
is exactly 0 (bound 0, so the spike is asserted).  No bound can tell it apart."""
import numpy as np
import pytest
import torch

import trainref as tr

F64 = np.float64


class _Triangle(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u):
        ctx.save_for_backward(u)
        return (u >= 0).to(u.dtype)

    @staticmethod
    def backward(ctx, g):
        (u,) = ctx.saved_tensors
        return g * torch.clamp(1.0 - u.abs(), min=0.0)


def _torch_chain(p):
    """The chain of trainref.sim_fwd restated with torch modules in float64; loss = sum_t <h_t, dh_up[t]>."""
    H, R, T, sh = p["H"], p["R"], p["T"], p["shared"]
    G = 1 if sh else 2
    t64 = lambda a: torch.tensor(np.asarray(a, F64), dtype=torch.float64)
    z, bias, w_hh = t64(p["z"]).requires_grad_(), t64(p["bias"]).requires_grad_(), t64(p["w_hh"]).requires_grad_()
    bn = torch.nn.BatchNorm1d(H, eps=float(np.float32(p["eps"])), momentum=None if p["momentum"] is None else float(np.float32(p["momentum"]))).double().train()
    with torch.no_grad():
        bn.weight.copy_(t64(p["bn_w"])); bn.bias.copy_(t64(p["bn_b"]))
        bn.running_mean.copy_(t64(p["rm0"])); bn.running_var.copy_(t64(p["rv0"])); bn.num_batches_tracked.fill_(p["n0"])
    c0 = t64(p["c0"] if p["c0"] is not None else np.zeros((R, H))).requires_grad_()
    h = (t64(p["h0"]) != 0).double() if p["h0"] is not None else torch.zeros((R, H), dtype=torch.float64)
    c, out, loss = c0, dict(u=[], f=[], g=[], spikes=[], rm=[], rv=[]), 0.0
    for t in range(T):
        rec = h @ w_hh.t()
        pre_f = (z[t][:, :H] + bias[:H]) + rec[:, :H]
        pre_g = (z[t][:, (G - 1) * H:] + bias[H:]) + rec[:, (G - 1) * H:]
        f = torch.sigmoid(pre_f)
        u = bn(f * c + (1 - f) * pre_g)
        h = _Triangle.apply(u)
        c = u
        loss = loss + (h * t64(p["dh_up"][t])).sum()
        for k, v in (("u", u), ("f", f), ("g", pre_g), ("spikes", h), ("rm", bn.running_mean), ("rv", bn.running_var)):
            out[k].append(v.detach().clone().numpy())
    loss.backward()
    return {k: np.stack(v) for k, v in out.items()}, dict(z=z.grad.numpy(), bias=bias.grad.numpy(), w_hh=w_hh.grad.numpy(), c0=c0.grad.numpy(),
                                                         bn_w=bn.weight.grad.numpy(), bn_b=bn.bias.grad.numpy())


def _close(a, b, what):
    err, ref = float(np.abs(np.asarray(a, F64) - b).max()), float(np.abs(b).max())
    assert err <= 1e-12 * max(ref, 1e-300) or err == 0, f"{what}: {err:.3e} against {ref:.3e}"


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("case", ["control", "momenta_cum7", "state", "momenta_1"])
def test_reference_is_torch_float64(case, shared, T):
    p = tr.make_case(case, 16, 9, T, shared)
    ours = tr.free_chain(p)
    theirs, grads = _torch_chain(p)
    for k in ("u", "f", "g", "rm", "rv"):
        _close(ours[k], theirs[k], k)
    assert np.array_equal(ours["spikes"], theirs["spikes"])
    b = tr.sim_bwd(p, ours, dt=F64)
    H = p["H"]
    _close(b["d_z"] if shared else b["d_gates"], grads["z"], "d_z")
    _close(b["d_gates"].sum((0, 1)), grads["bias"], "d_bias")
    _close(b["dc"][0], grads["c0"], "dL/dc0 (through the forget gate)")
    _close(b["dbw"][0], grads["bn_w"], "d_bn_w")
    _close(b["dbb"][0], grads["bn_b"], "d_bn_b")
    hprev = np.concatenate([(p["h0"] != 0).astype(F64)[None] if p["h0"] is not None else np.zeros((1, p["R"], H)), ours["spikes"][:-1]])
    dzs = b["d_z"] if shared else b["d_gates"]
    _close(np.einsum("trn,trk->nk", dzs, hprev), grads["w_hh"], "d_w_hh")


@pytest.mark.parametrize("case", list(tr.CASES))
def test_kernel_form_within_bounds(case):
    """The fp32 emulation of the kernels' operation sequence -- either product order, row blocks of 16, 32 or all rows -- stays inside
    every bound, forward and backward, on every case and small geometry."""
    worst = tr.Worst()
    for H, R, sh in tr.SMALL_GEOMETRIES:
        p = tr.make_case(case, H, R, 2, sh)
        for order in ("k", "mfma4"):
            for rpb in (16, 32, R):
                dev = tr.sim_fwd(p, order, rpb)
                fails = tr.judge_fwd(p, dev, worst)
                fails += tr.judge_bwd(p, dev, tr.sim_bwd(p, dev, order, rpb), worst)
                assert not fails, (H, R, sh, order, rpb, fails[:5])
    print(f"\n{case}: worst error / bound  {worst.line()}")


@pytest.mark.parametrize("name", tr.BWD_CASES)
def test_kernel_form_within_bounds_synthetic_backward(name):
    worst = tr.Worst()
    for H, R, sh in [(16, 17, True), (32, 33, False), (16, 2, False), (48, 64, True)]:
        for use_bn in (True, False):
            p, fwd = tr.bwd_case(name, H, R, 3, sh, use_bn)
            for order, rpb in (("k", 16), ("mfma4", 32), ("mfma4", R)):
                fails = tr.judge_bwd(p, fwd, tr.sim_bwd(p, fwd, order, rpb), worst)
                assert not fails, (H, R, sh, use_bn, order, rpb, fails[:5])
    print(f"\nbackward {name}: worst error / bound  {worst.line()}")


def _rejections(mut):
    """{case: (largest |mutant - reference| / bound, its output)} over a few geometries; a mutant counts as rejected where that reaches 2 (no result
    within the bound of the mutant is within the bound of the reference), or -- the spike comparison -- where an ASSERTED spike differs."""
    where = tr.MUTANTS[mut][0]
    caught = {}
    for H, R, sh in [(16, 17, True), (32, 33, False), (16, 2, True)]:
        if where == "bwd":
            cases = [("bwd_" + n, tr.bwd_case(n, H, R, 3, sh)) for n in tr.BWD_CASES] + [(n, None) for n in ("control", "tails")]
        else:
            cases = [(n, None) for n in tr.CASES]
        for name, syn in cases:
            w = tr.Worst()
            if syn is not None:
                p, fwd = syn
                tr.judge_bwd(p, fwd, tr.sim_bwd(p, fwd, dt=F64), w, mut=mut)
            else:
                p = tr.make_case(name, H, R, 3, sh)
                if where == "bwd":
                    if not sh and mut == "dz_dpf_only":
                        continue
                    fwd = tr.free_chain(p)
                    tr.judge_bwd(p, fwd, tr.sim_bwd(p, fwd, dt=F64), w, mut=mut)
                elif where == "fwd32":
                    if p["bn_w"] is None:
                        continue
                    tr.judge_fwd(p, tr.sim_fwd(p, "k", R, mut=mut), w)
                else:
                    fails = tr.judge_fwd(p, tr.free_chain(p), w, mut=mut)
                    w.pop("unasserted", None)
                    if max(w.values(), default=0.0) <= 2.0 and any("spikes (asserted)" in f for f in fails):
                        w["spikes"] = np.inf  # (only `spike_gt` needs this: its membranes are the reference's, bit for bit)
            w.pop("unasserted", None)
            key = max(w, key=w.get, default=None)
            need = 1.0 if where == "fwd32" else 2.0  # (the fp32 form is judged like a device: outside the bound)
            if key is not None and w[key] > need and w[key] > caught.get(name, (0.0, None))[0]:
                caught[name] = (w[key], key)
    return caught


def test_every_mutant_is_rejected():
    table = {m: _rejections(m) for m in tr.MUTANTS}
    print()
    for m, caught in table.items():
        print(f"{m:18s} {tr.MUTANTS[m][1]:60s} caught by: " + ", ".join(f"{k} ({o} {v:.3g})" for k, (v, o) in sorted(caught.items())))
    assert all(table.values()), [m for m, c in table.items() if not c]
    assert "offset" in table["var_e2"] and "state" in table["h_value"] and "bn_scales" in table["spike_gt"]


@pytest.mark.parametrize("case", [c for c in tr.CASES])
def test_planted_properties_hold_and_cap(case):
    """Along a free-running fp64 chain of 7 steps every case keeps what it plants, and the reference alone -- |u_ref| <= bound --
    leaves at most CAP of any step's spikes unasserted, on every geometry."""
    worst = tr.Worst()
    for H, R, sh in tr.GEOMETRIES:
        p = tr.make_case(case, H, R, 7, sh)
        ch = tr.free_chain(p)
        if p["holds"] is not None:
            for t in range(7):
                assert p["holds"]({k: (v[t] if v is not None else None) for k, v in ch.items()}), (case, H, R, sh, t)
        fails = tr.judge_fwd(p, ch, worst, running_too=False)
        assert not fails, fails[:5]
    assert worst["unasserted"] <= tr.CAP
    print(f"\n{case}: largest unasserted share of a step {worst['unasserted']:.5f}")


def test_blocking_table():
    """The row blockings the geometry grid was chosen for (train_geometry restated in trainref.blocking)."""
    assert tr.blocking(2, 16, True) == (1, 16) and tr.blocking(17, 48, False) == (2, 16) and tr.blocking(33, 32, True) == (3, 16)
    assert tr.blocking(130, 224, False) == (9, 16) and tr.blocking(64, 320, True) == (4, 16)
    assert tr.blocking(512, 320, True) == (8, 64) and tr.blocking(513, 320, True) == (7, 80)


FWD_OUTPUTS = ("spikes", "u", "xhat", "f", "g", "invstd", "rm", "rv")
BWD_OUTPUTS = ("d_gates", "d_z", "dc", "dbw", "dbb")


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_value_that_is_no_number_fails_in_every_output(bad):
    """An element a kernel did not write (the device tests prefill with NaN) or an inf / inf of a tail: planted in each output in turn --
    one element, a whole row, the last step -- the comparison must report that output."""
    p = tr.make_case("tails", 16, 17, 3, True)
    dev = tr.sim_fwd(p, "mfma4", 16)
    back = tr.sim_bwd(p, dev, "mfma4", 16)
    assert not tr.judge_fwd(p, dev, tr.Worst()) and not tr.judge_bwd(p, dev, back, tr.Worst())
    for where in ("element", "row", "last step"):
        idx = {"element": (1, 16, 3), "row": (1, 16), "last step": (2,)}[where]
        for k in FWD_OUTPUTS:
            d = {n: (None if v is None else v.copy()) for n, v in dev.items()}
            d[k][idx[:d[k].ndim] if d[k].ndim == 3 else (idx[0], 3)] = bad
            w = tr.Worst()
            assert tr.judge_fwd(p, d, w), (k, where)
            assert not all(np.isfinite(v) for v in w.values()) or k == "spikes", (k, where, w.line())
        for k in BWD_OUTPUTS:
            d = {n: (None if v is None else v.copy()) for n, v in back.items()}
            d[k][idx[:d[k].ndim] if d[k].ndim == 3 else (idx[0], 3)] = bad
            w = tr.Worst()
            assert tr.judge_bwd(p, dev, d, w), (k, where)
            assert not all(np.isfinite(v) for v in w.values()), (k, where, w.line())
    w = tr.Worst()
    assert w.see("x", np.array([0.0, np.nan]), np.array([1.0, 1.0])) == np.inf and w["x"] == np.inf
