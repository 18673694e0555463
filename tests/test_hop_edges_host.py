"""CPU checks of tests/hopref.py before a GPU is involved: a planted case survives the state-dict -> folded-parameter mapping of
engine.fold_batchnorm (threshold's exact zeros and +-1e-30 shifts, bn_signs' zero, negative and 8.0 scales) and loads into the
modules strictly; on every geometry x case tests/test_hop_edges.py runs, the fp64 reference ALONE -- layer 0 on the oracle's features
of the same seeded spectra, every layer above on the reference's own spikes -- leaves at most 2 % of the elements unasserted,
`saturated` fires every neuron and its integer sums reach K QMAX for every H used; and the two mutations of hop_layer_role's cell the
GPU file is meant to catch (`>` for `>=`, a dropped gate-bias difference) are rejected in the model setting by scanref's emulation.
numpy, the oracle and engine.fold_batchnorm only (no library call)."""
import numpy as np
import pytest

import hopref as hr
import scanref as sr
from oracle import Oracle
from oracle.model import forward_from_stft, spec_from_frozen_kwargs, spec_from_live_kwargs

NAMES = list(sr.CASES)
F32 = np.float32
# the reference does not depend on hop or on counting: one entry per (front, kwargs, B)
HOST_GEOMS = {}
for _g, (_front, _kw, _B, _hop, _count) in hr.GEOMS.items():
    if _g not in hr.REFUSED and not any(v[0] == _front and v[1] is _kw and v[2] == _B for v in HOST_GEOMS.values()):
        HOST_GEOMS[_g] = (_front, _kw, _B)
MODELS = {}  # one entry per model
for _g, _v in HOST_GEOMS.items():
    if not any(w[1] is _v[1] for w in MODELS.values()):
        MODELS[_g] = _v[:2]
_cache = {}


def folded(sd, pre):
    from spiking_fullsubnet_amd.engine import fold_batchnorm
    return fold_batchnorm(sd[pre + "batchnorm.weight"], sd[pre + "batchnorm.bias"], sd[pre + "batchnorm.running_mean"],
                          sd[pre + "batchnorm.running_var"])


def host_stacks(front, sd):
    """hopref.held_stacks from the state dict alone: the planted weights are on the 24-bit grid already (packing is the identity,
    test_scanref_host.py), the scale and shift are the engine's folding."""
    def cell(pre, l):
        H = sd[pre + "weight_hh"].shape[1]
        a, b = folded(sd, pre)
        return dict(H=H, H_real=H, G=sd[pre + "weight_hh"].shape[0] // H, kind="x32" if l == 0 else "spike", W_hh=sd[pre + "weight_hh"],
                    W_ih=sd[pre + "weight_ih"], bias=sd[pre + "bias_ih"], alpha=a, beta=b)

    seqs = ["fb_model."]
    g = 0
    while f"sb_model.sb_models.{g}.sequence_model.layers.0.cell.weight_hh" in sd:
        seqs.append(f"sb_model.sb_models.{g}.")
        g += 1
    out = []
    for s in seqs:
        layers, l = [], 0
        while f"{s}sequence_model.layers.{l}.cell.weight_hh" in sd:
            layers.append(cell(f"{s}sequence_model.layers.{l}.cell.", l))
            l += 1
        out.append(layers)
    return out


def layer0_inputs(front, kw, sd, stft):
    """[x [T][R][I] per sequence model] from the oracle's features (fp64, cast to fp32: what a layer-0 kernel is handed)."""
    if front == "cirm":
        o = Oracle("f64")
        x = np.ascontiguousarray((np.abs(stft.astype(np.complex128)) ** kw["fdrc"]).transpose(2, 0, 1))  # [T, B, F]
        return [o.layer_norm(x, sd["fb_model.pre_layer_norm.weight"], sd["fb_model.pre_layer_norm.bias"]).astype(F32)]
    spec = spec_from_live_kwargs(kw) if front == "live" else spec_from_frozen_kwargs(kw)
    res = forward_from_stft(spec, sd, stft, precision="f64")
    return [np.asarray(res["fb_all"][0], F32)] + [np.asarray(a[0], F32) for a in res["sb_all"]]


def reference_alone(geom, name):
    if (geom, name) not in _cache:
        front, kw, B = HOST_GEOMS[geom]
        sd, cases = hr.plant(front, kw, name)
        stacks = host_stacks(front, sd)
        xs = layer0_inputs(front, kw, sd, hr.spectrum(B, 257, hr.T, hr.geom_seed(geom)))
        tally = hr.Tally(f"{geom} {name} (reference alone)")
        refs = []
        for stack, x in zip(stacks, xs):
            inp, per = x, []
            for hd in stack:
                p = hr.layer_case(hd, inp)
                ref = sr.layer(p)
                assert np.isfinite(ref["y"]).all() and np.isfinite(ref["tol"]).all()
                tally.add(sr.compare(ref["spk"], ref), 0.0, ref["spk"], ref["smax"])
                per.append((p, ref))
                inp = ref["spk"]
            refs.append(per)
        _cache[geom, name] = (tally, refs, sd, cases)
    return _cache[geom, name]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("geom", sorted(MODELS))
def test_planted_properties_survive_the_folding(geom, name):
    front, kw = MODELS[geom]
    sd, cases = hr.plant(front, kw, name)
    assert len(cases) == len(hr.cell_prefixes(sd)) >= 2
    for pre, p in cases.items():
        a, b = folded(sd, pre)
        np.testing.assert_array_equal(a, p["alpha"], err_msg=pre)  # the folded inverse deviation is exactly 1
        np.testing.assert_array_equal(b, p["beta"], err_msg=pre)   # (value: -0.0 may come back as +0.0, the same membrane test)
        np.testing.assert_array_equal(sr.dequantise(sd[pre + "weight_hh"]), sd[pre + "weight_hh"])
        H = p["H"]
        if name == "threshold":
            g1, g2, g3 = sr.threshold_groups(H)
            allg = np.concatenate([g1, g2, g3])
            assert (b[g1] == 0).all() and (b[g3] == 0).all() and (a[g1[::2]] < 0).all() and (a[g2] > 0).all()
            np.testing.assert_array_equal(b[g2], np.where(np.arange(len(g2)) % 2 == 0, 1.0, -1.0).astype(F32) * F32(1e-30))
            for g in range(sd[pre + "weight_hh"].shape[0] // H):
                assert not sd[pre + "weight_hh"][g * H + allg].any() and not sd[pre + "weight_ih"][g * H + allg].any()
            assert not sd[pre + "bias_ih"][allg].any() and not sd[pre + "bias_ih"][H + allg].any()
        if name == "bn_signs":
            j = np.arange(H)
            assert (a[j % 29 == 4] == 0).all() and (a[j % 31 == 7] == 8.0).all() and (a < 0).sum() >= H // 4
        if name == "saturated":
            q, _ = sr.quantise(sd[pre + "weight_hh"])
            assert (np.abs(q) == sr.QMAX).all() and (b == 200.0).all()


@pytest.mark.parametrize("geom", sorted(MODELS))
def test_planted_state_dict_loads_strictly(geom):
    import torch
    import spiking_fullsubnet_amd as pkg
    front, kw = MODELS[geom]
    if front == "cirm":
        from spiking_fullsubnet_amd.modeling_cirm_gsn import Model
        m = Model(**kw)
    else:
        m = (pkg.SpikingFullSubNet if front == "live" else pkg.Separator)(**kw)
    sd, _ = hr.plant(front, kw, "control")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("geom", sorted(HOST_GEOMS))
def test_reference_alone_leaves_at_most_two_percent_unasserted(geom, name):
    tally, refs, sd, cases = reference_alone(geom, name)
    tally.done()  # the 2 % cap of test_scan_edges.py: a condition on the cases in the model setting, not a measurement
    for per in refs:
        for l, (p, ref) in enumerate(per):
            if name == "saturated":
                assert ref["spk"].all(), "a saturated neuron did not fire"
                assert ref["smax"] == p["H"] * sr.QMAX, (geom, l, ref["smax"])  # the recurrent sum from frame 1 on (layers >= 1: the input's too)
            if name == "threshold":
                g1, g2, g3 = sr.threshold_groups(p["H"])
                assert (ref["y"][:, :, g1] == 0).all() and (ref["tol"][:, :, g1] == 0).all() and ref["spk"][:, :, g1].all()
                assert (ref["spk"][:, :, g2] == (p["beta"][g2] > 0)).all() and (np.abs(ref["y"][:, :, g2]) > ref["tol"][:, :, g2]).all()
            if name == "tails":
                assert np.abs(p["bias"][:p["H"]]).max() > 88.8


@pytest.mark.parametrize("geom", ["tiny-B3", "m-B1", "tiny_g2-B1", "cirm_tiny-B3"])
@pytest.mark.parametrize("mut,name", [("gt", "threshold"), ("no_db", "control")])
def test_cell_mutations_are_rejected_in_the_model_setting(geom, mut, name):
    """`>` for `>=` in the cell, or the gate-bias difference dropped (separate gates: the cell gate on the forget gate's bias): the fp32
    emulation of the kernels' order with that mutation fails `compare` in the first sequence model's layer 0 AND layer 1."""
    _, refs, _, _ = reference_alone(geom, name)
    for p, ref in refs[0][:2]:
        out = sr.fp32_kernel_form(p, mut)
        assert not sr.compare(out["spk"], ref, None).ok, (geom, mut, p["kind"])
        good = sr.fp32_kernel_form(p)
        assert sr.compare(good["spk"], ref, None).ok
