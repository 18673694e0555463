"""CPU checks of tests/scanref.py itself, before a GPU is involved: the integer restatement of the weight packing equals the library's
pack / unpack; the fp64 layer equals Oracle("f64").gsn_layer on the oracle's own (unquantised) weight handling; both fp32 emulations of
the step sit inside the derived bound with half of it to spare on every case and geometry test_scan_edges.py runs, with at most 2 % of
the elements left unasserted; every mutant of the emulation is rejected on its named case; and the arithmetic claims the kernels'
comments make (integer recombination up to K = 256, float recombination up to K = 320) hold as assertions.  The same pins, criterion and
mutants for the kinds the streaming hops add (scanref.HOP_GRID: "x32", and "spike" / "x32" with separate gate weights).
No GPU is needed, but test_quantise_is_the_librarys_packing calls the library's HOST packing functions, so the library must have been
built (build()), as for tests/test_host_cpu.py; everything else here is numpy and the oracle."""
import numpy as np
import pytest

import scanref as sr
from oracle import Oracle

R, T = 16, sr.T_MAX  # (rows are independent: 16 rows of 9 frames pose every case; the GPU file runs up to 48 rows of the same generator)
_cache = {}


def _case(name, H, shared, kind, I=38, bits=24):
    key = (name, H, shared, kind, I, bits)
    if key not in _cache:
        p = sr.make_case(name, H, shared, kind, I, bits, R=R, T=T)
        _cache[key] = (p, sr.layer(p))
    return _cache[key]


def test_quantise_is_the_librarys_packing():
    from spiking_fullsubnet_amd.engine import pack_w3, unpack_w3
    rng = np.random.default_rng(0)
    mats = [rng.uniform(-0.1, 0.1, (48, 70)).astype(np.float32), sr._scaled_rows(rng, 64, 96, 5), sr._sat_rows(32, 64, 24, -8),
            np.zeros((16, 64), np.float32), sr.make_case("digit_extremes", 64, True, "zin", R=2, T=1)["W_hh"]]
    for w in mats:
        for bits in (24, 16):
            q, dq = sr.quantise(w, bits)
            pk, dqp = pack_w3(w, bits)
            np.testing.assert_array_equal(dqp[:len(w)].astype(np.float64), dq)
            np.testing.assert_array_equal(unpack_w3(pk, dqp, *w.shape), (q * dq[:, None]).astype(np.float32))
            np.testing.assert_array_equal(sr.dequantise(sr.dequantise(w, bits), bits), sr.dequantise(w, bits))  # packing again is the identity
    q, _ = sr.quantise(mats[-1])
    d0, d1, d2 = sr.digits(q)
    assert set(np.unique(np.stack([d0, d1])).tolist()) <= {-128, -1, 0, 127} and set(np.unique(d2).tolist()) <= {-1, 0, 127}
    np.testing.assert_array_equal(d2 * 65536 + d1 * 256 + d0, q)


@pytest.mark.parametrize("name", ["control", "tails"])
@pytest.mark.parametrize("H,shared,kind", [(64, True, "zin"), (48, False, "zin"), (96, True, "spike"), (80, True, "x"), (96, False, "spike"),
                                           (80, True, "x32"), (80, False, "x32")])
def test_reference_equals_the_fp64_oracle(name, H, shared, kind):
    """Unquantised weights on both sides.  The oracle forms its own input product; a given zin goes in as x with an identity W_ih and
    its biases taken out (shared gates: (0, b_g - b_f), so that its two gate sums are zin and zin + (b_g - b_f))."""
    p = sr.make_case(name, H, shared, kind, R=7, T=T)
    ref = sr.layer(p, quant=False)
    G = 1 if shared else 2
    if kind == "zin":
        x, w_ih = p["zin"], np.eye(G * H)
        b64 = p["bias"].astype(np.float64)
        bias = np.concatenate([np.zeros(H), b64[H:] - b64[:H]]) if shared else np.zeros(2 * H)
    else:
        x, w_ih, bias = (p["s_in"] if kind == "spike" else p["x"]), p["W_ih"], p["bias"]
    bn = (p["alpha"], p["beta"], np.zeros(H), np.ones(H))  # eps = 0: invstd = 1, the folded scale and shift pass through exactly
    spk, mem, hT, cT = Oracle("f64").gsn_layer(x, w_ih, p["W_hh"], bias, bn=bn, shared=shared, h0=p["h0"], c0=p["c0"], eps=0.0)
    np.testing.assert_array_equal(spk > 0.5, ref["spk"])
    scale = np.maximum(np.abs(ref["y"]), 1.0)
    assert np.max(np.abs(mem - ref["y"]) / scale) <= 1e-13
    np.testing.assert_array_equal(hT > 0.5, ref["spk"][-1])
    if name == "tails":
        pf = p["zin"][:, :, :H] if kind == "zin" else p["bias"][:H]
        assert pf.min() < -88.8 and pf.max() > 17 and np.abs(pf).max() <= 120


@pytest.mark.parametrize("H,shared,kind,I,bits", sr.GRID, ids=[f"H{g[0]}-{'shared' if g[1] else 'separate'}-{g[2]}-I{g[3]}-w{g[4]}" for g in sr.GRID])
def test_both_fp32_forms_are_inside_the_bound_with_half_to_spare(H, shared, kind, I, bits):
    for name in sr.CASES:
        p, ref = _case(name, H, shared, kind, I, bits)
        assert np.isfinite(ref["y"]).all() and np.isfinite(ref["tol"]).all(), name
        strict = sr.layer(p, rnd=sr.U)  # a first-order count of 1u per rounding: printed, so that what the 2u unit gives away stays visible
        for form in (sr.fp32_kernel_form, sr.fp32_reference_form):
            out = form(p)
            assert np.isfinite(out["y"]).all(), (name, form.__name__)
            res = sr.compare(out["spk"], ref, out["y"])
            r1 = sr.worst(out["y"], strict["y"], strict["tol"])
            print(f"{name:16s} H={H} {form.__name__:20s} ratio {res.ratio:.3f} (1u per rounding: {r1:.3f}) unasserted {res.unasserted:.5f} "
                  f"median tol {np.median(ref['tol']):.2e}")
            assert res.ok and res.ratio <= 0.5 and res.unasserted <= 0.02, (name, form.__name__, res)
        if name == "saturated":
            assert ref["spk"].all(), "a saturated neuron did not fire"


@pytest.mark.parametrize("H", [224, 256, 320])
def test_second_layer_of_a_stack_is_inside_the_bound(H):
    for name in sr.CASES:
        p0, ref0 = _case(name, H, True, "zin")
        p1 = sr.next_layer(p0, ref0, name)
        if name == "saturated":
            np.testing.assert_array_equal(p1["s_in"], ref0["spk"].astype(np.int8))
        ref1 = sr.layer(p1)
        for form in (sr.fp32_kernel_form, sr.fp32_reference_form):
            out = form(p1)
            res = sr.compare(out["spk"], ref1, out["y"])
            assert res.ok and res.ratio <= 0.5 and res.unasserted <= 0.02, (name, form.__name__, res)


def test_threshold_groups_are_decided_as_constructed():
    for H, shared, kind, I, bits in sr.GRID:
        p, ref = _case("threshold", H, shared, kind, I, bits)
        g1, g2, g3 = sr.threshold_groups(H)
        assert (ref["y"][:, :, g1] == 0).all() and (ref["tol"][:, :, g1] == 0).all() and ref["spk"][:, :, g1].all()
        assert (ref["y"][:, :, g3] == 0).all() and ref["spk"][:, :, g3].all()
        assert (ref["y"][0][:, g2] == p["beta"][g2].astype(np.float64)).all()
        assert (ref["spk"][:, :, g2] == (p["beta"][g2] > 0)).all()
        assert (np.abs(ref["y"][:, :, g2]) > ref["tol"][:, :, g2]).all() and (ref["tol"][:, :, g2] < 1e-5 * np.abs(ref["y"][:, :, g2])).all()


def _rejected(p, ref, mut):
    return [f.__name__ for f in (sr.fp32_kernel_form, sr.fp32_reference_form) if not sr.compare((o := f(p, mut))["spk"], ref, o["y"]).ok]


# mutant -> (cases that must reject it, cases that must NOT: the gap the case closes), on H = 224 / 256 shared gates with a given input term
MUTANT_CASES = {
    "gt": (["threshold"], ["control"]),
    "no_db": (["control"], []),
    "wrap31": (["saturated"], ["control", "tails", "bn_signs"]),
    "abs_alpha": (["bn_signs"], []),
    "bf16_in": (["control"], []),
    "drop_d0": (["control", "digit_extremes"], []),
}


@pytest.mark.parametrize("mut", sr.MUTANTS)
@pytest.mark.parametrize("H", [224, 256])
def test_mutants_are_rejected_on_their_named_case(mut, H):
    caught, missed = MUTANT_CASES[mut]
    for name in caught:
        p, ref = _case(name, H, True, "zin")
        assert len(_rejected(p, ref, mut)) == 2, (mut, name)
    for name in missed:
        p, ref = _case(name, H, True, "zin")
        assert _rejected(p, ref, mut) == [], (mut, name)


def test_input_term_mutants_are_rejected_on_the_fused_kind():
    for mut in ("wrap31", "drop_d0", "bf16_in"):
        name = "saturated" if mut == "wrap31" else "control"
        p, ref = _case(name, 256, True, "spike")
        assert len(_rejected(p, ref, mut)) == 2, mut


@pytest.mark.parametrize("I", [38, 64])
def test_mutants_are_rejected_on_the_real_valued_input_kind(I):
    """Kind "x" (fused-x, stack layer 0): its input-term bound is the widest of the three, so the mutants are shown to bite there too."""
    p, ref = _case("control", 224, True, "x", I)
    for mut in ("bf16_in", "no_db", "drop_d0"):
        assert len(_rejected(p, ref, mut)) == 2, (mut, I)
    p, ref = _case("saturated", 256, True, "x", I)
    assert len(_rejected(p, ref, "wrap31")) == 2
    p, ref = _case("threshold", 224, True, "x", I)
    assert len(_rejected(p, ref, "gt")) == 2
    p, ref = _case("bn_signs", 224, True, "x", I)
    assert len(_rejected(p, ref, "abs_alpha")) == 2


HOP_IDS = [f"H{g[0]}-{'shared' if g[1] else 'separate'}-{g[2]}-I{g[3]}" for g in sr.HOP_GRID]


@pytest.mark.parametrize("H,shared,kind,I", sr.HOP_GRID, ids=HOP_IDS)
def test_hop_kinds_are_inside_the_bound_with_half_to_spare(H, shared, kind, I):
    """The same criterion on the cells of the streaming hops: "x32" (both summation orders: four accumulators by chunk / one fmaf
    chain) and "spike", shared and separate gate weights."""
    for name in sr.CASES:
        p, ref = _case(name, H, shared, kind, I)
        assert np.isfinite(ref["y"]).all() and np.isfinite(ref["tol"]).all(), name
        for form in (sr.fp32_kernel_form, sr.fp32_reference_form):
            out = form(p)
            assert np.isfinite(out["y"]).all(), (name, form.__name__)
            res = sr.compare(out["spk"], ref, out["y"])
            print(f"{name:16s} H={H} I={I} {kind} {form.__name__:20s} ratio {res.ratio:.3f} unasserted {res.unasserted:.5f}")
            assert res.ok and res.ratio <= 0.5 and res.unasserted <= 0.02, (name, form.__name__, res)
        if name == "saturated":
            assert ref["spk"].all(), "a saturated neuron did not fire"
            if kind == "spike":
                assert ref["smax"] == H * sr.QMAX
        if name == "tails":
            assert np.abs(p["bias"]).max() > 88.8


# mutant -> a case that must reject it, for every new (kind, sharing)
HOP_MUTANT_CASE = dict(gt="threshold", no_db="control", wrap31="saturated", abs_alpha="bn_signs", bf16_in="control", drop_d0="control")


@pytest.mark.parametrize("mut", sr.MUTANTS)
@pytest.mark.parametrize("H,shared,kind,I", [(320, True, "x32", 64), (224, True, "x32", 158), (320, False, "x32", 64), (224, False, "spike", 38),
                                             (320, False, "spike", 38), (268, True, "x32", 257)])
def test_mutants_are_rejected_on_the_hop_kinds(H, shared, kind, I, mut):
    """Both emulations of every mutant fail `compare` on at least one case -- the mutant's own is tried first -- for "x32" (either
    sharing) and "spike" with separate gates.  (wrap31 folds at +-2^30: a width whose saturated sum stays below that has nothing to
    reject; none of these is that narrow.  drop_d0 under a wide layer-0 product: the K + 1 roundings of "x32" at K = 158 hide a dropped low digit of the
    mild weights; `saturated`, whose low digits are all +-127, does not.)"""
    if mut == "wrap31" and H * sr.QMAX < 2 ** 30:
        return
    names = [HOP_MUTANT_CASE[mut]] + [n for n in sr.CASES if n != HOP_MUTANT_CASE[mut]]
    hit = next((n for n in names if len(_rejected(*_case(n, H, shared, kind, I), mut)) == 2), None)
    print(f"{mut} H={H} {'shared' if shared else 'separate'} {kind} I={I}: rejected on {hit}")
    assert hit is not None, (mut, H, shared, kind)


def test_arithmetic_claims():
    """sfsn_scan3_dev.h / s3j_recombine / scan3i / scan3x: (a2 << 16) + (a1 << 8) + a0 stays inside int32 up to K = 256 (every partial sum:
    the full sum less the low plane's <= K 128); recombine3 (sfsn_scan_dev.h): |a1 256 + a0| < 2^24 and |a2| < 2^16 up to K = 320."""
    assert sr.QMAX == 8355711
    assert 256 * sr.QMAX < 2 ** 31 and 256 * sr.QMAX + 256 * 128 < 2 ** 31
    assert 257 * sr.QMAX + 257 * 128 >= 2 ** 31 - 2 ** 24  # (the margin is 0.4 %: nothing to give away)
    assert 320 * (128 * 256 + 128) < 2 ** 24 and 320 * 128 < 2 ** 16
    assert 320 * sr.QMAX >= 2 ** 31  # why H = 320 needs the float form
    for K in (224, 256, 320):
        for kind in ("zin", "spike"):
            p, ref = _case("saturated", K, True, kind)
            assert ref["smax"] == K * sr.QMAX, (K, kind, ref["smax"])
            q, _ = sr.quantise(p["W_hh"])
            assert (np.abs(q) == sr.QMAX).all()
    p, ref = _case("saturated", 224, True, "zin", bits=16)
    assert ref["smax"] == 224 * sr.Q16MAX * 256
    p, ref = _case("saturated", 320, False, "zin")
    assert ref["smax"] == 320 * sr.QMAX
    for name in ("control", "tails", "bn_signs"):
        assert _case(name, 256, True, "zin")[1]["smax"] < 2 ** 30  # today's distribution never comes near: why nothing noticed
