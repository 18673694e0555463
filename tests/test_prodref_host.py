"""tests/prodref.py checked on the CPU: the spike reference against the library's packing, the restated dispatch against the list of
compiled forms, the case generators against their stated domain, the fp32 emulations (and a correctly rounded fp32 chain) against
every bound on every case, and every deliberately wrong variant against the case that is named for it.  Nothing is left unasserted:
prodref.check looks at every element of every buffer, canaries included."""
import numpy as np
import pytest

import prodref as pr
import scanref as sr

HOST_REAL = [pr.SMALLEST["bf3"], pr.SMALLEST["f32mfma"], pr.SMALLEST["plain"], pr.PLAIN_N, (65, 94, 224), (70, 162, 64), (64, 192, 32)]
HOST_SPIKE = (65, 224, 40)  # |S| reaches 224 QMAX > 2^30: wrap31 has something to fold


def _real(c, kind):
    return pr.real_reference(c["x"], c["w"], c["b"], kind)


def test_spike_reference_is_the_librarys_packing():
    """quantise == sfsn_w3_pack_bits on every spike case, and `want` == the older test's expression on the unpacked weights."""
    from spiking_fullsubnet_amd.engine import pack_w3, unpack_w3
    for name in pr.SPIKE_CASES:
        for bits in (24, 16):
            c = pr.spike_case(name, 20, 100, 40, bits)
            q, dq = sr.quantise(c["w"], bits)
            pk, dqp = pack_w3(c["w"], bits)
            np.testing.assert_array_equal(dqp[:40].astype(np.float64), dq)
            wq = unpack_w3(pk, dqp, 40, 100)
            np.testing.assert_array_equal(wq, (q * dq[:, None]).astype(np.float32))
            ref = pr.spike_reference(c["s"], c["w"], c["b"], bits)
            old = (c["s"][:, :100].astype(np.float64) @ wq.astype(np.float64).T).astype(np.float32) + (0 if c["b"] is None else c["b"])
            e = ref["exact"]
            assert np.array_equal(ref["want"][e], old.astype(np.float32)[e]), (name, bits)
            assert np.isfinite(ref["y"]).all() and (sr.worst(ref["want"], ref["y"], ref["tol"]) <= 0.5), (name, bits)


def test_spike_rows_are_padded_with_zeros_and_hold_every_kind_of_row():
    for K in pr.SPIKE_K:
        s = pr.spike_case("control", 33, K, 8)["s"]
        assert s.shape == (33, pr.pad64(K)) and not s[:, K:].any() and set(np.unique(s)) <= {0, 1}
        assert not s[0].any() and s[1, :K].all() and 0 < s[3, :K].mean() < 1


def test_restated_dispatch_reaches_every_compiled_form():
    seen, forms = set(), set()
    for N in pr.REAL_N:
        for K in pr.REAL_K:
            for M in pr.REAL_M:
                f = pr.form(M, K, N, N + 4)
                forms.add(f)
                if f == "bf3":
                    seen.add((pr.pick_tiling(N)[0], pr.ksb(K)))
    assert sorted(seen) == sorted(pr.BF3_INSTANCES) and {"f32mfma", "plain", "unsupported"} <= forms
    assert pr.form(64, 192, 224, 224) != "bf3" and (2, 6) not in pr.BF3_INSTANCES   # TPW KSB = 12, not instantiated
    assert pr.form(64, 193, 64, 64) == "unsupported"                                 # 13 chunks of 16
    assert pr.form(64, 191, 64, 64) == "f32mfma" and pr.form(64, 38, 64, 64, 4) == "f32mfma" and pr.form(64, 38, 64, 64, 8) == "bf3"
    assert pr.form(33, 38, 64, 64) == "plain" and pr.form(65, 38, 62, 64) == "plain" and pr.form(65, 38, 64, 66) == "plain"
    assert pr.form(64, 192, 320, 320) == "plain"  # the fp32 fast kernel's two x tiles and 324-float rows exceed its LDS budget
    for name, (M, K, N) in pr.SMALLEST.items():
        assert pr.form(M, K, N, N) == name
    assert all(pr.form(M, K, N, N + 4) == "f32mfma" for N, K in pr.F32MFMA_NK for M in (65, 209))
    assert pr.form(65, 191, 224, 224) == "plain" and pr.form(65, 159, 320, 320) == "plain"  # ... and the next wider ones do not
    assert pr.multi_ok(64, 38, 64, 64) and not pr.multi_ok(64, 38, 320, 320) and not pr.multi_ok(64, 39, 64, 64)
    sf = {pr.spike_form(M, K, N, N) for K in pr.SPIKE_K for N in pr.SPIKE_N for M in (47, 209)}
    assert sf == {"fast", "generic"}
    assert pr.spike_form(209, 64, 64, 64, 4) == "generic" and pr.spike_form(209, 64, 64, 64, 2) == "invalid"
    assert pr.spike_form(209, 64, 6, 8) == "generic" and pr.spike_form(209, 321, 64, 64) == "unsupported"
    # a single launch wraps (a workgroup takes a second tile) at the shapes the GPU file uses
    for n_cu in (64, 256, 304):
        assert pr.grid("bf3", 64 * (n_cu + 3) + 5, 64, n_cu) == n_cu < n_cu + 4
        assert pr.grid("fast", 64 * (2 * n_cu + 3) + 5, 64, n_cu) == 2 * n_cu and pr.grid("fast", 64 * (n_cu + 3) + 5, 192, n_cu) == n_cu
        assert pr.grid("f32mfma", 64 * (pr.F32_GRID_CAP + 3) + 5, 64, n_cu) == pr.F32_GRID_CAP
    assert pr.deal_blocks([3.0, 1.0], [100, 100], 8) == [6, 2] and pr.deal_blocks([1e9, 1.0], [3, 9], 256) == [3, 1]


def test_case_generators_stay_in_the_stated_domain():
    for M, K, N in HOST_REAL:
        for name in pr.REAL_CASES:
            c = pr.real_case(name, M, K, N)
            assert c["x"].shape == (M, K) and c["w"].shape == (N, K) and c["x"].dtype == np.float32, (name, M, K, N)
            assert pr.in_domain(c), (name, M, K, N)
            if name.startswith("one_hot"):
                assert ((c["x"] != 0).sum(1) == 1).all() and (c["w"] != 0).all()
                assert np.array_equal(np.nonzero(c["x"])[1], np.arange(M) % K)
    assert (pr.real_case("row_scales", 65, 38, 64)["w"][7] == 0).all() and pr.real_case("no_bias", 65, 38, 64)["b"] is None
    c = pr.real_case("cancel", 65, 38, 64)
    z, _ = _real(c, "f32")
    a = np.abs(c["x"].astype(np.float64)) @ np.abs(c["w"].astype(np.float64)).T
    assert (np.abs(z) < a * 2.0 ** -11).all()  # the sum all but cancels
    bad = dict(c, x=c["x"] * np.float32(2.0 ** -70))
    assert not pr.in_domain(bad)


def test_emulations_are_inside_every_bound_on_every_case():
    """The bf3 emulation under the "x" bound; the correctly rounded k-ordered fp32 chain under the "x32" bound AND under the "x" bound
    (which is wider for every n >= 1): all of them through prodref.check on a buffer with a gap."""
    worst = dict(bf3=0.0, f32=0.0, f32_under_bf3=0.0)
    for M, K, N in HOST_REAL:
        for name in pr.REAL_CASES:
            c = pr.real_case(name, M, K, N)
            for em, kind, key in ((pr.emulate_bf3, "bf3", "bf3"), (pr.emulate_f32, "f32", "f32"), (pr.emulate_f32, "bf3", "f32_under_bf3")):
                z, tol = _real(c, kind)
                assert np.isfinite(z).all() and np.isfinite(tol).all()
                ok, why, r = pr.check(pr.lay_out(em(c["x"], c["w"], c["b"]), M + 2, N + 4), M, N, z, tol)
                assert ok, (name, M, K, N, key, why)
                worst[key] = max(worst[key], r)
    print("worst error/tolerance of the emulations:", {k: round(v, 3) for k, v in worst.items()})
    assert worst["f32"] <= 0.5  # a correctly rounded evaluation uses at most half of a 2u-per-rounding count


# the case that must reject each wrong variant at the smallest bf3 shape (M = 65: one full tile and a one-row second tile)
REAL_MUTANT_CASE = dict(drop_x1w1="control", drop_x1w2="one_hot_x8", drop_x2w1="one_hot_w8", drop_x1w3="one_hot_x8", drop_x2w2="one_hot_16",
                        drop_x3w1="one_hot_w8", trunc_split="one_hot_edge", no_bias="control", zero_last_kstep="one_hot_x8",
                        last_row_repeat="one_hot_16", stale_tile="one_hot_x8", pitch_n="control")


@pytest.mark.parametrize("mut", pr.REAL_MUTANTS)
def test_real_mutants_are_rejected_on_their_named_case(mut):
    M, K, N = pr.SMALLEST["bf3"]
    c = pr.real_case(REAL_MUTANT_CASE[mut], M, K, N)
    z, tol = _real(c, "bf3")
    ok, why, r = pr.check(pr.lay_out(pr.emulate_bf3(c["x"], c["w"], c["b"], mut), M + 2, N + 4, mut), M, N, z, tol)
    print(f"{mut}: rejected on {c['name']} ({why})")
    assert not ok, (mut, r)


@pytest.mark.parametrize("mut", ["no_bias", "last_row_repeat", "stale_tile", "pitch_n"])
def test_fp32_form_mutants_are_rejected(mut):
    M, K, N = pr.SMALLEST["f32mfma"]
    c = pr.real_case(REAL_MUTANT_CASE[mut], M, K, N)
    z, tol = _real(c, "f32")
    ok, why, r = pr.check(pr.lay_out(pr.emulate_f32(c["x"], c["w"], c["b"], mut), M + 2, N + 4, mut), M, N, z, tol)
    assert not ok, (mut, r)


def test_stale_tile_is_rejected_by_control_with_several_workgroups():
    """The wrap shapes of the GPU file in small: nblk workgroups, rows of the second pass take the rows 64 nblk before them; the control
    case draws every tile from its own generator."""
    M, K, N = 64 * 5 + 5, 38, 64
    for name in ("control", "one_hot_w8"):
        c = pr.real_case(name, M, K, N)
        z, tol = _real(c, "bf3")
        assert pr.check(pr.lay_out(pr.emulate_bf3(c["x"], c["w"], c["b"]), M, N), M, N, z, tol)[0]
        assert not pr.check(pr.lay_out(pr.emulate_bf3(c["x"], c["w"], c["b"], "stale_tile", 2), M, N), M, N, z, tol)[0], name


SPIKE_MUTANT_CASE = dict(drop_d0="control", wrap31="saturated", stale_tile="control", pitch_n="control")


def _spike_check(c, y, M, N, mut=None):
    ref = pr.spike_reference(c["s"], c["w"], c["b"], c["bits"])
    return pr.check(pr.lay_out(y, M + 2, N + 4, mut), M, N, ref["y"], ref["tol"], ref["every"], ref["want"]) + (ref,)


@pytest.mark.parametrize("bits", [24, 16])
def test_spike_emulation_is_inside_the_reference_and_mutants_are_not(bits):
    M, K, N = HOST_SPIKE
    worst, inexact = 0.0, 0
    for name in pr.SPIKE_CASES:
        c = pr.spike_case(name, M, K, N, bits)
        ok, why, r, ref = _spike_check(c, pr.emulate_spike(c["s"], c["w"], c["b"], bits), M, N)
        assert ok, (name, bits, why)
        worst, inexact = max(worst, r), inexact + int((~ref["exact"]).sum())
        if name == "saturated":
            assert ref["smax"] >= 2 ** 30 and not ref["exact"].all() and ref["exact"].any()
    print(f"spike emulation, {bits} bits: worst error/tolerance {worst:.3f}; {inexact} results with |S| >= 2^24 are held by the bound")
    assert inexact > 0
    for mut in pr.SPIKE_MUTANTS:
        if mut == "drop_d0" and bits == 16:
            continue  # the low digit plane of 16-bit weights is zero: nothing to drop
        c = pr.spike_case(SPIKE_MUTANT_CASE[mut], M, K, N, bits)
        ok, why, r, _ = _spike_check(c, pr.emulate_spike(c["s"], c["w"], c["b"], bits, mut), M, N, mut)
        print(f"{mut}: rejected on {c['name']} ({why})")
        assert not ok, (mut, bits, r)
