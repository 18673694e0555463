"""Streaming the frozen front-end with GIVEN normalisation statistics, the parts that need no GPU: the plan of the one-launch hop
(``sfsn_hop_stages``) accepts ``SFSN_NORM_LAPLACE`` / ``SFSN_NORM_GAUSSIAN`` when the clips' statistics are supplied and plans them
exactly as it plans LayerNorm; ``engine.NormStats`` says what is wrong with statistics it cannot take; the module wrappers refuse
the keyword where the model takes no statistics and name it where the model needs them."""
import ctypes

import pytest
import torch

import refweights as rw

KEEP = ctypes.create_string_buffer(64)
A = (ctypes.addressof(KEEP) + 15) // 16 * 16  # any aligned non-NULL address: the plan never dereferences device pointers


def hop_desc(norm, mu=None, ln_w=None, ln_b=None, B=1, hop=1, waveform=False):
    """The baseline_m geometry (frozen and live share it), every sequence with the given normalisation."""
    from spiking_fullsubnet_amd import _lib
    kw = rw.LIVE_M

    def seq(dst, H, P, nl, lo, n_units, ctr, nbr, ctr_fb, nbr_fb, df, fc):
        dst.n_layers, dst.H, dst.P, dst.df, dst.fc = nl, H, P, df, fc
        dst.feat.lo, dst.feat.n_units, dst.feat.ctr, dst.feat.nbr, dst.feat.ctr_fb, dst.feat.nbr_fb = lo, n_units, ctr, nbr, ctr_fb, nbr_fb
        dst.feat.norm, dst.feat.mu, dst.feat.ln_w, dst.feat.ln_b, dst.feat.ln_eps = norm, mu, ln_w, ln_b, 1e-5
        dst.w_p, dst.w_p_dq, dst.b_p = A, A, A
        for l in range(nl):
            o = dst.layer[l]
            o.w_hh, o.w_hh_dq, o.bias, o.bn_alpha, o.bn_beta, o.c, o.spikes = A, A, A, A, A, A, A
            o.h[0], o.h[1] = A, A
            if l == 0:
                o.w_ih_frag = A
            else:
                o.w_ih, o.w_ih_dq = A, A

    d = _lib.HopDesc()
    seq(d.fb, kw["fb_hidden_size"], kw["fb_proj_size"], kw["fb_num_layers"], 0, 1, kw["fb_input_size"], 0, 0, 0, 0, 0)
    cut, ctr, nbr, df = kw["freq_cutoffs"], kw["center_freq_sizes"], kw["neighbor_freq_sizes"], kw["df_orders"]
    for g in range(3):
        seq(d.sb[g], kw["sb_hidden_size"], 2 * ctr[g] * df[g], kw["sb_num_layers"], cut[g], (cut[g + 1] - cut[g]) // ctr[g], ctr[g], nbr[g],
            ctr[g], 0, df[g], ctr[g])
    d.n_groups, d.B, d.F, d.S, d.hop, d.D, d.fdrc = 3, B, 257, 1, hop, max(df) - 1, 0.5
    d.inp_ri = d.hist_ri = d.enh_ri = d.enh_mag = A
    if waveform:
        d.wave_in = d.wave_state = d.ola_state = d.wave_out = d.window = d.spec_g = d.enh_g = A
    return d


def stages(d):
    from spiking_fullsubnet_amd import _lib
    out = (ctypes.c_int * 128)()
    n = _lib.lib().sfsn_hop_stages(ctypes.byref(d), out, 32)
    return n if n < 0 else [tuple(out[4 * i:4 * i + 4]) for i in range(n)]


@pytest.mark.parametrize("B,hop,waveform", [(1, 1, False), (3, 4, False), (2, 1, True)])
def test_given_statistics_are_planned_like_layernorm(B, hop, waveform):
    from spiking_fullsubnet_amd import _lib
    ln = stages(hop_desc(_lib.NORM_LAYERNORM, ln_w=A, ln_b=A, B=B, hop=hop, waveform=waveform))
    assert isinstance(ln, list) and len(ln) >= 11
    assert stages(hop_desc(_lib.NORM_LAPLACE, mu=A, B=B, hop=hop, waveform=waveform)) == ln
    assert stages(hop_desc(_lib.NORM_GAUSSIAN, mu=A, ln_w=A, B=B, hop=hop, waveform=waveform)) == ln
    if (B, hop, waveform) == (1, 1, False):  # the table tests/test_host_cpu.py pins for LayerNorm
        assert ln == [(0, 0, 0, 3), (0, 1, 3, 3), (1, 0, 6, 2), (2, 0, 8, 2), (3, 0, 10, 2), (1, 1, 12, 2), (2, 1, 14, 2), (3, 1, 16, 2),
                      (1, -1, 18, 1), (2, -1, 19, 1), (3, -1, 20, 1)]


def test_statistics_the_plan_refuses():
    from spiking_fullsubnet_amd import _lib
    assert stages(hop_desc(_lib.NORM_LAPLACE)) == _lib.SFSN_EUNSUPPORTED               # no statistics: the utterance norm is not causal
    assert stages(hop_desc(_lib.NORM_GAUSSIAN, mu=A)) == _lib.SFSN_EINVAL              # the standard deviations are missing
    assert stages(hop_desc(_lib.NORM_GAUSSIAN, ln_w=A)) == _lib.SFSN_EINVAL
    assert stages(hop_desc(_lib.NORM_LAPLACE, mu=A + 2)) == _lib.SFSN_EINVAL           # floats sit on 4-byte boundaries
    assert stages(hop_desc(_lib.NORM_GAUSSIAN, mu=A + 1, ln_w=A)) == _lib.SFSN_EINVAL
    assert stages(hop_desc(_lib.NORM_GAUSSIAN, mu=A, ln_w=A + 2)) == _lib.SFSN_EINVAL
    assert isinstance(stages(hop_desc(_lib.NORM_GAUSSIAN, mu=A + 4, ln_w=A + 8)), list)
    one = hop_desc(_lib.NORM_LAPLACE, mu=A)
    one.sb[1].feat.mu = None  # every sequence needs its own
    assert stages(one) == _lib.SFSN_EUNSUPPORTED


def test_norm_stats_say_what_is_wrong():
    import spiking_fullsubnet_amd as pkg
    from spiking_fullsubnet_amd.engine import NormStats
    lap = pkg.Separator(**rw.FROZEN_TINY)._spec()
    gau = pkg.Separator(**rw.FROZEN_TINY_GAUSS)._spec()
    B, ng = 3, lap.n_groups
    ok = NormStats(torch.ones(B), torch.ones(ng, B))
    ok.validate(lap, B, "cpu")
    okg = NormStats(torch.ones(B), torch.ones(ng, B), torch.ones(B), torch.ones(ng, B))
    okg.validate(gau, B, "cpu")
    with pytest.raises(ValueError, match="mu_fb.*shape"):
        NormStats(torch.ones(B + 1), torch.ones(ng, B)).validate(lap, B, "cpu")
    with pytest.raises(ValueError, match="mu_sb.*shape"):
        NormStats(torch.ones(B), torch.ones(B, ng + 1)).validate(lap, B, "cpu")
    with pytest.raises(ValueError, match="mu_fb.*shape"):
        ok.validate(lap, B - 1, "cpu")
    with pytest.raises(ValueError, match="mu_sb.*float32"):
        NormStats(torch.ones(B), torch.ones(ng, B, dtype=torch.float64)).validate(lap, B, "cpu")
    with pytest.raises(ValueError, match="mu_fb.*cuda:0"):
        ok.validate(lap, B, "cuda:0")
    with pytest.raises(ValueError, match="sd_fb is missing"):
        ok.validate(gau, B, "cpu")
    with pytest.raises(ValueError, match="sd_sb is missing"):
        NormStats(torch.ones(B), torch.ones(ng, B), torch.ones(B)).validate(gau, B, "cpu")
    with pytest.raises(ValueError, match="sd_sb.*shape"):
        NormStats(torch.ones(B), torch.ones(ng, B), torch.ones(B), torch.ones(B)).validate(gau, B, "cpu")
    with pytest.raises(ValueError, match="offline_gaussian_norm"):
        okg.validate(lap, B, "cpu")
    with pytest.raises(ValueError, match="takes no utterance statistics.*LayerNorm"):
        ok.validate(pkg.SpikingFullSubNet(**rw.LIVE_TINY)._spec(), B, "cpu")
    with pytest.raises(ValueError, match="takes no utterance statistics.*cumulative"):
        ok.validate(pkg.Separator(**rw.FROZEN_TINY_CUM)._spec(), B, "cpu")
    # select / to keep the layout: clips along the last axis, in the order asked for
    st = NormStats(torch.arange(3.0), torch.arange(9.0).reshape(3, 3), torch.arange(3.0) + 10, None)
    two = st.select([2, 0])
    assert two.mu_fb.tolist() == [2.0, 0.0] and two.mu_sb.tolist() == [[2.0, 0.0], [5.0, 3.0], [8.0, 6.0]]
    assert two.sd_fb.tolist() == [12.0, 10.0] and two.sd_sb is None
    assert st.select(torch.tensor([1])).mu_sb.shape == (3, 1)
    moved = st.to("cpu")
    assert torch.equal(moved.mu_sb, st.mu_sb) and moved.sd_sb is None


def test_module_wrappers_on_cpu_modules():
    import spiking_fullsubnet_amd as pkg
    from spiking_fullsubnet_amd.engine import NormStats
    ok = NormStats(torch.ones(1), torch.ones(3, 1))
    live = pkg.SpikingFullSubNet(**rw.LIVE_TINY).eval()
    with pytest.raises(ValueError, match="takes no utterance statistics"):
        live.streaming(norm_stats=ok)
    cum = pkg.Separator(**rw.FROZEN_TINY_CUM).eval()
    with pytest.raises(ValueError, match="takes no utterance statistics"):
        cum.streaming(norm_stats=ok)
    with pytest.raises(ValueError, match="computes no utterance statistics"):
        cum.norm_stats(torch.zeros(1, 2048))
    for kw in (rw.FROZEN_TINY, rw.FROZEN_TINY_GAUSS):
        frozen = pkg.Separator(**kw).eval()
        with pytest.raises(NotImplementedError, match="norm_stats"):  # the statistics are what is missing, and the message says so
            frozen.streaming()
        with pytest.raises(RuntimeError, match="no CPU path"):  # with them the session is defined -- on a HIP device
            frozen.streaming(norm_stats=ok)
        with pytest.raises(RuntimeError, match="no CPU path"):
            frozen.norm_stats(torch.zeros(1, 2048))
