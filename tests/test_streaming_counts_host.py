"""CPU-only checks of the C ABI behind streaming spike counts: sfsn_hop_desc.spike_slots and its sizing helper, the launch plan
with counting on, and the argument checks of sfsn_spike_count_rows (all of them run before anything touches a device)."""
import ctypes

import numpy as np

import refweights as rw


def hop_desc(B=1, hop=1, waveform=False, kw=rw.LIVE_M):
    """A baseline_m descriptor whose pointers are any non-NULL address (the plan never dereferences device pointers)."""
    from spiking_fullsubnet_amd import _lib
    keep = ctypes.create_string_buffer(64)
    a = ctypes.addressof(keep)

    def seq(dst, H, P, nl, lo, n_units, ctr, nbr, df, fc):
        dst.n_layers, dst.H, dst.P, dst.df, dst.fc = nl, H, P, df, fc
        dst.feat.lo, dst.feat.n_units, dst.feat.ctr, dst.feat.nbr, dst.feat.ctr_fb, dst.feat.nbr_fb = lo, n_units, ctr, nbr, ctr if df else 0, 0
        dst.feat.norm, dst.feat.ln_w, dst.feat.ln_b, dst.feat.ln_eps = _lib.NORM_LAYERNORM, a, a, 1e-5
        dst.w_p, dst.w_p_dq, dst.b_p = a, a, a
        for l in range(nl):
            o = dst.layer[l]
            o.w_hh, o.w_hh_dq, o.bias, o.bn_alpha, o.bn_beta, o.c, o.spikes = a, a, a, a, a, a, a
            o.h[0], o.h[1] = a, a
            if l == 0:
                o.w_ih_frag = a
            else:
                o.w_ih, o.w_ih_dq = a, a

    d = _lib.HopDesc()
    seq(d.fb, kw["fb_hidden_size"], kw["fb_proj_size"], kw["fb_num_layers"], 0, 1, kw["fb_input_size"], 0, 0, 0)
    cut, ctr, nbr, df = kw["freq_cutoffs"], kw["center_freq_sizes"], kw["neighbor_freq_sizes"], kw["df_orders"]
    units = []
    for g in range(3):
        units.append((cut[g + 1] - cut[g]) // ctr[g])
        seq(d.sb[g], kw["sb_hidden_size"], 2 * ctr[g] * df[g], kw["sb_num_layers"], cut[g], units[-1], ctr[g], nbr[g], df[g], ctr[g])
    d.n_groups, d.B, d.F, d.S, d.hop, d.D, d.fdrc = 3, B, 257, 1, hop, max(df) - 1, 0.5
    d.inp_ri = d.hist_ri = d.enh_ri = d.enh_mag = a
    if waveform:
        d.wave_in = d.wave_state = d.ola_state = d.wave_out = d.window = d.spec_g = d.enh_g = a
    d._keep = keep
    return d, units


def test_hop_desc_appends_spike_slots_and_sizes_them():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    names = [f[0] for f in _lib.HopDesc._fields_]
    assert names[-2:] == ["clip_start", "spike_slots"]  # appended: every earlier field keeps its offset
    assert _lib.HopDesc.spike_slots.offset > _lib.HopDesc.clip_start.offset
    assert _lib.ABI_VERSION == 21 == L.sfsn_abi_version()
    kw = rw.LIVE_M
    for B, hop in ((1, 1), (3, 1), (5, 4)):
        d, units = hop_desc(B, hop)
        want = kw["fb_num_layers"] * B * kw["fb_hidden_size"] // 4 + \
            sum(kw["sb_num_layers"] * B * u * kw["sb_hidden_size"] // 4 for u in units)
        assert L.sfsn_hop_spike_slots(ctypes.byref(d)) == want
        d.spike_slots = ctypes.addressof(d._keep)
        assert L.sfsn_hop_spike_slots(ctypes.byref(d)) == want  # (the pointer does not change the layout)
    bad, _ = hop_desc(hop=30)  # a descriptor the launch refuses has no slots
    assert L.sfsn_hop_spike_slots(ctypes.byref(bad)) == 0
    assert L.sfsn_hop_spike_slots(None) == 0


def test_stream_hop_plan_is_unchanged_with_counting_on():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    out = (ctypes.c_int * 128)()
    for waveform in (False, True):
        d, _ = hop_desc(waveform=waveform)
        n0 = L.sfsn_hop_stages(ctypes.byref(d), out, 32)
        plain = [tuple(out[4 * i:4 * i + 4]) for i in range(n0)]
        slots = (ctypes.c_uint * 64)()
        d.spike_slots = ctypes.addressof(slots)
        n = L.sfsn_hop_stages(ctypes.byref(d), out, 32)
        assert [tuple(out[4 * i:4 * i + 4]) for i in range(n)] == plain
        if not waveform:  # the plan test_host_cpu pins for baseline_m at B = 1
            assert plain == [(0, 0, 0, 3), (0, 1, 3, 3), (1, 0, 6, 2), (2, 0, 8, 2), (3, 0, 10, 2), (1, 1, 12, 2), (2, 1, 14, 2),
                             (3, 1, 16, 2), (1, -1, 18, 1), (2, -1, 19, 1), (3, -1, 20, 1)]
        else:
            assert n == 13 and plain[1] == (0, -2, 3, 1) and plain[-1] == (0, -3, 22, 1)


def test_spike_count_rows_rejects_bad_arguments():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    buf = np.zeros(4096 + 64, dtype=np.int8)
    base = (buf.ctypes.data + 15) // 16 * 16
    cnt = np.zeros(16, dtype=np.uint64)

    def job(**kw):
        j = _lib.RowCount()
        j.spikes_i8, j.T, j.R, j.HP, j.rows_per_clip, j.counts = base, 4, 4, 64, 2, cnt.ctypes.data
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def call(jobs, t0=1, nt=2, n=None):
        arr = (_lib.RowCount * max(len(jobs), 1))(*jobs)
        return L.sfsn_spike_count_rows(arr, len(jobs) if n is None else n, t0, nt, None)

    E = _lib.SFSN_EINVAL
    assert L.sfsn_spike_count_rows(None, 1, 0, 1, None) == E
    assert call([job()], n=0) == E
    assert call([job()] * 17) == E                       # more than SFSN_MAX_COUNT_TENSORS
    assert call([job()], t0=-1) == E
    assert call([job()], nt=0) == E
    assert call([job()], t0=3, nt=2) == E                # frames beyond T
    assert call([job(spikes_i8=None)]) == E
    assert call([job(counts=None)]) == E
    assert call([job(R=0)]) == E
    assert call([job(T=0)]) == E
    assert call([job(HP=0)]) == E
    assert call([job(HP=40)]) == E                       # not a whole number of 16-byte vectors
    assert call([job(rows_per_clip=0)]) == E
    assert call([job(R=5)]) == E                         # ragged: R % rows_per_clip != 0
    assert call([job(spikes_i8=base + 4)]) == E          # misaligned
    assert call([job(), job(HP=40)]) == E                # any bad tensor refuses the whole launch
    assert not cnt.any()                                 # nothing was written
