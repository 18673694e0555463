"""CPU checks behind tests/test_stream_migrate.py and tests/test_cirm_migrate.py (``export_state`` / ``import_state``,
csrc/sfsn_state.hip): the six entry points are declared and exported without an ABI bump, the per-clip blob sizes are recomputed
here from the layout include/sfsn.h states, every argument refusal is answered before any launch (no call below reaches a device),
and ``ClipState``'s host side: select, parking in host memory, the torch.save round trip and the signature comparison."""
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch

import refweights as rw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sfsn_hop_state_bytes", "sfsn_hop_state_export", "sfsn_hop_state_import", "sfsn_fullband_hop_state_bytes",
         "sfsn_fullband_hop_state_export", "sfsn_fullband_hop_state_import")

_keep = ctypes.create_string_buffer(256)
A = (ctypes.addressof(_keep) + 63) // 64 * 64  # a non-NULL, 64-byte aligned address: nothing below dereferences device pointers


def pad16(n):
    return (n + 15) // 16 * 16


def test_the_entry_points_are_exported_and_declared_without_an_abi_bump():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "sfsn.h")).read()
    nargs = dict(zip(NAMES, (1, 5, 6, 3, 8, 9)))
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
        decl = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl, f"{name} is not declared in sfsn.h"
        assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == len(getattr(L, name).argtypes) == nargs[name], name
    assert re.search(r"#define\s+SFSN_ABI_VERSION\s+21\b", header) and _lib.ABI_VERSION == 21 and L.sfsn_abi_version() == 21


# ---- descriptors the hops' plans accept, built on the host -------------------------------------------------------------------------
def hop_desc(kw, B=3, hop=1, waveform=False, slots=False, cum=False, launch_index=0):
    from spiking_fullsubnet_amd import _lib

    def seq(dst, H, P, nl, lo, n_units, ctr, nbr, ctr_fb, nbr_fb, df, fc):
        dst.n_layers, dst.H, dst.P, dst.df, dst.fc = nl, H, P, df, fc
        dst.feat.lo, dst.feat.n_units, dst.feat.ctr, dst.feat.nbr, dst.feat.ctr_fb, dst.feat.nbr_fb = lo, n_units, ctr, nbr, ctr_fb, nbr_fb
        if cum:
            dst.feat.norm, dst.cum[0], dst.cum[1] = _lib.NORM_CUMLAPLACE, A, A
        else:
            dst.feat.norm, dst.feat.ln_w, dst.feat.ln_b, dst.feat.ln_eps = _lib.NORM_LAYERNORM, A, A, 1e-5
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
    S = kw.get("num_spks", 1)
    seq(d.fb, kw["fb_hidden_size"], kw["fb_proj_size"], kw["fb_num_layers"], 0, 1, kw["fb_input_size"], 0, 0, 0, 0, 0)
    cut, ctr, nbr, df = kw["freq_cutoffs"], kw["center_freq_sizes"], kw["neighbor_freq_sizes"], kw["df_orders"]
    for g in range(3):
        seq(d.sb[g], kw["sb_hidden_size"], 2 * ctr[g] * df[g] * S, kw["sb_num_layers"], cut[g], (cut[g + 1] - cut[g]) // ctr[g], ctr[g], nbr[g],
            ctr[g], 0, df[g], ctr[g])
    d.n_groups, d.B, d.F, d.S, d.hop, d.D, d.fdrc = 3, B, 257, S, hop, max(df) - 1, 0.5
    d.inp_ri = d.hist_ri = d.enh_ri = d.enh_mag = A
    d.launch_index = launch_index
    if waveform:
        d.wave_in = d.wave_state = d.ola_state = d.wave_out = d.window = d.spec_g = d.enh_g = A
    if slots:
        d.spike_slots = A
    return d


def hop_bytes_from_the_header(kw, waveform, slots, cum):
    """include/sfsn.h, "Blob of sfsn_hop_state_export", restated: sections in order, each at the next multiple of 16."""
    S = kw.get("num_spks", 1)
    cut, ctr, df = kw["freq_cutoffs"], kw["center_freq_sizes"], kw["df_orders"]
    seqs = [(1, kw["fb_hidden_size"], kw["fb_num_layers"])] + [((cut[g + 1] - cut[g]) // ctr[g], kw["sb_hidden_size"], kw["sb_num_layers"])
                                                               for g in range(3)]
    off = 0
    for units, H, nl in seqs:
        for _ in range(nl):
            off = pad16(off) + units * H          # h: int8 [units][H]
            off = pad16(off) + units * H * 4      # c: float [units][H]
    if cum:
        for units, _, _ in seqs:
            off = pad16(off) + units * 4
    if slots:
        for units, H, nl in seqs:
            for _ in range(nl):
                off = pad16(off) + units * (H // 4) * 4
    D = max(df) - 1
    fcov = max(cut[g] + (cut[g + 1] - cut[g]) // ctr[g] * ctr[g] for g in range(3))
    if D > 0:
        off = pad16(off) + fcov * D * 8
    if waveform:
        off = pad16(off) + 2048
        off = pad16(off) + S * 2048
    return pad16(off)


@pytest.mark.parametrize("kw", [rw.LIVE_M, rw.LIVE_TINY_2SPK], ids=["baseline_m", "tiny_2spk"])
@pytest.mark.parametrize("waveform,slots,cum", [(False, False, False), (True, False, False), (False, True, False), (False, False, True),
                                                (True, True, True)])
def test_hop_state_bytes_is_the_layout_the_header_states(kw, waveform, slots, cum):
    from spiking_fullsubnet_amd import _lib
    from spiking_fullsubnet_amd.clip_state import hop_sections
    L = _lib.lib()
    want = hop_bytes_from_the_header(kw, waveform, slots, cum)
    for B, k in ((1, 0), (3, 1), (5, 2 ** 32 - 1)):  # per clip: neither the batch nor the launch parity enters
        assert L.sfsn_hop_state_bytes(ctypes.byref(hop_desc(kw, B=B, waveform=waveform, slots=slots, cum=cum, launch_index=k))) == want
    # the session's restatement (ClipState.sections) agrees, and its sections tile the blob without overlap
    cut, ctr, df = kw["freq_cutoffs"], kw["center_freq_sizes"], kw["df_orders"]
    seqs = [("fb", 1, kw["fb_hidden_size"], kw["fb_num_layers"])] + [(f"sb{g}", (cut[g + 1] - cut[g]) // ctr[g], kw["sb_hidden_size"],
                                                                      kw["sb_num_layers"]) for g in range(3)]
    layout, nbytes = hop_sections(seqs, cum, slots, cut[3], max(df) - 1, waveform, kw.get("num_spks", 1))
    assert nbytes == want
    assert all(a % 16 == 0 and a < b for _, a, b in layout) and all(x[2] <= y[1] for x, y in zip(layout, layout[1:])) and layout[-1][2] <= want
    names = [n for n, _, _ in layout]
    assert ("cum" in names) == cum and ("slots" in names) == slots and ("wave" in names) == ("ola" in names) == waveform and "hist" in names


def test_a_descriptor_the_hop_refuses_has_no_state():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    assert L.sfsn_hop_state_bytes(None) == 0
    assert L.sfsn_hop_state_bytes(ctypes.byref(_lib.HopDesc())) == 0
    assert L.sfsn_hop_state_bytes(ctypes.byref(hop_desc(rw.LIVE_M, hop=30))) == 0  # D + hop > 32
    assert L.sfsn_fullband_hop_state_bytes(None, 0, 0) == 0
    assert L.sfsn_fullband_hop_state_bytes(ctypes.byref(_lib.FullbandHopDesc()), 0, 0) == 0
    assert L.sfsn_fullband_hop_state_bytes(ctypes.byref(fullband_desc(F=129)), 0, 0) == 0          # F <= 192: not the hop's
    assert L.sfsn_fullband_hop_state_bytes(ctypes.byref(fullband_desc(F=320)), 0, 1) == 0          # waveform: 257 bins only
    assert L.sfsn_fullband_hop_state_bytes(ctypes.byref(fullband_desc()), 1, 1) == 0               # no counted waveform launch


def fullband_desc(Hp=32, nl=3, F=257, S=1, df=3, B=3, hop=1, launch_index=0):
    from spiking_fullsubnet_amd import _lib
    d = _lib.FullbandHopDesc()
    d.n_layers, d.Hp, d.B, d.F, d.S, d.df, d.hop, d.D, d.act, d.unshared = nl, Hp, B, F, S, df, hop, df - 1, 0, 0
    for l in range(nl):
        o = d.layer[l]
        o.h[0], o.h[1], o.c = A, A, A
    d.hist_ri[0], d.hist_ri[1] = A, A
    d.launch_index = launch_index
    return d


def fullband_bytes_from_the_header(Hp, nl, F, S, df, counted, wave):
    off = 0
    for _ in range(nl):
        off = pad16(off) + Hp        # h: int8 [Hp]
        off = pad16(off) + Hp * 4    # c: float [Hp]
    if counted:
        for _ in range(nl):
            off = pad16(off) + (Hp // 4) * 4
    if df > 1:
        off = pad16(off) + F * (df - 1) * 8
    if wave:
        off = pad16(off) + 2048
        off = pad16(off) + S * 2048
    return pad16(off)


@pytest.mark.parametrize("geo", [dict(Hp=32, nl=3, F=257, S=1, df=3), dict(Hp=272, nl=4, F=257, S=2, df=5), dict(Hp=48, nl=1, F=257, S=1, df=1)],
                         ids=["tiny", "recipe_2spk", "df1"])
@pytest.mark.parametrize("counted,wave", [(0, 0), (1, 0), (0, 1)])
def test_fullband_hop_state_bytes_is_the_layout_the_header_states(geo, counted, wave):
    from spiking_fullsubnet_amd import _lib
    from spiking_fullsubnet_amd.clip_state import fullband_sections
    L = _lib.lib()
    want = fullband_bytes_from_the_header(counted=counted, wave=wave, **geo)
    for B, k in ((1, 0), (16, 3)):
        assert L.sfsn_fullband_hop_state_bytes(ctypes.byref(fullband_desc(B=B, launch_index=k, **geo)), counted, wave) == want
    layout, nbytes = fullband_sections(geo["nl"], geo["Hp"], bool(counted), geo["F"], geo["df"] - 1, bool(wave), geo["S"])
    assert nbytes == want and all(a % 16 == 0 and a < b for _, a, b in layout)
    assert ("hist" in dict((n, 0) for n, _, _ in layout)) == (geo["df"] > 1)


# ---- refusals, all before any launch -------------------------------------------------------------------------------------------------
def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_hop_state_calls_refuse_bad_arguments_before_any_launch():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    EINVAL, EUNSUP = _lib.SFSN_EINVAL, _lib.SFSN_EUNSUPPORTED
    d = ctypes.byref(hop_desc(rw.LIVE_TINY, B=3))

    def both(desc, clips, n, blob, b0=0):
        a = L.sfsn_hop_state_export(desc, clips, n, blob, None) if b0 == 0 else None
        b = L.sfsn_hop_state_import(desc, clips, n, blob, b0, None)
        assert a is None or a == b
        return b

    assert both(None, ints(0), 1, A) == EINVAL
    assert both(d, None, 1, A) == EINVAL
    assert both(d, ints(0), 1, None) == EINVAL
    assert both(d, ints(0), 0, A) == EINVAL
    assert both(d, ints(0), -1, A) == EINVAL
    assert both(d, ints(3), 1, A) == EINVAL               # outside [0, B)
    assert both(d, ints(-1), 1, A) == EINVAL
    assert both(d, ints(0, 2, 0), 3, A) == EINVAL         # listed twice
    assert both(d, ints(0), 1, A, b0=-1) == EINVAL
    for mis in (1, 4, 8):
        assert both(d, ints(0), 1, A + mis) == EINVAL     # the blob is 16-byte aligned
    many = ints(*range(257))
    assert both(ctypes.byref(hop_desc(rw.LIVE_TINY, B=300)), many, 257, A) == EUNSUP      # more than 256 clips: the caller splits
    assert both(ctypes.byref(hop_desc(rw.LIVE_TINY, B=65536)), ints(0), 1, A) == EUNSUP
    assert both(ctypes.byref(_lib.HopDesc()), ints(0), 1, A) == EUNSUP                    # a descriptor the hop refuses
    assert both(ctypes.byref(hop_desc(rw.LIVE_TINY, hop=31)), ints(0), 1, A) == EUNSUP
    bad = hop_desc(rw.LIVE_TINY, B=3)
    bad.fb.layer[0].c = A + 2                                                             # a misaligned state pointer
    assert both(ctypes.byref(bad), ints(0), 1, A) == EINVAL


def test_fullband_hop_state_calls_refuse_bad_arguments_before_any_launch():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    EINVAL, EUNSUP = _lib.SFSN_EINVAL, _lib.SFSN_EUNSUPPORTED
    d = ctypes.byref(fullband_desc(B=3))

    def both(desc, clips, n, blob, b0=0, slots=None, wave=None, ola=None):
        a = L.sfsn_fullband_hop_state_export(desc, slots, wave, ola, clips, n, blob, None) if b0 == 0 else None
        b = L.sfsn_fullband_hop_state_import(desc, slots, wave, ola, clips, n, blob, b0, None)
        assert a is None or a == b
        return b

    assert both(None, ints(0), 1, A) == EINVAL
    assert both(d, None, 1, A) == EINVAL
    assert both(d, ints(0), 1, None) == EINVAL
    assert both(d, ints(0), 0, A) == EINVAL
    assert both(d, ints(3), 1, A) == EINVAL
    assert both(d, ints(-2), 1, A) == EINVAL
    assert both(d, ints(1, 1), 2, A) == EINVAL
    assert both(d, ints(0), 1, A, b0=-1) == EINVAL
    assert both(d, ints(0), 1, A + 8) == EINVAL
    assert both(d, ints(0), 1, A, wave=A) == EINVAL                      # wave_state without ola_state
    assert both(d, ints(0), 1, A, slots=A, wave=A, ola=A) == EUNSUP      # the waveform launch has no counted form
    assert both(ctypes.byref(fullband_desc(B=17)), ints(0), 1, A) == EUNSUP
    assert both(ctypes.byref(fullband_desc(F=129)), ints(0), 1, A) == EUNSUP
    assert both(ctypes.byref(fullband_desc(F=320)), ints(0), 1, A, wave=A, ola=A) == EUNSUP
    bad = fullband_desc(B=3)
    bad.layer[1].h[0] = None
    assert both(ctypes.byref(bad), ints(0), 1, A) == EINVAL


# ---- ClipState on the host ---------------------------------------------------------------------------------------------------------
def hand_made(n=4, nbytes=64, stats=True, calls=True):
    from spiking_fullsubnet_amd import ClipState
    blob = (torch.arange(n * nbytes, dtype=torch.int64) * 7 % 251).to(torch.uint8).view(n, nbytes)
    st = (torch.arange(n, dtype=torch.float32) + 1, torch.arange(3 * n, dtype=torch.float32).view(3, n), None, None) if stats else None
    sig = (("model", "spiking_fullsubnet"), ("tier", "one_launch"), ("hop", 1), ("waveform", calls), ("df", (2, 3, 1)))
    return ClipState(blob, np.arange(n) + 10, (np.arange(n) + 11) if calls else None, st, sig,
                     (("fb.l0.h", 0, 16), ("fb.l0.c", 16, 48), ("hist", 48, 60)))


def same(a, b):
    assert torch.equal(a.blob, b.blob) and a.blob.dtype == torch.uint8
    assert np.array_equal(a.frames, b.frames) and a.frames.dtype == b.frames.dtype == np.int64
    assert (a.calls is None) == (b.calls is None) and (a.calls is None or np.array_equal(a.calls, b.calls))
    assert (a.stats is None) == (b.stats is None)
    if a.stats is not None:
        assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a.stats, b.stats))
    assert a.signature == b.signature and a.layout == b.layout


def test_clip_state_select_park_and_save():
    s = hand_made()
    assert len(s) == 4 and s.sections() == {"fb.l0.h": (0, 16), "fb.l0.c": (16, 48), "hist": (48, 60)}
    t = s.select([2, 0])
    assert len(t) == 2 and torch.equal(t.blob, s.blob[[2, 0]]) and t.frames.tolist() == [12, 10] and t.calls.tolist() == [13, 11]
    assert torch.equal(t.stats[0], torch.tensor([3.0, 1.0])) and torch.equal(t.stats[1], s.stats[1][:, [2, 0]]) and t.stats[2] is None
    assert t.signature == s.signature and t.layout == s.layout
    t.blob.zero_()
    assert int(s.blob.sum()) > 0  # (a copy)
    with pytest.raises(IndexError):
        s.select([4])
    same(s.to("cpu"), s)
    assert s.to("cpu").device.type == "cpu"
    for state in (s, hand_made(stats=False, calls=False)):
        f = io.BytesIO()
        torch.save(state, f)
        f.seek(0)
        back = torch.load(f, weights_only=False)
        assert type(back) is type(state)
        same(back, state)
    with pytest.raises(TypeError):
        type(s)(s.blob.float(), s.frames, None, None, s.signature, s.layout)
    with pytest.raises(ValueError):
        type(s)(s.blob, s.frames[:3], None, None, s.signature, s.layout)


def test_the_signature_comparison_names_the_differing_field():
    s = hand_made()
    s.check_signature(s.signature)
    for field, value in (("hop", 2), ("tier", "per_kernel"), ("waveform", False), ("df", (2, 1, 1)), ("model", "cirm_gsn")):
        other = tuple((k, value if k == field else v) for k, v in s.signature)
        with pytest.raises(ValueError, match=rf"\b{field}\b"):
            s.check_signature(other)
    with pytest.raises(ValueError, match="count_spikes"):
        s.check_signature(s.signature + (("count_spikes", True),))


def test_import_checks_shared_by_the_sessions():
    from spiking_fullsubnet_amd.clip_state import check_import, clip_list
    s = hand_made()
    check_import(s, [0, 1, 2, 3], "cpu")
    with pytest.raises(TypeError):
        check_import(s.blob, [0], "cpu")
    with pytest.raises(RuntimeError, match=r"\.to\("):
        check_import(s, [0, 1, 2, 3], "cuda:0")
    with pytest.raises(RuntimeError, match="4 clips for 2"):
        check_import(s, [0, 1], "cpu")
    assert clip_list(None, 3, "x") == [0, 1, 2] and clip_list(torch.tensor([2, 0]), 3, "x") == [2, 0]
    with pytest.raises(ValueError, match="distinct"):
        clip_list([1, 1], 3, "import_state")
    with pytest.raises(IndexError):
        clip_list([3], 3, "import_state")
    for bad in ([1.0], [True], torch.zeros((1, 1), dtype=torch.long), 5, "01"):
        with pytest.raises(TypeError):
            clip_list(bad, 3, "import_state")
