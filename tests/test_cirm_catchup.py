"""``FullbandStreamingSession.catch_up`` / ``catch_up_wave`` with ``sfsn_fullband_hop_seed`` / ``sfsn_fullband_hop_advance``: a backlog of
N frames on clips of a running cIRM-GSN session goes through the offline kernels, started from the state the session carries, and the
end state comes back -- the session is where ``N / hop`` calls of ``step`` (``c`` calls of ``step_wave``) would have left it.

Every comparison is ``torch.equal``: against a control session that only steps, against ``forward_stft`` on the concatenation, and
``export_state`` of both sessions section by section, layer 0 included -- the hop is bit-identical to the offline sequence
(include/sfsn.h), so there is no reservation and no tolerance.  The recipe's deep filter reaches back D = 2 frames: the backlogs run
over N < D, N = D, N > D and 16, after 0, 5 and 6 launches (a fresh clip and both launch parities)."""
import ctypes

import numpy as np
import pytest
import torch

from test_cirm_streaming import TINY, _spectrum, model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F129 = dict(TINY, n_fft=256, hop_length=64, win_length=256, input_size=129, proj_size=129)  # 256-point frames: the graph tier only
MODES = {"one_launch": (TINY, dict(one_launch=True)), "counted": (TINY, dict(one_launch=True, count_spikes=True)),
         "graph": (TINY, dict(one_launch=False)), "graph_counted": (TINY, dict(one_launch=False, count_spikes=True)),
         "graph_f129": (F129, dict(one_launch=False))}
D = TINY["df_order"] - 1
K_FIRST, MORE = (0, 5, 6), 4


def backlogs(hop):
    """hop, D - 1 and D + 1 at the nearest positive multiple of hop (away from D), D, 16."""
    up = lambda n: -(-n // hop) * hop  # noqa: E731
    return sorted({hop, max((D - 1) // hop * hop, hop), up(D), up(D + 1), 16})


def session(mode, B, hop=1):
    kw, skw = MODES[mode]
    s = model(**kw).streaming(batch=B, hop=hop, **skw)
    assert s.one_launch is skw["one_launch"] and (s.one_launch or s._graph is not None)
    return s


def real(x):
    return torch.view_as_real(x) if x.is_complex() else x


def steps(sess, X, t0, t1, rows=None):
    """Step frames [t0, t1) of X -> (enh [.., t1 - t0] as real, mag); rows: [(clip of X, its first frame)] per session clip."""
    hop, outs = sess.hop, []
    for j, t in enumerate(range(t0, t1, hop)):
        if rows is None:
            x = X[:, :, t:t + hop]
        else:
            x = torch.stack([X[b, :, tb + j * hop:tb + (j + 1) * hop] for b, tb in rows])
        outs.append(sess.step(x.contiguous()))
    if not outs:
        return None
    return torch.cat([real(o[0]) for o in outs], -2), (None if outs[0][1] is None else torch.cat([o[1] for o in outs], -1))


def cat(parts):
    parts = [p for p in parts if p is not None]
    return torch.cat([p[0] for p in parts], -2), (None if parts[0][1] is None else torch.cat([p[1] for p in parts], -1))


def as_pair(out):
    return real(out[0]), out[1]


def same(a, b):
    return torch.equal(a[0], b[0]) and (a[1] is None) == (b[1] is None) and (a[1] is None or torch.equal(a[1], b[1]))


def cut(pair, t0, t1, clips=None):
    e, m = pair
    if clips is not None:
        e, m = e[clips], (None if m is None else m[clips])
    return e[..., t0:t1, :], (None if m is None else m[..., t0:t1])


def counts(summary):
    return [int(x.count) for x in summary[1:-1]]


def same_export(a, b, where):
    sa, sb = a.export_state(), b.export_state()
    assert sa.layout == sb.layout and sa.frames.tolist() == sb.frames.tolist(), where
    assert (sa.calls is None) == (sb.calls is None) and (sa.calls is None or sa.calls.tolist() == sb.calls.tolist()), where
    for name, lo, hi in sa.layout:
        assert torch.equal(sa.blob[:, lo:hi], sb.blob[:, lo:hi]), f"{where}: section {name}"
    return [name for name, _, _ in sa.layout]


_REF = {}


def reference(mode, B, hop, T, seed):
    """(spectrum, what a session that only steps returns for it); computed once per key, left unchanged; checked against the
    offline forward of the whole spectrum."""
    key = (mode, B, hop, T, seed)
    if key not in _REF:
        kw, _ = MODES[mode]
        X = _spectrum(B, kw["input_size"], T, seed)
        sess = session(mode, B, hop)
        out = steps(sess, X, 0, T)
        sess.check_errors()
        off = model(**kw).engine().forward_stft(X)
        assert same(out, (real(off["enh_stft"]), off["enh_mag"])) and float(out[0].abs().max()) > 0
        _REF[key] = (X, out)
    return _REF[key]


# ---- 1. step, catch up, step: against a control that only steps (and, through it, the offline forward) -------------------------
@pytest.mark.parametrize("hop", [1, 2])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_step_catch_up_step_equals_stepping_and_offline(mode, B, hop):
    Ns = backlogs(hop)
    assert Ns[0] == hop and 16 in Ns and D in Ns and any(D < N < 16 for N in Ns) and (hop > 1 or D - 1 in Ns)
    T = (max(K_FIRST) + MORE) * hop + max(Ns)
    X, C = reference(mode, B, hop, T, 31 + B)
    sess, ctl = session(mode, B, hop), session(mode, B, hop)
    for k in K_FIRST:
        for N in Ns:
            where = f"{k} launches, N = {N}"
            t0, t1 = k * hop, k * hop + N
            t2 = t1 + MORE * hop
            sess.reset()
            head = steps(sess, X, 0, t0)
            got = as_pair(sess.catch_up(X[:, :, t0:t1]))
            assert got[0].shape == C[0][..., t0:t1, :].shape and same(got, cut(C, t0, t1)), where
            assert sess.clip_frames().tolist() == [t1] * B, where
            tail = steps(sess, X, t1, t2)
            sess.check_errors()
            assert same(cat([head, got, tail]), cut(C, 0, t2)), where
            ctl.reset()
            steps(ctl, X, 0, t2)
            assert sess.clip_frames().tolist() == ctl.clip_frames().tolist() == [t2] * B, where
            names = same_export(sess, ctl, where)
            assert {"l0.h", "l0.c", "l2.c", "hist"} <= set(names) and (("slots" in names or "rows" in names) == ("counted" in mode))
            if "counted" in mode:
                for b in range(B):
                    assert counts(sess.spike_summary([b])) == counts(ctl.spike_summary([b])), where
                assert sum(counts(sess.spike_summary())) > 0
    ctl.check_errors()


# ---- 2. one clip of three catches up while the others step; any order of clips; the launch counter about to wrap ---------------
@pytest.mark.parametrize("hop,wrap", [(1, 0), (1, 2 ** 32 - 3), (2, 2 ** 32 - 3), (1, 2 ** 31 - 2)])
def test_one_clip_catches_up_while_the_others_step(hop, wrap):
    B, n0, N, n1 = 3, 5, 8, 6
    T = (n0 + n1) * hop + N + 10
    X, C = reference("counted", B, hop, T, 41)
    sess = session("counted", B, hop)
    if wrap:  # the launch counter about to wrap, or the origins at the edge of the int32 the session's tensor holds them in
        sess._hop["desc"].launch_index = wrap
        sess._hop["origin"].fill_(sess._as_i32(wrap))
    t1 = n0 * hop
    assert same(steps(sess, X, 0, t1), cut(C, 0, t1))
    got = as_pair(sess.catch_up(X[1:2, :, t1:t1 + N], clips=[1]))
    assert same(got, cut(C, t1, t1 + N, [1]))
    assert sess.clip_frames().tolist() == [t1, t1 + N, t1]
    out = steps(sess, X, 0, n1 * hop, rows=[(0, t1), (1, t1 + N), (2, t1)])
    t2 = t1 + n1 * hop
    assert same(cut(out, 0, None, [0, 2]), cut(C, t1, t2, [0, 2])) and same(cut(out, 0, None, [1]), cut(C, t1 + N, t2 + N, [1]))
    # clips in another order take their own rows: clips 2 and 0 catch up with clip 1
    got = as_pair(sess.catch_up(X[[2, 0], :, t2:t2 + N], clips=[2, 0]))
    assert same(got, cut(C, t2, t2 + N, [2, 0]))
    assert sess.clip_frames().tolist() == [t2 + N] * 3
    out = steps(sess, X, t2 + N, t2 + N + 2 * hop)
    sess.check_errors()
    assert same(out, cut(C, t2 + N, t2 + N + 2 * hop))
    ctl = session("counted", B, hop)
    steps(ctl, X, 0, t2 + N + 2 * hop)
    same_export(sess, ctl, "after both backlogs")
    for b in range(B):
        assert counts(sess.spike_summary([b])) == counts(ctl.spike_summary([b]))


@pytest.mark.parametrize("mode", ["graph", "graph_counted"])
def test_clips_in_any_order_in_the_per_kernel_tier(mode):
    B, N = 3, 5
    X, C = reference(mode, B, 1, 20, 43)
    sess = session(mode, B)
    steps(sess, X, 0, 4)
    got = as_pair(sess.catch_up(X[[2, 0], :, 4:4 + N], clips=[2, 0]))
    assert same(got, cut(C, 4, 4 + N, [2, 0]))
    out = steps(sess, X, 0, 3, rows=[(0, 4 + N), (1, 4), (2, 4 + N)])
    sess.check_errors()
    assert same(cut(out, 0, None, [0, 2]), cut(C, 4 + N, 7 + N, [0, 2])) and same(cut(out, 0, None, [1]), cut(C, 4, 7, [1]))
    assert sess.clip_frames().tolist() == [7 + N, 7, 7 + N]


def test_the_per_kernel_tier_launched_eagerly():
    B, k, N = 3, 5, 7
    X, C = reference("graph_counted", B, 1, 20, 43)
    m = model(**TINY)
    sess, ctl = (m.streaming(batch=B, one_launch=False, graph=False, count_spikes=True) for _ in range(2))
    assert sess._hop is None and sess._graph is None
    got = cat([steps(sess, X, 0, k), as_pair(sess.catch_up(X[:, :, k:k + N])), steps(sess, X, k + N, k + N + MORE)])
    sess.check_errors()
    assert same(got, cut(C, 0, k + N + MORE))
    steps(ctl, X, 0, k + N + MORE)
    same_export(sess, ctl, "eager")
    assert counts(sess.spike_summary([1])) == counts(ctl.spike_summary([1])) and sess.clip_frames().tolist() == [k + N + MORE] * B


# ---- 3. a restarted clip with stale rows; chunk after chunk ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["counted", "graph_counted"])
def test_a_restarted_clip_catches_up_like_a_fresh_session_and_chunks_equal_one_call(mode):
    B, P = 3, 12
    X, C = reference(mode, B, 1, 20, 44)
    Y, CY = reference(mode, 1, 1, 20, 45)  # another utterance, a session of its own
    sess = session(mode, B)
    steps(sess, X, 0, 6)
    sess.reset(clips=[1])  # (the one-launch tier only moves the origin: the rows still hold the old utterance)
    got = as_pair(sess.catch_up(Y[:, :, :P], clips=[1]))
    assert same(got, cut(CY, 0, P))
    fresh = session(mode, 1)
    assert same(as_pair(fresh.catch_up(Y[:, :, :P])), got)
    assert sess.clip_frames().tolist() == [6, P, 6] and fresh.clip_frames().tolist() == [P]
    chunks = session(mode, 1)
    parts = [as_pair(chunks.catch_up(Y[:, :, a:b])) for a, b in ((0, 5), (5, 6), (6, P))]
    assert same(cat(parts), got)
    for j in range(4):
        x = X[:, :, 6 + j:7 + j].clone()
        x[1] = Y[0, :, P + j:P + j + 1]
        o = as_pair(sess.step(x.contiguous()))
        for other in (fresh, chunks):
            assert same(as_pair(other.step(Y[:, :, P + j:P + j + 1].contiguous())), cut(CY, P + j, P + j + 1)), j
        assert same(cut(o, 0, None, [1]), cut(CY, P + j, P + j + 1)) and same(cut(o, 0, None, [0, 2]), cut(C, 6 + j, 7 + j, [0, 2])), j
    for s in (sess, fresh, chunks):
        s.check_errors()
    same_export(chunks, fresh, "chunks")
    assert counts(sess.spike_summary([1])) == counts(fresh.spike_summary()) == counts(chunks.spike_summary())
    assert sum(counts(fresh.spike_summary())) > 0


# ---- 5. the two launches write the listed clips' rows of the launch-k halves and nothing else -----------------------------------
def test_the_launches_leave_every_other_row_alone():
    from spiking_fullsubnet_amd import _lib
    B, N, Bp, b0, clips = 3, 3, 4, 1, [2, 0]
    sess = session("counted", B)
    X, _ = reference("counted", B, 1, 20, 46)
    steps(sess, X, 0, 5)  # launch_index 5: the next launch reads half 1
    h, eng, L = sess._hop, sess.eng, sess.eng.lib
    Hp, HP8, nl, F, T = eng.Hp, eng.HP8, eng.spec.layers, sess.F, D + N
    par = h["desc"].launch_index & 1
    assert par == 1
    st, work = h["st"], h["work"]
    g = torch.Generator(device="cpu").manual_seed(5)
    # the halves no launch reads next hold a mark of their own, so a write to the wrong half shows
    for l in range(nl):
        st["h"][l][1 - par].fill_(1)
    st["hist"][1 - par].fill_(-3.0)
    watched = dict(scratch=h["scratch"], z0=work["z0"], slots=h["slots"], hist=st["hist"])
    watched.update({f"spikes{l}": work["spikes"][l] for l in range(nl)})
    watched.update({f"h{l}": st["h"][l] for l in range(nl)})
    watched.update({f"c{l}": st["c"][l] for l in range(nl)})
    before = {k: v.clone() for k, v in watched.items()}
    arr = (ctypes.c_int * 2)(*clips)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    f32 = dict(dtype=torch.float32, device=DEV)
    # seed: rows b0, b0 + 1 of tensors of Bp rows
    flat = torch.full((nl, 2, Bp, Hp), 7.0, **f32)
    buf = torch.full((Bp, F, T, 2), 7.0, **f32)
    dst = _lib.FullbandSeedDst()
    dst.Bp, dst.T, dst.b0, dst.stft_ri = Bp, T, b0, buf.data_ptr()
    for l in range(nl):
        dst.layer[l].h, dst.layer[l].c = flat[l, 0].data_ptr(), flat[l, 1].data_ptr()
    assert L.sfsn_fullband_hop_seed(h["ref"], ctypes.c_void_p(h["slots"].data_ptr()), None, arr, 2, ctypes.byref(dst), stream) == 0
    torch.cuda.synchronize()
    for k, v in watched.items():
        assert torch.equal(v, before[k]), f"seed wrote {k}"
    assert bool((flat[:, :, [0, 3]] == 7.0).all()) and bool((buf[[0, 3]] == 7.0).all()) and bool((buf[:, :, D:] == 7.0).all())
    for i, b in enumerate(clips):
        for l in range(nl):
            assert torch.equal(flat[l, 0, b0 + i], st["h"][l][par, b, :Hp].float()) and torch.equal(flat[l, 1, b0 + i], st["c"][l][b])
        assert torch.equal(buf[b0 + i, :, :D], st["hist"][par, b])
    assert float(flat[:, 0, b0:b0 + 2].sum()) > 0 and float(buf[b0:b0 + 2, :, :D].abs().max()) > 0
    # advance: made-up results of N frames
    s8 = [(torch.rand((N, Bp, HP8), generator=g) < 0.4).to(torch.int8).to(DEV) for _ in range(nl)]
    for t in s8:
        t[:, :, Hp:] = 0
    cs = torch.randn((nl, Bp, Hp), generator=g).to(DEV)
    new = torch.randn((Bp, F, T, 2), generator=g).to(DEV)
    src = _lib.FullbandAdvanceSrc()
    src.Bp, src.N, src.b0, src.T, src.stft_ri = Bp, N, b0, T, new.data_ptr()
    for l in range(nl):
        src.layer[l].spikes_i8, src.layer[l].c = s8[l].data_ptr(), cs[l].data_ptr()
    k0 = h["desc"].launch_index
    assert L.sfsn_fullband_hop_advance(h["ref"], ctypes.c_void_p(h["slots"].data_ptr()), None, None, arr, 2, ctypes.byref(src), stream) == 0
    torch.cuda.synchronize()
    assert h["desc"].launch_index == k0
    for k in ["scratch", "z0"] + [f"spikes{l}" for l in range(nl)]:
        assert torch.equal(watched[k], before[k]), f"advance wrote {k}"
    assert torch.equal(st["hist"][1 - par], before["hist"][1 - par]) and torch.equal(st["hist"][par, 1], before["hist"][par, 1])
    slots, slots0 = h["slots"].view(nl, B, Hp // 4), before["slots"].view(nl, B, Hp // 4)
    assert torch.equal(slots[:, 1], slots0[:, 1])
    for l in range(nl):
        assert torch.equal(st["h"][l][1 - par], before[f"h{l}"][1 - par]) and torch.equal(st["h"][l][par, 1], before[f"h{l}"][par, 1])
        assert torch.equal(st["h"][l][par][:, Hp:], before[f"h{l}"][par][:, Hp:])  # (the row's padding is nobody's)
        assert torch.equal(st["c"][l][1], before[f"c{l}"][1])
        for i, b in enumerate(clips):
            assert torch.equal(st["h"][l][par, b, :Hp], s8[l][N - 1, b0 + i, :Hp]) and torch.equal(st["c"][l][b], cs[l, b0 + i])
            add = s8[l][:, b0 + i, :Hp].to(torch.int32).reshape(N, Hp // 4, 4).sum((0, 2), dtype=torch.int32)
            assert torch.equal(slots[l, b], slots0[l, b] + add)
    for i, b in enumerate(clips):
        assert torch.equal(st["hist"][par, b], new[b0 + i, :, T - D:])


# ---- 6. waveform ---------------------------------------------------------------------------------------------------------------------
def samples(B, calls, seed):
    return torch.from_numpy((0.05 * np.random.default_rng(seed).standard_normal((B, 128 * calls))).astype(np.float32)).to(DEV)


def wave_calls(sess, W, c0, c1, rows=None):
    """Calls [c0, c1) -> [B, S, 128 (c1 - c0)] on the device; rows: [(clip of W, its first call)] per session clip."""
    outs = []
    for j, c in enumerate(range(c0, c1)):
        x = W[:, 128 * c:128 * (c + 1)] if rows is None else torch.stack([W[b, 128 * (cb + j):128 * (cb + j + 1)] for b, cb in rows])
        outs.append(sess.step_wave_host(x.cpu()).to(DEV).clone() if sess.host_io else sess.step_wave(x.contiguous()))
    return torch.cat(outs, -1) if outs else None


WAVE_C0, WAVE_C = (0, 1, 2, 5), (1, 2, 3, 4, 9)
_WREF = {}


def wave_reference(B, host, calls, seed):
    key = (B, host, calls, seed)
    if key not in _WREF:
        m = model(**TINY)
        W = samples(B, calls, seed)
        sess = m.streaming(batch=B, waveform=True, host_io=host)
        out = wave_calls(sess, W, 0, calls)
        sess.check_errors()
        _WREF[key] = (W, out)
    return _WREF[key]


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("B", [1, 3])
def test_step_wave_catch_up_wave_step_wave(B, host):
    calls = max(WAVE_C0) + max(WAVE_C) + MORE
    W, C = wave_reference(B, host, calls, 51 + B)
    m = model(**TINY)
    sess, ctl = (m.streaming(batch=B, waveform=True, host_io=host) for _ in range(2))
    for c0 in WAVE_C0:
        for c in WAVE_C:
            where = f"{c0} calls, c = {c}"
            sess.reset()
            head = wave_calls(sess, W, 0, c0)
            r = sess.catch_up_wave(W[:, 128 * c0:128 * (c0 + c)])
            assert r.shape == (B, 1, 128 * c) and r.device.type == "cuda", where
            assert torch.equal(r, C[..., 128 * c0:128 * (c0 + c)]), where
            assert sess.clip_calls().tolist() == [c0 + c] * B and sess.clip_frames().tolist() == [c0 + c - 1] * B, where
            tail = wave_calls(sess, W, c0 + c, c0 + c + MORE)
            sess.check_errors()
            assert torch.equal(torch.cat([x for x in (head, r, tail) if x is not None], -1), C[..., :128 * (c0 + c + MORE)]), where
            ctl.reset()
            wave_calls(ctl, W, 0, c0 + c + MORE)
            names = same_export(sess, ctl, where)
            assert {"wave", "ola", "hist", "l0.c"} <= set(names)
    assert bool(C[..., 384:].any())
    ctl.check_errors()


def test_catch_up_wave_of_one_clip_and_the_two_kinds():
    B, c0, c = 3, 5, 4
    W, C = wave_reference(B, False, 18, 54)
    V, CV = wave_reference(1, False, 18, 55)  # another utterance, a session of its own
    sess = model(**TINY).streaming(batch=B, waveform=True)
    wave_calls(sess, W, 0, c0)
    r = sess.catch_up_wave(W[1:2, 128 * c0:128 * (c0 + c)], clips=[1])
    assert torch.equal(r, C[1:2, :, 128 * c0:128 * (c0 + c)])
    assert sess.clip_calls().tolist() == [c0, c0 + c, c0]
    out = wave_calls(sess, W, 0, 3, rows=[(0, c0), (1, c0 + c), (2, c0)])
    assert torch.equal(out[[0, 2]], C[[0, 2], :, 128 * c0:128 * (c0 + 3)]) and torch.equal(out[1], C[1, :, 128 * (c0 + c):128 * (c0 + c + 3)])
    # clip 2 restarts: it has made no call, the others have -- two kinds, two frame counts
    sess.reset(clips=[2])
    before = sess.clip_calls().tolist()
    with pytest.raises(ValueError, match=r"clip 2\b.*clip 0\b"):
        sess.catch_up_wave(W[:, :256])
    with pytest.raises(ValueError, match=r"clip 2\b.*clip 1\b"):
        sess.catch_up_wave(W[1:3, :256], clips=[1, 2])
    assert sess.clip_calls().tolist() == before
    r = sess.catch_up_wave(V[:, :128 * 6], clips=[2])  # its rows still hold the old utterance
    assert torch.equal(r, CV[..., :128 * 6]) and sess.clip_calls().tolist() == [c0 + 3, c0 + c + 3, 6]
    out = wave_calls(sess, torch.cat([W, V]), 0, 4, rows=[(0, c0 + 3), (1, c0 + c + 3), (3, 6)])
    sess.check_errors()
    assert torch.equal(out[2], CV[0, :, 128 * 6:128 * 10]) and bool(out[2].any())
    assert torch.equal(out[0], C[0, :, 128 * (c0 + 3):128 * (c0 + 7)]) and torch.equal(out[1], C[1, :, 128 * (c0 + c + 3):128 * (c0 + c + 7)])


# ---- 7. coverage edges ---------------------------------------------------------------------------------------------------------------
def _edge(m, B, F, want_one_launch, seed, k=5, N=16):
    X = _spectrum(B, F, k + N + MORE, seed)
    off = m.engine().forward_stft(X)
    want = (real(off["enh_stft"]).clone(), off["enh_mag"].clone())
    sess, ctl = m.streaming(batch=B), m.streaming(batch=B)
    assert sess.one_launch is want_one_launch
    got = cat([steps(sess, X, 0, k), as_pair(sess.catch_up(X[:, :, k:k + N])), steps(sess, X, k + N, k + N + MORE)])
    sess.check_errors()
    m.engine().check_stack_errors()
    assert same(got, want) and float(want[0].abs().max()) > 0
    assert same(steps(ctl, X, 0, k + N + MORE), want)
    same_export(sess, ctl, f"B = {B}")


def test_the_recipe_geometry():
    from test_cirm_gsn import recipe_model
    m = recipe_model()[0].cuda()
    assert m.engine().Hp == 272 and m.engine().spec.layers == 4  # (Hp > 256: the stack launch's input-term workgroups)
    _edge(m, 1, 257, True, 61)


@pytest.mark.parametrize("B,one_launch", [(16, True), (17, False)])
def test_sixteen_clips_in_one_launch_and_seventeen_in_the_per_kernel_tier(B, one_launch):
    _edge(model(**TINY), B, 257, one_launch, 60 + B)


# ---- 8. refusals, each compared with what the sibling raises for the same mistake ---------------------------------------------------
def raised(fn):
    try:
        fn()
    except Exception as e:  # noqa: BLE001
        return type(e)
    return None


def test_refusals_are_the_siblings():
    import primeref as pr
    from test_stream_advance import model_of
    sib = model_of("live_tiny")
    sx = torch.from_numpy(pr.spectra("live_tiny", 3)).to(DEV)
    sw = torch.from_numpy(pr.waves("live_tiny", 3)).to(DEV)
    sib_spec, sib_wave = sib.streaming(batch=3, hop=2), sib.streaming(batch=3, waveform=True)
    sib_wave.step_wave(sw[:, :128].contiguous())
    m = model(**TINY)
    X, W = _spectrum(3, 257, 8, 71), samples(3, 4, 72)
    spec, wave = m.streaming(batch=3, hop=2), m.streaming(batch=3, waveform=True)
    wave.step_wave(W[:, :128].contiguous())
    cases = [  # (what the table says, the sibling's call, ours)
        (RuntimeError, lambda: sib_wave.advance(sx[..., :4]), lambda: wave.catch_up(X[..., :4])),               # wrong mode
        (RuntimeError, lambda: sib_spec.advance_wave(sw[:, :256]), lambda: spec.catch_up_wave(W[:, :256])),
        (RuntimeError, lambda: sib_spec.advance(sx[..., :4].cpu()), lambda: spec.catch_up(X[..., :4].cpu())),    # device
        (RuntimeError, lambda: sib_wave.advance_wave(sw[:, :256].cpu()), lambda: wave.catch_up_wave(W[:, :256].cpu())),
        (RuntimeError, lambda: sib_spec.advance(sx[..., :4].real.contiguous()), lambda: spec.catch_up(X[..., :4].real.contiguous())),  # dtype
        (RuntimeError, lambda: sib_wave.advance_wave(sw[:, :256].double()), lambda: wave.catch_up_wave(W[:, :256].double())),
        (RuntimeError, lambda: sib_spec.advance(sx[:, :100, :4]), lambda: spec.catch_up(X[:, :100, :4])),        # F
        (RuntimeError, lambda: sib_spec.advance(sx[:2, :, :4]), lambda: spec.catch_up(X[:2, :, :4])),            # rows != len(clips)
        (RuntimeError, lambda: sib_spec.advance(sx[:2, :, :4], clips=[1]), lambda: spec.catch_up(X[:2, :, :4], clips=[1])),
        (RuntimeError, lambda: sib_wave.advance_wave(sw[:2, :256]), lambda: wave.catch_up_wave(W[:2, :256])),
        (ValueError, lambda: sib_spec.advance(sx[:2, :, :4], clips=[1, 1]), lambda: spec.catch_up(X[:2, :, :4], clips=[1, 1])),  # duplicates
        (ValueError, lambda: sib_wave.advance_wave(sw[:2, :256], clips=[0, 0]), lambda: wave.catch_up_wave(W[:2, :256], clips=[0, 0])),
        (IndexError, lambda: sib_spec.advance(sx[:1, :, :4], clips=[3]), lambda: spec.catch_up(X[:1, :, :4], clips=[3])),        # out of range
        (IndexError, lambda: sib_wave.advance_wave(sw[:1, :256], clips=[-1]), lambda: wave.catch_up_wave(W[:1, :256], clips=[-1])),
        (TypeError, lambda: sib_spec.advance(sx[:1, :, :4], clips=[0.5]), lambda: spec.catch_up(X[:1, :, :4], clips=[0.5])),     # non-integer
        (TypeError, lambda: sib_wave.advance_wave(sw[:1, :256], clips=[True]), lambda: wave.catch_up_wave(W[:1, :256], clips=[True])),
    ]
    for bad in (3, 1, 0):  # not a multiple of hop; less than a hop; nothing
        cases.append((ValueError, lambda bad=bad: sib_spec.advance(sx[..., :bad]), lambda bad=bad: spec.catch_up(X[..., :bad])))
    for bad in (200, 0):
        cases.append((ValueError, lambda bad=bad: sib_wave.advance_wave(sw[:, :bad]), lambda bad=bad: wave.catch_up_wave(W[:, :bad])))
    for i, (want, theirs, ours) in enumerate(cases):
        assert raised(theirs) is want and raised(ours) is want, (i, want, raised(theirs), raised(ours))
    # nothing above changed the sessions
    assert spec.frames_done == 0 and spec.clip_frames().tolist() == [0, 0, 0] and wave.clip_calls().tolist() == [1, 1, 1]
    for s in (spec, wave, m.streaming(batch=3, one_launch=False), m.streaming(batch=17)):
        for name in ("prime", "prime_wave", "advance", "advance_wave"):  # (pinned by three existing test files)
            assert not hasattr(s, name), name
        assert hasattr(s, "catch_up") and hasattr(s, "catch_up_wave")
    e = as_pair(spec.catch_up(X[..., :4]))
    off = m.engine().forward_stft(X)
    assert torch.equal(e[0], real(off["enh_stft"])[..., :4, :]) and torch.equal(e[1], off["enh_mag"][..., :4])
