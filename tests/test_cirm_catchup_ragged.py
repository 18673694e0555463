"""``FullbandStreamingSession.catch_up_ragged`` / ``catch_up_wave_ragged`` with ``sfsn_fullband_hop_advance_ragged``: one call takes a
backlog of ITS OWN length per clip and returns, and leaves behind, exactly what the single-clip ``catch_up`` / ``catch_up_wave`` calls
would have.

Two sessions with the same past: one makes the ragged call, the other one single-clip call per clip.  Every comparison is
``torch.equal`` -- the results over each clip's own frames (zeros past them, NaN in the caller's padding), ``clip_frames()`` /
``clip_calls()``, the spike counts, ``export_state`` section by section, and three more launches behind the call -- in both tiers,
layer 0 included: the hop is bit-identical to the offline sequence (include/sfsn.h), so there is no reservation and no tolerance.  The
stepping-only references of tests/test_cirm_catchup.py are compared too."""
import ctypes
import functools

import pytest
import torch

from test_cirm_catchup import D, DEV, MODES, as_pair, counts, cut, reference, same, same_export, session, steps, wave_calls, wave_reference
from test_cirm_streaming import TINY, _spectrum, model

pytestmark = pytest.mark.gpu

NAN = complex(float("nan"), float("nan"))
MORE = 3
T_REF = {1: 80, 2: 64}  # frames of the stepping-only references (shared by the tests of a mode and hop)


def nan_padded(X, clips, starts, lens, Nmax):
    """Row i: clips[i]'s frames [starts[i], starts[i] + lens[i]) of X, NaN behind them up to Nmax."""
    rows = torch.full((len(clips), X.shape[1], Nmax), NAN, dtype=X.dtype, device=X.device)
    for i, (c, t, n) in enumerate(zip(clips, starts, lens)):
        rows[i, :, :n] = X[c, :, t:t + n]
    return rows


def ragged_and_singles(rag, one, X, clips, starts, lens, Nmax, where):
    """The ragged call on ``rag``, the single-clip calls on ``one``; the results compared.  Returns the ragged call's."""
    got = as_pair(rag.catch_up_ragged(nan_padded(X, clips, starts, lens, Nmax), lens, clips=clips))
    assert got[0].shape[0] == len(clips) and got[0].shape[-2] == Nmax and (got[1] is None or got[1].shape[-1] == Nmax), where
    for i, (c, t, n) in enumerate(zip(clips, starts, lens)):
        single = as_pair(one.catch_up(X[c:c + 1, :, t:t + n].contiguous(), clips=[c]))
        assert same(cut(got, 0, n, [i]), single), f"{where}: clip {c}, its {n} frames"
        tail = cut(got, n, Nmax, [i])
        assert not bool(tail[0].any()) and (tail[1] is None or not bool(tail[1].any())), f"{where}: clip {c}, past its frames"
    assert float(got[0].abs().max()) > 0
    return got


def agree(rag, one, where, counted):
    assert rag.clip_frames().tolist() == one.clip_frames().tolist(), where
    names = same_export(rag, one, where)
    assert {"l0.h", "l0.c", "hist"} <= set(names) and (("slots" in names or "rows" in names) == counted), where
    if counted:
        for b in range(rag.B):
            assert counts(rag.spike_summary([b])) == counts(one.spike_summary([b])), f"{where}: counts of clip {b}"


def more_steps(rag, one, X, pos, where):
    """MORE launches on both sessions, clip b continuing at frame pos[b] of X's row b; returns what they gave."""
    rows = [(b, p) for b, p in enumerate(pos)]
    a, b = steps(rag, X, 0, MORE * rag.hop, rows=rows), steps(one, X, 0, MORE * one.hop, rows=rows)
    assert same(a, b), f"{where}: {MORE} more launches"
    return a


def full_case(rag, one, mode, X, C, k, clips, lens, Nmax, where):
    """Both sessions from zero: k launches, the backlog on ``clips``, MORE launches; everything compared, the reference included."""
    hop, B = rag.hop, rag.B
    t0 = k * hop
    for s in (rag, one):
        s.reset()
        steps(s, X, 0, t0)
    got = ragged_and_singles(rag, one, X, clips, [t0] * len(clips), lens, Nmax, where)
    for i, (c, n) in enumerate(zip(clips, lens)):
        assert same(cut(got, 0, n, [i]), cut(C, t0, t0 + n, [c])), f"{where}: clip {c} against stepping"
    pos = [t0] * B
    for c, n in zip(clips, lens):
        pos[c] = t0 + n
    assert rag.clip_frames().tolist() == pos, where
    agree(rag, one, where, "counted" in mode)
    out = more_steps(rag, one, X, pos, where)
    for b in range(B):  # (an unlisted clip steps on unchanged)
        assert same(cut(out, 0, None, [b]), cut(C, pos[b], pos[b] + MORE * hop, [b])), f"{where}: clip {b} steps on"
    agree(rag, one, where + ", later", "counted" in mode)
    for s in (rag, one):
        s.check_errors()


# ---- 1. modes and lengths: after 0, 5 and 6 launches, N_b < D, = D, > D together, a permutation, an unlisted clip -----------------
@pytest.mark.parametrize("hop", [1, 2])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_one_ragged_call_equals_the_single_clip_calls(mode, hop):
    B = 3
    X, C = reference(mode, B, hop, T_REF[hop], 131)
    rag, one = session(mode, B, hop), session(mode, B, hop)
    lens = (1, 17, 40) if hop == 1 else (2, 18, 40)
    for k, Nmax in ((0, 40), (5, 40), (6, 44)):  # a fresh clip and both launch parities; rows wider than the longest clip
        full_case(rag, one, mode, X, C, k, [0, 1, 2], list(lens), Nmax, f"{k} launches, {lens}")
    around_d = [1, 2, 3] if hop == 1 else [2, 4, 6]
    assert hop > 1 or (around_d[0] < D == around_d[1] < around_d[2])
    full_case(rag, one, mode, X, C, 5, [0, 1, 2], around_d, max(around_d), f"around D: {around_d}")
    full_case(rag, one, mode, X, C, 6, [2, 0, 1], [lens[1], lens[2], lens[0]], 40, "a permutation of the clips")
    full_case(rag, one, mode, X, C, 5, [2, 0], [lens[1], lens[0]], 24, "clip 1 is not listed")
    if rag._hop is not None:
        assert rag.launches["advance_ragged"] == 6 and rag.launches["seed"] == 6 and "advance" not in rag.launches
        assert one.launches["advance"] == 17 and "advance_ragged" not in one.launches


# ---- 2. the layer-0 input product's form: a clip of 70 frames takes the split product alone, the others do not --------------------
def test_each_clip_takes_the_input_product_its_own_call_takes():
    mode, B = "graph_f129", 3
    X, C = reference(mode, B, 1, T_REF[1], 131)
    rag, one = session(mode, B), session(mode, B)
    before = dict(rag.eng.launches)
    full_case(rag, one, mode, X, C, 5, [0, 1, 2], [1, 17, 70], 70, "(1, 17, 70) at 129 bins")
    ran = {k: v - before.get(k, 0) for k, v in rag.eng.launches.items()}
    assert ran.get("inproj_alone", 0) >= 1 and ran.get("inproj_wide", 0) == 0  # (the rows of the two short clips again, in the fp32 form)


# ---- 3. clip kinds: a restarted clip and a never-stepped clip beside a running one; launch counters at the edges -------------------
@pytest.mark.parametrize("mode,wrap", [("counted", 0), ("counted", 2 ** 32 - 3), ("counted", 2 ** 31 - 2), ("graph_counted", 0)])
def test_a_restarted_and_a_fresh_clip_beside_a_running_one(mode, wrap):
    B, k = 3, 5
    X, C = reference(mode, B, 1, T_REF[1], 131)
    Y, CY = reference(mode, 1, 1, 20, 45)  # another utterance, a session of its own
    XY = torch.cat([X[:, :, :20], Y])      # row 3: the other utterance
    rag, one = session(mode, B), session(mode, B)
    for s in (rag, one):
        if wrap:  # the launch counter about to wrap, or the origins at the edge of the int32 the session's tensor holds them in
            s._hop["desc"].launch_index = wrap
            s._hop["origin"].fill_(s._as_i32(wrap))
        for t in range(k):  # clip 2 is held from the start: it has never stepped
            s.tick(X[:, :, t:t + 1].contiguous(), [0, 1])
        s.reset(clips=[1])  # (the one-launch tier only moves the origin: the rows still hold the old utterance)
        assert s.clip_frames().tolist() == [k, 0, 0]
    # (rows of XY, clips of the session: clip 1 takes the other utterance, clip 2 its own from frame 0)
    rows = nan_padded(XY, [3, 2], [0, 0], [3, 9], 12)
    got = as_pair(rag.catch_up_ragged(rows, [3, 9], clips=[1, 2]))
    singles = [as_pair(one.catch_up(Y[:, :, :3].contiguous(), clips=[1])), as_pair(one.catch_up(X[2:3, :, :9].contiguous(), clips=[2]))]
    assert same(cut(got, 0, 3, [0]), singles[0]) and same(cut(got, 0, 9, [1]), singles[1])
    assert same(singles[0], cut(CY, 0, 3)) and same(singles[1], cut(C, 0, 9, [2]))
    assert not bool(cut(got, 3, 12, [0])[0].any()) and not bool(cut(got, 9, 12, [1])[0].any())
    assert rag.clip_frames().tolist() == [k, 3, 9]
    agree(rag, one, "restarted and fresh", True)
    for j in range(MORE):
        x = torch.stack([X[0, :, k + j:k + j + 1], Y[0, :, 3 + j:4 + j], X[2, :, 9 + j:10 + j]]).contiguous()
        a, b = as_pair(rag.step(x)), as_pair(one.step(x))
        assert same(a, b), j
        assert same(cut(a, 0, None, [0]), cut(C, k + j, k + j + 1, [0])) and same(cut(a, 0, None, [1]), cut(CY, 3 + j, 4 + j))
        assert same(cut(a, 0, None, [2]), cut(C, 9 + j, 10 + j, [2])), j
    agree(rag, one, "restarted and fresh, later", True)
    assert rag.clip_frames().tolist() == [k + MORE, 3 + MORE, 9 + MORE]
    for s in (rag, one):
        s.check_errors()


# ---- 4. equal lengths are catch_up itself, plus padding of the result ---------------------------------------------------------------
@pytest.mark.parametrize("mode", ["one_launch", "graph"])
def test_equal_lengths_delegate_to_catch_up(mode):
    B, k, N, Nmax = 3, 5, 7, 10
    X, C = reference(mode, B, 1, T_REF[1], 131)
    rag, one = session(mode, B), session(mode, B)
    for s in (rag, one):
        steps(s, X, 0, k)
    ran = []
    for s in (rag, one):
        before = (dict(s.launches), dict(s.eng.launches))
        if s is rag:
            got = as_pair(s.catch_up_ragged(nan_padded(X, [0, 1, 2], [k] * 3, [N] * 3, Nmax), [N] * 3))
        else:
            want = as_pair(s.catch_up(X[:, :, k:k + N].contiguous()))
        ran.append([{key: v - b.get(key, 0) for key, v in now.items() if v != b.get(key, 0)} for now, b in zip((s.launches, s.eng.launches), before)])
    assert ran[0] == ran[1] and "advance_ragged" not in ran[0][0] and "layer_scan" not in ran[0][1], ran
    assert same(cut(got, 0, N), want) and got[0].shape[-2] == Nmax and not bool(cut(got, N, Nmax)[0].any()) and not bool(cut(got, N, Nmax)[1].any())
    agree(rag, one, "equal lengths", False)
    more_steps(rag, one, X, [k + N] * B, "equal lengths")


# ---- 5. tiers: 16 clips in one launch, 17 in the per-kernel tier; the recipe geometry -----------------------------------------------
def _listed_of_many(m, B, F, want_one_launch, seed, clips, lens, k=5):
    Nmax = max(lens)
    X = _spectrum(B, F, k + Nmax + MORE, seed)
    rag, one = m.streaming(batch=B), m.streaming(batch=B)
    assert rag.one_launch is want_one_launch
    for s in (rag, one):
        steps(s, X, 0, k)
    ragged_and_singles(rag, one, X, clips, [k] * len(clips), lens, Nmax, f"B = {B}")
    pos = [k] * B
    for c, n in zip(clips, lens):
        pos[c] = k + n
    agree(rag, one, f"B = {B}", False)
    more_steps(rag, one, X, pos, f"B = {B}")
    agree(rag, one, f"B = {B}, later", False)
    for s in (rag, one):
        s.check_errors()


@pytest.mark.parametrize("B,one_launch", [(16, True), (17, False)])
def test_sixteen_clips_in_one_launch_and_seventeen_in_the_per_kernel_tier(B, one_launch):
    _listed_of_many(model(**TINY), B, 257, one_launch, 160 + B, [3, B - 1, 0, 9, 7], [1, 16, 5, 2, 11])


@functools.lru_cache(maxsize=None)
def _recipe():
    from test_cirm_gsn import recipe_model
    return recipe_model()[0].cuda()


def test_the_recipe_geometry():
    m = _recipe()
    assert m.engine().H == 268 and m.engine().Hp == 272 and m.engine().spec.layers == 4
    _listed_of_many(m, 3, 257, True, 161, [0, 1, 2], [3, 8, 16])
    m.engine().check_stack_errors()


# ---- 6. the launch writes the listed clips' rows of the launch-k halves, at each clip's own frame, and nothing else ------------------
def test_the_launch_leaves_every_other_row_alone():
    from spiking_fullsubnet_amd import _lib
    B, Nmax, Bp, b0, clips, lens = 3, 6, 4, 1, [2, 0], [1, 4]
    sess = session("counted", B)
    X, _ = reference("counted", B, 1, T_REF[1], 131)
    steps(sess, X, 0, 5)  # launch_index 5: the next launch reads half 1
    h, eng, L = sess._hop, sess.eng, sess.eng.lib
    Hp, HP8, nl, F, T = eng.Hp, eng.HP8, eng.spec.layers, sess.F, D + Nmax
    par = h["desc"].launch_index & 1
    assert par == 1
    st, work = h["st"], h["work"]
    g = torch.Generator(device="cpu").manual_seed(15)
    for l in range(nl):  # the halves no launch reads next hold a mark of their own, so a write to the wrong half shows
        st["h"][l][1 - par].fill_(1)
    st["hist"][1 - par].fill_(-3.0)
    watched = dict(scratch=h["scratch"], z0=work["z0"], slots=h["slots"], hist=st["hist"], origin=h["origin"])
    watched.update({f"spikes{l}": work["spikes"][l] for l in range(nl)})
    watched.update({f"h{l}": st["h"][l] for l in range(nl)})
    watched.update({f"c{l}": st["c"][l] for l in range(nl)})
    before = {k: v.clone() for k, v in watched.items()}
    s8 = [(torch.rand((Nmax, Bp, HP8), generator=g) < 0.4).to(torch.int8).to(DEV) for _ in range(nl)]
    for t in s8:
        t[:, :, Hp:] = 0
    mem = torch.randn((nl, Nmax, Bp, Hp), generator=g).to(DEV)
    new = torch.randn((Bp, F, T, 2), generator=g).to(DEV)
    mem[:, :, [0, 3]] = float("nan")  # rows of clips that are not listed, and every frame past a clip's own: never read
    new[[0, 3]] = float("nan")
    for i, n in enumerate(lens):
        mem[:, n:, b0 + i] = float("nan")
        new[b0 + i, :, D + n:] = float("nan")
    frames = torch.tensor([-7, lens[0], lens[1], 1000], dtype=torch.int32, device=DEV)  # (rows 0 and 3 are nobody's)
    src = _lib.FullbandAdvanceRaggedSrc()
    src.Bp, src.Nmax, src.b0, src.T, src.frames, src.stft_ri = Bp, Nmax, b0, T, frames.data_ptr(), new.data_ptr()
    for l in range(nl):
        src.layer[l].spikes_i8, src.layer[l].membrane = s8[l].data_ptr(), mem[l].data_ptr()
    arr = (ctypes.c_int * 2)(*clips)
    k0 = h["desc"].launch_index
    rc = L.sfsn_fullband_hop_advance_ragged(h["ref"], ctypes.c_void_p(h["slots"].data_ptr()), None, None, arr, 2, ctypes.byref(src),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert h["desc"].launch_index == k0
    for k in ["scratch", "z0", "origin"] + [f"spikes{l}" for l in range(nl)]:
        assert torch.equal(watched[k], before[k]), f"the launch wrote {k}"
    assert torch.equal(st["hist"][1 - par], before["hist"][1 - par]) and torch.equal(st["hist"][par, 1], before["hist"][par, 1])
    slots, slots0 = h["slots"].view(nl, B, Hp // 4), before["slots"].view(nl, B, Hp // 4)
    assert torch.equal(slots[:, 1], slots0[:, 1])
    for l in range(nl):
        assert torch.equal(st["h"][l][1 - par], before[f"h{l}"][1 - par]) and torch.equal(st["h"][l][par, 1], before[f"h{l}"][par, 1])
        assert torch.equal(st["h"][l][par][:, Hp:], before[f"h{l}"][par][:, Hp:])  # (the row's padding is nobody's)
        assert torch.equal(st["c"][l][1], before[f"c{l}"][1])
        for i, (b, n) in enumerate(zip(clips, lens)):
            assert torch.equal(st["h"][l][par, b, :Hp], s8[l][n - 1, b0 + i, :Hp]) and torch.equal(st["c"][l][b], mem[l, n - 1, b0 + i])
            add = s8[l][:n, b0 + i, :Hp].to(torch.int32).reshape(n, Hp // 4, 4).sum((0, 2), dtype=torch.int32)
            assert torch.equal(slots[l, b], slots0[l, b] + add)
    for i, (b, n) in enumerate(zip(clips, lens)):  # N_b = 1 < D: the tail of the row's history, then the frame
        assert torch.equal(st["hist"][par, b], new[b0 + i, :, n:D + n])
    assert not bool(torch.isnan(st["hist"]).any()) and not any(bool(torch.isnan(c).any()) for c in st["c"])


# ---- 7. waveform sessions: both kinds of clip, host_io, a mixed call -------------------------------------------------------------------
def nan_samples(W, clips, starts, calls, cmax):
    rows = torch.full((len(clips), 128 * cmax), float("nan"), dtype=W.dtype, device=W.device)
    for i, (c, a, n) in enumerate(zip(clips, starts, calls)):
        rows[i, :128 * n] = W[c, 128 * a:128 * (a + n)]
    return rows


@pytest.mark.parametrize("host", [False, True])
def test_catch_up_wave_ragged_for_both_kinds_of_clip(host):
    B, total = 3, 24
    W, C = wave_reference(B, host, total, 154)
    m = model(**TINY)
    rag, one = (m.streaming(batch=B, waveform=True, host_io=host) for _ in range(2))
    # (calls made before, the clips, each clip's calls in the backlog, the width of the rows in calls)
    cases = [(5, [0, 1, 2], [1, 5, 12], 12),  # clips that have made calls
             (4, [2, 0, 1], [5, 12, 1], 13),  # ... in another order, in wider rows
             (1, [0, 1, 2], [1, 5, 12], 12),  # ... one call: no frame yet, and no overlap-add sums
             (0, [0, 1, 2], [1, 2, 9], 9),    # clips without a call: c_b - 1 frames, one of them none at all
             (0, [1, 2, 0], [9, 1, 2], 10),
             (3, [2, 1], [2, 7], 7)]          # clip 0 is not listed
    for c0, clips, calls, cmax in cases:
        where = f"{c0} calls, clips {clips}, {calls}"
        for s in (rag, one):
            s.reset()
            wave_calls(s, W, 0, c0)
        r = rag.catch_up_wave_ragged(nan_samples(W, clips, [c0] * len(clips), calls, cmax), [128 * n for n in calls], clips=clips)
        assert r.shape == (len(clips), 1, 128 * cmax) and r.device.type == "cuda", where
        pos = [c0] * B
        for i, (c, n) in enumerate(zip(clips, calls)):
            single = one.catch_up_wave(W[c:c + 1, 128 * c0:128 * (c0 + n)].contiguous(), clips=[c])
            assert torch.equal(r[i:i + 1, :, :128 * n], single), f"{where}: clip {c}"
            assert torch.equal(single, C[c:c + 1, :, 128 * c0:128 * (c0 + n)]), f"{where}: clip {c} against stepping"
            assert not bool(r[i, :, 128 * n:].any()), f"{where}: clip {c}, past its samples"
            pos[c] = c0 + n
        assert rag.clip_calls().tolist() == one.clip_calls().tolist() == pos, where
        assert rag.clip_frames().tolist() == one.clip_frames().tolist() == [max(p - 1, 0) for p in pos], where
        names = same_export(rag, one, where)
        assert {"wave", "ola", "hist", "l0.h", "l0.c"} <= set(names)
        rows = [(b, p) for b, p in enumerate(pos)]
        a, b = wave_calls(rag, W, 0, MORE, rows=rows), wave_calls(one, W, 0, MORE, rows=rows)
        assert torch.equal(a, b), f"{where}: {MORE} more calls"
        for c in range(B):
            assert torch.equal(a[c], C[c, :, 128 * pos[c]:128 * (pos[c] + MORE)]), f"{where}: clip {c} steps on"
        same_export(rag, one, where + ", later")
        for s in (rag, one):
            s.check_errors()
    assert bool(C[..., 384:].any())
    # the two kinds in one call: catch_up_wave's ValueError, and nothing moved
    rag.reset()
    wave_calls(rag, W, 0, 4)
    rag.reset(clips=[2])
    before, state = rag.clip_calls().tolist(), rag.export_state()
    with pytest.raises(ValueError, match=r"catch_up_wave: clip 2\b.*clip 0\b.*one call per kind"):
        rag.catch_up_wave_ragged(W[:, :512].contiguous(), [128, 256, 512])
    assert rag.clip_calls().tolist() == before and torch.equal(rag.export_state().blob, state.blob)
