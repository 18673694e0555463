"""``StreamingSession.prime`` / ``prime_wave`` and ``sfsn_hop_prime``: a recorded prefix runs through the offline kernels, one launch
(or, in the per-kernel tier, a handful of row copies) transplants its end state, and the session's next hop continues as if the
prefix had been streamed.

Compared with ``torch.equal`` against BOTH references -- the offline forward of the whole clip and a session that streamed
everything -- on the fixtures of the existing streaming tests (tests/primeref.py: LIVE_TINY, LIVE_TINY_2SPK, LIVE_TINY_UNSHARED, the
frozen front-end with the cumulative norm and with given offline-norm statistics), B in {1, 3}, hop in {1, 2}, both tiers, prefixes
of one launch, D, D + one launch, an odd number of launches and 40 of 60 frames.  The state after ``prime`` equals the streamed
session's buffer by buffer; the one exception the header states -- layer 0's membranes in the one-launch tier, which are the offline
forward's -- is held to hopref / scanref's fp64 bound for kind "x32".  tests/test_stream_prime_host.py shows on the CPU that no
layer-0 membrane of these seeds lies within that bound of the threshold, which is what makes the bit-for-bit comparison legitimate."""
import ctypes

import numpy as np
import pytest
import torch

import hopref as hr
import primeref as pr
import scanref as sr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_models = {}


def model_of(name, seed=None):
    key = (name, seed)
    if key not in _models:
        import spiking_fullsubnet_amd as pkg
        front, kw, _ = pr.FIXTURES[name]
        m = (pkg.SpikingFullSubNet if front == "live" else pkg.Separator)(**kw)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in pr.state_dict(name, seed).items()}, strict=True)
        _models[key] = m.eval().to(DEV)
    return _models[key]


def own_stats(name, model, stft):
    """The clips' own offline-norm statistics where the fixture's norm needs them."""
    if name != "frozen_tiny":
        return None
    return model.engine().forward_stft(stft, want_layers=False, return_norm_stats=True)["norm_stats"]


def offline(model, stft, stats, **kw):
    if stats is not None:
        kw["norm_stats"] = stats
    return model.engine().forward_stft(stft, want_layers=False, **kw)


def real(x):
    return torch.view_as_real(x) if x.is_complex() else x


def pool_view(part, ptr, shape, dtype, pool=None):
    """A buffer of the one-launch hop, found by its descriptor pointer inside the part's arena (as hopref.states does)."""
    base = part["spool"].data_ptr()
    pool = part["spool"] if pool is None else pool
    off = int(ptr) - base
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    assert 0 <= off and off + nbytes <= pool.numel()
    return pool[off:off + nbytes].view(dtype).view(shape)


def hop_buffers(sess, pool=None):
    """{name: (tensor, rows per clip)} of every state buffer the NEXT launch of a one-launch session reads; the leading dimension of
    each tensor is clip-major.  `pool`: the same views of another byte tensor of the arena's size (a mask)."""
    hp = sess._hop
    assert len(hp["parts"]) == 1
    part = hp["parts"][0]
    desc, spec, nb = part["desc"], sess.eng.spec, part["nb"]
    par = int(desc.launch_index) & 1
    out = {}
    seqs = list(zip([desc.fb] + [desc.sb[g] for g in range(spec.n_groups)], [sess.eng.fb] + list(sess.eng.sb)))
    for s, (dst, seq) in enumerate(seqs):
        u = 1 if s == 0 else spec.units(s - 1)
        R, H = nb * u, seq.H
        HP = (H + 63) // 64 * 64
        for l in range(len(seq.cells)):
            out[f"h.{s}.{l}"] = (pool_view(part, dst.layer[l].h[par], (R, HP), torch.int8, pool), u)
            out[f"c.{s}.{l}"] = (pool_view(part, dst.layer[l].c, (R, H), torch.float32, pool), u)
        if dst.cum[par]:
            out[f"cum.{s}"] = (pool_view(part, dst.cum[par], (R,), torch.float32, pool), u)
    if sess.D:
        out["hist"] = (pool_view(part, desc.hist_ri, (nb, sess.F, sess.D, 2), torch.float32, pool), 1)
    if sess.waveform:
        out["wave_state"] = (pool_view(part, desc.wave_state, (nb, 512), torch.float32, pool), 1)
        out["ola_state"] = (pool_view(part, desc.ola_state, (nb * spec.num_spks, 512), torch.float32, pool), spec.num_spks)
    return out


def snapshot(sess):
    """Clones of every state tensor of the session (the buffers its next hop reads)."""
    if sess._hop is None:
        out = {}
        for tag, d in (("fb", sess.fb), ("sb", sess.sb)):
            for l, layer in enumerate(d["states"]):
                for i, (h, c) in enumerate(layer):
                    out[f"{tag}.h.{l}.{i}"], out[f"{tag}.c.{l}.{i}"] = h.clone(), c.clone()
        out["hist"] = real(sess.hist).clone()
        if sess._rows is not None:
            out["rows"] = sess._rows.clone()
        return out
    out = {k: v.clone() for k, (v, _) in hop_buffers(sess).items()}
    slots = sess._hop["parts"][0]["slots"]
    if slots is not None:
        out["slots"] = slots.clone()
    return out


def book(sess):
    """The bookkeeping a caller can see."""
    out = dict(frames_done=sess.frames_done, clip_frames=sess.clip_frames.tolist(), clip_calls=sess.clip_calls.tolist())
    if sess.count_spikes:
        fb_all, sb_all = sess.spike_summary()
        out["counts"] = [int(x.count) for x in fb_all[1:-1]] + [int(x.count) for a in sb_all for x in a[1:-1]]
        out["shapes"] = [tuple(x.shape) for x in fb_all] + [tuple(x.shape) for a in sb_all for x in a]
    return out


def layer0_bound(model, stft, stats, got):
    """got[s]: the session's layer-0 membranes [R][H] of sequence model s after the frames of `stft`; each inside the fp64 bound of
    kind "x32" on the rows whose spikes the reference decides (hopref.check_stack's rule for c)."""
    eng = model.engine()
    kw = dict(norm_stats=stats) if stats is not None else {}
    res = eng.forward_stft(stft, want_layers=True, **kw)
    alls = [res["fb_all"]] + list(res["sb_all"])
    worst = 0.0
    for s, seq in enumerate([eng.fb] + list(eng.sb)):
        hd = hr.held(seq.cells[0], seq.H, seq.cells[0].G, True)
        ref = sr.layer(hr.layer_case(hd, alls[s][0].cpu().numpy()))
        cmp_ = sr.compare(alls[s][1].cpu().numpy(), ref)
        assert cmp_.ok, cmp_.why
        ratio = sr.final_ratio(got[s].cpu().numpy(), ref, cmp_.t_valid)
        assert ratio <= 1.0, f"sequence model {s}: layer-0 membranes {ratio:.3g} x the x32 bound"
        worst = max(worst, ratio)
    return worst


def same_state(a, b, one_launch, where):
    assert a.keys() == b.keys(), where
    loose = []
    for k in a:
        if one_launch and k.startswith("c.") and k.endswith(".0"):
            loose.append(k)  # layer 0's membranes: the offline forward's, not the hop's (include/sfsn.h); see layer0_bound
            continue
        assert torch.equal(a[k], b[k]), f"{where}: state buffer {k}"
    return loose


CASES = [(n, B, hop, ol) for n in pr.FIXTURES for B in (1, 3) for hop in (1, 2) for ol in (True, False)
         if not (n == "frozen_tiny_cum" and not ol)]  # (the cumulative norm streams through the one-launch hop only)


@pytest.mark.parametrize("name,B,hop,one_launch", CASES, ids=[f"{n}-B{B}-hop{h}-{'one' if o else 'graph'}" for n, B, h, o in CASES])
def test_prime_then_step_equals_offline_and_streamed(name, B, hop, one_launch):
    model = model_of(name)
    stft = torch.from_numpy(pr.spectra(name, B)).to(DEV)
    stats = own_stats(name, model, stft)
    off = offline(model, stft, stats)
    Ns = pr.prefix_lengths(hop, pr.df_reach(name))
    kw = dict(batch=B, hop=hop, one_launch=one_launch, graph=True, count_spikes=True, norm_stats=stats)
    streamed = model.streaming(**kw)
    assert (streamed._hop is not None) == one_launch and (one_launch or streamed._graph is not None)
    snaps, es, ms = {}, [], []
    for k in range(pr.T // hop):
        e, m = streamed.step(stft[..., k * hop:(k + 1) * hop].contiguous())
        es.append(e)
        ms.append(m)
        if (k + 1) * hop in Ns:
            snaps[(k + 1) * hop] = (snapshot(streamed), book(streamed))
    streamed.check_errors()
    es, ms = torch.cat(es, -1), torch.cat(ms, -1)
    assert torch.equal(real(es), real(off["enh_stft"])) and torch.equal(ms, off["enh_mag"])  # (the premise: the references agree)
    primed = model.streaming(**kw)
    for N in Ns:
        primed.reset()
        e0, m0 = primed.prime(stft[..., :N])
        assert torch.equal(real(e0), real(off["enh_stft"][..., :N])) and torch.equal(m0, off["enh_mag"][..., :N]), N
        snap, bk = snapshot(primed), book(primed)
        loose = same_state(snap, snaps[N][0], one_launch, f"N = {N}")
        assert bk == snaps[N][1], (N, bk, snaps[N][1])
        if loose and N in (17, 18):
            for which in (snap, snaps[N][0]):  # (primed: the offline forward's membranes; streamed: the hop's -- the same bound)
                ratio = layer0_bound(model, stft[..., :N].contiguous(), stats, [which[k] for k in sorted(loose)])
            print(f"PRIME {name} B={B} hop={hop}: layer-0 membranes after {N} frames at {ratio:.3f} of the x32 bound")
        pe, pm = [], []
        for k in range(N // hop, pr.T // hop):
            e, m = primed.step(stft[..., k * hop:(k + 1) * hop].contiguous())
            pe.append(e)
            pm.append(m)
        primed.check_errors()
        pe, pm = torch.cat(pe, -1), torch.cat(pm, -1)
        assert torch.equal(real(pe), real(off["enh_stft"][..., N:])) and torch.equal(pm, off["enh_mag"][..., N:]), N
        assert torch.equal(real(pe), real(es[..., N:])) and torch.equal(pm, ms[..., N:]), N
        assert book(primed) == book(streamed), N


# ---- per-clip priming ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hop,one_launch,wrap", [("live_tiny", 1, True, False), ("live_tiny", 1, True, True), ("live_tiny", 2, True, True),
                                                     ("live_tiny_2spk", 2, False, False), ("live_tiny", 1, False, False),
                                                     ("frozen_tiny_cum", 1, True, False), ("frozen_tiny", 2, True, False)])
def test_one_clip_is_primed_while_the_others_go_on(name, hop, one_launch, wrap):
    B, P, n0 = 3, 12, 10  # after n0 hops clip 1 is primed with the first P frames of another utterance
    model = model_of(name)
    stft = torch.from_numpy(pr.spectra(name, B)).to(DEV)
    # the new utterance of clip 1: the first 44 frames of clip 2 (frames the host file has cleared; the offline norm: with the
    # statistics of that whole clip, so that its membranes are the cleared ones)
    other = stft[2:3, :, :44].contiguous()
    stats = own_stats(name, model, stft)
    s_other = None if stats is None else stats.select([2])
    off_other = offline(model, other, s_other)
    kw = dict(batch=B, hop=hop, one_launch=one_launch, graph=True, count_spikes=True, norm_stats=stats)
    sess, plain = model.streaming(**kw), model.streaming(**kw)
    if wrap:  # the launch counter about to wrap: the unsigned origin arithmetic (tags and parities only depend on the counter)
        for part in sess._hop["parts"]:
            part["desc"].launch_index = 2 ** 32 - 3
            part["origin"].fill_(sess._as_i32(2 ** 32 - 3))
    n_steps = n0 + (44 - P) // hop
    outs, plains = [], []
    for k in range(n_steps):
        if k == n0:
            if s_other is not None:
                sess.set_norm_stats(s_other, clips=[1])
            sess.prime(stft[:1, :, :2 * hop], clips=[1])  # primed twice: the second replaces the first
            e0, m0 = sess.prime(other[..., :P], clips=[1])
            assert torch.equal(real(e0), real(off_other["enh_stft"][..., :P])) and torch.equal(m0, off_other["enh_mag"][..., :P])
            assert sess.clip_frames.tolist() == [n0 * hop, P, n0 * hop]
        x = stft[..., k * hop:(k + 1) * hop].clone()
        plains.append(plain.step(x.contiguous()))
        if k >= n0:
            x[1] = other[0, :, P + (k - n0) * hop:P + (k - n0 + 1) * hop]
        outs.append(sess.step(x.contiguous()))
    sess.check_errors()
    plain.check_errors()
    for i in (0, 1):
        got, ref = torch.cat([o[i] for o in outs], -1), torch.cat([o[i] for o in plains], -1)
        assert torch.equal(real(got[[0, 2]]), real(ref[[0, 2]])), "the clips that were not primed"
        assert torch.equal(real(got[1, ..., :n0 * hop]), real(ref[1, ..., :n0 * hop]))
        want = (off_other["enh_stft"], off_other["enh_mag"])[i][0, ..., P:]
        assert torch.equal(real(got[1, ..., n0 * hop:]), real(want)), "the primed clip against the offline forward of its utterance"
    fresh = model.streaming(**dict(kw, batch=1, norm_stats=s_other))
    fresh.prime(other[..., :P])
    fe = torch.cat([fresh.step(other[..., P + j * hop:P + (j + 1) * hop].contiguous())[0] for j in range((44 - P) // hop)], -1)
    assert torch.equal(real(fe[0]), real(torch.cat([o[0] for o in outs], -1)[1, ..., n0 * hop:])), "against a fresh one-clip session primed alike"
    assert sess.clip_frames.tolist() == [n_steps * hop, 44, n_steps * hop]
    a, b = sess.spike_summary([1]), fresh.spike_summary()
    assert [int(x.count) for x in a[0][1:-1]] == [int(x.count) for x in b[0][1:-1]]
    assert [[int(x.count) for x in g[1:-1]] for g in a[1]] == [[int(x.count) for x in g[1:-1]] for g in b[1]]
    # prime, then reset(clips): the clip starts from silence like a fresh session
    sess.prime(other[..., :P], clips=[1])
    sess.reset(clips=[1])
    fresh.reset()
    for j in range(6):
        x = stft[..., j * hop:(j + 1) * hop].clone()
        x[1] = other[0, :, j * hop:(j + 1) * hop]
        e = sess.step(x.contiguous())[0]
        assert torch.equal(real(e[1]), real(fresh.step(other[..., j * hop:(j + 1) * hop].contiguous())[0][0])), j
        assert torch.equal(real(e[1]), real(off_other["enh_stft"][0, ..., j * hop:(j + 1) * hop])), j
    sess.check_errors()


def test_clips_in_any_order_take_their_own_rows():
    name, B = "live_tiny", 3
    model = model_of(name)
    stft = torch.from_numpy(pr.spectra(name, B)).to(DEV)
    off = offline(model, stft, None)
    for one_launch in (True, False):
        sess = model.streaming(batch=B, one_launch=one_launch)
        e0, _ = sess.prime(stft[[2, 0], :, :9], clips=[2, 0])
        assert torch.equal(real(e0), real(off["enh_stft"][[2, 0], ..., :9]))
        x = stft[..., 9:10].clone()
        x[1] = stft[1, :, :1]  # clip 1 was never primed: it is at its frame 0
        e, _ = sess.step(x.contiguous())
        assert torch.equal(real(e[[0, 2]]), real(off["enh_stft"][[0, 2], ..., 9:10]))
        assert torch.equal(real(e[1]), real(off["enh_stft"][1, ..., :1]))
        assert sess.clip_frames.tolist() == [10, 1, 10]


def test_a_session_cut_into_parts_primes_each_part_with_its_own_descriptor():
    name, B, N = "live_tiny", 256, 17
    model = model_of(name)
    stft = torch.from_numpy(pr.spectra(name, 3)).to(DEV)  # the three clips the host file has cleared ...
    off = offline(model, stft, None)
    sess = model.streaming(batch=B, count_spikes=True)
    parts = [(p["b0"], p["nb"]) for p in sess._hop["parts"]]
    assert len(parts) > 1, "256 clips ask for more workgroups than one launch may hold"
    clips = [5, parts[1][0] - 1, parts[1][0]]  # ... on clips of two parts, either side of the cut
    e0, m0 = sess.prime(stft[..., :N], clips=clips)
    assert torch.equal(real(e0), real(off["enh_stft"][..., :N])) and torch.equal(m0, off["enh_mag"][..., :N])
    for j in range(6):
        x = torch.zeros((B, sess.F, 1), dtype=torch.complex64, device=DEV)
        x[clips] = stft[..., N + j:N + j + 1]
        e, m = sess.step(x)
        assert torch.equal(real(e[clips]), real(off["enh_stft"][..., N + j:N + j + 1])) and torch.equal(m[clips], off["enh_mag"][..., N + j:N + j + 1]), j
    sess.check_errors()
    assert sess.clip_frames[clips].tolist() == [N + 6] * 3 and sess.clip_frames[0] == 6
    one = model.streaming(batch=3, count_spikes=True)
    for k in range(N + 6):
        one.step(stft[..., k:k + 1].contiguous())
    a, b = sess.spike_summary(clips), one.spike_summary()
    assert [int(x.count) for x in a[0][1:-1]] == [int(x.count) for x in b[0][1:-1]]
    assert [[int(x.count) for x in g[1:-1]] for g in a[1]] == [[int(x.count) for x in g[1:-1]] for g in b[1]]


# ---- waveform --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B", [("live_tiny", 3), ("live_tiny", 1), ("live_tiny_2spk", 3), ("frozen_tiny_cum", 3)])
def test_prime_wave_then_step_wave(name, B):
    seed = pr.WAVE_FIXTURES[name]
    model = model_of(name, seed)
    S = pr.FIXTURES[name][1].get("num_spks", 1)
    w = torch.from_numpy(pr.waves(name, B)).to(DEV)
    y = model(w)[0].reshape(B, S, -1)
    streamed = model.streaming(batch=B, waveform=True, count_spikes=True)
    outs, snaps = [], {}
    for k in range(pr.CALLS):
        outs.append(streamed.step_wave(w[:, 128 * k:128 * (k + 1)].contiguous()))
        if k + 1 in pr.WAVE_C:
            snaps[k + 1] = (snapshot(streamed), book(streamed))
    streamed.check_errors()
    for k in range(3, pr.CALLS):
        assert torch.equal(outs[k], y[:, :, 128 * (k - 3):128 * (k - 2)]), k
    outs = torch.cat(outs, -1)
    primed = model.streaming(batch=B, waveform=True, count_spikes=True)
    for c in pr.WAVE_C:
        primed.reset()
        r = primed.prime_wave(w[:, :128 * c])
        assert r.shape == (B, S, 128 * c) and not bool(r[..., :384].any())
        assert torch.equal(r, outs[..., :128 * c]), c
        snap, bk = snapshot(primed), book(primed)
        same_state(snap, snaps[c][0], True, f"c = {c}")
        assert torch.equal(snap["wave_state"], snaps[c][0]["wave_state"]) and torch.equal(snap["ola_state"], snaps[c][0]["ola_state"])
        assert bk == snaps[c][1], (c, bk, snaps[c][1])
        rest = torch.cat([primed.step_wave(w[:, 128 * k:128 * (k + 1)].contiguous()) for k in range(c, pr.CALLS)], -1)
        primed.check_errors()
        assert torch.equal(rest, outs[..., 128 * c:]), c
        for k in range(max(c, 3), pr.CALLS):
            assert torch.equal(rest[..., 128 * (k - c):128 * (k - c + 1)], y[:, :, 128 * (k - 3):128 * (k - 2)]), (c, k)
        assert book(primed) == book(streamed), c


@pytest.mark.parametrize("n0", [0, 7])
def test_prime_wave_of_one_clip(n0):
    """n0 = 0: nobody has called yet -- the other clips' utterances begin with the next call."""
    name, B, c = "live_tiny", 3, 4
    model = model_of(name, pr.WAVE_FIXTURES[name])
    w = torch.from_numpy(pr.waves(name, B)).to(DEV)
    u = w[2:3]  # clip 1 goes on with clip 2's samples (frames the host file has cleared)
    sess, plain, fresh = (model.streaming(batch=b, waveform=True) for b in (B, B, 1))
    outs, plains = [], []
    for k in range(n0):
        outs.append(sess.step_wave(w[:, 128 * k:128 * (k + 1)].contiguous()))
        plains.append(plain.step_wave(w[:, 128 * k:128 * (k + 1)].contiguous()))
    r = sess.prime_wave(u[:, :128 * c], clips=[1])
    assert torch.equal(r, fresh.prime_wave(u[:, :128 * c]))
    assert sess.clip_calls.tolist() == [n0, c, n0] and sess.clip_frames.tolist() == [max(n0 - 1, 0), c - 1, max(n0 - 1, 0)]
    y = model(u)[0].reshape(1, 1, -1)
    for j in range(12):
        x = w[:, 128 * (n0 + j):128 * (n0 + j + 1)].clone()
        x[1] = u[0, 128 * (c + j):128 * (c + j + 1)]
        o, p_ = sess.step_wave(x.contiguous()), plain.step_wave(w[:, 128 * (n0 + j):128 * (n0 + j + 1)].contiguous())
        f = fresh.step_wave(u[:, 128 * (c + j):128 * (c + j + 1)].contiguous())
        assert torch.equal(o[[0, 2]], p_[[0, 2]]), j
        assert torch.equal(o[1], f[0]), j
        assert torch.equal(o[1], y[0, :, 128 * (c + j - 3):128 * (c + j - 2)]), j
    sess.check_errors()
    assert sess.clip_calls.tolist() == [n0 + 12, c + 12, n0 + 12]


def test_prime_wave_with_host_io():
    name, B, c = "live_tiny", 3, 5
    model = model_of(name, pr.WAVE_FIXTURES[name])
    w = torch.from_numpy(pr.waves(name, B)).to(DEV)
    y = model(w)[0].reshape(B, 1, -1)
    sess = model.streaming(batch=B, waveform=True, host_io=True)
    r = sess.prime_wave(w[:, :128 * c])
    assert r.device.type == "cuda" and torch.equal(r[..., 384:], y[:, :, :128 * (c - 3)])
    for k in range(c, c + 8):
        o = sess.step_wave_host(w[:, 128 * k:128 * (k + 1)].cpu())
        assert torch.equal(o, y[:, :, 128 * (k - 3):128 * (k - 2)].cpu()), k
    sess.check_errors()


# ---- sfsn_hop_prime called directly ----------------------------------------------------------------------------------------
def test_the_launch_writes_the_listed_clips_rows_and_nothing_else():
    name, B, c = "live_tiny_2spk", 3, 6
    model = model_of(name, pr.WAVE_FIXTURES[name])
    w = torch.from_numpy(pr.waves(name, B)).to(DEV)
    sess = model.streaming(batch=B, waveform=True, count_spikes=True)
    part = sess._hop["parts"][0]
    part["desc"].launch_index = 5  # (an odd index: the other halves of the double buffers)
    part["spool"].fill_(0x5A)  # sentinels in and around every state buffer of the arena, the tagged scratch included
    part["slots"].fill_(0x5A5A5A5A)
    before, slots_before = part["spool"].clone(), part["slots"].clone()
    mask = torch.zeros_like(part["spool"])
    fcov = max(sess.eng.spec.cutoffs[g] + sess.eng.spec.units(g) * sess.eng.spec.ctr[g] for g in range(sess.eng.spec.n_groups))
    for k, (v, u) in hop_buffers(sess, mask).items():
        iv, one = (v, 1) if v.dtype == torch.int8 else (v.view(torch.int32), 0x01010101)  # (every byte of a marked element non-zero)
        if k == "hist":
            iv[1, :fcov] = one  # (the hop keeps no history of the pass-through bins)
        elif k.startswith("h."):
            H = sess.eng.fb.H if k.startswith("h.0.") else sess.eng.sb[0].H
            iv[u:2 * u, :H] = one  # (padding columns stay as they are: zero in a session)
        else:
            iv[u:2 * u] = one
    sess.prime_wave(w[1:2, :128 * c], clips=[1])
    torch.cuda.synchronize()
    changed = part["spool"] != before
    assert not bool((changed & (mask == 0)).any()), "a byte outside clip 1's rows changed"
    assert bool(changed.any())
    for k, (v, u) in hop_buffers(sess).items():
        sent = torch.full_like(v, 0).view(torch.uint8).fill_(0x5A).view(v.dtype)
        assert torch.equal(v[:u], sent[:u]) and torch.equal(v[2 * u:], sent[2 * u:]), f"{k}: rows of clips 0 and 2"
    # the same state as a session of its own leaves, buffer by buffer (rows of clip 1)
    alone = model.streaming(batch=1, waveform=True, count_spikes=True)
    alone._hop["parts"][0]["desc"].launch_index = 5
    alone.prime_wave(w[1:2, :128 * c])
    for (k, (v, u)), (_, (v1, _)) in zip(hop_buffers(sess).items(), hop_buffers(alone).items()):
        if k.startswith("h."):
            H = sess.eng.fb.H if k.startswith("h.0.") else sess.eng.sb[0].H
            assert torch.equal(v[u:2 * u, :H], v1[:, :H]), k
        elif k == "hist":
            assert torch.equal(v[1, :fcov], v1[0, :fcov]), k
        else:
            assert torch.equal(v[u:2 * u], v1), k
    # slots: [sequence][layer][row][H / 4]; clip 1's rows hold counts, the others the sentinel
    spec, off = sess.eng.spec, 0
    got, one = part["slots"], alone._hop["parts"][0]["slots"]
    o1 = 0
    for s, seq in enumerate([sess.eng.fb] + list(sess.eng.sb)):
        u = 1 if s == 0 else spec.units(s - 1)
        n = B * u * (seq.H // 4)
        for _ in seq.cells:
            blk, ref = got[off:off + n].view(B, -1), slots_before[off:off + n].view(B, -1)
            assert torch.equal(blk[[0, 2]], ref[[0, 2]])
            assert torch.equal(blk[1], one[o1:o1 + n // B])
            assert int(blk[1].max()) <= 4 * (c - 1)
            off, o1 = off + n, o1 + n // B
    assert off == got.numel()


def test_the_entry_point_refuses_bad_arguments():
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    model = model_of("live_tiny")
    sess = model.streaming(batch=3, hop=2, one_launch=True)
    ref = sess._hop["parts"][0]["ref"]
    src = _lib.PrimeSrc()
    src.Bp, src.N, src.b0 = 1, 4, 0

    def call(desc=ref, clips=(1,), n=None, s=src):
        arr = (ctypes.c_int * max(len(clips), 1))(*clips)
        return L.sfsn_hop_prime(desc, arr if clips is not None else None, len(clips) if n is None else n, ctypes.byref(s) if s is not None else None, None)

    assert L.sfsn_hop_prime(None, (ctypes.c_int * 1)(0), 1, ctypes.byref(src), None) == _lib.SFSN_EINVAL
    assert L.sfsn_hop_prime(ref, None, 1, ctypes.byref(src), None) == _lib.SFSN_EINVAL
    assert call(s=None) == _lib.SFSN_EINVAL
    assert call(clips=(), n=0) == _lib.SFSN_EINVAL                 # an empty list
    assert call(clips=(3,)) == _lib.SFSN_EINVAL and call(clips=(-1,)) == _lib.SFSN_EINVAL  # outside the batch
    two = _lib.PrimeSrc()
    two.Bp, two.N = 2, 4
    assert call(clips=(1, 1), s=two) == _lib.SFSN_EINVAL          # listed twice
    assert call(clips=(0, 1)) == _lib.SFSN_EINVAL                  # more clips than the prefix has
    odd = _lib.PrimeSrc()
    odd.Bp, odd.N = 1, 3
    assert call(s=odd) == _lib.SFSN_EINVAL                         # N is not a multiple of hop
    odd.N = 0
    assert call(s=odd) == _lib.SFSN_EINVAL                         # no frame at all (a spectral session)
    assert call() == _lib.SFSN_EINVAL                              # valid geometry, NULL source tensors: refused, not launched
    torch.cuda.synchronize()
    sess.check_errors()


# ---- refusals of the session ------------------------------------------------------------------------------------------------
def test_what_prime_refuses():
    model = model_of("live_tiny")
    stft = torch.from_numpy(pr.spectra("live_tiny", 3)).to(DEV)
    w = torch.from_numpy(pr.waves("live_tiny", 3)).to(DEV)
    res = model.streaming(batch=1, waveform=True, host_io=True, resident=True)
    with pytest.raises(NotImplementedError, match="resident"):
        res.prime_wave(w[:1, :256])
    with pytest.raises(NotImplementedError, match="resident"):
        res.prime(stft[:1, :, :4])
    res.close()
    from spiking_fullsubnet_amd.modeling_cirm_gsn import Model
    cirm = Model(**hr.CIRM_TINY).eval().to(DEV).streaming()
    assert not hasattr(cirm, "prime") and not hasattr(cirm, "prime_wave")  # (a follow-up: fullband_streaming.py)
    spec_s, wave_s = model.streaming(batch=3, hop=2), model.streaming(batch=3, waveform=True)
    with pytest.raises(RuntimeError):
        wave_s.prime(stft[..., :4])
    with pytest.raises(RuntimeError):
        spec_s.prime_wave(w[:, :256])
    with pytest.raises(RuntimeError):
        spec_s.prime(stft[..., :4].cpu())
    with pytest.raises(RuntimeError):
        wave_s.prime_wave(w[:, :256].cpu())
    with pytest.raises(RuntimeError):
        spec_s.prime(stft[..., :4].real.contiguous())  # dtype
    with pytest.raises(RuntimeError):
        spec_s.prime(stft[:2, :, :4])  # two clips for a session of three
    for bad in (3, 1, 0):  # not a multiple of hop; less than a hop; nothing
        with pytest.raises(ValueError):
            spec_s.prime(stft[..., :bad])
    with pytest.raises(ValueError):
        wave_s.prime_wave(w[:, :200])
    with pytest.raises(IndexError):
        spec_s.prime(stft[:1, :, :4], clips=[3])
    with pytest.raises(ValueError):
        spec_s.prime(stft[:2, :, :4], clips=[1, 1])
    with pytest.raises(TypeError):
        spec_s.prime(stft[:1, :, :4], clips=[0.5])
    assert spec_s.frames_done == 0 and spec_s.clip_frames.tolist() == [0, 0, 0]  # nothing above changed the session
    off = offline(model, stft, None)
    e = torch.cat([spec_s.step(stft[..., 2 * k:2 * k + 2].contiguous())[0] for k in range(3)], -1)
    assert torch.equal(real(e), real(off["enh_stft"][..., :6]))
