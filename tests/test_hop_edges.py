"""The one-launch streaming hops -- sfsn_stream_hop (stream_hop_kernel<ONE, G, GIVEN>, layer roles hop_layer_role<L0, ONE, G, GIVEN>) and
sfsn_fullband_stream_hop / _counted (fbh_layer_role<L0, COUNT>) -- against tests/scanref.py's fp64 layer and derived bound, with every
case of scanref.CASES planted in every GSN cell of the model (tests/hopref.py; tests/test_hop_edges_host.py validates planting,
reference and cases on the CPU).  Nine frames (odd; test_scan_edges.TS's longest), one launch at a time on the default stream,
`one_launch` forced on.

Geometries (hopref.GEOMS): KS = 1 (LIVE_TINY, H 48 / 32); KS = 5 and 4 with a partial last slice (LIVE_M, H 320 / 224); K = 256 exactly;
the multi-frame form (hop 3); G = 2 (separate gate weights); GIVEN layer 0 (the frozen front-end with given statistics); the cIRM-GSN
hop at H = 268 (Hp = 272, four layers) and at the tiny fixture's H = 20, hop 1 and 3, and its counted kernel; B = 1 and 3 (16-row tiles
with 1 or 3 live rows, sub-band rows = B x units).
Dropped: Separator(**FROZEN_TINY) -- its last group has 2 * 64 * 3 = 384 projection columns and sfsn_hop.hip's plan refuses a
sequence model with P > 256 (test_refused_geometry_is_refused asserts the refusal); the same front-end with the deep-filter orders
tests/test_frozen_streaming.py uses (P <= 256) takes its place as an additional row.

Per test: (1) fp64 -- every layer and launch through hopref.check_stack; (2) the header's promise -- the spikes and (through c, sub-band
models) the membranes after every launch of forward_stft(..., want_membrane=True) on the concatenated frames, enh_stft / enh_mag of
the default offline forward, bit for bit, as include/sfsn.h states it since this file's first run: that run found layer 0's
membranes of sfsn_stream_hop different from the offline forward's in the low bits on EVERY case (up to 592 ulp in `control`, fp64
check passed on both sides): its input product adds the 16-column chunks into four accumulators, the offline kernels into one (or
take the bf16 split).  The claim was corrected, not the kernel (check_bits's docstring has the rule now asserted); the cIRM-GSN hop
runs sfsn_fullband_input_proj's own chain and is held to every bit (its engine returns no membranes: spikes and outputs); (3) counts
where the session counts; (6) at most 2 % of the elements unasserted, one HOP_EDGES line (profiles/hop_edges.md keeps the first run's).
test_restart: (4).  test_planted_state: (5).  No tolerance is chosen here: every bound comes from scanref.layer."""
import numpy as np
import pytest
import torch

import hopref as hr
import scanref as sr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = list(sr.CASES)
RUN = [g for g in hr.GEOMS if g not in hr.REFUSED]


def build(front, kw, name):
    import spiking_fullsubnet_amd as pkg
    sd, cases = hr.plant(front, kw, name)
    if front == "cirm":
        from spiking_fullsubnet_amd.modeling_cirm_gsn import Model
        m = Model(**kw)
    else:
        m = (pkg.SpikingFullSubNet if front == "live" else pkg.Separator)(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.eval().to(DEV), cases


def open_session(front, model, B, hop, count, stats):
    kw = dict(batch=B, hop=hop, one_launch=True, count_spikes=count)
    if front == "frozen":
        kw["norm_stats"] = stats
    sess = model.streaming(**kw)
    assert sess._hop is not None
    return sess


def units_of(front, model):
    """Rows per clip of every sequence model."""
    if front == "cirm":
        return [1]
    spec = model.engine().spec
    return [1] + [spec.units(g) for g in range(spec.n_groups)]


def offline(front, model, stft, stats):
    """dict(x[s] [T][R][I], spk[s][l] [T][R][H] 0 / 1, mem[s][l] or None, enh, mag) of the offline forward(s) on the whole spectrum."""
    eng = model.engine()

    def n(t):
        return t.detach().cpu().numpy()

    if front == "cirm":
        res = eng.forward_stft(stft, want_layers=True)
        lay = res["all_layers"]
        out = dict(x=[n(lay[0])], spk=[[n(s) for s in lay[1:-1]]], mem=None)
        plain = eng.forward_stft(stft)
    else:
        kw = dict(norm_stats=stats) if stats is not None else {}
        res = eng.forward_stft(stft, want_membrane=True, **kw)
        alls, mems = [res["fb_all"]] + list(res["sb_all"]), [res["fb_mem"]] + list(res["sb_mem"])
        out = dict(x=[n(a[0]) for a in alls], spk=[[n(s) for s in a[1:-1]] for a in alls], mem=[[n(m) for m in ms] for ms in mems])
        plain = eng.forward_stft(stft, **kw)
    eng.check_stack_errors()
    out["enh"], out["mag"] = plain["enh_stft"].clone(), (None if plain["enh_mag"] is None else plain["enh_mag"].clone())
    return out


def rows_of(clips, u):
    return np.concatenate([np.arange(b * u, (b + 1) * u) for b in clips])


def check_model(tally, stacks, xs, rec, hop, units, clips, t0, t1, state=None, skip_sb0=False, where=""):
    """Every sequence model on frames [t0, t1) of the given clips; xs[s]: layer-0 rows of exactly these frames (all rows of the batch).
    Validity goes up the layers and from the full-band stack to every sub-band row of the same clip (whose layer 0 reads its projection).
    Returns the references [s][l]."""
    t_fb, refs = None, []
    for s, stack in enumerate(stacks):
        rows = rows_of(clips, units[s])
        t_up = None if s == 0 or t_fb is None else np.repeat(t_fb, units[s])
        skip0 = skip_sb0 and s > 0
        tv, r = hr.check_stack(tally, stack, None if skip0 else xs[s][:, rows], rec, s, hop, rows, t0, t1, None if state is None else state[s],
                               None if skip0 else t_up, skip0, where)
        refs.append(r)
        if s == 0:
            t_fb = tv
    return refs


def check_bits(rec, off, hop, stacks, clips, units, t0, t_off, n, what, refs, strict0):
    """Session frames [t0, t0 + n) of the clips against offline frames [t_off, t_off + n), as include/sfsn.h states it.

    strict0 (the cIRM-GSN hop: layer 0's input product is sfsn_fullband_input_proj's own fmaf chain): every spike of every layer is the
    offline forward's.  Otherwise (sfsn_stream_hop: four accumulators against the offline kernels' one, or their bf16 split) layer 0 may
    differ from the offline forward -- but only on neurons the fp64 reference leaves undecided, and a row counts as equal up to its
    first such frame; before it c after a launch is within twice the reference's bound of the offline membrane (each side is within
    one).  From equal inputs on -- the layers above, and the sub-band rows of a clip while its full-band rows are equal -- spikes and
    (through c after every launch) membranes are the offline forward's bit for bit.  Returns (frames of each clip that are equal
    throughout, layer-0 disagreements, worst layer-0 |c - membrane| / bound)."""
    tt = np.arange(n)[:, None]
    t_fb, flips, worst0 = None, 0, 0.0
    clip_ok = np.full(len(clips), n)
    for s, stack in enumerate(stacks):
        rows = rows_of(clips, units[s])
        tv = np.full(len(rows), n) if s == 0 or t_fb is None else np.repeat(t_fb, units[s])
        for l, hd in enumerate(stack):
            Hr = hd["H_real"]
            got = rec["spk"][s][l][t0:t0 + n, rows, :Hr] & 1
            want = off["spk"][s][l][t_off:t_off + n, rows]
            assert np.isin(want, (0.0, 1.0)).all()
            diff = got != want.astype(np.uint8)
            live = tt < tv[None]
            tag = f"{what} seq {s} layer {l}"
            if l == 0 and not strict0:
                ref = refs[s][0]
                dec = ((np.abs(ref["y"]) > ref["tol"]) | (ref["tol"] == 0))[:, :, :Hr]
                anyd = (diff & live[:, :, None]).any(-1)
                first = np.minimum(np.where(anyd.any(0), anyd.argmax(0), n), tv)
                upto = (tt <= first[None]) & live
                assert not (diff & dec & upto[:, :, None]).any(), f"{tag}: the hop and the offline forward disagree on a neuron the fp64 reference decides"
                flips += int((diff & upto[:, :, None]).sum())
                tv = first
            else:
                assert not (diff & live[:, :, None]).any(), f"{tag}: spikes differ from the offline forward's on equal inputs"
            if off["mem"] is None:
                continue
            for k in range(t0 // hop, (t0 + n) // hop):
                tl = (k + 1) * hop - 1 - t0
                ok = tv > tl
                c, m = rec["c"][s][l][k][rows][ok], off["mem"][s][l][tl + t_off, rows][ok]
                if l == 0 and not strict0:
                    r = sr.worst(c, m.astype(np.float64), 2.0 * refs[s][0]["tol"][tl][ok])
                    assert r <= 1.0, f"{tag}: c after launch {k} is {2 * r:.3g} x the bound away from the offline membrane"
                    worst0 = max(worst0, 2 * r)
                else:
                    np.testing.assert_array_equal(c.view(np.int32), m.view(np.int32),
                                                  err_msg=f"{tag}: c after launch {k} is not the offline membrane, bit for bit")
        if s == 0:
            t_fb = tv
        clip_ok = np.minimum(clip_ok, tv.reshape(len(clips), units[s]).min(1))
    return clip_ok, flips, worst0


def check_outputs(rec, off, clips, clip_ok, t0, t_off, what):
    """enh_stft / enh_mag of every clip over the frames in which all its rows were the offline forward's."""
    for b, v in zip(clips, clip_ok):
        if v > 0:
            same(rec["enh"][b, ..., t0:t0 + v], off["enh"][b, ..., t_off:t_off + v], f"{what} enh_stft of clip {b}")
            if off["mag"] is not None:
                same(rec["mag"][b, ..., t0:t0 + v], off["mag"][b, ..., t_off:t_off + v], f"{what} enh_mag of clip {b}")


def same(a, b, what):
    a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (a, b))
    assert a.shape == b.shape and torch.isfinite(b).all() and float(b.abs().max()) > 0, what
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ from the offline forward"


def spikes_counted(rec, s, l, rows, H):
    return int((rec["spk"][s][l][:, rows, :H] & 1).sum())


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("geom", RUN)
def test_hop_against_fp64_and_offline(geom, name):
    front, kw, B, hop, count = hr.GEOMS[geom]
    model, _ = build(front, kw, name)
    stft = torch.from_numpy(hr.spectrum(B, 257, hr.T, hr.geom_seed(geom))).to(DEV)
    stats = model.norm_stats(stft) if front == "frozen" else None
    off = offline(front, model, stft, stats)
    sess = open_session(front, model, B, hop, count, stats)
    rec = hr.record(sess, stft)
    stacks, units = hr.held_stacks(model.engine()), units_of(front, model)
    tally = hr.Tally(f"{geom} {name}")
    clips = list(range(B))
    refs = check_model(tally, stacks, off["x"], rec, hop, units, clips, 0, hr.T)
    clip_ok, flips, worst0 = check_bits(rec, off, hop, stacks, clips, units, 0, 0, hr.T, f"{geom} {name}", refs, front == "cirm")
    check_outputs(rec, off, clips, clip_ok, 0, 0, f"{geom} {name}")
    print(f"HOP_BITS {geom} {name}: layer-0 disagreements with the offline forward {flips}, frames equal throughout per clip {clip_ok.tolist()}, "
          f"worst layer-0 |c - offline membrane| / bound {worst0:.3f}")
    assert front != "cirm" or (clip_ok == hr.T).all()
    if count:
        for b in clips:
            summ = sess.spike_summary([b])
            lists = [summ] if front == "cirm" else [summ[0]] + list(summ[1])
            for s, (lst, stack) in enumerate(zip(lists, stacks)):
                for l, hd in enumerate(stack):
                    assert int(lst[1 + l].count) == spikes_counted(rec, s, l, rows_of([b], units[s]), hd["H_real"]), (b, s, l)
    if name == "saturated":
        assert tally.smax == max(hd["H_real"] for stack in stacks for hd in stack) * sr.QMAX  # (every neuron fires from frame 0 on)
    tally.done()


def test_refused_geometry_is_refused():
    """Separator(**FROZEN_TINY): P = 384 > 256 in its last group (hopref.REFUSED) -- the library refuses, nothing mis-runs."""
    for geom, why in hr.REFUSED.items():
        front, kw, B, hop, count = hr.GEOMS[geom]
        model, _ = build(front, kw, "control")
        stft = torch.from_numpy(hr.spectrum(B, 257, hr.T, hr.geom_seed(geom))).to(DEV)
        with pytest.raises(NotImplementedError):
            model.streaming(batch=B, hop=hop, one_launch=True, norm_stats=model.norm_stats(stft))


@pytest.mark.parametrize("name", NAMES)
def test_restart(name):
    """LIVE_TINY, B = 3, hop 1: reset(clips=[1]) after frame 4.  Clip 1's frames 5.. against a reference (and an offline forward)
    started from zero state at frame 5 -- the launch reads its state as zero (`fresh`) --, clips 0 and 2 against the uninterrupted one."""
    front, kw, B, hop, _ = hr.GEOMS["tiny-B3"]
    cut = 5
    model, _ = build(front, kw, name)
    stft = torch.from_numpy(hr.spectrum(B, 257, hr.T, hr.geom_seed("restart"))).to(DEV)
    off = offline(front, model, stft, None)
    tail = offline(front, model, stft[:, :, cut:].contiguous(), None)
    sess = open_session(front, model, B, hop, False, None)
    rec = hr.record(sess, stft, before=lambda k: sess.reset(clips=[1]) if k == cut else None)
    assert sess.clip_frames.tolist() == [hr.T, hr.T - cut, hr.T]
    stacks, units = hr.held_stacks(model.engine()), units_of(front, model)
    tally = hr.Tally(f"restart tiny-B3 {name}")
    for what, ref_off, xs, clips, t0, t_off, n in (("clips 0, 2", off, off["x"], [0, 2], 0, 0, hr.T),
                                                  ("clip 1 before", off, [x[:cut] for x in off["x"]], [1], 0, 0, cut),
                                                  ("clip 1 restarted", tail, tail["x"], [1], cut, 0, hr.T - cut)):
        refs = check_model(tally, stacks, xs, rec, hop, units, clips, t0, t0 + n, where=what)
        clip_ok, flips, _ = check_bits(rec, ref_off, hop, stacks, clips, units, t0, t_off, n, what, refs, False)
        check_outputs(rec, ref_off, clips, clip_ok, t0, t_off, what)
        print(f"HOP_BITS restart {name} {what}: layer-0 disagreements {flips}, frames equal throughout {clip_ok.tolist()}")
    tally.done()


@pytest.mark.parametrize("name", ["saturated", "tails", "threshold"])
@pytest.mark.parametrize("geom", ["tiny-B3", "cirm-B3"])
def test_planted_state(geom, name):
    """fp64 only: the case's (h0, c0) -- saturated's all-ones h0, tails' c0 in +-5, threshold's +-0.0 -- written into the buffers the next
    launch reads (hopref.write_state).  Sub-band session: before the first launch; the full-band stack on the offline features (which
    do not depend on state), the sub-band layers >= 1 on the device's layer-0 spikes (a sub-band layer 0 reads the full-band projection,
    which now differs from any offline forward's: not compared).  cIRM-GSN session: its first launch reads every clip's state as zero
    (fbh_fresh: clip_start is always set), so frame 0 runs from zero and the state is planted before launch 1."""
    front, kw, B, hop, _ = hr.GEOMS[geom]
    model, cases = build(front, kw, name)
    stft = torch.from_numpy(hr.spectrum(B, 257, hr.T, hr.geom_seed(geom))).to(DEV)
    off = offline(front, model, stft, None)
    sess = open_session(front, model, B, hop, False, None)
    stacks, units = hr.held_stacks(model.engine()), units_of(front, model)
    it = iter(cases.values())
    planted = []
    for s, stack in enumerate(stacks):
        per = []
        for hd in stack:
            p = next(it)
            R, H = B * units[s], hd["H"]
            h0, c0 = np.zeros((R, H), np.float32), np.zeros((R, H), np.float32)
            h0[:, :p["H"]], c0[:, :p["H"]] = p["h0"][:R], p["c0"][:R]
            per.append((h0, c0))
        planted.append(per)
    at = 1 if front == "cirm" else 0
    write = [[(h0[:, :hd["H_real"]], c0[:, :hd["H_real"]]) for (h0, c0), hd in zip(per, stack)] for per, stack in zip(planted, stacks)]
    rec = hr.record(sess, stft, before=lambda k: hr.write_state(sess, write) if k == at else None)
    tally = hr.Tally(f"planted state {geom} {name}")
    clips = list(range(B))
    if at:
        check_model(tally, stacks, [x[:at * hop] for x in off["x"]], rec, hop, units, clips, 0, at * hop, where="before planting")
    check_model(tally, stacks, [x[at * hop:] for x in off["x"]], rec, hop, units, clips, at * hop, hr.T, state=planted, skip_sb0=True, where="planted")
    if name == "saturated":
        assert (rec["spk"][0][0][at * hop:, :, :stacks[0][0]["H_real"]] & 1).all()
    tally.done()
