"""The one-launch streaming hops (sfsn_stream_hop: hop_layer_role<L0, ONE, G, GIVEN>; sfsn_fullband_stream_hop: fbh_layer_role<L0, COUNT>)
under tests/scanref.py's fp64 layer and derived bound.  A helper module like scanref.py (not a conftest).  Three parts:

* `plant`: a model's usual state dict with every GSN cell's parameters replaced by a scanref case's (layer 0: kind "x32", layers above:
  "spike"; every cell seeded by its own key).  BatchNorm is planted as weight = alpha, bias = beta, running_mean = 0 and the
  running_var whose folded inverse deviation is exactly 1 in the engine's fp32 folding.  The reference never trusts that mapping:
  `held` reads back what the engine holds for a cell (scale, shift, biases; the weights through the library's unpacking) and the
  reference runs on those.  tests/test_hop_edges_host.py checks on the CPU that the planted properties survive the folding.
* `states` / `record`: the session's per-layer state -- the spike scratch [hop][R][pad64(H)] (bit 0 of a byte is the spike, the other
  bits the launch's tag), the two h buffers and c -- as views of the session's own device memory (the sub-band session keeps them in
  a per-part arena: found by the descriptor's pointers as offsets into it), copied out after every launch; `write_state` puts a
  planted (h0, c0) where the next launch reads it.  No product code is changed for this.
* `check_stack`: scanref.compare per layer over a range of frames and rows, each layer's reference on the DEVICE'S OWN inputs (layer 0:
  the layer-input rows of the offline forward; above: the device's spikes of the layer below), validity carried upwards through
  t_up; after every launch c within the propagated bound of y[t_last] on the rows still valid, h[next parity] = the last frame's
  spikes, padding columns (and padded neurons) zero.

GEOMS is the table of sessions both test files run (the host file: the reference alone on the oracle's features)."""
import zlib

import numpy as np

import refweights as rw
import scanref as sr

F32 = np.float32
T = 9  # test_scan_edges.TS's longest: odd, so hop 3 ends on a launch boundary and hop 1 runs both state parities five / four times

CIRM = dict(n_fft=512, hop_length=128, win_length=512, fdrc=0.5, input_size=257, hidden_size=268, num_layers=4, proj_size=257,
            output_activate_function=False, df_order=3, use_pre_layer_norm_fb=True, bn=True, shared_weights=True, sequence_model="GSN",
            num_spks=1)  # test_cirm_gsn.RECIPE
CIRM_TINY = dict(CIRM, hidden_size=20, num_layers=3)  # test_cirm_streaming.TINY
K256 = dict(rw.LIVE_TINY, fb_hidden_size=256, sb_hidden_size=64)
TINY_G2 = dict(rw.LIVE_TINY, shared_weights=False)
M_G2 = dict(rw.LIVE_M, shared_weights=False)
# FROZEN_TINY's last group has 2 * 64 * 3 = 384 projection columns: hop_plan_seq refuses P > 256 (sfsn_hop.hip); the same front-end with
# the orders tests/test_frozen_streaming.py uses is covered
FROZEN_TINY_COVERED = dict(rw.FROZEN_TINY, sb_df_orders=[3, 2, 1])

# name -> (front, kwargs, B, hop, count_spikes)
GEOMS = {
    "tiny-B1": ("live", rw.LIVE_TINY, 1, 1, False), "tiny-B3": ("live", rw.LIVE_TINY, 3, 1, False),
    "m-B1": ("live", rw.LIVE_M, 1, 1, False), "m-B3": ("live", rw.LIVE_M, 3, 1, False),
    "k256-B1": ("live", K256, 1, 1, False), "k256-B3": ("live", K256, 3, 1, False),
    "tiny-B3-hop3": ("live", rw.LIVE_TINY, 3, 3, False), "m-B3-hop3": ("live", rw.LIVE_M, 3, 3, False),
    "tiny_g2-B1": ("live", TINY_G2, 1, 1, False), "tiny_g2-B3-hop3": ("live", TINY_G2, 3, 3, False), "m_g2-B1": ("live", M_G2, 1, 1, False),
    "frozen_tiny-B3": ("frozen", rw.FROZEN_TINY, 3, 1, False),
    "frozen_tiny_covered-B1": ("frozen", FROZEN_TINY_COVERED, 1, 1, False), "frozen_tiny_covered-B3": ("frozen", FROZEN_TINY_COVERED, 3, 1, False),
    "tiny-B3-counted": ("live", rw.LIVE_TINY, 3, 1, True),
    "cirm-B1": ("cirm", CIRM, 1, 1, False), "cirm-B3": ("cirm", CIRM, 3, 1, False), "cirm-B3-hop3": ("cirm", CIRM, 3, 3, False),
    "cirm_tiny-B1": ("cirm", CIRM_TINY, 1, 1, False), "cirm_tiny-B3": ("cirm", CIRM_TINY, 3, 1, False),
    "cirm_tiny-B3-hop3": ("cirm", CIRM_TINY, 3, 3, False),
    "cirm-B3-counted": ("cirm", CIRM, 3, 1, True),
}
REFUSED = {"frozen_tiny-B3": "hop_plan_seq: a sequence model's projection has more than 256 columns (group 2: P = 2 * 64 * 3 = 384)"}


def spectrum(B, F, n_frames, seed):
    """Complex-normal spectrum [B, F, T] scaled like tests/test_cirm_streaming.py's."""
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((B, F, n_frames)) + 1j * rng.standard_normal((B, F, n_frames))) * 0.5).astype(np.complex64)


def geom_seed(geom):
    return zlib.crc32(geom.encode()) % 1000


# ----------------------------------------------------------------------------------------------------------------------
# planting
# ----------------------------------------------------------------------------------------------------------------------
def base_state_dict(front, kw, seed=3):
    """The model's usual numpy state dict (refweights; cIRM-GSN: the same distributions under its own key names)."""
    if front == "live":
        return rw.live_state_dict(kw, seed)
    if front == "frozen":
        return rw.frozen_state_dict(kw, seed)
    rng = np.random.default_rng(seed)
    sd = {}
    F, S = kw["input_size"], kw["num_spks"]
    rw._sequence_model(rng, "fb_model.", F, kw["hidden_size"], kw["num_layers"], kw["proj_size"] * S * kw["df_order"] * 2, kw["shared_weights"],
                       kw["bn"], kw["use_pre_layer_norm_fb"], "proj", sd)
    return sd


def unit_var(eps=1e-5):
    """The fp32 running_var whose folded inverse deviation 1 / sqrt(var + eps) is exactly 1 in fp32 (engine.fold_batchnorm's operations)."""
    v = F32(1) - F32(eps)
    cands = [v]
    for _ in range(8):
        cands = [np.nextafter(cands[0], F32(0))] + cands + [np.nextafter(cands[-1], F32(2))]
    best = min(cands, key=lambda c: abs(float(F32(1) / np.sqrt(F32(c) + F32(eps))) - 1.0))
    return F32(best)


def cell_prefixes(sd):
    return [k[:-len("weight_hh")] for k in sd if k.endswith("cell.weight_hh")]


def cell_case(name, prefix, sd):
    """The scanref case of the cell at `prefix` of state dict `sd`: its (H, I, sharing) from the shapes, "x32" at layer 0."""
    w_hh, w_ih = sd[prefix + "weight_hh"], sd[prefix + "weight_ih"]
    H = w_hh.shape[1]
    layer = int(prefix.split("layers.")[1].split(".")[0])
    return sr.make_case(name, H, w_hh.shape[0] == H, "x32" if layer == 0 else "spike", I=w_ih.shape[1], T=1, salt=prefix)


def plant(front, kw, name, seed=3):
    """(state dict with case `name` in every GSN cell, {prefix: the case})."""
    sd = base_state_dict(front, kw, seed)
    cases = {}
    for pre in cell_prefixes(sd):
        p = cases[pre] = cell_case(name, pre, sd)
        assert sd[pre + "weight_hh"].shape == p["W_hh"].shape and sd[pre + "weight_ih"].shape == p["W_ih"].shape, pre
        sd[pre + "weight_hh"], sd[pre + "weight_ih"], sd[pre + "bias_ih"] = p["W_hh"].copy(), p["W_ih"].astype(F32), p["bias"].copy()
        assert pre + "batchnorm.weight" in sd, "the cases plant a BatchNorm scale and shift"
        H = p["H"]
        sd[pre + "batchnorm.weight"], sd[pre + "batchnorm.bias"] = p["alpha"].copy(), p["beta"].copy()
        sd[pre + "batchnorm.running_mean"], sd[pre + "batchnorm.running_var"] = np.zeros(H, F32), np.full(H, unit_var(), F32)
    return sd, cases


# ----------------------------------------------------------------------------------------------------------------------
# what the engine holds
# ----------------------------------------------------------------------------------------------------------------------
def held(cell, H, G, layer0, H_real=None):
    """The parameters of one cell as the engine holds them on the device (engine._Cell / fullband_engine._Layer; H: rows per gate as
    held, the padded size for the cIRM-GSN model, whose real size is H_real)."""
    from spiking_fullsubnet_amd.engine import unpack_w3

    def n(t):
        return t.detach().cpu().numpy()

    d = dict(H=H, G=G, H_real=H if H_real is None else H_real, kind="x32" if layer0 else "spike")
    d["W_hh"] = unpack_w3(n(cell.w_hh_q), n(cell.w_hh_dq), G * H, H)
    if layer0:
        d["W_ih"] = n(cell.w_ih_f32).astype(F32)
        assert d["W_ih"].shape[0] == G * H
    else:
        assert len(cell.w_ih_q) == G
        d["W_ih"] = np.concatenate([unpack_w3(n(pk), n(dq), H, H) for pk, dq in cell.w_ih_q])
    d["bias"], d["alpha"], d["beta"] = n(cell.bias).astype(F32), n(cell.alpha).astype(F32), n(cell.beta).astype(F32)
    assert d["bias"].shape == (2 * H,) and d["alpha"].shape == (H,) and d["beta"].shape == (H,)
    for k in ("W_hh", "W_ih"):
        if k == "W_hh" or not layer0:
            np.testing.assert_array_equal(sr.dequantise(d[k]), d[k], err_msg="the unpacked weights are on the 24-bit row grid")
    return d


def held_stacks(engine):
    """[[held cell per layer] per sequence model]: full-band first, then the sub-band groups (cIRM-GSN: one stack)."""
    if hasattr(engine, "layers"):
        return [[held(c, engine.Hp, engine.G, l == 0, engine.H) for l, c in enumerate(engine.layers)]]
    return [[held(c, s.H, c.G, l == 0) for l, c in enumerate(s.cells)] for s in [engine.fb] + list(engine.sb)]


# ----------------------------------------------------------------------------------------------------------------------
# the session's state
# ----------------------------------------------------------------------------------------------------------------------
def states(sess):
    """[[dict(spikes [hop][R][HP] int8, h (two [R][HP] int8), c [R][H] fp32) per layer] per sequence model]: views of the session's
    device memory; and a function returning the index of the next launch."""
    import torch
    hp = sess._hop
    assert hp is not None
    if "st" in hp:  # the cIRM-GSN session keeps one tensor per buffer
        st, work = hp["st"], hp["work"]
        out = [[dict(spikes=work["spikes"][l], h=[st["h"][l][0], st["h"][l][1]], c=st["c"][l]) for l in range(len(st["c"]))]]
        return out, lambda: int(hp["desc"].launch_index)
    assert len(hp["parts"]) == 1, "the batches of these tests fit one launch"
    part = hp["parts"][0]
    desc, pool = part["desc"], part["spool"]
    base, spec, nb, hop = pool.data_ptr(), sess.eng.spec, part["nb"], sess.hop

    def view(ptr, shape, dtype):
        off = int(ptr) - base
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        assert 0 <= off and off + nbytes <= pool.numel(), "a state pointer outside the part's arena"
        return pool[off:off + nbytes].view(dtype).view(shape)

    out = []
    for i, (dst, seq) in enumerate(zip([desc.fb] + [desc.sb[g] for g in range(spec.n_groups)], [sess.eng.fb] + list(sess.eng.sb))):
        R, H = nb * (1 if i == 0 else spec.units(i - 1)), seq.H
        HP = (H + 63) // 64 * 64
        out.append([dict(spikes=view(dst.layer[l].spikes, (hop, R, HP), torch.int8), h=[view(dst.layer[l].h[j], (R, HP), torch.int8) for j in (0, 1)],
                         c=view(dst.layer[l].c, (R, H), torch.float32)) for l in range(len(seq.cells))])
    return out, lambda: int(desc.launch_index)


def write_state(sess, planted):
    """planted[s][l] = (h0 [R][H] 0 / 1, c0 [R][H]) or None: into h[launch_index & 1] and c, the buffers the next launch reads."""
    import torch
    st, index = states(sess)
    par = index() & 1
    for s, layers in enumerate(planted):
        for l, hc in enumerate(layers):
            if hc is None:
                continue
            h0, c0 = hc
            H = h0.shape[1]
            st[s][l]["h"][par][:, :H].copy_(torch.from_numpy(np.ascontiguousarray(h0, np.int8)))
            st[s][l]["c"][:, :H].copy_(torch.from_numpy(np.ascontiguousarray(c0, F32)))
    torch.cuda.synchronize()


def record(sess, stft, before=None):
    """Steps the session through stft [B, F, T] (a device tensor), one launch at a time on the default stream, and copies the state
    out after every launch.  before(k): called before launch k (a restart, a planted state).  Returns dict(spk[s][l] uint8 [T][R][HP]
    (raw bytes), c[s][l] [launches][R][H], h[s][l] [launches][R][HP]: the buffer the NEXT launch reads, enh, mag)."""
    import torch
    st, index = states(sess)
    hop = sess.hop
    rec = dict(spk=[[[] for _ in s] for s in st], c=[[[] for _ in s] for s in st], h=[[[] for _ in s] for s in st])
    outs, mags = [], []
    for k, t0 in enumerate(range(0, stft.shape[2], hop)):
        if before is not None:
            before(k)
        e, m = sess.step(stft[:, :, t0:t0 + hop].contiguous())
        torch.cuda.synchronize()
        outs.append(e)
        mags.append(m)
        par = index() & 1
        for s, layers in enumerate(st):
            for l, d in enumerate(layers):
                rec["spk"][s][l].append(d["spikes"].cpu().numpy().view(np.uint8))
                rec["c"][s][l].append(d["c"].cpu().numpy())
                rec["h"][s][l].append(d["h"][par].cpu().numpy().view(np.uint8))
    sess.check_errors()
    for key, cat in (("spk", np.concatenate), ("c", np.stack), ("h", np.stack)):
        rec[key] = [[cat(x) for x in s] for s in rec[key]]
    rec["enh"], rec["mag"] = torch.cat(outs, -1), (None if mags[0] is None else torch.cat(mags, -1))
    return rec


# ----------------------------------------------------------------------------------------------------------------------
# comparison
# ----------------------------------------------------------------------------------------------------------------------
class Tally:
    """Worst error / tolerance (of c: the hops return no membranes), the unasserted share and the largest integer sum of one test."""

    def __init__(self, tag):
        self.tag, self.ratio, self.n, self.open, self.spikes, self.smax = tag, 0.0, 0, 0.0, 0, 0

    def add(self, res, ratio, spk, smax):
        self.ratio = max(self.ratio, ratio)
        self.n += spk.size
        self.open += res.unasserted * spk.size
        self.spikes += int(spk.sum())
        self.smax = max(self.smax, smax)

    def done(self):
        share = self.open / max(self.n, 1)
        print(f"HOP_EDGES {self.tag}: worst error / tolerance {self.ratio:.3f}, unasserted {share:.5f}")
        assert share <= 0.02, f"{self.tag}: {share:.4f} of the elements unasserted"
        assert self.spikes > 0


def layer_case(hd, inp, h0=None, c0=None):
    """The scanref case of a held cell on input `inp` [T][R][I] (layer 0) / [T][R][>= H] spikes (above)."""
    n_frames, R = inp.shape[:2]
    H = hd["H"]
    p = dict(H=H, R=R, T=n_frames, shared=hd["G"] == 1, kind=hd["kind"], bits=24, W_hh=hd["W_hh"], W_ih=hd["W_ih"], bias=hd["bias"],
             alpha=hd["alpha"], beta=hd["beta"], h0=np.zeros((R, H), F32) if h0 is None else np.asarray(h0, F32),
             c0=np.zeros((R, H), F32) if c0 is None else np.asarray(c0, F32))
    p["x" if hd["kind"] == "x32" else "s_in"] = np.ascontiguousarray(inp, F32) if hd["kind"] == "x32" else np.ascontiguousarray(inp[:, :, :H]).astype(np.int8)
    return p


def check_stack(tally, stack, x0, rec, s, hop, rows, t0, t1, state=None, t_up=None, skip0=False, where=""):
    """Frames [t0, t1) (whole launches) of rows `rows` of sequence model s against the fp64 reference started from `state` (per layer
    (h0, c0) of these rows, or None: zero) at frame t0.  x0 [t1 - t0][rows][I]: layer 0's input rows for exactly these frames and rows
    (None with skip0: layer 0 is not compared, layer 1 starts with t_up as given).  Returns (the last layer's t_valid, the layers'
    references: None where not compared)."""
    assert t0 % hop == 0 and t1 % hop == 0
    refs = []
    for l, hd in enumerate(stack):
        H, Hr = hd["H"], hd["H_real"]
        raw = rec["spk"][s][l][t0:t1, rows]
        spk = raw[:, :, :H] & 1
        tag = f"{tally.tag} {where} seq {s} layer {l}"
        assert not raw[:, :, H:].any(), f"{tag}: padding columns of the spike scratch"
        assert not spk[:, :, Hr:].any(), f"{tag}: a padded neuron fired"
        if l == 0 and skip0:
            refs.append(None)
            continue
        inp = x0 if l == 0 else rec["spk"][s][l - 1][t0:t1, rows] & 1
        hc = (None, None) if state is None or state[l] is None else (state[l][0][rows], state[l][1][rows])
        ref = sr.layer(layer_case(hd, inp, *hc))
        assert np.isfinite(ref["y"]).all() and np.isfinite(ref["tol"]).all(), tag
        res = sr.compare(spk, ref, None, t_up)
        assert res.ok, f"{tag}: {res.why}"
        worst = 0.0
        for k in range(t0 // hop, t1 // hop):
            tl = (k + 1) * hop - 1 - t0
            c, h = rec["c"][s][l][k][rows], rec["h"][s][l][k][rows]
            live = res.t_valid > tl
            fr = sr.worst(c[live][:, :H], ref["y"][tl][live], ref["tol"][tl][live])
            assert fr <= 1.0, f"{tag}: c after launch {k} is {fr:.3g} x the tolerance"
            worst = max(worst, fr)
            np.testing.assert_array_equal(h[:, :H], spk[tl], err_msg=f"{tag}: h after launch {k} is not the last frame's spikes")
            assert not h[:, H:].any(), f"{tag}: padding columns of h"
        tally.add(res, worst, spk, ref["smax"])
        refs.append(ref)
        t_up = res.t_valid
    return t_up, refs
