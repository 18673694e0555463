"""Scoring ragged batches on the device (sfsn_pit_sdr_ragged; PITWrapper(..., lengths=), PITWrapper.per_clip, metric.SISDR) against
sfsn_pit_sdr on each clip alone -- bit for bit where the ragged contract says so -- and against the composition and the derived bounds
of tests/pitraggedref.py elsewhere.  Through the C ABI every output is pre-filled with NaN (perm with -1) and the padding of est and
ref is NaN, so an element that is not written, or a padding sample that is read, fails the comparison."""
import ctypes

import numpy as np
import pytest
import torch

import pitraggedref as prr
import pitref
import refweights as rw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = [c[0] for c in prr.CASES]
ZM = [True, False]
_refs = {}


def _case(name, zm):
    """(NaN-padded est, NaN-padded ref, cotangent, lengths, composition) of a case, computed once and shared (never modified)."""
    if (name, zm) not in _refs:
        e, t = prr.make_inputs(name)
        w = prr.cotangent(name)
        lens = prr.lengths(name)
        _refs[name, zm] = (prr.padded(e, lens), prr.padded(t, lens), w, lens, prr.reference(e, t, lens, zm, cot=w))
    return _refs[name, zm]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _lens(lens):
    return torch.tensor(lens, dtype=torch.int32, device=DEV)


def _host(x):
    return x.cpu().numpy() if x is not None else None


def _bits(a, b):
    """Equal bit for bit (NaN == NaN of the same bits, +0 != -0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _c_plain(e, t, zm=True, eps=pitref.EPS, cot=None, want_grad=True):
    """sfsn_pit_sdr on [B, S, L] device tensors -> dict of numpy results; outputs pre-filled with NaN (perm with -1)."""
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    B, S, n = e.shape
    pit_mode = cot is None
    pair = torch.full((B, S, S), float("nan"), device=DEV)
    perm = torch.full((B, S), -1, dtype=torch.int32, device=DEV) if pit_mode else None
    loss = torch.full((1,), float("nan"), device=DEV) if pit_mode else None
    grad = torch.full_like(e, float("nan")) if want_grad else None
    reordered = torch.full_like(e, float("nan")) if pit_mode else None
    scratch = torch.empty(L.sfsn_pit_sdr_scratch_bytes(B, S, n), dtype=torch.uint8, device=DEV)
    ptr = lambda x: x.data_ptr() if x is not None else None
    _lib.check(L.sfsn_pit_sdr(e.data_ptr(), t.data_ptr(), B, S, n, int(zm), eps, ptr(cot), pair.data_ptr(), ptr(perm), ptr(loss), ptr(grad),
                              ptr(reordered), scratch.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "sfsn_pit_sdr")
    torch.cuda.synchronize()
    return dict(pair=_host(pair), perm=_host(perm), loss=(_host(loss)[0] if pit_mode else None), grad=_host(grad), reordered=_host(reordered))


def _c_ragged(e, t, lens, zm=True, eps=pitref.EPS, cot=None, want_grad=True, want_reordered=True, stream=None):
    """sfsn_pit_sdr_ragged on [B, S, Lmax] device tensors with the lengths `lens` -> dict of numpy results (None where not asked for)."""
    from spiking_fullsubnet_amd import _lib
    L = _lib.lib()
    B, S, n = e.shape
    st = torch.cuda.current_stream() if stream is None else stream
    pit_mode = cot is None
    with torch.cuda.stream(st):
        clip_len = _lens(lens)
        pair = torch.full((B, S, S), float("nan"), device=DEV)
        perm = torch.full((B, S), -1, dtype=torch.int32, device=DEV) if pit_mode else None
        clip_loss = torch.full((B,), float("nan"), device=DEV) if pit_mode else None
        loss = torch.full((1,), float("nan"), device=DEV) if pit_mode else None
        grad = torch.full_like(e, float("nan")) if want_grad else None
        reordered = torch.full_like(e, float("nan")) if pit_mode and want_reordered else None
        si_sdr = torch.full((B, S), float("nan"), device=DEV) if pit_mode else None
        scratch = torch.empty(L.sfsn_pit_sdr_scratch_bytes(B, S, n), dtype=torch.uint8, device=DEV)
        ptr = lambda x: x.data_ptr() if x is not None else None
        _lib.check(L.sfsn_pit_sdr_ragged(e.data_ptr(), t.data_ptr(), B, S, n, clip_len.data_ptr(), int(zm), eps, ptr(cot), pair.data_ptr(),
                                         ptr(perm), ptr(clip_loss), ptr(loss), ptr(grad), ptr(reordered), ptr(si_sdr), scratch.data_ptr(),
                                         ctypes.c_void_p(st.cuda_stream)), "sfsn_pit_sdr_ragged")
    st.synchronize()
    return dict(pair=_host(pair), perm=_host(perm), clip_loss=_host(clip_loss), loss=(_host(loss)[0] if pit_mode else None), grad=_host(grad),
                reordered=_host(reordered), si_sdr=_host(si_sdr))


def _min_losses(pair):
    """fp32 of each clip's smallest permutation loss from the fp32 `pair`, added as the kernel adds them (fp64, j ascending, / S)."""
    B, S, _ = pair.shape
    out = np.zeros(B, np.float32)
    for b in range(B):
        best = None
        for p in pitref.all_perms(S):
            l = 0.0
            for j in range(S):
                l += float(pair[b, p[j], j])
            l /= S
            best = l if best is None or l < best else best
        out[b] = np.float32(best)
    return out


@pytest.mark.parametrize("zm", ZM)
@pytest.mark.parametrize("name", [c[0] for c in pitref.CASES])
def test_full_lengths_have_the_bits_of_the_equal_length_call(name, zm):
    e, t = (_t(x) for x in pitref.make_inputs(name))
    w = _t(pitref.cotangent(name))
    B, S, n = e.shape
    plain, got = _c_plain(e, t, zm), _c_ragged(e, t, [n] * B, zm)
    for k in ("pair", "perm", "loss", "grad", "reordered"):
        assert _bits(got[k], plain[k]), k
    assert _bits(got["clip_loss"], _min_losses(plain["pair"]))
    assert np.all(np.isfinite(got["si_sdr"]))
    fwd = _c_ragged(e, t, [n] * B, zm, want_grad=False)
    assert fwd["grad"] is None
    for k in ("pair", "perm", "loss", "reordered", "clip_loss", "si_sdr"):
        assert _bits(fwd[k], got[k]), k
    plain_pw, got_pw = _c_plain(e, t, zm, cot=w), _c_ragged(e, t, [n] * B, zm, cot=w)
    assert _bits(got_pw["pair"], plain_pw["pair"]) and _bits(got_pw["grad"], plain_pw["grad"])


@pytest.mark.parametrize("zm", ZM)
@pytest.mark.parametrize("name", NAMES)
def test_ragged_table_clip_by_clip(name, zm):
    e, t, w, lens, ref = _case(name, zm)
    de, dt_, dw = _t(e), _t(t), _t(w)
    got = _c_ragged(de, dt_, lens, zm)
    got_pw = _c_ragged(de, dt_, lens, zm, cot=dw)
    for k in ("pair", "clip_loss", "loss", "grad", "reordered", "si_sdr"):
        assert not np.any(np.isnan(got[k])), k  # every element written, no padding sample read
    assert got["perm"].min() >= 0 and not np.any(np.isnan(got_pw["pair"])) and not np.any(np.isnan(got_pw["grad"]))
    for b, n in enumerate(lens):  # the bits of sfsn_pit_sdr on a contiguous copy of the clip alone
        eb, tb = _t(e[b:b + 1, :, :n]), _t(t[b:b + 1, :, :n])
        alone = _c_plain(eb, tb, zm, want_grad=False)
        assert _bits(got["pair"][b], alone["pair"][0]) and _bits(got["perm"][b], alone["perm"][0]), (b, n)
        assert _bits(got["clip_loss"][b:b + 1], np.array([alone["loss"]], np.float32)), (b, n)
        alone_pw = _c_plain(eb, tb, zm, cot=_t(w[b:b + 1]))
        assert _bits(got_pw["pair"][b], alone_pw["pair"][0]) and _bits(got_pw["grad"][b, :, :n], alone_pw["grad"][0]), (b, n)
        assert _bits(got["reordered"][b, :, :n], e[b, got["perm"][b], :n]), (b, n)  # the gather of the input's bits
        for x in (got["grad"], got["reordered"], got_pw["grad"]):  # +0.0 on every tail
            assert not x[b, :, n:].view(np.uint32).any(), (b, n)
    bad, used = prr.outside(got, ref)  # pair, clip_loss, loss, the PIT gradient and si_sdr within the bounds; perm, reordered equal
    bad_pw, used_pw = prr.outside(dict(pair=got_pw["pair"], grad_pw=got_pw["grad"]), ref)
    print(name, zm, "share of each bound used:", used, used_pw)
    assert not bad and not bad_pw, (bad, used, bad_pw, used_pw)
    fwd = _c_ragged(de, dt_, lens, zm, want_grad=False)  # forward only, and forward without reordered: the same bits
    bare = _c_ragged(de, dt_, lens, zm, want_grad=False, want_reordered=False)
    assert fwd["grad"] is None and bare["reordered"] is None and _bits(fwd["reordered"], got["reordered"])
    for k in ("pair", "perm", "clip_loss", "loss", "si_sdr"):
        assert _bits(fwd[k], got[k]) and _bits(bare[k], got[k]), k
    assert _bits(_c_ragged(de, dt_, lens, zm, cot=dw, want_grad=False)["pair"], got["pair"])


def test_lengths_outside_the_row_are_clamped_on_the_device():
    """The C ABI trusts nothing it reads on the device: a length beyond the row is the row's, a negative one is an empty clip (NaN
    results for that clip, zeros in its rows of grad_est and reordered) and its neighbours are untouched."""
    e, t, _, lens, _ = _case("r3s2", True)
    good = _c_ragged(_t(e), _t(t), lens)
    got = _c_ragged(_t(e), _t(t), [1 << 30, -5, lens[2]])
    assert not got["grad"][1].view(np.uint32).any() and not got["reordered"][1].view(np.uint32).any()
    for k in ("pair", "perm", "clip_loss", "si_sdr", "reordered"):
        assert _bits(got[k][0], good[k][0]) and _bits(got[k][2], good[k][2]), k


@pytest.mark.parametrize("name,zm", [("r3s2", True), ("r2s3_odd", False), ("r5s4", True), ("r3s2_chunks", True)])
def test_python_drop_ins_return_the_bits_of_the_c_call(name, zm):
    from spiking_fullsubnet_amd import metric, pit
    e, t, w, lens, ref = _case(name, zm)
    c = _c_ragged(_t(e), _t(t), lens, zm)
    wrapper = pit.PITWrapper(pit.PairwiseNegSDR(zero_mean=zm))
    est = _t(e).requires_grad_(True)
    loss, reordered = wrapper(est, _t(t), lengths=lens)
    assert loss.shape == () and loss.item() == float(c["loss"]) and _bits(_host(reordered), c["reordered"])
    assert loss.requires_grad and not reordered.requires_grad
    (2.5 * loss).backward()  # backward scales the stored gradient
    assert _bits(_host(est.grad), (np.float32(2.5) * c["grad"]).astype(np.float32))
    for lengths in (torch.tensor(lens), _lens(lens)):  # a CPU int tensor; an int32 device tensor (trusted, no host work)
        l2, r2, perm, pair = wrapper.full(_t(e), _t(t), lengths=lengths)
        assert torch.equal(l2, loss.detach()) and torch.equal(r2, reordered)
        assert perm.dtype == torch.int64 and np.array_equal(_host(perm), c["perm"]) and _bits(_host(pair), c["pair"])
    per = wrapper.per_clip(_t(e), _t(t), lengths=lens)  # agrees with full, adds the clips' own numbers
    assert torch.equal(per.perm, perm) and torch.equal(per.pair, pair) and torch.equal(per.reordered, reordered)
    assert _bits(_host(per.loss), c["clip_loss"]) and _bits(_host(per.si_sdr), c["si_sdr"])
    assert all(x.device.type == "cuda" for x in per)
    # PairwiseNegSDR alone with lengths, backpropagated through a weighted sum: a second ragged call in pairwise mode
    est2 = _t(e).requires_grad_(True)
    pw = pit.PairwiseNegSDR(zero_mean=zm)(est2, _t(t), lengths=lens)
    assert _bits(_host(pw.detach()), c["pair"])
    (pw * _t(w)).sum().backward()
    assert _bits(_host(est2.grad), _c_ragged(_t(e), _t(t), lens, zm, cot=_t(w))["grad"])
    # metric.SISDR: rows as given.  On a clip's matched rows it is per_clip's row; its mean is the reference's reduce_mean value
    sisdr = metric.SISDR()
    for b, n in enumerate(lens):
        rows = sisdr(per.reordered[b, :, :n], _t(t[b, :, :n]), reduce_mean=False)["si_sdr"]
        assert rows.device.type == "cuda" and torch.equal(rows, per.si_sdr[b])
        mean = sisdr(per.reordered[b, :, :n], _t(t[b, :, :n]))["si_sdr"]
        assert isinstance(mean, float) and mean == float(per.si_sdr[b].mean())
        assert sisdr(per.reordered[b], _t(t[b]), lengths=n)["si_sdr"] == mean  # the padded rows with the clip's length
        one = sisdr(per.reordered[b, 0, :n], _t(t[b, 0, :n]), reduce_mean=False)["si_sdr"]  # [L]
        assert one.shape == () and float(one) == float(per.si_sdr[b, 0])
    batch = sisdr(per.reordered, _t(t), reduce_mean=False, lengths=lens)["si_sdr"]  # [B, S, L] with lengths
    assert torch.equal(batch, per.si_sdr)
    m, mtol = prr.sisdr_mean(ref["si_sdr"], ref["si_sdr_tol"])
    assert abs(sisdr(per.reordered, _t(t), lengths=lens)["si_sdr"] - m) <= mtol


@pytest.mark.parametrize("name,zm", [("b3s2_L1000", True), ("b2s3_L4097", False)])
def test_lengths_none_is_todays_path(name, zm):
    from spiking_fullsubnet_amd import pit
    e, t = (_t(x) for x in pitref.make_inputs(name))
    c = _c_plain(e, t, zm)
    wrapper = pit.PITWrapper(pit.PairwiseNegSDR(zero_mean=zm))
    est = e.clone().requires_grad_(True)
    loss, reordered, perm, pair = wrapper.full(est, t, lengths=None)
    loss.backward()
    assert loss.item() == float(c["loss"]) and _bits(_host(reordered), c["reordered"]) and _bits(_host(pair), c["pair"])
    assert np.array_equal(_host(perm), c["perm"]) and _bits(_host(est.grad), c["grad"])
    per = wrapper.per_clip(e, t)  # every clip full length: the equal-length call's bits, clip by clip
    assert torch.equal(per.pair, pair) and torch.equal(per.perm, perm) and torch.equal(per.reordered, reordered)
    assert _bits(_host(per.loss), _min_losses(c["pair"]))
    assert _bits(_host(pit.PairwiseNegSDR(zero_mean=zm)(e, t)), c["pair"])


def test_two_streams_and_a_graph_replay_are_bit_identical():
    from spiking_fullsubnet_amd import pit
    e, t, _, lens, _ = _case("r3s2_chunks", True)
    a = _c_ragged(_t(e), _t(t), lens)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    b = _c_ragged(_t(e), _t(t), lens, stream=side)
    for k in a:
        assert _bits(a[k], b[k]), k
    # device lengths make no host work, so the call captures; the replay reads the lengths then in the tensor
    wrapper = pit.PITWrapper(pit.PairwiseNegSDR())
    de, dt_, dl = _t(e), _t(t), _lens([7, 7, 7])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        per = wrapper.per_clip(de, dt_, lengths=dl)
    dl.copy_(_lens(lens))
    g.replay()
    torch.cuda.synchronize()
    assert _bits(_host(per.loss), a["clip_loss"]) and _bits(_host(per.si_sdr), a["si_sdr"]) and _bits(_host(per.reordered), a["reordered"])


def test_forward_ragged_then_per_clip_equals_each_clip_alone():
    """The evaluation loop of the wsj0-mix recipes on one tiny two-speaker live model: four clips of different lengths through
    forward_ragged and per_clip, against model(clip) and PITWrapper.full on each clip alone."""
    import spiking_fullsubnet_amd as pkg
    kw = rw.LIVE_TINY_2SPK
    m = pkg.SpikingFullSubNet(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in rw.live_state_dict(kw, 12).items()}, strict=True)
    m = m.eval().to(DEV)
    lens = [2944, 1500, 2048, 777]
    rng = np.random.default_rng(21)
    waves = _t((0.05 * rng.standard_normal((4, max(lens)))).astype(np.float32))
    refs = _t((0.05 * rng.standard_normal((4, 2, max(lens)))).astype(np.float32))
    wrapper = pkg.PITWrapper(pkg.PairwiseNegSDR())
    with torch.no_grad():
        y = m.forward_ragged(waves, lens)[0]
        assert y.shape == refs.shape
        per = wrapper.per_clip(y, refs, lengths=lens)
        for b, n in enumerate(lens):
            y_b = m(waves[b:b + 1, :n].contiguous())[0]
            loss, reordered, perm, pair = wrapper.full(y_b, refs[b:b + 1, :, :n].contiguous())
            assert torch.equal(per.perm[b], perm[0]) and torch.equal(per.pair[b], pair[0]), b
            assert _bits(_host(per.loss[b:b + 1]), _host(loss.reshape(1))), b
            assert torch.equal(per.reordered[b, :, :n], reordered[0]) and not bool(per.reordered[b, :, n:].any()), b
    assert bool(torch.isfinite(per.si_sdr).all())
