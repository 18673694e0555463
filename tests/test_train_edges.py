"""The training-mode layer calls of csrc/sfsn_train.hip on the device, step by step against the fp64 reference of tests/trainref.py.

Every call goes through the C ABI as training.GSNLayerTrainFn / GSNLayersTrainFn make it: on the current stream, one launch at a time,
each call and direction with a freshly zeroed scratch buffer, the error word (the scratch's last four words) read after a synchronise
following every launch.  Three kernel families see the same inputs:

* "chain": sfsn_gsn_train_seq_fwd_multi / _bwd_multi driven ONE FRAME PER CALL (T = 1, the chunked form of the ABI: h0 / c0 / has_prev /
  dc_in / dc_out), which hands out dL/dc of every step;
* "whole": the whole sequence in one launch (sfsn_gsn_train_seq_fwd / _bwd, or the multi entries) -- must equal the chain BIT FOR BIT in
  every output, the running statistics, d_bn_w / d_bn_b and dc_out; its forward is also judged against fp64 directly;
* "step": sfsn_gsn_train_step_fwd / _bwd, a launch per time step with a k-ordered fma chain for the products -- judged against the same
  fp64 step under the same bound (NOT bit for bit against the others: the products differ in summation order).

Every reference step is evaluated on the device's own carried state (trainref.judge_fwd / judge_bwd), so no spike flip can cascade.
Each test prints, per output, the worst error / bound it saw (lines starting with TRAIN_EDGES)."""
import ctypes

import numpy as np
import pytest
import torch

import trainref as tr
from spiking_fullsubnet_amd import _lib, training

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def _up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, F32)).to(DEV)


def _ptr(t, off=0):
    return None if t is None else t.data_ptr() + 4 * off


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _finish(scrs):
    """Wait for the launch and fail with the exchange message if it set an error word."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a device fault: nothing more may be started on this GPU from this process
        pytest.exit(f"device fault, session ended: {e}", returncode=3)
    for s in scrs:
        if int(s[-4:].max().item()) != 0:
            pytest.fail(training._EXCHANGE_FAILED)


def _ok(rc, what):
    assert rc == _lib.SFSN_OK, f"{what}: status {rc}"


class Call:
    """One layer call's tensors on the device.  `saved`: synthetic forward tensors (backward-only cases)."""

    def __init__(self, p, saved=None):
        self.p, (T, R, H) = p, (p["T"], p["R"], p["H"])
        self.use_bn, self.sh = p["bn_w"] is not None, p["shared"]
        self.GH = H if self.sh else 2 * H
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=DEV)
        self.z, self.w, self.bias, self.bn_w, self.bn_b = (_up(p[k]) for k in ("z", "w_hh", "bias", "bn_w", "bn_b"))
        self.dh_up, self.h0 = _up(p["dh_up"]), _up(p["h0"])
        self.has_state = p["c0"] is not None
        self.zero = z(R, H)
        self.saved = saved
        self.reset()

    def reset(self):
        p, (T, R, H) = self.p, (self.p["T"], self.p["R"], self.p["H"])
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=DEV)
        nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)
        self.u = nan(T + 1, R, H)  # frame 0: the membrane before the first frame (c0, or zero) -- what has_prev lets the backward read
        self.u[0] = _up(p["c0"]) if self.has_state else 0
        self.spikes, self.f, self.g = nan(T, R, H), nan(T, R, H), nan(T, R, H)
        self.xhat, self.invstd = (nan(T, R, H), nan(T, H)) if self.use_bn else (None, None)
        if self.saved is not None:
            s = self.saved
            self.u[1:], self.f, self.g = _up(s["u"]), _up(s["f"]), _up(s["g"])
            self.xhat, self.invstd = _up(s["xhat"]), _up(s["invstd"])
        stats = self.use_bn and p["stats"]
        self.rm, self.rv = (_up(p["rm0"]), _up(p["rv0"])) if stats else (None, None)
        self.rm_t, self.rv_t = [], []
        self.d_gates, self.d_z, self.dc = nan(T, R, 2 * H), (nan(T, R, H) if self.sh else None), nan(T, R, H)
        self.dbw, self.dbb = (z(H), z(H)) if self.use_bn else (None, None)
        self.dbw_t, self.dbb_t = {}, {}

    # -- ABI structs for frames [t0, t0 + n) -------------------------------------------------------------------------
    def fwd_struct(self, c, t0, n, scr):
        p, R, H, GH = self.p, self.p["R"], self.p["H"], self.GH
        c.z, c.w_hh, c.bias, c.bn_w, c.bn_b = _ptr(self.z, t0 * R * GH), _ptr(self.w), _ptr(self.bias), _ptr(self.bn_w), _ptr(self.bn_b)
        c.running_mean, c.running_var = _ptr(self.rm), _ptr(self.rv)
        c.momentum, c.eps, c.R, c.T = tr.mom_arg(p, t0), float(p["eps"]), R, n
        c.spikes, c.u, c.f, c.g = _ptr(self.spikes, t0 * R * H), _ptr(self.u, (t0 + 1) * R * H), _ptr(self.f, t0 * R * H), _ptr(self.g, t0 * R * H)
        c.xhat, c.invstd, c.scratch = _ptr(self.xhat, t0 * R * H), _ptr(self.invstd, t0 * H), scr.data_ptr()
        if t0 > 0:
            c.h0, c.c0 = _ptr(self.spikes, (t0 - 1) * R * H), _ptr(self.u, t0 * R * H)
        elif self.has_state:
            c.h0, c.c0 = _ptr(self.h0), _ptr(self.u)
        else:
            c.h0, c.c0 = None, None

    def bwd_struct(self, c, t0, n, scr):
        p, T, R, H, GH = self.p, self.p["T"], self.p["R"], self.p["H"], self.GH
        c.w_hh, c.dh_up, c.u, c.f, c.g, c.R, c.T = _ptr(self.w), _ptr(self.dh_up, t0 * R * H), _ptr(self.u, (t0 + 1) * R * H), _ptr(self.f, t0 * R * H), _ptr(self.g, t0 * R * H), R, n
        c.xhat, c.invstd, c.bn_w = _ptr(self.xhat, t0 * R * H), _ptr(self.invstd, t0 * H), _ptr(self.bn_w)
        c.d_gates, c.d_z, c.d_bn_w, c.d_bn_b = _ptr(self.d_gates, t0 * R * 2 * H), _ptr(self.d_z, t0 * R * H), _ptr(self.dbw), _ptr(self.dbb)
        c.scratch = scr.data_ptr()
        c.has_prev = int(t0 > 0 or self.has_state)
        c.dc_in = None if t0 + n == T else _ptr(self.dc, (t0 + n) * R * H)
        c.dc_out = _ptr(self.dc, t0 * R * H)

    def snap_fwd(self):
        if self.rm is not None:
            self.rm_t.append(self.rm.clone()); self.rv_t.append(self.rv.clone())

    def snap_bwd(self, t):
        if self.use_bn:
            self.dbw_t[t], self.dbb_t[t] = self.dbw.clone(), self.dbb.clone()

    # -- results in trainref's layout --------------------------------------------------------------------------------
    def fwd_out(self):
        n = lambda t: None if t is None else t.cpu().numpy()
        st = lambda l: np.stack([x.cpu().numpy() for x in l]) if l else None
        return dict(spikes=n(self.spikes), u=n(self.u[1:]), xhat=n(self.xhat), f=n(self.f), g=n(self.g), invstd=n(self.invstd),
                    rm=st(self.rm_t), rv=st(self.rv_t), rm_end=n(self.rm), rv_end=n(self.rv))

    def bwd_out(self):
        n = lambda t: None if t is None else t.cpu().numpy()
        T = self.p["T"]
        st = lambda d: np.stack([d[t].cpu().numpy() for t in range(T)]) if len(d) == T else None
        return dict(d_gates=n(self.d_gates), d_z=n(self.d_z), dc=n(self.dc), dbw=st(self.dbw_t), dbb=st(self.dbb_t), dbw_end=n(self.dbw), dbb_end=n(self.dbb))


def _scr_seq(c):
    return torch.zeros((_lib.lib().sfsn_train_seq_scratch_bytes(c.p["R"], c.p["H"]) // 4,), dtype=torch.int32, device=DEV)


def _multi_check(calls):
    L, H, sh = _lib.lib(), calls[0].p["H"], calls[0].sh
    Rs = (ctypes.c_int * len(calls))(*[c.p["R"] for c in calls])
    _ok(L.sfsn_gsn_train_multi_check(Rs, len(calls), H, int(sh)), f"sfsn_gsn_train_multi_check({list(Rs)}, H={H})")


def _launch_multi(calls, t0s, ns, fwd):
    """ONE launch of the multi entry for frames [t0, t0 + n) of every call."""
    L, H, sh = _lib.lib(), calls[0].p["H"], calls[0].sh
    _multi_check(calls)
    arr = ((_lib.TrainSeqFwd if fwd else _lib.TrainSeqBwd) * len(calls))()
    scrs = [_scr_seq(c) for c in calls]
    for i, c in enumerate(calls):
        (c.fwd_struct if fwd else c.bwd_struct)(arr[i], t0s[i], ns[i], scrs[i])
    with torch.cuda.device(DEV):
        fn = L.sfsn_gsn_train_seq_fwd_multi if fwd else L.sfsn_gsn_train_seq_bwd_multi
        _ok(fn(arr, len(calls), max(ns), H, int(sh), _stream()), fn.__name__)
    _finish(scrs)


def run_chain(calls, backward=True, forward=True):
    """One frame per launch, forward t = 0 .. T - 1 and backward t = T - 1 .. 0 (calls of different T: a call leaves the launches beyond
    its last frame)."""
    Tm = max(c.p["T"] for c in calls)
    for t in (range(Tm) if forward else ()):
        live = [c for c in calls if t < c.p["T"]]
        _launch_multi(live, [t] * len(live), [1] * len(live), True)
        for c in live:
            c.snap_fwd()
    for t in (range(Tm - 1, -1, -1) if backward else ()):
        live = [c for c in calls if t < c.p["T"]]
        _launch_multi(live, [t] * len(live), [1] * len(live), False)
        for c in live:
            c.snap_bwd(t)


def run_whole(calls, forward=True, plain=False):
    """The whole sequence in one launch per direction.  plain: the single-call entries (one call, no start state)."""
    L = _lib.lib()
    if not plain:
        if forward:
            _launch_multi(calls, [0] * len(calls), [c.p["T"] for c in calls], True)
        _launch_multi(calls, [0] * len(calls), [c.p["T"] for c in calls], False)
        return
    (c,) = calls
    p, T, R, H = c.p, c.p["T"], c.p["R"], c.p["H"]
    P = ctypes.c_void_p
    _multi_check(calls)
    with torch.cuda.device(DEV):
        if forward:
            scr = _scr_seq(c)
            _ok(L.sfsn_gsn_train_seq_fwd(P(_ptr(c.z)), P(_ptr(c.w)), P(_ptr(c.bias)), P(_ptr(c.bn_w)), P(_ptr(c.bn_b)), P(_ptr(c.rm)), P(_ptr(c.rv)),
                                         tr.mom_arg(p, 0), float(p["eps"]), T, R, H, int(c.sh), P(_ptr(c.zero)), P(_ptr(c.spikes)), P(_ptr(c.u, R * H)),
                                         P(_ptr(c.xhat)), P(_ptr(c.f)), P(_ptr(c.g)), P(_ptr(c.invstd)), P(scr.data_ptr()), _stream()), "sfsn_gsn_train_seq_fwd")
            _finish([scr])
        scr = _scr_seq(c)
        _ok(L.sfsn_gsn_train_seq_bwd(P(_ptr(c.w)), P(_ptr(c.dh_up)), P(_ptr(c.u, R * H)), P(_ptr(c.xhat)), P(_ptr(c.f)), P(_ptr(c.g)), P(_ptr(c.invstd)),
                                     P(_ptr(c.bn_w)), T, R, H, int(c.sh), None, P(_ptr(c.d_gates)), P(_ptr(c.d_z)), None, P(_ptr(c.dbw)), P(_ptr(c.dbb)),
                                     P(scr.data_ptr()), _stream()), "sfsn_gsn_train_seq_bwd")
        _finish([scr])


def run_steps(c, forward=True):
    """The step entries, a launch per time step, dc_next / dc_prev carried explicitly."""
    L, p, T, R, H, GH = _lib.lib(), c.p, c.p["T"], c.p["R"], c.p["H"], c.GH
    P = ctypes.c_void_p
    _ok(L.sfsn_gsn_train_step_check(R, H, int(c.sh)), f"sfsn_gsn_train_step_check(R={R}, H={H})")
    scr_new = lambda: torch.zeros((L.sfsn_train_scratch_bytes(H) // 4,), dtype=torch.int32, device=DEV)
    RH = R * H
    with torch.cuda.device(DEV):
        for t in (range(T) if forward else ()):
            scr = scr_new()
            mom = tr.mom_arg(p, t)
            hp = _ptr(c.spikes, (t - 1) * RH) if t else (_ptr(c.h0) if c.has_state else _ptr(c.zero))
            _ok(L.sfsn_gsn_train_step_fwd(P(_ptr(c.z, t * R * GH)), P(_ptr(c.w)), P(_ptr(c.bias)), P(hp), P(_ptr(c.u, t * RH)), P(_ptr(c.bn_w)), P(_ptr(c.bn_b)),
                                          P(_ptr(c.rm)), P(_ptr(c.rv)), mom if mom >= 0 else 1.0 / -mom, float(p["eps"]), R, H, int(c.sh), P(_ptr(c.spikes, t * RH)),
                                          P(_ptr(c.u, (t + 1) * RH)), P(_ptr(c.xhat, t * RH)), P(_ptr(c.f, t * RH)), P(_ptr(c.g, t * RH)), P(_ptr(c.invstd, t * H)),
                                          P(scr.data_ptr()), 1, _stream()), "sfsn_gsn_train_step_fwd")
            _finish([scr])
            c.snap_fwd()
        dzs = c.d_z if c.sh else c.d_gates
        for t in range(T - 1, -1, -1):
            scr, last = scr_new(), t == T - 1
            _ok(L.sfsn_gsn_train_step_bwd(None if last else P(_ptr(dzs, (t + 1) * R * GH)), P(_ptr(c.w)), P(_ptr(c.dh_up, t * RH)), None,
                                          None if last else P(_ptr(c.dc, (t + 1) * RH)), P(_ptr(c.u, (t + 1) * RH)), P(_ptr(c.xhat, t * RH)), P(_ptr(c.f, t * RH)),
                                          P(_ptr(c.g, t * RH)), P(_ptr(c.u, t * RH)), P(_ptr(c.invstd, t * H)), P(_ptr(c.bn_w)), R, H, int(c.sh),
                                          P(_ptr(c.d_gates, t * R * 2 * H)), P(_ptr(c.d_z, t * RH)), P(_ptr(c.dc, t * RH)), P(_ptr(c.dbw)), P(_ptr(c.dbb)),
                                          P(scr.data_ptr()), 1, _stream()), "sfsn_gsn_train_step_bwd")
            _finish([scr])
            c.snap_bwd(t)


def _same_bits(a, b, what, fails):
    """Equal words -- and numbers: the outputs are prefilled with NaN, so an element neither launch wrote would compare equal."""
    for k in a:
        if a[k] is None or b.get(k) is None:
            continue
        if not (np.isfinite(a[k]).all() and np.isfinite(b[k]).all()):
            fails.append(f"{what}: {k} holds {int((~np.isfinite(a[k])).sum())} / {int((~np.isfinite(b[k])).sum())} values that are not finite")
        x, y = np.ascontiguousarray(a[k], F32).view(np.uint32), np.ascontiguousarray(b[k], F32).view(np.uint32)
        if not np.array_equal(x, y):
            fails.append(f"{what}: {k} differs in {int((x != y).sum())} of {x.size} words")


FWD_BITS = ("spikes", "u", "xhat", "f", "g", "invstd", "rm_end", "rv_end")
BWD_BITS = ("d_gates", "d_z", "dbw_end", "dbb_end")


def check_calls(ps, worst, saved=None, steps=True, plain=False):
    """The three kernel families on the cases `ps` (one launch holds all of them: a multi launch when there are several).  Returns the
    list of failures; fills worst['chain' | 'whole' | 'step'] with error / bound figures."""
    fails = []
    syn = saved is not None
    calls = [Call(p, None if not syn else saved[i]) for i, p in enumerate(ps)]
    fwd_of = lambda c, o: dict(u=c.saved["u"], xhat=c.saved["xhat"], f=c.saved["f"], g=c.saved["g"], invstd=c.saved["invstd"]) if syn else o
    # (1) one frame per launch against fp64
    run_chain(calls, forward=not syn)
    chain = [(c.fwd_out(), c.bwd_out()) for c in calls]
    for c, (fo, bo) in zip(calls, chain):
        if not syn:
            fails += ["chain " + s for s in tr.judge_fwd(c.p, fo, worst["chain"])]
        fails += ["chain " + s for s in tr.judge_bwd(c.p, fwd_of(c, fo), bo, worst["chain"])]
    # (2) the whole sequence in one launch: the chain bit for bit; its forward against fp64 directly
    for c in calls:
        c.reset()
    run_whole(calls, forward=not syn, plain=plain)
    for c, (fo, bo) in zip(calls, chain):
        wf, wb = c.fwd_out(), c.bwd_out()
        if not syn:
            _same_bits({k: wf[k] for k in FWD_BITS}, fo, f"whole == chain ({c.p['name']}, forward)", fails)
            fails += ["whole " + s for s in tr.judge_fwd(c.p, wf, worst["whole"], running_too=False)]
        _same_bits({k: wb[k] for k in BWD_BITS}, bo, f"whole == chain ({c.p['name']}, backward)", fails)
        if not plain:  # dc_out of the whole call is dL/dc carried out of its FIRST frame (the plain entries do not hand it out)
            _same_bits(dict(dc0=wb["dc"][0]), dict(dc0=bo["dc"][0]), f"whole == chain ({c.p['name']}, dc_out)", fails)
    # (3) the step entries against fp64
    for c in (calls if steps else ()):
        c.reset()
        run_steps(c, forward=not syn)
        fo, bo = c.fwd_out(), c.bwd_out()
        if not syn:
            fails += ["step " + s for s in tr.judge_fwd(c.p, fo, worst["step"])]
        fails += ["step " + s for s in tr.judge_bwd(c.p, fwd_of(c, fo), bo, worst["step"])]
    return fails


def _worsts():
    return dict(chain=tr.Worst(), whole=tr.Worst(), step=tr.Worst())


def _report(tag, worst):
    for fam, w in worst.items():
        if w:
            print(f"TRAIN_EDGES {tag} {fam}: {w.line()}")


@pytest.mark.parametrize("name", list(tr.CASES))
@pytest.mark.parametrize("H,R,shared", tr.GEOMETRIES, ids=[f"H{H}-R{R}-{'shared' if s else 'separate'}" for H, R, s in tr.GEOMETRIES])
def test_cases_against_fp64(H, R, shared, name):
    """(1), (2), (3): a case on a geometry at T in {1, 2, 7} -- one-frame chain and step entries under the fp64 bounds with the spike rule
    and its cap, the whole-sequence call equal to the chain bit for bit (the plain entries; the `state` case, whose start state only the
    multi entries take, through those -- with dc_out)."""
    assert tr.blocking(R, H, shared)[0] <= 16
    fails, worst = [], _worsts()
    for T in tr.TS:
        p = tr.make_case(name, H, R, T, shared)
        fails += check_calls([p], worst, plain=p["c0"] is None)
    _report(f"case={name} H={H} R={R} shared={int(shared)}", worst)
    assert not fails, fails[:12]


@pytest.mark.parametrize("name", tr.BWD_CASES)
def test_synthetic_backward(name):
    """(4): saved tensors at the kinks of the triangle, forget gates of 0 / 1 / 2^-30 / 1 - 2^-24, all-zero xhat columns -- both kernel
    families, with and without BatchNorm."""
    fails, worst = [], _worsts()
    for H, R, sh, T in [(16, 17, True, 7), (32, 33, False, 2), (16, 2, False, 1), (48, 64, True, 2), (320, 513, True, 2)]:
        for use_bn in (True, False):
            p, fwd = tr.bwd_case(name, H, R, T, sh, use_bn)
            fails += check_calls([p], worst, saved=[fwd])
    _report(f"case=bwd_{name}", worst)
    assert not fails, fails[:12]


def test_multi_three_calls():
    """n = 3, R = (40, 17, 200) at H = 48, per-call T = (7, 5, 7): row blocks of 16 rows, 3, 2 and 13 of them, 54 (shared) or 108
    (separate gates) workgroups.  The call of 5 frames leaves the chain after its last one, so frames 5 and 6 of the chain run as launches
    of TWO calls while the whole-sequence launch they are compared with holds three.  The bit-for-bit comparison stands on the calls'
    row blocks being the same in both, and they are: a call's blocking depends on the other calls of its launch only when the launch
    does not fit the device's workgroup slots at the first target of seq_dir_geometry's list, and 54 or 108 workgroups fit any count of
    slots (a compute unit alone holds several of these workgroups, the device has 256 units).  For a launch that IS re-blocked
    (test_multi_eight_calls_reblocked) the same comparison would not hold, which is why all its calls have the same T."""
    fails = []
    for sh in (True, False):
        worst = _worsts()
        for names in (("tails", "state", "offset"), ("constant", "bn_scales", "momenta_cum7"), ("no_bn", "no_bn", "no_bn")):
            ps = [tr.make_case(n, 48, R, T, sh) for n, R, T in zip(names, (40, 17, 200), (7, 5, 7))]
            fails += check_calls(ps, worst, steps=False)
        _report(f"multi3 shared={int(sh)}", worst)
    assert not fails, fails[:12]


def test_multi_eight_calls_reblocked():
    """n = 8 at H = 320 (shared), R = 96 or close: at the single call's target every call takes 6 row blocks of 16 rows, 8 x 120 = 960
    workgroups.  What follows is DERIVED from the formulas of csrc/sfsn_train.hip and the 160 KB of LDS of a compute unit; no test can
    observe a launch's geometry, and none asserts it.  BACKWARD: seq_lds_bwd at 16 rows per block is 45,408 bytes of dynamic LDS (plus
    the kernel's static 1 KB reduction array): at most 3 workgroups per compute unit, 768 slots on 256 units, fewer than 960 whatever
    the registers allow -- seq_dir_geometry walks down its target list (128: still 6 blocks; 96: 4 asked, 3 row blocks of 32 rows, 8 x
    60 = 480 workgroups at 68,784 bytes, two per unit).  FORWARD: seq_lds_fwd is 30,048 bytes, five workgroups per unit by the LDS,
    1280 slots: the forward keeps its 6 blocks of 16 rows unless the occupancy query answers less for another reason.  So the launch
    is expected to be re-blocked in the backward direction only.  Either way the comparison is sound: with the one-frame chain OF THE
    SAME EIGHT CALLS (all of T = 7, so every launch of the chain holds the eight calls and gets the blocking of the whole-sequence
    launch) and with fp64; not with single calls bit for bit (their row blocks would differ, and with them the order of the row sums)."""
    Rs = (96, 96, 90, 96, 81, 96, 96, 96)
    names = ("control", "tails", "constant", "var_eps", "offset", "bn_scales", "momenta_cum0", "state")
    worst = _worsts()
    ps = [tr.make_case(n, 320, R, 7, True) for n, R in zip(names, Rs)]
    fails = check_calls(ps, worst, steps=False)
    _report("multi8", worst)
    assert not fails, fails[:12]


# scripts/exp_train_shapes.py's shapes (H, R, T, shared, BatchNorm), asserted instead of printed
SHAPES = [(16, 2, 1, True, True), (16, 3, 2, True, True), (32, 17, 3, False, True), (32, 64, 9, True, False), (224, 600, 12, True, True),
          (320, 64, 10, True, True), (320, 70, 6, False, True), (48, 130, 7, True, True), (224, 1700, 4, True, True)]


@pytest.mark.parametrize("H,R,T,shared,bn", SHAPES)
def test_exp_train_shapes(H, R, T, shared, bn):
    """(5): one step, one row block, ragged last row block, separate gates, no BatchNorm, the full-band size, 16 row blocks of 112 rows."""
    assert tr.blocking(R, H, shared)[0] <= 16
    worst = _worsts()
    p = tr.make_case("control" if bn else "no_bn", H, R, T, shared)
    fails = check_calls([p], worst, plain=True)
    _report(f"shape H={H} R={R} T={T} shared={int(shared)} bn={int(bn)}", worst)
    assert not fails, fails[:12]
