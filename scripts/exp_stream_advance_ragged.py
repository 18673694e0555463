"""StreamingSession.advance_ragged -- k clips of a 16-clip session, each with a backlog of its own length, in ONE call -- against the
loop of k single-clip advance calls and against the same frames through queued step(..., clips=) hops
(profiles/stream_advance_ragged.md).  baseline_m; k = 1, 2, 3, 4, 8 listed clips, distinct lengths between 32 and 125 frames, behind
200 frames of history; p50 of alternating iterations, host clock from a synchronised stream to a synchronised stream.  Run on the
MI355X box: python scripts/exp_stream_advance_ragged.py [iterations] [out.md] [one|graph]   (graph: the per-kernel tier)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
import refweights as rw
from test_hip_parity import build_module

DEV = torch.device("cuda:0")
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 100
out_path = sys.argv[2] if len(sys.argv) > 2 else None
one_launch = "auto" if len(sys.argv) <= 3 or sys.argv[3] == "one" else False
B, HIST, NMAX = 16, 200, 125
kw = rw.LIVE_M
model = build_module("live", kw, rw.live_state_dict(kw, 5))
rng = np.random.default_rng(7)
full = torch.from_numpy(((rng.standard_normal((B, 257, HIST + NMAX + 1)) + 1j * rng.standard_normal((B, 257, HIST + NMAX + 1))) * 0.5).astype(np.complex64)).to(DEV)
lines = ["| listed clips k | lengths | advance_ragged p50 (ms) | k x advance p50 (ms) | step(clips=) hops p50 (ms) | loop / ragged | hops / ragged | next hop equal: loop, hops |",
         "|---|---|---|---|---|---|---|---|"]
ragged, looped, stepped = (model.streaming(batch=B, one_launch=one_launch) for _ in range(3))
for k in (1, 2, 3, 4, 8):
    lens = [78] if k == 1 else [int(round(v)) for v in np.linspace(32, NMAX, k)]
    assert len(set(lens)) == k
    clips = [(2 * i + 1) % B for i in range(k)]
    N = max(lens)
    back = full[clips, :, HIST:HIST + N].contiguous()
    singles = [full[b:b + 1, :, HIST:HIST + n].contiguous() for b, n in zip(clips, lens)]
    hops = [(full[..., HIST + t:HIST + t + 1].contiguous(), [b for b, n in zip(clips, lens) if n > t]) for t in range(N)]

    def run_ragged():
        ragged.advance_ragged(back, lens, clips=clips)

    def run_loop():
        for b, x in zip(clips, singles):
            looped.advance(x, clips=[b])

    def run_hops():
        for x, who in hops:
            stepped.step(x, copy=False, clips=who)

    # equality first: the same history primed into the three sessions, the backlogs, then the hop behind them
    for s in (ragged, looped, stepped):
        s.reset()
        s.prime(full[..., :HIST].contiguous())
    run_ragged(); run_loop(); run_hops()
    nxt = torch.stack([full[b, :, HIST + n:HIST + n + 1] for b, n in zip(clips, lens)])
    x = full[..., HIST:HIST + 1].clone()
    x[clips] = nxt
    outs = [torch.view_as_real(s.step(x, clips=clips)[0][clips]).clone() for s in (ragged, looped, stepped)]
    same = ", ".join("yes" if torch.equal(outs[0], o) else "NO" for o in outs[1:])
    t_r, t_l, t_h = [], [], []
    for i in range(iters + 5):
        row = []
        for fn in (run_ragged, run_loop, run_hops):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); row.append(time.perf_counter() - t0)
        if i >= 5:
            t_r.append(row[0]); t_l.append(row[1]); t_h.append(row[2])
    a, b_, c = (np.median(t) * 1e3 for t in (t_r, t_l, t_h))
    lines.append(f"| {k} | {', '.join(map(str, lens))} | {a:.3f} | {b_:.3f} | {c:.3f} | {b_ / a:.2f} | {c / a:.2f} | {same} |")
    print(lines[-1], flush=True)
for s in (ragged, looped, stepped):
    s.check_errors()
text = "\n".join(lines) + "\n"
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write(text)
