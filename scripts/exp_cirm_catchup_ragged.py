"""FullbandStreamingSession.catch_up_ragged -- k clips of a 16-clip cIRM-GSN session, each with a backlog of its own length, in ONE call
-- against the loop of k single-clip catch_up calls and against the same frames through queued tick(frames, clips) hops
(profiles/cirm_catchup_ragged.md).  The recipe model (H = 268, 4 layers); k = 1, 2, 3, 4, 8 listed clips, distinct lengths between 8
and 125 frames, behind 200 frames of history; p50 of alternating iterations, host clock from a synchronised stream to a synchronised
stream.  Run on the MI355X box: python scripts/exp_cirm_catchup_ragged.py [iterations] [out.md] [one|graph]   (graph: the per-kernel tier)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
from test_cirm_gsn import recipe_model

DEV = torch.device("cuda:0")
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 100
out_path = sys.argv[2] if len(sys.argv) > 2 else None
one_launch = "auto" if len(sys.argv) <= 3 or sys.argv[3] == "one" else False
B, HIST, NMAX = 16, 200, 125
model = recipe_model()[0].to(DEV)
rng = np.random.default_rng(7)
full = torch.from_numpy(((rng.standard_normal((B, 257, HIST + NMAX + 1)) + 1j * rng.standard_normal((B, 257, HIST + NMAX + 1))) * 0.5).astype(np.complex64)).to(DEV)
lines = ["| listed clips k | lengths | catch_up_ragged p50 (ms) | k x catch_up p50 (ms) | tick hops p50 (ms) | loop / ragged | hops / ragged | next hop equal: loop, hops |",
         "|---|---|---|---|---|---|---|---|"]
ragged, looped, ticked = (model.streaming(batch=B, one_launch=one_launch) for _ in range(3))
assert ragged.one_launch is (one_launch == "auto")
for k in (1, 2, 3, 4, 8):
    lens = [66] if k == 1 else [int(round(v)) for v in np.linspace(8, NMAX, k)]
    assert len(set(lens)) == k
    clips = [(2 * i + 1) % B for i in range(k)]
    N = max(lens)
    back = full[clips, :, HIST:HIST + N].contiguous()
    singles = [full[b:b + 1, :, HIST:HIST + n].contiguous() for b, n in zip(clips, lens)]
    hops = [(full[..., HIST + t:HIST + t + 1].contiguous(), [b for b, n in zip(clips, lens) if n > t]) for t in range(N)]

    def run_ragged():
        ragged.catch_up_ragged(back, lens, clips=clips)

    def run_loop():
        for b, x in zip(clips, singles):
            looped.catch_up(x, clips=[b])

    def run_hops():
        for x, who in hops:
            ticked.tick(x, who, copy=False)

    # equality first: the same history caught up on in the three sessions, the backlogs, then the hop behind them
    for s in (ragged, looped, ticked):
        s.reset()
        s.catch_up(full[..., :HIST].contiguous())
    run_ragged(); run_loop(); run_hops()
    nxt = torch.stack([full[b, :, HIST + n:HIST + n + 1] for b, n in zip(clips, lens)])
    x = full[..., HIST:HIST + 1].clone()
    x[clips] = nxt
    outs = [torch.view_as_real(s.tick(x, clips)[0][clips]).clone() for s in (ragged, looped, ticked)]
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
for s in (ragged, looped, ticked):
    s.check_errors()
text = "\n".join(lines) + "\n"
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write(text)
