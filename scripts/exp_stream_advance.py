"""StreamingSession.advance on a running clip against the same backlog pushed through step() and against prime() over the whole
utterance so far (profiles/stream_advance.md).  baseline_m; a B = 1 session and one clip of a 16-clip session; backlogs of 8, 32, 125
and 1250 frames behind 10 s (1250 frames) of history; p50 of alternating iterations, host clock from a synchronised stream to a
synchronised stream.  Run on the MI355X box: python scripts/exp_stream_advance.py [iterations] [out.md] [one|graph]
(graph: the per-kernel tier, one_launch=False)."""
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
HIST = 1250
kw = rw.LIVE_M
model = build_module("live", kw, rw.live_state_dict(kw, 5))
rng = np.random.default_rng(7)
lines = ["| session | backlog N | step x N p50 (ms) | advance p50 (ms) | prime(10 s + N) p50 (ms) | step / advance | prime / advance | next hop equal |",
         "|---|---|---|---|---|---|---|---|"]
for B in (1, 16):
    full = torch.from_numpy(((rng.standard_normal((B, 257, 2 * HIST + 1)) + 1j * rng.standard_normal((B, 257, 2 * HIST + 1))) * 0.5).astype(np.complex64)).to(DEV)
    stepped, advanced, primed = (model.streaming(batch=B, one_launch=one_launch) for _ in range(3))
    clip = [B // 2]
    for N in (8, 32, 125, 1250):
        back = full[..., HIST:HIST + N].contiguous()
        frames = [back[..., t:t + 1].contiguous() for t in range(N)]
        mine = back[clip[0]:clip[0] + 1].contiguous()
        whole = full[clip[0]:clip[0] + 1, :, :HIST + N].contiguous()
        # equality first: 10 s of history primed into both sessions, the backlog stepped / advanced, then the hop behind it
        stepped.reset(); advanced.reset()
        stepped.prime(full[..., :HIST].contiguous()); advanced.prime(full[..., :HIST].contiguous())
        for x in frames:
            stepped.step(x, copy=False)
        advanced.advance(mine, clips=clip)
        nxt = full[..., HIST + N:HIST + N + 1].contiguous()
        a, b = stepped.step(nxt)[0], advanced.step(nxt)[0]
        same = torch.equal(torch.view_as_real(a[clip]), torch.view_as_real(b[clip]))
        t_step, t_adv, t_prime = [], [], []
        for i in range(iters + 5):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for x in frames:
                stepped.step(x, copy=False)
            torch.cuda.synchronize(); a = time.perf_counter() - t0
            torch.cuda.synchronize(); t0 = time.perf_counter()
            advanced.advance(mine, clips=clip)
            torch.cuda.synchronize(); b = time.perf_counter() - t0
            torch.cuda.synchronize(); t0 = time.perf_counter()
            primed.prime(whole, clips=clip)
            torch.cuda.synchronize(); c = time.perf_counter() - t0
            if i >= 5:
                t_step.append(a); t_adv.append(b); t_prime.append(c)
        a, b, c = (np.median(t) * 1e3 for t in (t_step, t_adv, t_prime))
        lines.append(f"| B = {B}, clip {clip[0]} | {N} | {a:.3f} | {b:.3f} | {c:.3f} | {a / b:.2f} | {c / b:.2f} | {'yes' if same else 'NO'} |")
        print(lines[-1], flush=True)
    for s in (stepped, advanced, primed):
        s.check_errors()
text = "\n".join(lines) + "\n"
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write(text)
