"""FullbandStreamingSession.catch_up on a running clip against the same backlog pushed through step() (profiles/cirm_catchup.md).  The
recipe's cIRM-GSN model (H = 268, 4 layers, random weights); a B = 1 session and one clip of a 16-clip session; backlogs of 8, 32,
125 and 1250 frames; p50 of alternating iterations, host clock from a synchronised stream to a synchronised stream.  Run on the
MI355X box: python scripts/exp_cirm_catchup.py [iterations] [out.md] [one|graph]  (graph: the per-kernel tier, one_launch=False)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
from test_cirm_gsn import recipe_model

DEV = torch.device("cuda:0")
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 100
out_path = sys.argv[2] if len(sys.argv) > 2 else None
one_launch = "auto" if len(sys.argv) <= 3 or sys.argv[3] == "one" else False
WARM = 20  # frames every clip has stepped before the backlog arrives (nothing in either path depends on a clip's age)
model = recipe_model()[0].to(DEV)
rng = np.random.default_rng(7)
lines = ["| session | backlog N | step x N p50 (ms) | catch_up p50 (ms) | step / catch_up | per stepped frame (us) | next hop equal |",
         "|---|---|---|---|---|---|---|"]
for B in (1, 16):
    full = torch.from_numpy(((rng.standard_normal((B, 257, WARM + 1251)) + 1j * rng.standard_normal((B, 257, WARM + 1251))) * 0.5).astype(np.complex64)).to(DEV)
    stepped, caught = (model.streaming(batch=B, one_launch=one_launch) for _ in range(2))
    clip = [B // 2]
    floor = []
    for N in (8, 32, 125, 1250):
        back = full[..., WARM:WARM + N].contiguous()
        frames = [back[..., t:t + 1].contiguous() for t in range(N)]
        mine = back[clip[0]:clip[0] + 1].contiguous()
        # equality first: the same warm-up in both sessions, the backlog stepped / caught up, then the hop behind it
        stepped.reset(); caught.reset()
        for t in range(WARM):
            x = full[..., t:t + 1].contiguous()
            stepped.step(x, copy=False); caught.step(x, copy=False)
        for x in frames:
            stepped.step(x, copy=False)
        caught.catch_up(mine, clips=clip)
        nxt = full[..., WARM + N:WARM + N + 1].contiguous()
        a, b = stepped.step(nxt)[0], caught.step(nxt)[0]
        same = torch.equal(torch.view_as_real(a[clip]), torch.view_as_real(b[clip]))
        t_step, t_catch = [], []
        for i in range(iters + 5):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for x in frames:
                stepped.step(x, copy=False)
            torch.cuda.synchronize(); a = time.perf_counter() - t0
            torch.cuda.synchronize(); t0 = time.perf_counter()
            caught.catch_up(mine, clips=clip)
            torch.cuda.synchronize(); b = time.perf_counter() - t0
            if i >= 5:
                t_step.append(a); t_catch.append(b)
        a, b = (np.median(t) * 1e3 for t in (t_step, t_catch))
        floor.append((b, a / N))
        lines.append(f"| B = {B}, clip {clip[0]} | {N} | {a:.3f} | {b:.3f} | {a / b:.2f} | {1e3 * a / N:.1f} | {'yes' if same else 'NO'} |")
        print(lines[-1], flush=True)
    # the floor: the shortest backlog's time; break-even: the floor over a stepped frame's cost (both from this table)
    fl, per = floor[0][0], np.median([p for _, p in floor])
    lines.append(f"| B = {B}, clip {clip[0]} | floor {fl:.3f} ms | | | | {1e3 * per:.1f} | break-even about {fl / per:.0f} frames |")
    print(lines[-1], flush=True)
    for s in (stepped, caught):
        s.check_errors()
    model.engine().check_stack_errors()
text = "\n".join(lines) + "\n"
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write(text)
