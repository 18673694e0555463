"""StreamingSession.prime against the same prefix pushed through step(): latency per prefix length (profiles/stream_prime.md).
baseline_m, B = 1 and 16, prefixes of 1, 10, 100 and 1250 frames; p50 of alternating iterations, host clock from a synchronised
stream to a synchronised stream.  Run on the MI355X box: python scripts/exp_stream_prime.py [iterations] [out.md] [one|graph]
(graph: the per-kernel tier, one_launch=False)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
import refweights as rw
from test_hip_parity import build_module

DEV = torch.device("cuda:0")
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 60
out_path = sys.argv[2] if len(sys.argv) > 2 else None
one_launch = "auto" if len(sys.argv) <= 3 or sys.argv[3] == "one" else False
kw = rw.LIVE_M
model = build_module("live", kw, rw.live_state_dict(kw, 5))
rng = np.random.default_rng(7)
lines = ["| B | prefix (frames) | step x N p50 (ms) | prime p50 (ms) | step / prime | one-launch tier |", "|---|---|---|---|---|---|"]
for B in (1, 16):
    full = torch.from_numpy(((rng.standard_normal((B, 257, 1250)) + 1j * rng.standard_normal((B, 257, 1250))) * 0.5).astype(np.complex64)).to(DEV)
    streamed, primed = model.streaming(batch=B, one_launch=one_launch), model.streaming(batch=B, one_launch=one_launch)
    for N in (1, 10, 100, 1250):
        stft = full[..., :N].contiguous()
        frames = [stft[..., t:t + 1].contiguous() for t in range(N)]
        # equality first: the hop after the prefix, primed against streamed
        streamed.reset()
        for x in frames:
            streamed.step(x, copy=False)
        primed.prime(stft)
        nxt = full[..., N % 1250:N % 1250 + 1].contiguous()
        same = torch.equal(torch.view_as_real(streamed.step(nxt)[0]), torch.view_as_real(primed.step(nxt)[0]))
        t_step, t_prime = [], []
        for i in range(iters + 5):
            streamed.reset()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for x in frames:
                streamed.step(x, copy=False)
            torch.cuda.synchronize(); a = time.perf_counter() - t0
            torch.cuda.synchronize(); t0 = time.perf_counter()
            primed.prime(stft)
            torch.cuda.synchronize(); b = time.perf_counter() - t0
            if i >= 5:
                t_step.append(a); t_prime.append(b)
        a, b = np.median(t_step) * 1e3, np.median(t_prime) * 1e3
        lines.append(f"| {B} | {N} | {a:.3f} | {b:.3f} | {a / b:.2f} | {primed._hop is not None} (next hop equal: {same}) |")
        print(lines[-1], flush=True)
    streamed.check_errors(); primed.check_errors()
text = "\n".join(lines) + "\n"
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write(text)
