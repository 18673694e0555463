"""Host-only cost of one forward: wall time of Engine.forward_stft up to its return, no synchronisation inside the timed span.

    python scripts/time_forward_host.py [--batch 4] [--frames 1000] [--calls 200]

The live baseline_m model (refweights.LIVE_M), default schedule (a forward alone: overlapped).  The device is synchronised before
every call, outside the span, so that the stack rule sees the forward alone and the queue is empty.  Prints one JSON line with the
median, the minimum and the 90th percentile in microseconds.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import numpy as np
    import torch

    import refweights as rw
    import spiking_fullsubnet_amd as pkg
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    model = pkg.SpikingFullSubNet(**rw.LIVE_M)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in rw.live_state_dict(rw.LIVE_M, 5).items()}, strict=True)
    eng = model.eval().to("cuda:0").engine()
    gen = torch.Generator().manual_seed(3)
    stft = torch.view_as_complex((0.1 * torch.randn((a.batch, 257, a.frames, 2), generator=gen)).to("cuda:0"))
    us = []
    for i in range(a.warmup + a.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = eng.forward_stft(stft)
        t1 = time.perf_counter()
        if i >= a.warmup:
            us.append((t1 - t0) * 1e6)
    torch.cuda.synchronize()
    eng.check_stack_errors()
    print(json.dumps(dict(metric="forward_stft_host_us", batch=a.batch, frames=a.frames, calls=a.calls, overlapped=res["overlapped"],
                          n_chunks=res["n_chunks"], median=round(float(np.median(us)), 2), min=round(float(np.min(us)), 2),
                          p90=round(float(np.percentile(us, 90)), 2))))


if __name__ == "__main__":
    main()
