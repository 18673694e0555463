#!/usr/bin/env python3
"""Per-hop latency of streaming sessions at the baseline_m geometry, B = 1, one frame per hop, one launch per hop.  The legs,
alternated block by block in one process:

    live          SpikingFullSubNet (LayerNorm front-end): the session the project's latency figure is about
    frozen_cum    Separator with cumulative_laplace_norm (running means carried in the hop's state)
    frozen_given  Separator with offline_laplace_norm, the clip's statistics given (streaming(norm_stats=...))

Timed with a host clock around `step(copy=False)` plus a stream synchronise: what a caller that needs the frame back waits for.

    python scripts/exp_frozen_stream.py [--legs live,frozen_cum,frozen_given] [--hops 4000] [--warmup 400] [--block 250]
    python scripts/exp_frozen_stream.py --legs live        (runs on a build without norm_stats too: the parent's figure)

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import refweights as rw  # noqa: E402
import spiking_fullsubnet_amd as pkg  # noqa: E402

LEGS = ("live", "frozen_cum", "frozen_given")


def module(cls, kw, sd):
    m = cls(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.eval().cuda()


def session(leg, frames):
    if leg == "live":
        return module(pkg.SpikingFullSubNet, rw.LIVE_M, rw.live_state_dict(rw.LIVE_M, 5)).streaming(batch=1, one_launch=True)
    if leg == "frozen_cum":
        return module(pkg.Separator, rw.FROZEN_M_CUM, rw.frozen_state_dict(rw.FROZEN_M_CUM, 36)).streaming(batch=1, one_launch=True)
    m = module(pkg.Separator, rw.FROZEN_M, rw.frozen_state_dict(rw.FROZEN_M, 44))
    return m.streaming(batch=1, one_launch=True, norm_stats=m.norm_stats(torch.cat(frames, -1)))


def run(sess, frames, n, stream):
    us = np.empty(n)
    for i in range(n):
        t0 = time.perf_counter()
        sess.step(frames[i % len(frames)], copy=False)
        stream.synchronize()
        us[i] = (time.perf_counter() - t0) * 1e6
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--hops", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=400)
    ap.add_argument("--block", type=int, default=250)
    a = ap.parse_args()
    legs = [k for k in a.legs.split(",") if k]
    assert all(k in LEGS for k in legs), legs
    g = torch.Generator("cuda").manual_seed(0)
    frames = [torch.view_as_complex(torch.randn(1, 257, 1, 2, device="cuda", generator=g) * 0.5) for _ in range(64)]
    stream = torch.cuda.current_stream()
    sessions = {k: session(k, frames) for k in legs}
    samples = {k: [] for k in legs}
    for s in sessions.values():
        run(s, frames, a.warmup, stream)
    done = 0
    while done < a.hops:  # the legs take turns, a block of hops each, so that drift of the machine falls on all alike
        n = min(a.block, a.hops - done)
        for k, s in sessions.items():
            samples[k].append(run(s, frames, n, stream))
        done += n
    from spiking_fullsubnet_amd import _lib
    out = dict(hops=a.hops, block=a.block, device=torch.cuda.get_device_name(), source_hash=_lib.source_hash())
    for k, s in sessions.items():
        s.check_errors()
        us = np.concatenate(samples[k])
        out[k] = dict(p50_us=round(float(np.percentile(us, 50)), 2), p99_us=round(float(np.percentile(us, 99)), 2),
                      min_us=round(float(us.min()), 2), mean_us=round(float(us.mean()), 2))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
