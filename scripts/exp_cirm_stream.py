#!/usr/bin/env python3
"""cIRM-GSN streaming latency per hop (modeling_cirm_gsn.Model.streaming at the recipe's geometry: H = 268, 4 layers, F = 257, df 3,
BatchNorm, LayerNorm, shared gates), B clips, `hop` frames per step.  The legs, alternated block by block in one process:

    one_launch   sfsn_fullband_stream_hop, one launch per hop
    counted      the same with count_spikes=True: sfsn_fullband_stream_hop_counted, per-lane spike slots inside the launch
    graph        the per-kernel sequence replayed from its HIP graph
    eager        the per-kernel sequence launched kernel by kernel
    wave         (hop 1) samples in, samples out on the device: sfsn_fullband_stream_hop_wave, step_wave(copy=False) + synchronise
    wave_host    (hop 1) samples in, samples out on the host: step_wave_host (pinned buffers, completion words, no synchronise)

Timed with a host clock around `step(copy=False)` plus a stream synchronise: what a caller that needs the frame back waits for.

    python scripts/exp_cirm_stream.py [--batch 1] [--hop 1] [--hops 2000] [--warmup 200] [--block 250]
    rocprofv3 --kernel-trace --stats -- python scripts/exp_cirm_stream.py --trace one_launch   (a leg alone, 200 hops, for kernel time)

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

from test_cirm_gsn import recipe_model  # noqa: E402

LEGS = {"one_launch": dict(one_launch=True), "counted": dict(one_launch=True, count_spikes=True), "graph": dict(one_launch=False, graph=True), "eager": dict(one_launch=False, graph=False),
        "wave": dict(waveform=True), "wave_host": dict(waveform=True, host_io=True)}
WAVE_LEGS = ("wave", "wave_host")


def run(sess, frames, n, stream):
    us = np.empty(n)
    for i in range(n):
        t0 = time.perf_counter()
        sess.step(frames[i % len(frames)], copy=False)
        stream.synchronize()
        us[i] = (time.perf_counter() - t0) * 1e6
    return us


def run_wave(sess, chunks, n, stream):
    us = np.empty(n)
    if sess.host_io:
        for i in range(n):
            x = chunks[i % len(chunks)]
            t0 = time.perf_counter()
            sess.step_wave_host(x)
            us[i] = (time.perf_counter() - t0) * 1e6
        return us
    for i in range(n):
        t0 = time.perf_counter()
        sess.step_wave(chunks[i % len(chunks)], copy=False)
        stream.synchronize()
        us[i] = (time.perf_counter() - t0) * 1e6
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--hop", type=int, default=1)
    ap.add_argument("--hops", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--block", type=int, default=250)
    ap.add_argument("--trace", choices=sorted(LEGS))
    a = ap.parse_args()
    m, _ = recipe_model(seed=3)
    m = m.cuda()
    g = torch.Generator("cuda").manual_seed(0)
    frames = [torch.view_as_complex(torch.randn(a.batch, 257, a.hop, 2, device="cuda", generator=g) * 0.5) for _ in range(64)]
    chunks = [torch.randn(a.batch, 128, device="cuda", generator=g) * 0.05 for _ in range(64)]
    data = {k: frames for k in LEGS}
    data.update(wave=chunks, wave_host=[c.cpu() for c in chunks])
    legs = {k: kw for k, kw in LEGS.items() if a.hop == 1 or k not in WAVE_LEGS}  # (a waveform session computes one frame per call)
    stream = torch.cuda.current_stream()
    if a.trace:
        sess = m.streaming(batch=a.batch, hop=a.hop, **LEGS[a.trace])
        (run_wave if a.trace in WAVE_LEGS else run)(sess, data[a.trace], 200, stream)
        sess.check_errors()
        print(json.dumps(dict(leg=a.trace, launches=sess.launches)))
        return
    sessions = {k: m.streaming(batch=a.batch, hop=a.hop, **kw) for k, kw in legs.items()}
    samples = {k: [] for k in legs}
    for k, s in sessions.items():
        (run_wave if k in WAVE_LEGS else run)(s, data[k], a.warmup, stream)
    done = 0
    while done < a.hops:  # the legs take turns, a block of hops each, so that drift of the machine falls on all alike
        n = min(a.block, a.hops - done)
        for k, s in sessions.items():
            samples[k].append((run_wave if k in WAVE_LEGS else run)(s, data[k], n, stream))
        done += n
    out = dict(batch=a.batch, hop=a.hop, hops=a.hops, device=torch.cuda.get_device_name())
    for k, s in sessions.items():
        s.check_errors()
        us = np.concatenate(samples[k])
        out[k] = dict(p50_us=round(float(np.percentile(us, 50)), 2), p99_us=round(float(np.percentile(us, 99)), 2),
                      min_us=round(float(us.min()), 2), mean_us=round(float(us.mean()), 2))
    out["one_launch_over_graph_p50"] = round(out["one_launch"]["p50_us"] / out["graph"]["p50_us"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
