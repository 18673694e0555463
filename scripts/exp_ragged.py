#!/usr/bin/env python3
"""Clips of different lengths: one clip per forward against one ragged batch (profiles/ragged_batches.md).

Models: baseline_m live (LIVE_M) and frozen with the offline Laplace norm (FROZEN_M), refweights state dicts.  Clips: 16 and 64,
lengths drawn once (seed 0) uniformly from 2 ... 8 s at 16 kHz.  Three legs, alternated repetition by repetition in one process:

    loop      model(wave_b[None, :L_b]) for every clip: the path that exists without per-clip lengths (the baseline)
    ragged    one model.forward_ragged(waves, lengths) on the batch padded to the longest clip
    buckets   the clips sorted by length into 4 buckets, one forward_ragged per bucket, each padded to its own longest clip
              (the bucket tensors are built before the clock starts: batching is the data loader's work)

Timed with a host clock around the leg plus a stream synchronise, p50 of the repetitions after warm-up; every leg returns all
clips' enhanced waveforms.  `--layer-outputs`: what the forwards return for the layers ("counts": what a validation loop that
logs SynOPs needs; "tensors": the reference's API; "none").

    python scripts/exp_ragged.py [--clips 16,64] [--models live,frozen] [--reps 20] [--warmup 3] [--layer-outputs counts,tensors]

Prints one JSON line per (model, clips, layer outputs)."""
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

SR, N_BUCKETS = 16000, 4


def module(name):
    cls, kw, sd = (pkg.SpikingFullSubNet, rw.LIVE_M, rw.live_state_dict(rw.LIVE_M, 5)) if name == "live" else \
        (pkg.Separator, rw.FROZEN_M, rw.frozen_state_dict(rw.FROZEN_M, 44))
    m = cls(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.eval().cuda()


def clips(n):
    rng = np.random.default_rng(0)
    lengths = [int(v) for v in rng.integers(2 * SR, 8 * SR + 1, n)]
    waves = np.zeros((n, max(lengths)), np.float32)
    for b, L in enumerate(lengths):
        waves[b, :L] = 0.05 * rng.standard_normal(L)
    return torch.from_numpy(waves).cuda(), lengths


def buckets(waves, lengths):
    order = sorted(range(len(lengths)), key=lambda b: lengths[b])
    per = -(-len(order) // N_BUCKETS)
    out = []
    for i in range(0, len(order), per):
        idx = order[i:i + per]
        lens = [lengths[b] for b in idx]
        out.append((waves[idx][:, :max(lens)].contiguous(), lens))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", default="16,64")
    ap.add_argument("--models", default="live,frozen")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layer-outputs", default="counts,tensors")
    a = ap.parse_args()
    from spiking_fullsubnet_amd import _lib
    stream = torch.cuda.current_stream()
    for name in a.models.split(","):
        m = module(name)
        for n in (int(v) for v in a.clips.split(",")):
            waves, lengths = clips(n)
            bks = buckets(waves, lengths)
            legs = dict(
                loop=lambda: [m(waves[b:b + 1, :L])[0] for b, L in enumerate(lengths)],
                ragged=lambda: m.forward_ragged(waves, lengths)[0],
                buckets=lambda: [m.forward_ragged(w, lens)[0] for w, lens in bks])
            for mode in a.layer_outputs.split(","):
                m.layer_outputs = mode
                ms = {k: [] for k in legs}
                with torch.no_grad():
                    for rep in range(a.warmup + a.reps):
                        for k, fn in legs.items():  # the legs take turns, so that drift of the machine falls on all alike
                            stream.synchronize()
                            t0 = time.perf_counter()
                            fn()
                            stream.synchronize()
                            if rep >= a.warmup:
                                ms[k].append((time.perf_counter() - t0) * 1e3)
                m.engine().check_stack_errors()
                out = dict(model=name, clips=n, layer_outputs=mode, reps=a.reps, seconds_of_audio=round(sum(lengths) / SR, 1),
                           padded_seconds=round(n * max(lengths) / SR, 1), bucket_padded_seconds=round(sum(w.numel() for w, _ in bks) / SR, 1),
                           device=torch.cuda.get_device_name(), source_hash=_lib.source_hash())
                for k, v in ms.items():
                    p50 = float(np.percentile(v, 50))
                    out[k] = dict(p50_ms=round(p50, 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3), clips_per_s=round(n / p50 * 1e3, 1))
                print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
