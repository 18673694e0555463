#!/usr/bin/env python
"""Scoring a ragged batch on one MI355X: ONE `PITWrapper.per_clip(est, ref, lengths)` call on the padded batch (two launches, nothing
read back) against the loop that equal-length scoring makes necessary -- per clip: a slice of both tensors, `PITWrapper.full` on it,
and audiozen.metric.SISDR's formula in ATen on the reordered rows.

    python scripts/exp_ragged_score.py [--clips 64 16] [--iters 200] [--warmup 10] [--seed 0] [--out FILE.json]

Workloads: clips of 2 to 8 s (seeded, uniform), at 8 kHz with two speakers (wsj0-mix) and at 16 kHz with one (intel_ndns, REVERB).
Legs, alternating inside one run (single, loop, loop_item, single, ...):
  single     one per_clip call; lengths uploaded from the host list each time (as a validation step would)
  loop       the per-clip loop with every value left on the device
  loop_item  the same loop reading each clip's SI-SDR back with .item(), as the reference's SISDR does
Every iteration is timed twice over: a host clock around the leg up to a device synchronise (wall) and a pair of HIP events around
its enqueue (device span).  p50 and p99 of both are reported per leg.  Before timing, the loop's perm, pair and loss are compared bit
for bit with the single call's and the SI-SDR values to 1e-3 dB.  Prints one JSON line per workload.  Needs a GPU: no CPU fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = (("8k_2spk", 8000, 2), ("16k_1spk", 16000, 1))


def aten_sisdr(est, ref):
    """audiozen.metric.SISDR's formula on [S, L] device tensors, per row (reduce_mean=False), left on the device."""
    eps = torch.finfo(est.dtype).eps
    s = ref - ref.mean(-1, keepdim=True)
    a = est - est.mean(-1, keepdim=True)
    dot = (s * a).sum(-1, keepdim=True)
    proj = (dot * s + eps) / ((s ** 2).sum(-1, keepdim=True) + eps)
    noise = a - proj
    return 10 * torch.log10(((proj ** 2).sum(-1) + eps) / ((noise ** 2).sum(-1) + eps) + eps)


def percentiles(xs):
    return dict(p50=float(np.percentile(xs, 50)), p99=float(np.percentile(xs, 99)), min=float(np.min(xs)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, nargs="+", default=[64, 16])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_ragged_score.py needs a GPU")
    from spiking_fullsubnet_amd.pit import PairwiseNegSDR, PITWrapper
    dev = "cuda:0"
    wrapper = PITWrapper(PairwiseNegSDR())
    lines = []
    for tag, sr, S in WORKLOADS:
        for B in args.clips:
            rng = np.random.default_rng(args.seed + B + sr)
            lens = [int(n) for n in rng.integers(2 * sr, 8 * sr + 1, size=B)]
            L = max(lens)
            g = torch.Generator().manual_seed(args.seed + B + sr)
            ref = 0.1 * torch.randn(B, S, L, generator=g)
            sigma = torch.stack([torch.randperm(S, generator=g) for _ in range(B)])
            est = 0.7 * torch.stack([ref[b, sigma[b]] for b in range(B)]) + 0.05 * torch.randn(B, S, L, generator=g)
            for b, n in enumerate(lens):  # zero padding, as forward_ragged leaves it
                ref[b, :, n:] = 0
                est[b, :, n:] = 0
            ref, est = ref.to(dev), est.to(dev)

            def single():
                return wrapper.per_clip(est, ref, lengths=lens)

            def loop(item=False):
                out = []
                for b, n in enumerate(lens):
                    eb, rb = est[b:b + 1, :, :n].contiguous(), ref[b:b + 1, :, :n].contiguous()
                    loss, reordered, perm, pair = wrapper.full(eb, rb)
                    val = aten_sisdr(reordered[0], rb[0])
                    out.append((loss, perm, pair, val.mean().item() if item else val))
                return out

            legs = {"single": single, "loop": loop, "loop_item": lambda: loop(True)}
            with torch.no_grad():
                for fn in legs.values():
                    for _ in range(args.warmup):
                        fn()
                torch.cuda.synchronize()
                per, each = single(), loop()
                same = all(torch.equal(per.perm[b], each[b][1][0]) and torch.equal(per.pair[b], each[b][2][0])
                           and torch.equal(per.loss[b], each[b][0]) for b in range(B))
                sdr_diff = max(float((per.si_sdr[b] - each[b][3]).abs().max()) for b in range(B))
                wall = {k: [] for k in legs}
                span = {k: [] for k in legs}
                for _ in range(args.iters):
                    for name, fn in legs.items():
                        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        a.record()
                        fn()
                        z.record()
                        torch.cuda.synchronize()
                        wall[name].append((time.perf_counter() - t0) * 1e3)
                        span[name].append(a.elapsed_time(z))
            line = dict(workload=tag, clips=B, sources=S, sample_rate=sr, padded_samples=L, valid_samples=sum(lens), iters=args.iters,
                        device=torch.cuda.get_device_name(0), loop_bits_equal=bool(same), si_sdr_max_abs_diff_db=sdr_diff,
                        mean_si_sdr_db=float(per.si_sdr.mean()))
            for name in legs:
                line[f"{name}_wall_ms"] = percentiles(wall[name])
                line[f"{name}_event_ms"] = percentiles(span[name])
            line["loop_over_single_wall_p50"] = line["loop_wall_ms"]["p50"] / line["single_wall_ms"]["p50"]
            line["loop_item_over_single_wall_p50"] = line["loop_item_wall_ms"]["p50"] / line["single_wall_ms"]["p50"]
            print(json.dumps(line), flush=True)
            lines.append(line)
            del est, ref
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
