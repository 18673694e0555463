#!/usr/bin/env python
"""The recipe loss on whole utterances and the REVERB loss on one MI355X, forward and backward.

    python scripts/exp_ragged_loss.py [--clips 64 16] [--iters 100] [--warmup 10] [--seed 0] [--out FILE.json]

Two measurements, each with its legs alternating inside one run:
  ragged   `RecipeLoss()(est, tgt, lengths=lens)` on a padded batch of clips of 2 to 8 s at 16 kHz (seeded, uniform), ONE kernel call
           (leg `single`; the lengths are uploaded from the host list each time, as a training step would), against the loop that
           equal-length calls make necessary (leg `loop`): per clip a slice of both tensors and `RecipeLoss()` on it, the losses
           averaged with equal weights; both legs end in `backward()` to the padded estimate.
  reverb   `ReverbRecipeLoss()(est, ref)` at the REVERB recipe's 32 clips of 64,000 samples (leg `fused`) against the ATen composite
           (leg `aten`): freq_MAE and mag_MAE restated with torch.stft (2048-point Hann, hop 512, centred, reflect) plus F.l1_loss.
Every iteration is timed twice over: a host clock around the leg up to a device synchronise (wall) and a pair of HIP events around its
enqueue (device span).  p50 and p99 of both are reported per leg.  Before timing, the legs' losses and gradients are compared.  Prints
one JSON line per workload.  Needs a GPU: no CPU fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SR = 16000


def aten_reverb_loss(est, ref, window):
    """freq_MAE + mag_MAE + l1 in ATen on [B, L] device tensors (spectra of the [-1, L] view, means over every element)."""
    E = torch.stft(est, n_fft=2048, hop_length=512, window=window, return_complex=True)
    T = torch.stft(ref, n_fft=2048, hop_length=512, window=window, return_complex=True)
    freq = (E.real - T.real).abs().mean() + (E.imag - T.imag).abs().mean()
    mag = (E.abs() - T.abs()).abs().mean()
    return freq + mag + torch.nn.functional.l1_loss(est, ref)


def percentiles(xs):
    return dict(p50=float(np.percentile(xs, 50)), p99=float(np.percentile(xs, 99)), min=float(np.min(xs)))


def signals(B, L, seed, dev):
    g = torch.Generator().manual_seed(seed)
    tgt = 0.1 * torch.randn(B, L, generator=g)
    est = 0.7 * tgt + 0.05 * torch.randn(B, L, generator=g)
    return est.to(dev).requires_grad_(True), tgt.to(dev)


def timed(legs, est, iters, warmup):
    """{leg: wall ms}, {leg: event ms}; a leg is a function that ends in backward() to est."""
    for fn in legs.values():
        for _ in range(warmup):
            est.grad = None
            fn()
    torch.cuda.synchronize()
    wall, span = {k: [] for k in legs}, {k: [] for k in legs}
    for _ in range(iters):
        for name, fn in legs.items():
            est.grad = None
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            fn()
            z.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            span[name].append(a.elapsed_time(z))
    return wall, span


def report(line, legs, wall, span, base, other):
    for name in legs:
        line[f"{name}_wall_ms"] = percentiles(wall[name])
        line[f"{name}_event_ms"] = percentiles(span[name])
    line[f"{other}_over_{base}_wall_p50"] = line[f"{other}_wall_ms"]["p50"] / line[f"{base}_wall_ms"]["p50"]
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, nargs="+", default=[64, 16])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_ragged_loss.py needs a GPU")
    from spiking_fullsubnet_amd.loss import RecipeLoss, ReverbRecipeLoss
    dev = "cuda:0"
    name = torch.cuda.get_device_name(0)
    lines = []
    recipe = RecipeLoss()
    for B in args.clips:
        rng = np.random.default_rng(args.seed + B)
        lens = [int(n) for n in rng.integers(2 * SR, 8 * SR + 1, size=B)]
        L = (max(lens) + 3) // 4 * 4  # (a row stride of whole 16 bytes: the loop's one-row slices stay aligned, as the C ABI asks)
        est, tgt = signals(B, L, args.seed + B, dev)

        def single():
            loss = recipe(est, tgt, lengths=lens)[0]
            loss.backward()
            return loss.detach()

        def loop():
            total = None
            for b, n in enumerate(lens):
                one = recipe(est[b:b + 1, :n], tgt[b:b + 1, :n])[0]
                total = one if total is None else total + one
            total = total / B
            total.backward()
            return total.detach()

        legs = {"single": single, "loop": loop}
        est.grad = None
        l_single, g_single = single(), est.grad.clone()
        est.grad = None
        l_loop, g_loop = loop(), est.grad.clone()
        wall, span = timed(legs, est, args.iters, args.warmup)
        line = dict(workload="ragged", clips=B, sample_rate=SR, padded_samples=L, valid_samples=sum(lens), iters=args.iters, device=name,
                    loss_single=float(l_single), loss_loop=float(l_loop), grad_max_abs_diff=float((g_single - g_loop).abs().max()),
                    grad_max_abs=float(g_single.abs().max()))
        lines.append(report(line, legs, wall, span, "single", "loop"))
        del est, tgt, g_single, g_loop
        torch.cuda.empty_cache()
    B, L = 32, 64000
    est, ref = signals(B, L, args.seed + 1, dev)
    reverb, window = ReverbRecipeLoss(), torch.hann_window(2048, device=dev)

    def fused():
        loss = reverb(est, ref)[0]
        loss.backward()
        return loss.detach()

    def aten():
        loss = aten_reverb_loss(est, ref, window)
        loss.backward()
        return loss.detach()

    legs = {"fused": fused, "aten": aten}
    est.grad = None
    l_fused, g_fused = fused(), est.grad.clone()
    est.grad = None
    l_aten, g_aten = aten(), est.grad.clone()
    wall, span = timed(legs, est, args.iters, args.warmup)
    line = dict(workload="reverb", clips=B, samples=L, iters=args.iters, device=name, loss_fused=float(l_fused), loss_aten=float(l_aten),
                grad_max_abs_diff=float((g_fused - g_aten).abs().max()), grad_max_abs=float(g_fused.abs().max()))
    lines.append(report(line, legs, wall, span, "fused", "aten"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
