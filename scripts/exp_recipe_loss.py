#!/usr/bin/env python
"""Forward + backward of the recipe loss on one MI355X: the fused kernel (spiking_fullsubnet_amd.loss.RecipeLoss) against the ATen
composite a user of the reference would bolt on (freq_MAE, mag_MAE and SISNRLoss restated with torch.stft, then .backward()), on the
same tensors.

    python scripts/exp_recipe_loss.py [--rows 64 16] [--samples 128000] [--iters 60] [--warmup 10] [--out FILE.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/exp_recipe_loss.py --only fused --iters 5 --rows 64

Per shape: both sides are warmed up, then timed in alternating blocks (fused, ATen, fused, ATen) with one pair of HIP events per
iteration; p50 / p99 per block are printed, so the spread between the two ATen blocks (the same code run twice) is the yardstick a
difference has to exceed.  The loss values and the gradients of both sides are compared once (max difference) before timing.
Prints one JSON line per shape.  Needs a GPU: there is no CPU fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def aten_loss(est, tgt, window):
    E = torch.stft(est, n_fft=2048, hop_length=512, window=window, return_complex=True)
    T = torch.stft(tgt, n_fft=2048, hop_length=512, window=window, return_complex=True)
    freq = (E.real - T.real).abs().mean() + (E.imag - T.imag).abs().mean()
    E2 = torch.stft(est, n_fft=2048, hop_length=512, window=window, return_complex=True)  # mag_MAE transforms both again, as the reference does
    T2 = torch.stft(tgt, n_fft=2048, hop_length=512, window=window, return_complex=True)
    mag = (E2.abs() - T2.abs()).abs().mean()
    eps = torch.finfo(est.dtype).eps
    a, b = est - est.mean(-1, keepdim=True), tgt - tgt.mean(-1, keepdim=True)
    proj = (b * a).sum(-1, keepdim=True) * b / (b ** 2).sum(-1, keepdim=True)
    sisnr = (10 * torch.log10((proj ** 2).sum(-1) / (((a - proj) ** 2).sum(-1) + eps) + eps)).mean()
    return freq + mag + 0.001 * (100 - sisnr)


def timed(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in ev])
    return dict(p50_ms=float(np.percentile(ms, 50)), p99_ms=float(np.percentile(ms, 99)), min_ms=float(ms.min()), n=iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[64, 16])
    ap.add_argument("--samples", type=int, default=128000)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", choices=["fused", "aten"], default=None, help="run one side only (for a profiler run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_recipe_loss.py needs a GPU")
    from spiking_fullsubnet_amd.loss import RecipeLoss
    dev = "cuda:0"
    recipe = RecipeLoss()
    window = torch.hann_window(2048, device=dev)
    lines = []
    for rows in args.rows:
        g = torch.Generator().manual_seed(rows)
        clean = (0.1 * torch.randn(rows, args.samples, generator=g)).to(dev)
        est = (0.7 * clean + 0.05 * torch.randn(rows, args.samples, generator=g).to(dev)).requires_grad_(True)

        def fused():
            est.grad = None
            recipe(est, clean)[0].backward()

        def aten():
            est.grad = None
            aten_loss(est, clean, window).backward()

        sides = {"fused": fused, "aten": aten}
        if args.only:
            sides = {args.only: sides[args.only]}
        for fn in sides.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        line = dict(rows=rows, samples=args.samples, device=torch.cuda.get_device_name(0))
        if not args.only:
            fused()
            lf, gf = recipe(est, clean)[0].item(), est.grad.clone()
            aten()
            la = aten_loss(est, clean, window).item()
            line.update(loss_fused=lf, loss_aten=la, grad_max_abs_diff=float((gf - est.grad).abs().max()),
                        grad_max_abs=float(est.grad.abs().max()), grad_share_differing_by_1e_6=float(((gf - est.grad).abs() > 1e-6 * est.grad.abs().max()).float().mean()))
        for block in (0, 1):
            for name, fn in sides.items():
                line[f"{name}_block{block}"] = timed(fn, args.iters)
        if not args.only:
            line["speedup_p50"] = min(line["aten_block0"]["p50_ms"], line["aten_block1"]["p50_ms"]) / max(line["fused_block0"]["p50_ms"], line["fused_block1"]["p50_ms"])
            line["aten_block_spread_p50"] = abs(line["aten_block0"]["p50_ms"] - line["aten_block1"]["p50_ms"]) / line["aten_block0"]["p50_ms"]
        print(json.dumps(line), flush=True)
        lines.append(line)
        del est, clean
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
