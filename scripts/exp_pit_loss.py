#!/usr/bin/env python
"""Forward + backward of the wsj0-mix recipes' loss on one MI355X: the fused kernel (spiking_fullsubnet_amd.pit.PITWrapper: one call of
sfsn_pit_sdr) against the ATen composite a user of the reference runs (PITWrapper(PairwiseNegSDR()) of audiozen/pit.py restated
here: the broadcast [B,S,S,L] products, the one-hot einsum over the permutations, the per-clip Python loops that pick the permutation
and gather the sources -- which index with device values and so synchronise the host -- then .backward()), on the same tensors.

    python scripts/exp_pit_loss.py [--clips 64 16] [--sources 2] [--samples 32000] [--iters 400] [--warmup 20] [--blocks 3] [--out FILE.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/exp_pit_loss.py --only fused --iters 5 --warmup 2 --blocks 1 --clips 64

Per shape: both sides are warmed up, then timed in alternating blocks (fused, ATen, fused, ATen, ...), each block as ONE pair of HIP
events around `iters` iterations (the window is a few tenths of a second; the composite synchronises inside its own iterations, so
per-iteration events would not see its host time).  The blocks of one side are the same code run again: their spread is the yardstick
a difference has to exceed.  Loss, permutation and gradient of both sides are compared once before timing.  Algorithmic bytes: two reads
of both tensors and one write each of grad_est and reordered.  Prints one JSON line per shape.  Needs a GPU: there is no CPU fallback."""
import argparse
import json
import os
import sys
from itertools import permutations

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EPS = 1e-8


def aten_pit(est, ref):
    """(mean_loss, reordered, chosen indices): the reference's sequence of ATen operations."""
    S = est.shape[1]
    a = (est - est.mean(2, keepdim=True)).unsqueeze(2)
    r = (ref - ref.mean(2, keepdim=True)).unsqueeze(1)
    dot = (a * r).sum(3, keepdim=True)
    energy = (r ** 2).sum(3, keepdim=True) + EPS
    proj = dot * r / energy
    noise = a - proj
    pair = -(10 * torch.log10((proj ** 2).sum(3) / ((noise ** 2).sum(3) + EPS) + EPS))
    pwl = pair.transpose(-1, -2)
    perms = pwl.new_tensor(list(permutations(range(S))), dtype=torch.long)
    one_hot = pwl.new_zeros((*perms.size(), S)).scatter_(2, perms.unsqueeze(2), 1)
    loss_set = torch.einsum("bij,pij->bp", [pwl, one_hot]) / S
    min_loss, min_idx = torch.min(loss_set, dim=1)
    chosen = torch.stack([perms[m] for m in min_idx], dim=0)  # a Python loop over the clips, indexing with device values
    reordered = torch.stack([torch.index_select(s, 0, b) for s, b in zip(est, chosen)])
    return min_loss.mean(), reordered, chosen


def timed_block(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, nargs="+", default=[64, 16])
    ap.add_argument("--sources", type=int, default=2)
    ap.add_argument("--samples", type=int, default=32000)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--only", choices=["fused", "aten"], default=None, help="run one side only (for a profiler run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_pit_loss.py needs a GPU")
    from spiking_fullsubnet_amd.pit import PairwiseNegSDR, PITWrapper
    dev = "cuda:0"
    wrapper = PITWrapper(PairwiseNegSDR())
    S, L = args.sources, args.samples
    lines = []
    for B in args.clips:
        g = torch.Generator().manual_seed(B)
        ref = (0.1 * torch.randn(B, S, L, generator=g))
        sigma = torch.stack([torch.randperm(S, generator=g) for _ in range(B)])
        est = 0.7 * torch.stack([ref[b, sigma[b]] for b in range(B)]) + 0.05 * torch.randn(B, S, L, generator=g)
        ref, est = ref.to(dev), est.to(dev).requires_grad_(True)

        def fused():
            est.grad = None
            wrapper(est, ref)[0].backward()

        def aten():
            est.grad = None
            aten_pit(est, ref)[0].backward()

        sides = {"fused": fused, "aten": aten}
        if args.only:
            sides = {args.only: sides[args.only]}
        for fn in sides.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        nbytes = 6 * B * S * L * 4
        line = dict(clips=B, sources=S, samples=L, iters=args.iters, device=torch.cuda.get_device_name(0), algorithmic_bytes=nbytes)
        if not args.only:
            fused()
            lf, rf, pf, _ = wrapper.full(est, ref)
            gf = est.grad.clone()
            aten()
            la, ra, pa = aten_pit(est, ref)
            line.update(loss_fused=lf.item(), loss_aten=la.item(), perms_equal=bool(torch.equal(pf, pa)), reordered_equal=bool(torch.equal(rf, ra.detach())),
                        grad_max_abs_diff=float((gf - est.grad).abs().max()), grad_max_abs=float(est.grad.abs().max()))
        for name in sides:
            line[f"{name}_ms"] = []
        for _ in range(args.blocks):
            for name, fn in sides.items():
                line[f"{name}_ms"].append(timed_block(fn, args.iters))
        for name in sides:
            ms = line[f"{name}_ms"]
            line[f"{name}_spread"] = (max(ms) - min(ms)) / min(ms)
        line["fused_bytes_per_s" if "fused" in sides else "aten_bytes_per_s"] = nbytes / (min(line["fused_ms" if "fused" in sides else "aten_ms"]) * 1e-3)
        if not args.only:
            line["aten_over_fused_worst_pair"] = min(line["aten_ms"]) / max(line["fused_ms"])
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
