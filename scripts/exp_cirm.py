#!/usr/bin/env python3
"""cIRM-GSN forward timings (modeling_cirm_gsn.Model at the recipe's geometry: H = 268, 4 layers, df 3, BatchNorm, shared gates) on
the HIP kernels and, as the baseline, the same forward written as plain eager torch operations (the reference's cell loop with
torch.mm, LayerNorm, Linear and the deep filter as torch ops, on the same device).

    python scripts/exp_cirm.py [--shapes 64x1000,16x3751] [--iters 10] [--eager-iters 2] [--once]

--once: one forward of the first shape only (for `rocprofv3 --kernel-trace --stats -- python scripts/exp_cirm.py --once`).
Prints one JSON line per shape."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_cirm_gsn import recipe_model  # noqa: E402


@torch.no_grad()
def eager_forward(m, wave):
    """The reference's forward (modeling_cirm_gsn.py:206-245) as eager torch ops on the module's own parameters."""
    seq = m.fb_model
    B, L = wave.shape
    cmp = torch.stft(wave, m.n_fft, m.hop_length, m.win_length, window=torch.hann_window(m.n_fft, device=wave.device), return_complex=True)
    x = (cmp.abs() ** m.fdrc).permute(2, 0, 1)
    x = seq.pre_layer_norm(x)
    for layer in seq.sequence_model.layers:
        cell = layer.cell
        H = cell.hidden_size
        w_ih, w_hh = cell.weight_ih.repeat(2, 1), cell.weight_hh.repeat(2, 1)
        zin = torch.matmul(x, w_ih.t()) + cell.bias_ih
        h = torch.zeros(B, H, device=wave.device)
        c = torch.zeros(B, H, device=wave.device)
        outs = []
        for t in range(x.shape[0]):
            gates = zin[t] + torch.mm(h, w_hh.t())
            f, g = gates.chunk(2, 1)
            f = torch.sigmoid(f)
            c = cell.batchnorm(f * c + (1 - f) * g)
            h = (c >= 0).float()
            outs.append(h)
        x = torch.stack(outs)
    y = seq.proj(x).permute(1, 2, 0)  # [B, P, T]
    from spiking_fullsubnet_amd.modeling_cirm_gsn import deep_filter_torch
    enh = deep_filter_torch(cmp, y, m.df_order, m.num_spks)[:, 0]
    return torch.istft(enh, m.n_fft, m.hop_length, m.win_length, window=torch.hann_window(m.n_fft, device=wave.device), length=L)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x1000,16x3751")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--eager-iters", type=int, default=2)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    m, kw = recipe_model(seed=3)
    m = m.cuda()
    for shape in a.shapes.split(","):
        B, T = (int(v) for v in shape.split("x"))
        wave = torch.randn(B, (T - 1) * kw["hop_length"], device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 0.1
        if a.once:
            m(wave)
            torch.cuda.synchronize()
            print(json.dumps(dict(shape=[B, T], launches=m.engine().launches)))
            return
        p50, best = timed(lambda: m(wave), a.iters)
        # the hot path alone (between stft and istft)
        cmp = m._stft(wave)
        h50, hbest = timed(lambda: m.engine().forward_stft(cmp), a.iters)
        m.engine().check_stack_errors()
        e50, ebest = timed(lambda: eager_forward(m, wave), a.eager_iters)
        # (a sanity figure only: the eager loop's GEMMs sum in another order, and over hundreds of frames a spike chain with seeded
        #  random weights drifts apart; the parity tests compare against the oracle with the causal rule instead)
        y, _ = m(wave)
        ye = eager_forward(m, wave)
        rel = float((y - ye).norm() / ye.norm())
        print(json.dumps(dict(shape=[B, T], forward_ms_p50=round(p50, 3), forward_ms_min=round(best, 3), between_stft_istft_ms_p50=round(h50, 3),
                              between_stft_istft_ms_min=round(hbest, 3), eager_torch_ms_p50=round(e50, 1), eager_torch_ms_min=round(ebest, 1),
                              speedup_p50=round(e50 / p50, 1), rel_l2_vs_eager=rel, device=torch.cuda.get_device_name())), flush=True)


if __name__ == "__main__":
    main()
