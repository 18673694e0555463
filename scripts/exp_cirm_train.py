#!/usr/bin/env python3
"""cIRM-GSN TRAINING-step timings (modeling_cirm_gsn.Model at the recipe's geometry in train() mode: forward + backward, device
synchronised):

  a  the step with the HIP deep filter (sfsn_fullband_deepfilter_fwd / _bwd)
  b  the same step with the torch deep filter (training.TRAIN_FULLBAND_DF = False, what SFSN_TRAIN_FULLBAND_DF=0 selects)
  c  the step written as plain eager torch operations on the same device: the reference's cell loop with training-mode BatchNorm and the
     triangle surrogate, LayerNorm, Linear and the deep filter as torch ops, grad enabled, plus backward()

    python scripts/exp_cirm_train.py [--shapes 64x1000,16x3751] [--iters 10] [--eager-iters 2] [--steps N]

a and b alternate inside one process (they share the machine's state); --steps N: N steps of variant a only and nothing else (for
`rocprofv3 --kernel-trace --stats -- python scripts/exp_cirm_train.py --shapes 64x1000 --steps 3`).  One JSON line per shape."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_cirm_gsn import recipe_model  # noqa: E402


class Triangle(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u):
        ctx.save_for_backward(u)
        return (u >= 0).float()

    @staticmethod
    def backward(ctx, g):
        u, = ctx.saved_tensors
        return g * (1 - u.abs()).clamp(min=0)


def eager_forward(m, wave):
    """The reference's training forward (modeling_cirm_gsn.py:206-245) as eager torch ops on the module's own parameters."""
    from spiking_fullsubnet_amd.modeling_cirm_gsn import deep_filter_torch
    seq = m.fb_model
    B, L = wave.shape
    window = torch.hann_window(m.n_fft, device=wave.device)
    cmp = torch.stft(wave, m.n_fft, m.hop_length, m.win_length, window=window, return_complex=True, pad_mode="constant")
    x = seq.pre_layer_norm((cmp.abs() ** m.fdrc).permute(2, 0, 1))
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
            h = Triangle.apply(c)
            outs.append(h)
        x = torch.stack(outs)
    enh = deep_filter_torch(cmp, seq.proj(x).permute(1, 2, 0), m.df_order, m.num_spks)[:, 0]
    return torch.istft(enh, m.n_fft, m.hop_length, m.win_length, window=window, length=L), enh.abs()


def loss_of(out):
    return out[0].pow(2).mean() + out[1].mean()


def main():
    from spiking_fullsubnet_amd import training
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x1000,16x3751")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--eager-iters", type=int, default=2)
    ap.add_argument("--steps", type=int, default=0)
    a = ap.parse_args()
    m, kw = recipe_model(seed=3)
    m = m.cuda().train()
    state0 = {k: v.detach().clone() for k, v in m.state_dict().items()}

    def step(fn, hip_df=True):
        for p in m.parameters():
            p.grad = None
        old = training.TRAIN_FULLBAND_DF
        training.TRAIN_FULLBAND_DF = hip_df
        try:
            loss = loss_of(fn())
            loss.backward()
        finally:
            training.TRAIN_FULLBAND_DF = old
        return loss

    def timed_step(fn, hip_df=True):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = step(fn, hip_df)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), float(loss)

    for shape in a.shapes.split(","):
        B, T = (int(v) for v in shape.split("x"))
        wave = torch.randn(B, (T - 1) * kw["hop_length"], device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 0.1
        if a.steps:
            for _ in range(a.steps):
                step(lambda: m(wave))
            torch.cuda.synchronize()
            training.check_pending()
            print(json.dumps(dict(shape=[B, T], steps=a.steps)))
            return
        for hip in (True, False):  # warm-up of both variants
            timed_step(lambda: m(wave), hip)
        ms_a, ms_b = [], []
        for _ in range(a.iters):
            ms_a.append(timed_step(lambda: m(wave), True)[0])
            ms_b.append(timed_step(lambda: m(wave), False)[0])
        training.check_pending()
        # losses from the same BatchNorm state for a, b and c
        def from_start(fn, hip=True):
            with torch.no_grad():
                for k, v in m.state_dict().items():
                    v.copy_(state0[k])
            return timed_step(fn, hip)
        loss_a, loss_b = from_start(lambda: m(wave), True)[1], from_start(lambda: m(wave), False)[1]
        ms_c, loss_c = [], None
        for i in range(a.eager_iters + 1):  # (the first one is the warm-up)
            ms, loss_c = from_start(lambda: eager_forward(m, wave))
            if i:
                ms_c.append(ms)
        p50 = lambda v: sorted(v)[len(v) // 2]
        r = lambda v: round(v, 3)
        print(json.dumps(dict(shape=[B, T], a_hip_df_ms_p50=r(p50(ms_a)), a_ms_min=r(min(ms_a)), a_ms_max=r(max(ms_a)),
                              b_torch_df_ms_p50=r(p50(ms_b)), b_ms_min=r(min(ms_b)), b_ms_max=r(max(ms_b)),
                              c_eager_ms_p50=r(p50(ms_c)), c_ms_min=r(min(ms_c)), speedup_c_over_a=round(p50(ms_c) / p50(ms_a), 1),
                              loss_a=loss_a, loss_b=loss_b, loss_c=loss_c, device=torch.cuda.get_device_name())), flush=True)


if __name__ == "__main__":
    main()
