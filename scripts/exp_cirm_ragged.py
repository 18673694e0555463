#!/usr/bin/env python3
"""cIRM-GSN on clips of different lengths (profiles/cirm_ragged.md): the recipe's model (H = 268, 4 layers, 512-point frames), 16 and
64 clips of 2 ... 8 s from scripts/exp_ragged.py's seeded length draw.  Two comparisons, the legs of each alternated repetition by
repetition in one process, p50 of the repetitions after warm-up:

    forward   loop      model(wave_b[None, :L_b]) for every clip: the path that exists without per-clip lengths
              ragged    one model.forward_ragged(waves, lengths) on the batch padded to the longest clip
              (host clock around the leg plus a stream synchronise; both return every clip's enhanced waveform and magnitude)
    kernel    plain     sfsn_fullband_proj_deepfilter on the padded batch + sfsn_zero_tail_frames on enh_stft and on enh_mag
              ragged    sfsn_fullband_proj_deepfilter_ragged on the same buffers
              (device events around `--inner` back-to-back repetitions of the leg; the two legs' outputs are compared bit for bit first)

    python scripts/exp_cirm_ragged.py [--clips 16,64] [--reps 20] [--warmup 3] [--inner 10]

Prints one JSON line per clip count."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from exp_ragged import SR, clips  # noqa: E402
from spiking_fullsubnet_amd import _lib, ragged  # noqa: E402
from spiking_fullsubnet_amd.engine import _ptr  # noqa: E402
from spiking_fullsubnet_amd.modeling_cirm_gsn import Model  # noqa: E402

RECIPE = dict(n_fft=512, hop_length=128, win_length=512, fdrc=0.5, input_size=257, hidden_size=268, num_layers=4, proj_size=257,
              output_activate_function=False, df_order=3, use_pre_layer_norm_fb=True, bn=True, shared_weights=True, sequence_model="GSN",
              num_spks=1)


def recipe_model(seed=7):
    torch.manual_seed(seed)
    m = Model(**RECIPE)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.copy_(0.1 * torch.randn(mod.num_features, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(mod.num_features, generator=g))
    return m.eval().cuda()


def p50(v):
    return round(float(np.percentile(v, 50)), 4)


def stats(v, n):
    return dict(p50_ms=p50(v), min_ms=round(min(v), 4), max_ms=round(max(v), 4), clips_per_s=round(n / p50(v) * 1e3, 1))


def kernel_legs(m, waves, lengths):
    """The two epilogues on the buffers of one forward of the padded batch: (legs, frames, check)."""
    eng, hop = m.engine(), m.hop_length
    frames = ragged.frames_of(lengths, hop)
    both = ragged.upload([lengths, frames], waves.device)
    stft = m._stft_ragged(waves, both[0])
    eng.forward_stft(stft)  # leaves the last layer's int8 spikes of this batch in the engine's workspace
    B, F, T = stft.shape
    s8 = eng._workspace(B, T, eng._use_stack(B))["s8"][-1]
    ri = torch.view_as_real(stft.contiguous())
    L, st, S = eng.lib, eng._stream(), eng.spec.num_spks
    out = {k: (torch.empty((B, S, F, T, 2), device=waves.device), torch.empty((B, S, F, T), device=waves.device)) for k in ("plain", "ragged")}
    args = lambda enh, mag: (_ptr(ri), _ptr(s8), eng.Hp, _ptr(eng.proj_q), _ptr(eng.proj_dq), _ptr(eng.proj_b), eng.spec.act, B, F, T, S,
                             eng.spec.df, None, _ptr(enh), _ptr(mag), 0, T)
    fd = _ptr(both[1])

    def plain():
        enh, mag = out["plain"]
        _lib.check(L.sfsn_fullband_proj_deepfilter(*args(enh, mag), st), "sfsn_fullband_proj_deepfilter")
        _lib.check(L.sfsn_zero_tail_frames(_ptr(enh), B, S * F, T, 2, fd, st), "sfsn_zero_tail_frames")
        _lib.check(L.sfsn_zero_tail_frames(_ptr(mag), B, S * F, T, 1, fd, st), "sfsn_zero_tail_frames")

    def rag():
        enh, mag = out["ragged"]
        _lib.check(L.sfsn_fullband_proj_deepfilter_ragged(*args(enh, mag), fd, st), "sfsn_fullband_proj_deepfilter_ragged")

    def check():
        plain()
        rag()
        torch.cuda.synchronize()
        return all(torch.equal(a, b) for a, b in zip(out["plain"], out["ragged"]))

    return dict(plain=plain, ragged=rag), frames, check


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", default="16,64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    m = recipe_model()
    stream = torch.cuda.current_stream()
    for n in (int(v) for v in a.clips.split(",")):
        waves, lengths = clips(n)
        fwd = dict(loop=lambda: [m(waves[b:b + 1, :L]) for b, L in enumerate(lengths)], ragged=lambda: m.forward_ragged(waves, lengths))
        fms = {k: [] for k in fwd}
        with torch.no_grad():
            for rep in range(a.warmup + a.reps):
                for k, fn in fwd.items():  # the legs take turns, so that drift of the machine falls on both alike
                    stream.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    stream.synchronize()
                    if rep >= a.warmup:
                        fms[k].append((time.perf_counter() - t0) * 1e3)
            m.engine().check_stack_errors()
            legs, frames, check = kernel_legs(m, waves, lengths)
            equal = check()
            kms = {k: [] for k in legs}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for rep in range(a.warmup + a.reps):
                for k, fn in legs.items():
                    stream.synchronize()
                    e0.record(stream)
                    for _ in range(a.inner):
                        fn()
                    e1.record(stream)
                    stream.synchronize()
                    if rep >= a.warmup:
                        kms[k].append(e0.elapsed_time(e1) / a.inner)
        T = max(frames)
        out = dict(clips=n, reps=a.reps, inner=a.inner, seconds_of_audio=round(sum(lengths) / SR, 1), padded_seconds=round(n * max(lengths) / SR, 1),
                   frames=sum(frames), padded_frames=n * T, kernel_outputs_equal=equal, device=torch.cuda.get_device_name(),
                   source_hash=_lib.source_hash(), forward={k: stats(v, n) for k, v in fms.items()},
                   kernel={k: stats(v, n) for k, v in kms.items()})
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
