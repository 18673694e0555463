#!/usr/bin/env python3
"""Generate the cIRM-GSN TRAINING fixtures under tests/golden/ by running the REFERENCE model
(audiozen.models.cirm_gsn.modeling_cirm_gsn.Model) on the CPU, imported the way make_golden.py does:

    python tests/golden/make_golden_cirm_train.py [name ...]

One step each (tests/cirm_train_cases.CASES): ``.train()``, forward, a scalar loss that reaches every output, ``backward()`` --
``cirm_tiny_evalgrad`` the same in ``.eval()`` mode with a wave that requires grad.  Stored: the wave, the outputs, the loss, the
layer list (x_norm and proj whole for the tiny cases, their first four frames for the recipe case; spike trains packed), the
``near1e-4`` masks of the membranes, every parameter's gradient, the BatchNorm buffers after the step, and a checksum of the weights
(the tests rebuild them from the seed).  A fixture is cut into shards of less than 1 MiB (cirm_train_cases.shard_arrays).

The generator refuses to write a fixture in which a parameter's gradient is all zero, in which (tiny cases) any membrane lies within
1e-4 of the threshold, or in which (recipe case) more than 2e-4 of a layer's membranes do.  Nothing of the reference's source is
copied: the fixtures hold inputs and the reference's results.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))  # tests/

import cirm_train_cases as cases  # noqa: E402
from make_golden import import_reference, pack  # noqa: E402


def train_case(name):
    import torch
    from audiozen.models.cirm_gsn.efficient_spiking_neuron import GSUCell
    from audiozen.models.cirm_gsn.modeling_cirm_gsn import Model
    kw, seed, B, T, mode = cases.CASES[name]
    S, recipe = kw["num_spks"], kw["hidden_size"] > 64
    model = cases.build_model(Model, kw, seed)
    checksum = cases.state_checksum(model)
    model.train() if mode == "train" else model.eval()
    wave = cases.make_wave(kw, seed, B, T)
    if mode == "evalgrad":
        wave.requires_grad_(True)
    mem, kept = {}, {}

    def cell_hook(nm):
        def hook(_m, _inp, out):
            mem.setdefault(nm, []).append(out[1][1].detach().numpy().copy())
        return hook

    handles = [mod.register_forward_hook(cell_hook(n)) for n, mod in model.named_modules() if isinstance(mod, GSUCell)]

    def fb_hook(_m, _inp, out):
        kept["all"] = [a.detach().numpy().copy() for a in out[1]]

    handles.append(model.fb_model.register_forward_hook(fb_hook))
    res = model(wave)
    for h in handles:
        h.remove()
    loss = cases.loss_of(res, S)
    loss.backward()
    out = dict(wave=wave.detach().numpy(), enh_y=res[0].detach().numpy(), loss=np.asarray(float(loss)), checksum=np.array(checksum),
               kwargs=np.array(json.dumps(kw)), seed=np.asarray(seed), mode=np.array(mode), torch_version=np.array(torch.__version__))
    if S == 1:
        out["enh_mag"] = res[1].detach().numpy()
    if mode == "evalgrad":
        out["grad_wave"] = wave.grad.numpy()
    layers = kept["all"]
    out["x"] = layers[0][:4].copy() if recipe else layers[0]
    out["proj"] = layers[-1][:4].copy() if recipe else layers[-1]
    rates = []
    for l, nm in enumerate(sorted(mem)):
        m, s = np.stack(mem[nm]), layers[1 + l]
        assert s.shape == m.shape == (T, B, kw["hidden_size"]), (s.shape, m.shape)
        assert set(np.unique(s)) <= {0.0, 1.0}
        near = np.abs(m) < cases.TAU
        share = float(near.mean())
        if recipe:
            assert share <= 2e-4, f"{name} layer {l}: {share:.3g} of the membranes within {cases.TAU:g} of the threshold: take another seed"
        else:
            assert not near.any(), f"{name} layer {l}: {int(near.sum())} membranes within {cases.TAU:g} of the threshold: take another seed"
        out[f"spikes_shape/{l}"] = np.array(s.shape)
        out[f"spikes_packed/{l}"] = pack(s > 0.5)
        out[f"near{cases.TAU:g}/{l}"] = pack(near)
        rates.append((round(float(s.mean()), 3), share, float((np.abs(m) < 1e-3).mean())))
    for k, p in model.named_parameters():
        assert p.grad is not None and bool((p.grad != 0).any()), f"{name}: the gradient of {k} is zero"
        out[f"grad/{k}"] = p.grad.numpy()
    for k, b in model.named_buffers():
        out[f"buf/{k}"] = b.detach().numpy()
    for old in cases.shard_paths(HERE, name):
        os.remove(old)
    shards = cases.shard_arrays(out)
    for i, sh in enumerate(shards):
        path = os.path.join(HERE, f"{name}.npz" if i == 0 else f"{name}.{i}.npz")
        np.savez_compressed(path, **sh)
        assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
    total = sum(os.path.getsize(p) for p in cases.shard_paths(HERE, name))
    print(f"{name}: loss {float(loss):.6g}, {len(shards)} shard(s), {total} bytes; per layer (spike rate, share within 1e-4, within 1e-3): {rates}")


def main():
    import_reference()
    for name in (sys.argv[1:] or list(cases.CASES)):
        train_case(name)


if __name__ == "__main__":
    main()
