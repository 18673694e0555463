#!/usr/bin/env python3
"""Generate the cIRM-GSN fixtures under tests/golden/ by running the REFERENCE model (audiozen.models.cirm_gsn.modeling_cirm_gsn.Model)
on the CPU, importing the reference checkout and stubs the way make_golden.py does:

    python tests/golden/make_golden_cirm.py

Writes
  cirm_tiny.npz       H = 20 (not a multiple of 16), 3 layers, df 3, BatchNorm, shared gates, 1 speaker: seeded weights (sd/<name>),
                      the wave, the reference's STFT, LayerNorm rows, per-layer spikes (+ the near-threshold masks of parity.TAU),
                      enhanced spectrum, enh_y and enh_mag
  cirm_tiny_2spk.npz  the same with 2 speakers (the model returns (enh_y, [all_layer_outputs]))
  cirm_gsn_init.json  the recipe's [model] section and the name, shape, dtype and sha256 of every state-dict entry the reference
                      builds under torch.manual_seed(1234)
Nothing of the reference's source is copied: the fixtures hold inputs, synthetic weights and the reference's outputs.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))  # tests/

from make_golden import REF, import_reference, pack  # noqa: E402

TINY = dict(n_fft=512, hop_length=128, win_length=512, fdrc=0.5, input_size=257, hidden_size=20, num_layers=3, proj_size=257,
            output_activate_function=False, df_order=3, use_pre_layer_norm_fb=True, bn=True, shared_weights=True, sequence_model="GSN")
TAU = 1e-4  # parity.TAU


def tiny_case(fname, num_spks, seed, B=2, T=24):
    import torch
    from audiozen.models.cirm_gsn.modeling_cirm_gsn import Model
    from audiozen.models.cirm_gsn.efficient_spiking_neuron import GSUCell
    kw = dict(TINY, num_spks=num_spks)
    torch.manual_seed(seed)
    model = Model(**kw)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():  # BatchNorm statistics away from the identity, so that the fold is exercised
        for name, mod in model.named_modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.weight.copy_(1.0 + 0.3 * torch.rand(mod.num_features, generator=g))
                mod.bias.copy_(0.2 * torch.randn(mod.num_features, generator=g))
                mod.running_mean.copy_(0.1 * torch.randn(mod.num_features, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(mod.num_features, generator=g))
            if isinstance(mod, torch.nn.LayerNorm):
                mod.weight.copy_(1.0 + 0.2 * torch.randn(mod.normalized_shape, generator=g))
                mod.bias.copy_(0.1 * torch.randn(mod.normalized_shape, generator=g))
    model.eval()
    L = (T - 1) * kw["hop_length"]
    wave = (0.1 * torch.randn(B, L, generator=g)).float()
    mem, outs, spec = {}, {}, {}

    def cell_hook(name):
        def hook(_m, _inp, out):
            mem.setdefault(name, []).append(out[1][1].detach().numpy().copy())
        return hook

    handles = [mod.register_forward_hook(cell_hook(n)) for n, mod in model.named_modules() if isinstance(mod, GSUCell)]
    def fb_hook(_m, _inp, out):  # (returns None: the module's output stays what it was)
        outs["all"] = [a.detach().numpy().copy() for a in out[1]]

    handles.append(model.fb_model.register_forward_hook(fb_hook))
    istft = model.istft

    def tap_istft(x, *a, **k):
        spec["enh"] = x.detach().numpy().copy()
        return istft(x, *a, **k)

    model.istft = tap_istft
    with torch.no_grad():
        res = model(wave)
        mag, _, real, imag = model.stft(wave)
    for h in handles:
        h.remove()
    out = {f"sd/{k}": v.detach().numpy() for k, v in model.state_dict().items()}
    out["wave"] = wave.numpy()
    out["stft"] = torch.complex(real, imag).numpy().astype(np.complex64)
    out["enh_stft"] = spec["enh"].reshape(B, num_spks, *spec["enh"].shape[1:]).astype(np.complex64)
    out["enh_y"] = res[0].numpy()
    if num_spks == 1:
        out["enh_mag"] = res[1].numpy()
    all_layers = outs["all"]
    out["x"] = all_layers[0]
    names = sorted(mem)
    for l, name in enumerate(names):
        m = np.stack(mem[name])
        s = all_layers[1 + l]
        assert s.shape == m.shape, (s.shape, m.shape)
        out[f"spikes_shape/{l}"] = np.array(s.shape)
        out[f"spikes_packed/{l}"] = pack(s > 0.5)
        out[f"near{TAU:g}/{l}"] = pack(np.abs(m) < TAU)
    out["kwargs"] = np.array(json.dumps(kw))
    out["torch_version"] = np.array(torch.__version__)
    np.savez_compressed(os.path.join(HERE, fname), **out)
    print(fname, os.path.getsize(os.path.join(HERE, fname)), "bytes")


def init_case(seed=1234):
    import tomli
    import torch
    from audiozen.utils import instantiate
    recipe = "recipes/intel_ndns/cirm_gsn/default.toml"
    cfg = tomli.load(open(os.path.join(REF, recipe), "rb"))["model"]
    torch.manual_seed(seed)
    ref = instantiate(cfg["path"], args=cfg["args"])
    state = [dict(name=k, shape=list(v.shape), dtype=str(v.dtype).replace("torch.", ""),
                  sha256=hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest()) for k, v in ref.state_dict().items()]
    out = dict(recipe=recipe, path=cfg["path"], args=cfg["args"], seed=seed, state_dict=state,
               parameters=[n for n, _ in ref.named_parameters()], meta=dict(torch=torch.__version__))
    with open(os.path.join(HERE, "cirm_gsn_init.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("cirm_gsn_init.json", len(state))


def main():
    import_reference()
    tiny_case("cirm_tiny.npz", 1, 21)
    tiny_case("cirm_tiny_2spk.npz", 2, 22)
    init_case()


if __name__ == "__main__":
    main()
