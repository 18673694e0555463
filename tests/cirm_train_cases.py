"""The cIRM-GSN training fixtures' models and inputs, shared by the generator (tests/golden/make_golden_cirm_train.py, which builds
the REFERENCE's Model from these) and the tests (which build spiking_fullsubnet_amd's): both classes initialise bit for bit alike
under one seed (test_cirm_gsn_host.test_init_matches_reference_bit_for_bit), so a fixture stores a checksum of the weights, not the
weights."""
import hashlib

import numpy as np
import torch

TINY = dict(n_fft=512, hop_length=128, win_length=512, fdrc=0.5, input_size=257, hidden_size=20, num_layers=3, proj_size=257,
            output_activate_function=False, df_order=3, use_pre_layer_norm_fb=True, bn=True, shared_weights=True, sequence_model="GSN",
            num_spks=1)
RECIPE = dict(TINY, hidden_size=268, num_layers=4)  # recipes/intel_ndns/cirm_gsn/default.toml's [model.args]

# fixture name -> (constructor keywords, seed, B, T, mode)
CASES = {
    "cirm_tiny_train": (TINY, 31, 3, 24, "train"),
    "cirm_tiny_2spk_train": (dict(TINY, num_spks=2), 32, 3, 24, "train"),
    "cirm_tiny_nobn_train": (dict(TINY, num_layers=2, bn=False), 33, 3, 24, "train"),
    "cirm_tiny_unshared_train": (dict(TINY, shared_weights=False), 34, 3, 24, "train"),
    "cirm_tiny_evalgrad": (TINY, 35, 3, 24, "evalgrad"),
    # the recipe's model at the size live_m_train.npz uses; layer inputs / projections by their first four frames
    "cirm_recipe_train": (RECIPE, 41, 16, 32, "train"),
}
TAU = 1e-4


def build_model(model_cls, kw, seed):
    """model_cls(**kw) under torch.manual_seed(seed), BatchNorm / LayerNorm parameters and statistics moved off their identity values
    by a seeded CPU generator (as make_golden_cirm.tiny_case does)."""
    torch.manual_seed(seed)
    m = model_cls(**kw)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.weight.copy_(1.0 + 0.3 * torch.rand(mod.num_features, generator=g))
                mod.bias.copy_(0.2 * torch.randn(mod.num_features, generator=g))
                mod.running_mean.copy_(0.1 * torch.randn(mod.num_features, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(mod.num_features, generator=g))
            if isinstance(mod, torch.nn.LayerNorm):
                mod.weight.copy_(1.0 + 0.2 * torch.randn(mod.normalized_shape, generator=g))
                mod.bias.copy_(0.1 * torch.randn(mod.normalized_shape, generator=g))
    return m


def make_wave(kw, seed, B, T):
    g = torch.Generator().manual_seed(seed + 2)
    return (0.1 * torch.randn(B, (T - 1) * kw["hop_length"], generator=g)).float()


def state_checksum(model) -> str:
    h = hashlib.sha256()
    for k, v in model.state_dict().items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


def loss_of(out, num_spks):
    """A scalar that reaches every output: mean square of the enhanced waveform (+ the mean enhanced magnitude for one speaker)."""
    return out[0].pow(2).mean() + out[1].mean() if num_spks == 1 else out[0].pow(2).mean()


# ---- fixtures in shards: the project's contribution rules admit no committed file above 1 MiB (the larger fixtures under tests/golden
# predate that rule), so a fixture is cut into files below it -------------------------------------------------------------------
SHARD_BYTES = 950_000  # raw bytes per shard (npz compression only shrinks float data marginally)


def shard_arrays(arrays: dict):
    """Split {key: array} into a list of dicts of at most SHARD_BYTES raw bytes each; an array larger than that is cut along its first
    axis into parts stored as key@@i."""
    items = []
    for k, a in arrays.items():
        a = np.asarray(a)
        if a.nbytes <= SHARD_BYTES or a.ndim == 0:
            items.append((k, a))
            continue
        rows = max(1, int(SHARD_BYTES // (a.nbytes // a.shape[0])))
        for i, r0 in enumerate(range(0, a.shape[0], rows)):
            items.append((f"{k}@@{i}", a[r0:r0 + rows]))
    shards, cur, size = [], {}, 0
    for k, a in items:
        if cur and size + a.nbytes > SHARD_BYTES:
            shards.append(cur)
            cur, size = {}, 0
        cur[k] = a
        size += a.nbytes
    shards.append(cur)
    return shards


def shard_paths(gold_dir, name):
    import os
    paths, i = [], 0
    while True:
        p = os.path.join(gold_dir, f"{name}.npz" if i == 0 else f"{name}.{i}.npz")
        if not os.path.exists(p):
            return paths
        paths.append(p)
        i += 1


def load_fixture(gold_dir, name) -> dict:
    """All shards of a fixture as one {key: array}, split arrays joined."""
    paths = shard_paths(gold_dir, name)
    assert paths, f"{name}.npz is missing under {gold_dir}"
    flat = {}
    for p in paths:
        with np.load(p) as z:
            flat.update({k: z[k] for k in z.files})
    out, parts = {}, {}
    for k, a in flat.items():
        if "@@" in k:
            base, i = k.split("@@")
            parts.setdefault(base, {})[int(i)] = a
        else:
            out[k] = a
    for base, d in parts.items():
        out[base] = np.concatenate([d[i] for i in range(len(d))], axis=0)
    return out
