"""What tests/test_stream_prime.py (GPU) and tests/test_stream_prime_host.py (CPU) share: the fixtures, seeds, spectra, prefix lengths
and the index arithmetic of ``StreamingSession.prime`` / ``prime_wave``, restated in plain numpy.  A helper module like hopref.py (not
a conftest).

The seeds are not free: in the one-launch tier a primed layer-0 membrane is the offline forward's, which differs in its low bits from
the hop's (include/sfsn.h), so the comparison `primed == streamed == offline` is exact only where no layer-0 membrane of the frames
behind the prefix lies within that rounding of the threshold.  test_stream_prime_host.py asserts that for every entry below."""
import numpy as np

import hopref as hr
import refweights as rw

F32 = np.float32
T = 60        # frames per clip of the spectral tests
B_MAX = 3
CALLS = 28    # step_wave calls per clip of the waveform tests
WAVE_C = (1, 2, 3, 4, 5, 19)

TINY_LAP = dict(rw.FROZEN_TINY, sb_df_orders=[3, 2, 1])  # (as tests/test_frozen_streaming.py: one launch covers P <= 256)
TINY_CUM = dict(rw.FROZEN_TINY_CUM, sb_df_orders=[3, 2, 1])

# name -> (front, kwargs, seed of the weights and of the clips of the spectral tests): the first seed from the existing streaming
# tests' (11, 12, 13, 35, 41; then + 100, + 101, ...) that meets the exactness condition -- about one seed in twenty does
FIXTURES = {
    "live_tiny": ("live", rw.LIVE_TINY, 111),
    "live_tiny_2spk": ("live", rw.LIVE_TINY_2SPK, 112),
    "live_tiny_unshared": ("live", rw.LIVE_TINY_UNSHARED, 132),
    "frozen_tiny_cum": ("frozen", TINY_CUM, 173),
    "frozen_tiny": ("frozen", TINY_LAP, 141),  # offline_laplace_norm: streamed and primed with the clips' own statistics
}
# the waveform tests' seeds (weights and samples), chosen the same way
WAVE_FIXTURES = {"live_tiny": 117, "live_tiny_2spk": 12, "frozen_tiny_cum": 35}


def state_dict(name, seed=None):
    front, kw, own = FIXTURES[name]
    return hr.base_state_dict(front, kw, own if seed is None else seed)


def df_reach(name):
    """D = max(df) - 1, the frames of history the deep filter reaches back."""
    kw = FIXTURES[name][1]
    return max(kw["df_orders"] if "df_orders" in kw else kw["sb_df_orders"]) - 1


def spectra(name, B, n_frames=T):
    """[B, 257, n_frames] complex64; clip b is the same whatever B is (a B = 1 session streams clip 0 of the B = 3 batch)."""
    seed = FIXTURES[name][2]
    return np.stack([hr.spectrum(1, 257, n_frames, 1000 * seed + b)[0] for b in range(B)])


def waves(name, B, calls=CALLS):
    """[B, 128 * calls] float32 (rw.synth_wave's distribution), clip b the same whatever B is."""
    seed = WAVE_FIXTURES[name]
    return np.stack([rw.synth_wave(1, calls + 1, 2000 * seed + b)[0] for b in range(B)])


def prefix_lengths(hop, D):
    """The prefix lengths of the continuation tests: one launch, the deep filter's reach (rounded up to whole launches), one launch
    more, an ODD number of launches (17 frames at hop 1, 18 at hop 2: the parity of the double-buffered state) and 40."""
    up = -(-max(D, 1) // hop) * hop
    return sorted({hop, up, up + hop, 17 if hop == 1 else 18, 40})


# ---- the index arithmetic, restated ---------------------------------------------------------------------------------------
def origin(k, N, hop):
    """clip_start of a clip primed with N frames when the next launch has index k (uint32 arithmetic)."""
    return (k - N // hop) % (1 << 32)


def frame_index_at(k, org):
    """The frame index sfsn_stream_hop gives a clip with origin `org` in launch k: the unsigned difference."""
    return (k - org) % (1 << 32)


def frames_of_calls(c):
    """The frames of torch.stft(center=True) that c calls of 128 samples complete: frame f ends with sample 128 f + 256."""
    return [f for f in range(c + 1) if 128 * f + 256 <= 128 * c]


def ola_feed(M):
    """After the frames 0 .. M - 1 the accumulator's block j (128 samples each, j < 4) holds padded positions [128 (M + j), 128 (M + j + 1)):
    {j: [(frame, block of that frame's 512 samples)] in the order they are added}; block 3 is always empty."""
    out = {}
    for j in range(4):
        out[j] = [(f, M + j - f) for f in range(max(0, M - 3), M) if 0 <= M + j - f < 4]
    return out


def layer0_cells(name, seed=None):
    """Per sequence model (full-band first) the layer-0 cell as hopref.layer_case takes it, from the state dict alone (the engine's
    BatchNorm folding; no BatchNorm: scale 1, shift 0)."""
    from spiking_fullsubnet_amd.engine import fold_batchnorm
    sd = state_dict(name, seed)
    seqs, g = ["fb_model."], 0
    while f"sb_model.sb_models.{g}.sequence_model.layers.0.cell.weight_hh" in sd:
        seqs.append(f"sb_model.sb_models.{g}.")
        g += 1
    out = []
    for s in seqs:
        pre = f"{s}sequence_model.layers.0.cell."
        H = sd[pre + "weight_hh"].shape[1]
        if pre + "batchnorm.weight" in sd:
            a, b = fold_batchnorm(sd[pre + "batchnorm.weight"], sd[pre + "batchnorm.bias"], sd[pre + "batchnorm.running_mean"],
                                  sd[pre + "batchnorm.running_var"])
        else:
            a, b = np.ones(H, F32), np.zeros(H, F32)
        G = sd[pre + "weight_hh"].shape[0] // H
        bias = sd[pre + "bias_ih"]
        out.append(dict(H=H, H_real=H, G=G, kind="x32", W_hh=sd[pre + "weight_hh"], W_ih=sd[pre + "weight_ih"], bias=bias,
                        alpha=np.asarray(a, F32), beta=np.asarray(b, F32)))
    return out
