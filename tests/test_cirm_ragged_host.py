"""Ragged batches of the cIRM-GSN model, host side -- no GPU needed: the export of the length-aware projection + deep filter
(``sfsn_fullband_proj_deepfilter_ragged``), its argument checks -- every one answered before any launch, and the same answer its
sibling gives for the same arguments -- and the host pieces the module's ``forward_ragged`` rests on."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, SIBLING = "sfsn_fullband_proj_deepfilter_ragged", "sfsn_fullband_proj_deepfilter"
_P, _I = ctypes.c_void_p, ctypes.c_int


@pytest.fixture(scope="module")
def L():
    from spiking_fullsubnet_amd import _lib
    _lib.build()
    return _lib.lib()


def test_export_and_prototype(L):
    from spiking_fullsubnet_amd import _lib
    assert NAME in _lib.EXPORTS and hasattr(L, NAME)
    fn, sib = getattr(L, NAME), getattr(L, SIBLING)
    assert fn.restype is _I and list(fn.argtypes) == list(sib.argtypes)[:-1] + [_P, _P]  # the sibling's up to nt | clip_frames, stream
    header = open(os.path.join(ROOT, "include", "sfsn.h")).read()
    decl = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", header)
    assert decl, f"{NAME} is not declared in sfsn.h"
    assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == len(fn.argtypes)
    assert re.search(r"#define\s+SFSN_ABI_VERSION\s+21\b", header) and _lib.ABI_VERSION == 21 and L.sfsn_abi_version() == 21


class _Args:
    """Valid arguments over a dummy host buffer (never dereferenced: every case below is refused first).  Order: stft_ri, spikes_i8,
    H, w_packed, w_dq, bias, act, B, F, T, S, df, proj, enh_ri, enh_mag, t0, nt | clip_frames | stream."""
    KEYS = ("stft_ri", "spikes_i8", "H", "w_packed", "w_dq", "bias", "act", "B", "F", "T", "S", "df", "proj", "enh_ri", "enh_mag", "t0", "nt")

    def __init__(self):
        self.buf = (ctypes.c_char * 4096)()
        p = ctypes.addressof(self.buf)
        self.p = p + (-p) % 16

    def common(self, **over):
        p = self.p
        a = dict(stft_ri=p, spikes_i8=p, H=272, w_packed=p, w_dq=p, bias=p, act=0, B=3, F=257, T=35, S=1, df=3, proj=p, enh_ri=p,
                 enh_mag=p, t0=0, nt=35)
        assert set(over) <= set(a) | {"clip_frames"}
        a.update({k: v for k, v in over.items() if k != "clip_frames"})
        return [a[k] for k in self.KEYS]

    def ragged(self, L, **over):
        return getattr(L, NAME)(*self.common(**over), over.get("clip_frames", self.p), None)

    def plain(self, L, **over):
        return getattr(L, SIBLING)(*self.common(**over), None)


def test_null_pointers_are_refused(L):
    from spiking_fullsubnet_amd import _lib
    a = _Args()
    for name in ("stft_ri", "spikes_i8", "w_packed", "w_dq", "enh_ri", "clip_frames"):
        assert a.ragged(L, **{name: None}) == _lib.SFSN_EINVAL, name
    for name in ("stft_ri", "spikes_i8", "w_packed", "w_dq", "enh_ri"):  # the sibling's own required pointers: the same answer
        assert a.plain(L, **{name: None}) == _lib.SFSN_EINVAL, name


@pytest.mark.parametrize("over", [dict(B=0), dict(B=-1), dict(t0=1, nt=35), dict(t0=-1), dict(nt=0), dict(act=4), dict(act=-1), dict(H=0),
                                  dict(F=0), dict(T=0), dict(S=0), dict(df=0)])
def test_bad_sizes_are_einval_as_for_the_sibling(L, over):
    from spiking_fullsubnet_amd import _lib
    a = _Args()
    assert a.ragged(L, **over) == _lib.SFSN_EINVAL
    assert a.plain(L, **over) == _lib.SFSN_EINVAL


def test_misaligned_pointers_are_einval_as_for_the_sibling(L):
    from spiking_fullsubnet_amd import _lib
    a = _Args()
    for name, off in (("spikes_i8", 8), ("w_packed", 4), ("w_dq", 8), ("bias", 4), ("stft_ri", 4), ("enh_ri", 4), ("proj", 2), ("enh_mag", 1)):
        assert a.ragged(L, **{name: a.p + off}) == _lib.SFSN_EINVAL, name
        assert a.plain(L, **{name: a.p + off}) == _lib.SFSN_EINVAL, name
    assert a.ragged(L, clip_frames=a.p + 2) == _lib.SFSN_EINVAL  # an int32 array


@pytest.mark.parametrize("over", [dict(H=321), dict(H=400), dict(S=5), dict(df=17), dict(F=1026)])
def test_unsupported_sizes_are_the_siblings(L, over):
    from spiking_fullsubnet_amd import _lib
    a = _Args()
    assert a.ragged(L, **over) == _lib.SFSN_EUNSUPPORTED
    assert a.plain(L, **over) == _lib.SFSN_EUNSUPPORTED
    assert a.ragged(L, clip_frames=None, **over) == _lib.SFSN_EINVAL  # a NULL stays a NULL


def test_nullable_pointers_stay_nullable(L):
    """bias, proj and enh_mag may be NULL: with them NULL an otherwise bad call is still refused for its own reason."""
    from spiking_fullsubnet_amd import _lib
    a = _Args()
    assert a.ragged(L, bias=None, proj=None, enh_mag=None, df=17) == _lib.SFSN_EUNSUPPORTED
    assert a.ragged(L, bias=None, proj=None, enh_mag=None, act=9) == _lib.SFSN_EINVAL


# ---- the host pieces of forward_ragged ------------------------------------------------------------------------------------------
def test_length_checks_name_the_clip():
    from spiking_fullsubnet_amd import ragged
    assert ragged.check_frames([35, 1, 16], 3, 35) == [35, 1, 16]
    for fr, msg in (([35, 0, 3], r"frames\[1\] = 0: clip 1"), ([35, 3, 36], r"frames\[2\] = 36: clip 2"), ([35, 3], "one frame count per clip")):
        with pytest.raises(ValueError, match=msg):
            ragged.check_frames(fr, 3, 35)
    assert ragged.check_lengths([1, 127, 4480], 3, 4480, 128) == [1, 127, 4480]  # a single frame is fine: no Gaussian norm here
    for lens, msg in (([4480, 0, 3], r"lengths\[1\] = 0: clip 1"), ([4480, 3, 4481], r"lengths\[2\] = 4481: clip 2"),
                      ([4480, 3], "one length per clip")):
        with pytest.raises(ValueError, match=msg):
            ragged.check_lengths(lens, 3, 4480, 128)
    with pytest.raises(ValueError, match="not an integer"):
        ragged.check_frames([35, 2.5, 3], 3, 35)


def test_clip_summary_with_one_row_per_clip():
    """The full-band stack has one row per clip: ``clip(b)`` is the summary the clip-alone forward returns, shape (T_b, 1, H)."""
    from spiking_fullsubnet_amd import metric, ragged
    from spiking_fullsubnet_amd.engine import SpikeSummary
    frames, H, T = [35, 1, 16], 20, 35
    counts = torch.tensor([70, 3, 40])
    s = ragged.ClipSpikeSummary(counts, (T, len(frames), H), frames)
    assert s.rows_per_clip == 1 and s.numel() == sum(frames) * H and int(s.count) == 113
    for b, Tb in enumerate(frames):
        c = s.clip(b)
        assert type(c) is SpikeSummary and tuple(c.shape) == (Tb, 1, H) and int(c.count) == int(counts[b])
    x = torch.zeros(T, 3, 257)
    proj = torch.empty((T, 3, 1542), device="meta")
    fb, sb = ragged.clip_layers([x, s, s, proj], [], 1, frames)
    assert sb == [] and tuple(fb[0].shape) == (1, 1, 257) and tuple(fb[-1].shape) == (1, 1, 1542) and tuple(fb[1].shape) == (1, 1, H)
    alone = [torch.zeros(1, 1, 257), SpikeSummary(counts[1], (1, 1, H)), SpikeSummary(counts[1], (1, 1, H)), torch.empty((1, 1, 1542), device="meta")]
    assert metric.compute_synops(fb, [], shared_weights=True) == metric.compute_synops(alone, [], shared_weights=True)


def test_module_has_the_ragged_entry_points_and_refuses_without_a_device():
    """The signatures, and the refusals that need no device: an LSTM model, a CPU tensor."""
    import inspect
    from spiking_fullsubnet_amd.fullband_engine import FullbandEngine
    from spiking_fullsubnet_amd.modeling_cirm_gsn import Model
    assert "frames" in inspect.signature(Model.forward_stft).parameters
    assert list(inspect.signature(Model.forward_ragged).parameters) == ["self", "waves", "lengths"]
    sig = inspect.signature(FullbandEngine.forward_stft).parameters
    assert sig["frames"].default is None and sig["frames_dev"].default is None
    assert inspect.signature(FullbandEngine._launch_frames).parameters["frames_dev"].default is None
    kw = dict(n_fft=512, hop_length=128, win_length=512, fdrc=0.5, input_size=257, hidden_size=20, num_layers=2, proj_size=257,
              output_activate_function=False, df_order=3, shared_weights=True, num_spks=1)
    lstm = Model(sequence_model="LSTM", **kw).eval()
    with pytest.raises(NotImplementedError, match="LSTM"):
        lstm.forward_ragged(torch.zeros(2, 512), [512, 100])
    gsn = Model(sequence_model="GSN", **kw).eval()
    with pytest.raises(RuntimeError, match="HIP device"):
        gsn.forward_ragged(torch.zeros(2, 512), [512, 100])
    assert gsn._gaussian_norm() is False  # (the mixin's PathSpec question is not asked of this model)
    assert gsn._forward_kwargs() == dict(want_layers=False, want_counts=False)
