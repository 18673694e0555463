"""Launch traces of Engine.forward_stft: every C-ABI call of one forward as [entry point, its plain int / float arguments in
order, ordinal of its stream handle by first appearance].  What a host-side refactor of the engine must leave as it is.

    python scripts/record_forward_traces.py            # on the GPU: writes tests/golden/forward_traces.json

Every case runs on a model of its own (the engine remembers which launches the library refused, so a second forward of one engine
asks less than the first) and after a device synchronisation (the stack rule asks whether another forward is in flight).  Each
case is recorded twice; one that differs between the two is left out and named on stderr.  tests/test_forward_trace.py replays
the cases against the fixture.
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(ROOT, "tests", "golden", "forward_traces.json")
DEV = "cuda:0"
B = 2

# model ("live": refweights.LIVE_TINY, seed 11 | "frozen": refweights.FROZEN_TINY, seed 31), T, engine attributes, forward_stft arguments
CASES = {
    "live_T288_overlapped": dict(model="live", T=288),
    "live_T40_sequential": dict(model="live", T=40),
    "live_T40_seq_chunk16": dict(model="live", T=40, attrs=dict(seq_chunk=16)),
    "live_T40_pipeline_chunk16": dict(model="live", T=40, attrs=dict(pipeline_chunk=16), kwargs=dict(pipeline=True)),
    "live_T40_counts_only": dict(model="live", T=40, kwargs=dict(want_layers=False, want_counts=True)),
    "live_T40_ragged_40_23": dict(model="live", T=40, kwargs=dict(frames=[40, 23])),
    "frozen_T40": dict(model="frozen", T=40),
    "frozen_T40_norm_stats": dict(model="frozen", T=40, given_stats=True),
}


class LibTrace:
    """Proxy around the ctypes library of an engine: forwards every call and notes it."""

    def __init__(self, lib):
        self._lib, self.calls, self._streams = lib, [], {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            plain = [a for a in args if type(a) in (int, float)]
            assert all(abs(a) < 2 ** 40 for a in plain), (name, plain)  # (an address among them would not be reproducible)
            stream = None
            if fn.argtypes and fn.argtypes[-1] is ctypes.c_void_p and (args[-1] is None or isinstance(args[-1], ctypes.c_void_p)):
                key = None if args[-1] is None else args[-1].value
                stream = self._streams.setdefault(key, len(self._streams))
            self.calls.append([name, plain, stream])
            return fn(*args)
        return call


def _model(which):
    import numpy as np
    import torch

    import refweights as rw
    import spiking_fullsubnet_amd as pkg
    if which == "live":
        m, sd = pkg.SpikingFullSubNet(**rw.LIVE_TINY), rw.live_state_dict(rw.LIVE_TINY, 11)
    else:
        m, sd = pkg.Separator(**rw.FROZEN_TINY), rw.frozen_state_dict(rw.FROZEN_TINY, 31)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.eval().to(DEV)


def record(name):
    """The trace of one forward of the case `name`, on a fresh model."""
    import torch
    case = CASES[name]
    gen = torch.Generator().manual_seed(7)
    stft = (0.1 * torch.randn((B, 257, case["T"], 2), generator=gen)).to(DEV)
    stft = torch.view_as_complex(stft)
    kwargs = dict(case.get("kwargs", {}))
    if case.get("given_stats"):
        kwargs["norm_stats"] = _model(case["model"]).engine().forward_stft(stft, want_layers=False, return_norm_stats=True)["norm_stats"]
    eng = _model(case["model"]).engine()
    for k, v in case.get("attrs", {}).items():
        assert hasattr(eng, k), k
        setattr(eng, k, v)
    eng.lib = trace = LibTrace(eng.lib)
    torch.cuda.synchronize()
    eng.forward_stft(stft, **kwargs)
    torch.cuda.synchronize()
    eng.check_stack_errors()
    return trace.calls


def main():
    out = {}
    for name in CASES:
        a, b = record(name), record(name)
        if a != b:
            print(f"{name}: not deterministic, left out", file=sys.stderr)
            continue
        out[name] = a
        print(f"{name}: {len(a)} calls on {len({c[2] for c in a if c[2] is not None})} stream(s)")
    with open(sys.argv[1] if len(sys.argv) > 1 else FIXTURE, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
