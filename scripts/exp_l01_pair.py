"""Layers 0 + 1 of the sub-band stack in one 16-row launch (sfsn_gsn_layer_scan_l01, Engine.pair16) against the two per-layer launches,
one forward alone on the chip: the timed region's geometry (8, 16), whole-sequence launches, HIP-event time of the sub-band scans.
Per configuration: the per-layer launches (scanx:sb + scanf:sb), then the pair launch (stack:sb) for every hand-off lag in LAGS."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
import refweights as rw
import spiking_fullsubnet_amd as pkg

B, T = int(os.environ.get("B", 64)), int(os.environ.get("T", 1000))
LAGS = [int(v) for v in os.environ.get("LAGS", "0,2,4,8,16,32").split(",")]
dev = torch.device("cuda:0")
kw = rw.LIVE_M
sd = rw.live_state_dict(kw, 21)
m = pkg.SpikingFullSubNet(**kw)
m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
m = m.eval().to(dev)
x = m._stft(torch.from_numpy(rw.synth_wave(B, T, seed=0)).to(dev)).contiguous()
eng = m.engine()
eng.rows_per_wg, eng.stack_rows_fb_auto, eng.overlap_chunks, eng.stack_scan = (8, 16), 8, 0, False
ref = None
for rnd in range(3):
    for lag in [None] + LAGS:
        eng.pair16 = lag is not None
        if lag is not None:
            eng.stack_lag = lag
        for lean in (False, True):
            eng.timers, eng.timer_tags = {}, {"scanf:sb", "scanx:sb", "scan:sb", "stack:sb"}
            for _ in range(4):
                res = eng.forward_stft(x, pipeline=False, want_layers=not lean, want_counts=lean)
            s = eng.timer_summary()
            eng.timers = None
            same = ""
            if not lean:
                if ref is None:
                    ref = res["enh_mag"].clone()
                same = f"enh_mag identical: {bool(torch.equal(ref, res['enh_mag']))}"
            ms = {k: round(v["mean_ms"], 4) for k, v in s.items()}
            print(f"round {rnd} pair={'off' if lag is None else 'lag %d' % lag} lean={lean}: sub-band scans {round(sum(ms.values()), 4)} ms", ms, same, flush=True)
eng.check_stack_errors()
