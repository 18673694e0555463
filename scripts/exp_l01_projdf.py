"""The sub-band epilogue as a third tier of the layers 0 + 1 launch (sfsn_gsn_layer_scan_l01_projdf, Engine.pair16_epilogue) against the
pair launch followed by the epilogue launch, one forward alone on the chip: the timed region's geometry (8, 16), whole-sequence
launches, HIP-event time of the launches in question (stack:sb + projdf).  Per configuration: the two launches, then the one launch
for every number of epilogue workgroups in WGS (SFSN_L01E_WGS), with fp32 spikes and counts-only."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
import refweights as rw
import spiking_fullsubnet_amd as pkg

B, T = int(os.environ.get("B", 64)), int(os.environ.get("T", 1000))
WGS = [int(v) for v in os.environ.get("WGS", "16,24,32,48,64").split(",")]
dev = torch.device("cuda:0")
kw = rw.LIVE_M
sd = rw.live_state_dict(kw, 21)
m = pkg.SpikingFullSubNet(**kw)
m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
m = m.eval().to(dev)
x = m._stft(torch.from_numpy(rw.synth_wave(B, T, seed=0)).to(dev)).contiguous()
eng = m.engine()
eng.rows_per_wg, eng.stack_rows_fb_auto, eng.overlap_chunks, eng.stack_scan, eng.pair16 = (8, 16), 8, 0, False, True
ref = None
for rnd in range(3):
    for wgs in [None] + WGS:
        eng.pair16_epilogue = wgs is not None
        if wgs is not None:
            os.environ["SFSN_L01E_WGS"] = str(wgs)
        for lean in (False, True):
            eng.timers, eng.timer_tags = {}, {"stack:sb", "projdf"}
            eng.launches = {}
            for _ in range(4):
                res = eng.forward_stft(x, pipeline=False, want_layers=not lean, want_counts=lean)
            s = eng.timer_summary()
            eng.timers = None
            assert (eng.launches.get("l01_projdf", 0) == 4) == (wgs is not None) and eng.launches.get("l01_pair", 0) == 4, eng.launches
            same = ""
            if not lean:
                if ref is None:
                    ref = res["enh_mag"].clone()
                same = f"enh_mag identical: {bool(torch.equal(ref, res['enh_mag']))}"
            ms = {k: round(v["mean_ms"], 4) for k, v in s.items()}
            print(f"round {rnd} epilogue={'own launch' if wgs is None else 'in the scan launch, %d workgroups' % wgs} lean={lean}: "
                  f"{round(sum(ms.values()), 4)} ms", ms, same, flush=True)
eng.check_stack_errors()
