"""The stagger of the 16-row scan roles' compute waves (SFSN_S3J_STAGGER=<order mask>[,<priority mask>], sfsn_scan3j_dev.h), one forward
alone on the chip: the timed region's geometry (8, 16), B = 64, T = 1000, whole-sequence launches, HIP-event time of the launch in
question, the mean of 4 forwards, three rounds.  Per setting: gsn_scan_fusedx3_kernel (scanx:sb) and gsn_scan_fused3_kernel (scanf:sb)
alone (per-layer launches, layer 0 not merged), then the layers 0 + 1 + epilogue launch (stack:sb, gsn_scan_l01e_kernel); each with fp32
spikes and counts-only.  The candidate list is fixed: order mask in ORDERS, each with priority mask 0, the same slots, the complement.
enh_mag must be the same tensor in every setting.  SETTINGS=a,b;c,d overrides the list (`;` between settings); a library built with
-DSFSN_TIMING_EXPERIMENTS (scripts/build_exp_lib.sh, SFSN_LIB_PATH) also reads SFSN_S3J_LSPLIT / SFSN_S3Y_LSPLIT from the environment
this script is started in.  The last lines give, per setting and launch, the median of the rounds and their spread."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
import refweights as rw
import spiking_fullsubnet_amd as pkg

B, T = int(os.environ.get("B", 64)), int(os.environ.get("T", 1000))
ROUNDS = int(os.environ.get("ROUNDS", 3))
ORDERS = (0, 0b1100, 0b1010, 0b1000, 0b1110)
if os.environ.get("SETTINGS"):
    SETTINGS = [tuple(int(v, 0) for v in (s.split(",") + ["0"])[:2]) for s in os.environ["SETTINGS"].split(";")]
else:
    SETTINGS = []
    for o in ORDERS:
        for p in (0, o, ~o & 15):
            if (o, p) not in SETTINGS:
                SETTINGS.append((o, p))
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
table = {}
for rnd in range(ROUNDS):
    for o, p in SETTINGS:
        os.environ["SFSN_S3J_STAGGER"] = f"{o},{p}"
        for one in (False, True):
            eng.pair16 = eng.pair16_epilogue = eng.merge_layer0 = one
            for lean in (False, True):
                eng.timers, eng.timer_tags = {}, ({"stack:sb"} if one else {"scanx:sb", "scanf:sb"})
                eng.launches = {}
                for _ in range(4):
                    res = eng.forward_stft(x, pipeline=False, want_layers=not lean, want_counts=lean)
                s = eng.timer_summary()
                eng.timers = None
                assert eng.launches.get("l01_projdf", 0) == (4 if one else 0) and eng.launches.get("l0_merged", 0) == (4 if one else 0), eng.launches
                if ref is None:
                    ref = res["enh_mag"].clone()
                same = bool(torch.equal(ref, res["enh_mag"]))
                for k, v in s.items():
                    table.setdefault((o, p, k, lean), []).append(v["mean_ms"])
                print(f"round {rnd} order={o:04b} prio={p:04b} {'l01e' if one else 'per layer'} lean={lean}:",
                      {k: round(v["mean_ms"], 4) for k, v in s.items()}, f"enh_mag identical: {same}", flush=True)
                assert same, "a stagger setting changed the result"
eng.check_stack_errors()
print("\nmedian of the rounds [min .. max], ms per launch")
for (o, p, k, lean), v in sorted(table.items(), key=lambda kv: (kv[0][2], kv[0][3], kv[0][0], kv[0][1])):
    print(f"{k:9s} {'counts only' if lean else 'fp32 spikes'}  order={o:04b} prio={p:04b}  {np.median(v):.4f}  [{min(v):.4f} .. {max(v):.4f}]")
