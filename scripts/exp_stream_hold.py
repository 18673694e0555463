"""Holding clips (step(frames, clips=...), sfsn_stream_hop_held): p50 of one streaming call at B = 16, baseline_m, hop = 1, in ONE mode per
process -- so that two trees (this commit and its parent) can be measured alternately, each with its own library (profiles/stream_hold.md).
bench.py's streaming_measure: host clock from handing the frame over to a synchronised stream, 2,000 calls after 200 of warm-up.

    PYTHONPATH=<tree>:<tree>/tests python scripts/exp_stream_hold.py MODE LABEL [out.jsonl]

MODE: plain (step), held (step with clip 7 of 16 held), graph_plain / graph_held (the same on the per-kernel tier's captured graph),
workaround (export_state of clip 7, step, import_state: what a server did before).  The package and refweights come from PYTHONPATH
(the tree under test); the script itself reads nothing else of its own tree.  Prints one JSON line and appends it to out.jsonl."""
import json
import sys
import time

import numpy as np
import torch

import refweights as rw
import spiking_fullsubnet_amd as pkg

mode, label = sys.argv[1], sys.argv[2]
out = sys.argv[3] if len(sys.argv) > 3 else None
dev = torch.device("cuda:0")
B, HELD, steps, warmup = 16, 7, 2000, 200
kw = rw.LIVE_M
model = pkg.SpikingFullSubNet(**kw)
model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in rw.live_state_dict(kw, 21).items()}, strict=True)
model = model.eval().to(dev)
one_launch = not mode.startswith("graph")
sess = model.streaming(batch=B, hop=1, one_launch=one_launch)
assert (sess._hop is not None) == one_launch
g = torch.Generator(device="cpu").manual_seed(3)
frames = torch.view_as_complex((0.05 * torch.randn((steps + warmup, B, 257, 1, 2), generator=g)).to(dev))
active = [b for b in range(B) if b != HELD]


def call(x):
    if mode.endswith("plain"):
        sess.step(x, copy=False)
    elif mode.endswith("held"):
        sess.step(x, copy=False, clips=active)
    elif mode == "workaround":
        st = sess.export_state(clips=[HELD])
        sess.step(x, copy=False)
        sess.import_state(st, clips=[HELD])
    else:
        raise SystemExit(f"unknown mode {mode}")


lat, enq = [], []
for i in range(steps + warmup):
    x = frames[i]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call(x)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    if i >= warmup:
        lat.append(time.perf_counter() - t0)
        enq.append(t1 - t0)
sess.check_errors()
lat, enq = np.sort(np.asarray(lat)) * 1e6, np.sort(np.asarray(enq)) * 1e6
res = dict(mode=mode, label=label, p50_us=round(float(lat[len(lat) // 2]), 2), p10_us=round(float(lat[len(lat) // 10]), 2),
           p90_us=round(float(lat[int(len(lat) * 0.9)]), 2), min_us=round(float(lat[0]), 2),
           host_enqueue_p50_us=round(float(enq[len(enq) // 2]), 2))
if mode == "graph_held":  # what a held tick of this tier enqueues beside the replay: sections saved, sections put back, output fills
    n = len(sess._state_parts())
    res["row_copies"] = dict(index_select=n, index_copy=n, output_fills=2)
print(json.dumps(res))
if out:
    with open(out, "a") as f:
        f.write(json.dumps(res) + "\n")
