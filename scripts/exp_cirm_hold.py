"""Held ticks of a cIRM-GSN session (tick(frames, clips), sfsn_fullband_stream_hop_held): p50 and p99 of one streaming call at B = 16,
the recipe's model (H = 268), hop = 1, in ONE mode per process -- the modes are measured alternately, a process each
(profiles/cirm_hold.md).  bench.py's streaming_measure: host clock from handing the frame over to a synchronised stream, 2,000 calls
after 200 of warm-up; and the host's enqueue time (the call alone, before the synchronise).

    PYTHONPATH=<tree>:<tree>/tests python scripts/exp_cirm_hold.py MODE LABEL [out.jsonl]

MODE: plain (step), held (tick with clip 7 of 16 held), workaround (export_state of clip 7, step, import_state: what a server did
before), graph_plain / graph_held (the same two on the per-kernel tier's captured graph), wave_host_plain / wave_host_held
(step_wave_host / tick_wave_host of a host_io session: host clock from handing the samples over to the last completion word, no stream
synchronisation).  The package and the tests' helpers come from PYTHONPATH (the tree under test).  Prints one JSON line and appends it
to out.jsonl."""
import json
import sys
import time

import numpy as np
import torch

from test_cirm_gsn import recipe_model

mode, label = sys.argv[1], sys.argv[2]
out = sys.argv[3] if len(sys.argv) > 3 else None
dev = torch.device("cuda:0")
B, HELD, steps, warmup = 16, 7, 2000, 200
model = recipe_model()[0].to(dev)
wave = mode.startswith("wave_host")
one_launch = not mode.startswith("graph")
sess = model.streaming(batch=B, hop=1, one_launch=one_launch, waveform=wave, host_io=wave)
assert sess.one_launch is one_launch
g = torch.Generator(device="cpu").manual_seed(3)
if wave:
    feed = 0.05 * torch.randn((steps + warmup, B, 128), generator=g)
else:
    feed = torch.view_as_complex((0.05 * torch.randn((steps + warmup, B, 257, 1, 2), generator=g)).to(dev))
active = [b for b in range(B) if b != HELD]


def call(x):
    if mode in ("plain", "graph_plain"):
        sess.step(x, copy=False)
    elif mode in ("held", "graph_held"):
        sess.tick(x, active, copy=False)
    elif mode == "workaround":
        st = sess.export_state(clips=[HELD])
        sess.step(x, copy=False)
        sess.import_state(st, clips=[HELD])
    elif mode == "wave_host_plain":
        sess.step_wave_host(x)
    elif mode == "wave_host_held":
        sess.tick_wave_host(x, active)
    else:
        raise SystemExit(f"unknown mode {mode}")


lat, enq = [], []
for i in range(steps + warmup):
    x = feed[i]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call(x)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    if i >= warmup:
        lat.append((t1 if wave else time.perf_counter()) - t0)  # (host_io: the call returns with the samples on the host)
        enq.append(t1 - t0)
sess.check_errors()
lat, enq = np.sort(np.asarray(lat)) * 1e6, np.sort(np.asarray(enq)) * 1e6
res = dict(mode=mode, label=label, p50_us=round(float(lat[len(lat) // 2]), 2), p99_us=round(float(lat[int(len(lat) * 0.99)]), 2),
           p10_us=round(float(lat[len(lat) // 10]), 2), min_us=round(float(lat[0]), 2),
           host_enqueue_p50_us=round(float(enq[len(enq) // 2]), 2))
if mode == "graph_held":  # what a held tick of this tier enqueues beside the replay: sections saved, sections put back, output fills
    n = len(sess._state_parts())
    res["row_copies"] = dict(index_select=n, index_copy=n, output_fills=2)
print(json.dumps(res))
if out:
    with open(out, "a") as f:
        f.write(json.dumps(res) + "\n")
