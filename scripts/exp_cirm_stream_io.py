"""Outer samples inside the cIRM-GSN hop (Model.streaming_outer(resample=3, sample_format="s16"), sfsn_fullband_stream_hop_wave_io):
p50 / p99 of one ``step_wave_host`` call at the recipe's model (H = 268, 4 layers), B = 1 and B = 16 -- host clock from handing the
samples over to having the enhanced samples in host memory (``step_wave_host`` returns when the launch's completion words are in; the
three-launch mode ends in a stream synchronise), 2,000 calls after 200 of warm-up (profiles/cirm_stream_io.md).

    PYTHONPATH=<tree>:<tree>/tests python scripts/exp_cirm_stream_io.py MODE B LABEL [out.jsonl]        one mode, one process
    python scripts/exp_cirm_stream_io.py all --parent <parent tree> [--out out.jsonl]                      every mode, one child process each

MODE: default (a plain session: float32 at 16 kHz -- run from the parent tree and from this one, alternately, they are the same
kernels); io_3_s16 / io_3_f32 / io_1_s16 (the new sessions); three (``resample_down3`` + ``step_wave`` + ``resample_up3`` as three
launches, with the pinned copies to and from the device: what a caller with a 48 kHz int16 stream did before, on the device).  The
package and the tests' helpers come from PYTHONPATH (the tree under test).  ``all`` runs the children one at a time, each under
``timeout``, and stops at the first that does not end with status 0.  Prints one JSON line per measurement and appends it to
out.jsonl."""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS, WARMUP = 2000, 200


def driver(argv):
    parent = argv[argv.index("--parent") + 1]
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    here = os.path.dirname(HERE)
    plan = []
    for rep in range(2):  # the pair that must agree: alternately -- the parent's own spread is reported beside it
        for B in (1, 16):
            plan += [(parent, "default", B, f"parent#{rep}"), (here, "default", B, f"new#{rep}")]
    for rep in range(2):  # the three things to compare, alternately
        for B in (1, 16):
            plan += [(here, m, B, f"new#{rep}") for m in ("io_3_s16", "default", "three")]
    for B in (1, 16):
        plan += [(here, m, B, "new") for m in ("io_3_f32", "io_1_s16")]
    for tree, mode, B, label in plan:
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([tree, os.path.join(tree, "tests")]))
        cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), mode, str(B), label] + ([out] if out else [])
        rc = subprocess.run(cmd, env=env).returncode
        if rc != 0:
            raise SystemExit(f"{mode} B={B} ({label}) ended with status {rc}: nothing more is started")


def measure(mode, B, label, out):
    import numpy as np
    import torch

    from test_cirm_gsn import recipe_model

    dev = torch.device("cuda:0")
    model = recipe_model()[0].to(dev)
    rng = np.random.default_rng(3)
    n_calls = STEPS + WARMUP

    if mode == "default":
        sess = model.streaming(batch=B, waveform=True, host_io=True)
        xs = torch.from_numpy((0.05 * rng.standard_normal((n_calls, B, 128))).astype(np.float32))
        call = sess.step_wave_host
    elif mode.startswith("io_"):
        ratio, fmt = int(mode.split("_")[1]), mode.split("_")[2]
        sess = model.streaming_outer(batch=B, host_io=True, resample=ratio, sample_format=fmt)
        x = 0.05 * rng.standard_normal((n_calls, B, 128 * ratio))
        xs = torch.from_numpy(np.rint(x * 32768).astype(np.int16) if fmt == "s16" else x.astype(np.float32))
        call = sess.step_wave_host
    elif mode == "three":
        from spiking_fullsubnet_amd import spectral
        sess = model.streaming(batch=B, waveform=True)
        S = sess.S
        dec, itp = torch.zeros((B, 96), device=dev), torch.zeros((B * S, 32), device=dev)
        pin_in, pin_out = torch.zeros((B, 384), dtype=torch.int16).pin_memory(), torch.zeros((B * S, 384), dtype=torch.int16).pin_memory()
        xs = torch.from_numpy(np.rint(0.05 * rng.standard_normal((n_calls, B, 384)) * 32768).astype(np.int16))

        def call(x16):
            pin_in.copy_(x16)
            y, _ = spectral.resample_down3(pin_in.to(dev, non_blocking=True), dec)
            o = sess.step_wave(y, copy=False)
            z, _ = spectral.resample_up3(o.view(B * S, 128), itp, sample_format="s16")
            pin_out.copy_(z, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()
            return pin_out
    else:
        raise SystemExit(f"unknown mode {mode}")

    lat = []
    for i in range(n_calls):
        x = xs[i]
        t0 = time.perf_counter()
        call(x)
        t1 = time.perf_counter()
        if i >= WARMUP:
            lat.append(t1 - t0)
    sess.check_errors()
    lat = np.sort(np.asarray(lat)) * 1e6
    res = dict(mode=mode, B=B, label=label, p50_us=round(float(lat[len(lat) // 2]), 2), p99_us=round(float(lat[int(len(lat) * 0.99)]), 2),
               p10_us=round(float(lat[len(lat) // 10]), 2), min_us=round(float(lat[0]), 2), calls=STEPS,
               has_outer=hasattr(model, "streaming_outer"))  # (which tree the package came from)
    print(json.dumps(res), flush=True)
    if out:
        with open(out, "a") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "all":
        driver(sys.argv)
    else:
        measure(sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else None)
