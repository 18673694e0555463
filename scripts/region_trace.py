#!/usr/bin/env python3
"""What bench.py's timed region looks like in a `rocprofv3 --kernel-trace --output-format csv` run of the default command line.

    python scripts/region_trace.py <..._kernel_trace.csv> [--forwards 60]

The region is taken as every dispatch from the start of the `--forwards`-last `gsn_stack_fb_kernel` on (one per forward).  Printed, as
one JSON object: the region's length and dispatch count, the queues and streams seen, kernels running at once and the resident scan
workgroups (summed grids of the running `gsn_scan*` / `gsn_stack*` kernels, one workgroup per CU, as a share of 256 CUs) over the
inner 80 % of the region, time-weighted; the chain of one forward (a stream's dispatches up to and including a `projdf_kernel` or,
where the epilogue runs inside the scan launch, a `gsn_scan_l01e_kernel`, first
start to last end, and the sum of its spans), median over the forwards that lie inside the region; the median span per kernel.
Reads the file only."""
import argparse
import csv
import json
import re
import statistics
import sys


def short(name):
    name = re.sub(r"^void ", "", name)
    return re.sub(r"\(.*$", "", name)


def weighted(points, q):
    """Quantile q of a step function given as [(value, duration)]."""
    points = sorted(points)
    total = sum(d for _, d in points)
    acc = 0
    for v, d in points:
        acc += d
        if acc >= q * total:
            return v
    return points[-1][0]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("trace")
    ap.add_argument("--forwards", type=int, default=60)
    a = ap.parse_args()
    rows = []
    with open(a.trace, newline="") as f:
        for r in csv.DictReader(f):
            wg = max(int(r["Workgroup_Size_X"]) * int(r["Workgroup_Size_Y"]) * int(r["Workgroup_Size_Z"]), 1)
            grid = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])
            rows.append(dict(name=short(r["Kernel_Name"]), q=r["Queue_Id"], s=r["Stream_Id"], t0=int(r["Start_Timestamp"]), t1=int(r["End_Timestamp"]),
                             wgs=grid // wg))
    rows.sort(key=lambda r: r["t0"])
    fb = [r for r in rows if r["name"].startswith("gsn_stack_fb_kernel")]
    if len(fb) < a.forwards:
        sys.exit(f"only {len(fb)} gsn_stack_fb_kernel dispatches")
    # (the forward's first two kernels run before its gsn_stack_fb_kernel: the region opens with the earliest of that stream's chain)
    start = fb[-a.forwards]["t0"]
    reg = [r for r in rows if r["t0"] >= start]
    end = max(r["t1"] for r in reg)
    lo, hi = start + (end - start) // 10, end - (end - start) // 10
    ev = []
    for r in reg:
        scan = r["wgs"] if re.match(r"gsn_(scan|stack)", r["name"]) else 0
        ev += [(r["t0"], 1, scan), (r["t1"], -1, -scan)]
    ev.sort()
    n = res = 0
    at_once, resident, prev = [], [], None
    for t, dn, dr in ev:
        if prev is not None and t > prev:
            a0, a1 = max(prev, lo), min(t, hi)
            if a1 > a0:
                at_once.append((n, a1 - a0))
                resident.append((res, a1 - a0))
        n, res, prev = n + dn, res + dr, t
    tot = sum(d for _, d in at_once)
    out = dict(region_ms=(end - start) / 1e6, ms_per_forward=(end - start) / 1e6 / a.forwards, dispatches=len(reg),
               queues=sorted({r["q"] for r in reg}), streams=len({r["s"] for r in reg}),
               kernels_at_once=dict(median=weighted(at_once, 0.5), p10=weighted(at_once, 0.1), p90=weighted(at_once, 0.9), max=max(v for v, _ in at_once),
                                    mean=round(sum(v * d for v, d in at_once) / tot, 3),
                                    share={str(k): round(sum(d for v, d in at_once if v == k) / tot, 3) for k in sorted({v for v, _ in at_once})}),
               resident_scan_wgs=dict(mean=round(sum(v * d for v, d in resident) / tot, 1), median=weighted(resident, 0.5), p90=weighted(resident, 0.9),
                                      max=max(v for v, _ in resident), mean_share_of_256=round(sum(v * d for v, d in resident) / tot / 256, 3)))
    chains, sums = [], []
    for s in {r["s"] for r in reg}:
        cur = []
        for r in (r for r in reg if r["s"] == s):
            cur.append(r)
            if r["name"].startswith(("projdf_kernel", "gsn_scan_l01e_kernel")):  # (a forward's last launch, either way)
                if any(x["name"].startswith("gsn_stack_fb_kernel") for x in cur) and cur[0]["name"].startswith("features_kernel"):
                    chains.append((max(x["t1"] for x in cur) - cur[0]["t0"]) / 1e3)
                    sums.append(sum(x["t1"] - x["t0"] for x in cur) / 1e3)
                cur = []
    out["chain_us"] = dict(forwards=len(chains), median=round(statistics.median(chains), 1) if chains else None,
                           median_sum_of_spans=round(statistics.median(sums), 1) if sums else None)
    spans = {}
    for r in reg:
        spans.setdefault(r["name"], []).append((r["t1"] - r["t0"]) / 1e3)
    out["median_span_us"] = {k: dict(n=len(v), median=round(statistics.median(v), 1)) for k, v in sorted(spans.items(), key=lambda kv: -sum(kv[1]))[:12]}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
