#!/usr/bin/env python
"""Generate tests/golden/sisdr_metric.npz by running the REFERENCE's audiozen.metric.SISDR on the CPU in fp32 on every clip of
pitraggedref.CASES alone (est[b, :, :L_b] against ref[b, :, :L_b], rows as the generator made them: the identity matching):

    python tests/golden/make_golden_sisdr.py

The fixture is data only.  The inputs are held as their generator (pitraggedref.make_inputs: the case table's seeds) with a checksum
per case; per clip it stores the reference's value of every row (`<case>.rows` [B, S]: reduce_mean=True on one row at a time, which is
the row's value) and of the clip (`<case>.mean` [B]: reduce_mean=True on [S, L_b]), plus the torch version.  Nothing of the reference's
source is copied."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))  # tests/

import pitraggedref as prr  # noqa: E402
from make_golden import import_reference  # noqa: E402


def main():
    metric = import_reference()[3]
    import torch
    sisdr = metric.SISDR()
    out = {"torch_version": np.array(torch.__version__)}
    for case in prr.CASES:
        name, B, S = case[0], case[1], case[2]
        e, t = prr.make_inputs(name)
        out[f"{name}.checksum"] = np.array([np.abs(e).sum(dtype=np.float64), np.abs(t).sum(dtype=np.float64)])
        rows, mean = np.zeros((B, S), np.float32), np.zeros(B, np.float32)
        for b, n in enumerate(prr.lengths(name)):
            eb, tb = torch.from_numpy(e[b, :, :n].copy()), torch.from_numpy(t[b, :, :n].copy())
            for j in range(S):
                rows[b, j] = sisdr(eb[j], tb[j])["si_sdr"]
            mean[b] = sisdr(eb, tb)["si_sdr"]
        out[f"{name}.rows"], out[f"{name}.mean"] = rows, mean
        print(name, mean.tolist())
    path = os.path.join(HERE, "sisdr_metric.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
