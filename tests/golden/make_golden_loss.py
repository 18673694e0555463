#!/usr/bin/env python
"""Generate tests/golden/recipe_loss.npz by running the REFERENCE's loss functions (audiozen/loss.py: freq_MAE, mag_MAE, SISNRLoss)
on the CPU in fp32, on the inputs of lossref.GOLDEN_CASES:

    python tests/golden/make_golden_loss.py

The fixture is data only: per case the inputs, the three fp32 loss values, the trainer's total without its constant
(freq + mag - 0.001 sisnr, lossref.RECIPE_WEIGHTS) and the autograd gradient of that total with respect to the estimate.  Nothing of the
reference's source is copied."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))  # tests/

import lossref  # noqa: E402
from make_golden import import_reference  # noqa: E402


def main():
    import_reference()
    import torch
    from audiozen import loss as ref
    torch.manual_seed(0)
    out = {}
    c_freq, c_mag, c_sdr = lossref.RECIPE_WEIGHTS
    for name, shape, seed, eq in lossref.GOLDEN_CASES:
        e, t = lossref.make_inputs(shape, seed, eq)
        est = torch.from_numpy(e).requires_grad_(True)
        tgt = torch.from_numpy(t)
        freq, mag, sisnr = ref.freq_MAE(est, tgt), ref.mag_MAE(est, tgt), ref.SISNRLoss()(est, tgt)
        total = (c_freq * freq + c_mag * mag) + c_sdr * sisnr
        total.backward()
        out.update({f"{name}.est": e, f"{name}.tgt": t, f"{name}.grad": est.grad.numpy(),
                    f"{name}.values": np.array([freq.item(), mag.item(), sisnr.item(), total.item()], np.float32)})
        print(name, out[f"{name}.values"])
    path = os.path.join(HERE, "recipe_loss.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
