#!/usr/bin/env python
"""Generate tests/golden/reverb_loss.npz by running the REFERENCE's loss as the REVERB trainer composes it
(recipes/reverb/spiking_fullsubnet/trainer.py:34-37: audiozen/loss.py's freq_MAE and mag_MAE plus F.l1_loss) on the CPU in fp32, on the
inputs of lossref.GOLDEN_CASES:

    python tests/golden/make_golden_reverb_loss.py

The fixture is data only: per case the three fp32 loss values, their sum (the trainer's loss) and the autograd gradient of that sum
with respect to the estimate.  The inputs are lossref.make_inputs' (recipe_loss.npz holds them; they are not stored twice).  Nothing of
the reference's source is copied."""
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
    import torch.nn.functional as F
    from audiozen import loss as ref
    torch.manual_seed(0)
    out = {}
    for name, shape, seed, eq in lossref.GOLDEN_CASES:
        e, t = lossref.make_inputs(shape, seed, eq)
        est = torch.from_numpy(e).requires_grad_(True)
        tgt = torch.from_numpy(t)
        freq, mag, time = ref.freq_MAE(est, tgt), ref.mag_MAE(est, tgt), F.l1_loss(est, tgt)
        total = freq + mag + time
        total.backward()
        out.update({f"{name}.grad": est.grad.numpy(),
                    f"{name}.values": np.array([freq.item(), mag.item(), time.item(), total.item()], np.float32)})
        print(name, out[f"{name}.values"])
    path = os.path.join(HERE, "reverb_loss.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
