#!/usr/bin/env python
"""Generate tests/golden/pit_loss.npz by running the REFERENCE's PITWrapper(PairwiseNegSDR(zero_mean)) (audiozen/pit.py) on the CPU in
fp32, on the inputs of pitref.GOLDEN_CASES, with zero_mean True ("zm1") and False ("zm0"):

    python tests/golden/make_golden_pit.py

The fixture is data only.  The inputs are held as their generator (pitref.make_inputs: the case table's seeds), with a checksum per
case; per case and setting it stores the reference's pair [B,S,S], the chosen indices [B,S], the loss, the autograd gradient of the
loss with respect to the estimate, and the gradient of sum(w * pair) for the seeded w of pitref.cotangent (of both gradients every pitref.GOLDEN_STRIDE-th sample, to keep the file small); `reordered` is stored as the
boolean "equals est gathered by the chosen indices, bit for bit".  Nothing of the reference's source is copied."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))  # tests/

import pitref  # noqa: E402
from make_golden import import_reference  # noqa: E402


def main():
    import_reference()
    import torch
    from audiozen import pit as ref
    out = {}
    for case in pitref.GOLDEN_CASES:
        name = case[0]
        st = pitref.GOLDEN_STRIDE[name]
        e, t = pitref.make_inputs(name)
        w = torch.from_numpy(pitref.cotangent(name))
        out[f"{name}.checksum"] = np.array([np.abs(e).sum(dtype=np.float64), np.abs(t).sum(dtype=np.float64)])
        for zm in (True, False):
            key = f"{name}.zm{int(zm)}"
            wrapper = ref.PITWrapper(ref.PairwiseNegSDR(zero_mean=zm))
            est = torch.from_numpy(e).requires_grad_(True)
            tgt = torch.from_numpy(t)
            pair = wrapper.loss_func(est, tgt)
            _, idx = wrapper.find_best_perm(pair)
            loss, reordered = wrapper(est, tgt)
            loss.backward()
            est2 = torch.from_numpy(e).requires_grad_(True)
            (w * wrapper.loss_func(est2, tgt)).sum().backward()
            same = np.array_equal(reordered.detach().numpy().view(np.uint32),
                                  np.take_along_axis(e, idx.numpy()[:, :, None], axis=1).view(np.uint32))
            out.update({f"{key}.pair": pair.detach().numpy(), f"{key}.perm": idx.numpy(), f"{key}.loss": np.float32(loss.item()),
                        f"{key}.grad": est.grad.numpy()[..., ::st].copy(), f"{key}.grad_pw": est2.grad.numpy()[..., ::st].copy(), f"{key}.reordered_is_gather": np.array(same)})
            print(key, loss.item(), idx.numpy().tolist(), same)
    path = os.path.join(HERE, "pit_loss.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
