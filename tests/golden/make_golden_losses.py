#!/usr/bin/env python
"""Generate tests/golden/losses.npz by running the REFERENCE loss functions.

Like make_golden.py this runs only where the reference checkout exists.  It
imports mpjpe_error_3d (jl2), transition_error_3d (tl2), mae_error_3d (cl1) and
mse_error_3d (cl2) from the reference's engine/utils/loss.py and evaluates
them on the CPU in fp64, with and without joint weights, recording inputs,
weights, values and the reference's own autograd gradients.

Inputs and weights are drawn in fp32 and widened, so the fp32 kernels under
test see exactly the numbers the reference saw.

Cases (B, T, V):
  small     2,  3,  5   fewer points than one workgroup; positive weights
  twoframe  2,  2, 22   tl2 with a single difference; positive weights
  minmax    3, 25, 22   min-max-normalised weights: one exactly 0, one exactly 1
  positive  3, 25, 22   strictly positive weights

Keys: <case>/pred, <case>/targ (fp32), <case>/w (fp32), and for variant
``u`` (no weights) and ``w`` (weights): <case>/<variant>/<term>/value,
<case>/<variant>/<term>/grad (fp64).  The reference's cl2 gradient is NaN
wherever w_j * d_c == 0, so cl2 gradients are stored only where every weight
is positive (not for minmax/w).  Every stored array is asserted finite.

Usage:  python tests/golden/make_golden_losses.py
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))

sys.dont_write_bytecode = True
sys.path.insert(0, REF)

from engine.utils.loss import mae_error_3d, mpjpe_error_3d, mse_error_3d, transition_error_3d  # noqa: E402  (reference)

TERMS = {"jl2": mpjpe_error_3d, "tl2": transition_error_3d, "cl1": mae_error_3d, "cl2": mse_error_3d}
CASES = {"small": (2, 3, 5, "positive"), "twoframe": (2, 2, 22, "positive"), "minmax": (3, 25, 22, "minmax"),
         "positive": (3, 25, 22, "positive")}


def main():
    gen = torch.Generator().manual_seed(20240611)
    out = {}
    for name, (B, T, V, kind) in CASES.items():
        pred = torch.randn(B, T, V * 3, generator=gen, dtype=torch.float32)
        targ = pred + 0.5 * torch.randn(B, T, V * 3, generator=gen, dtype=torch.float32)
        raw = torch.empty(V, dtype=torch.float32).uniform_(0.1, 1.5, generator=gen)
        w = (raw - raw.min()) / (raw.max() - raw.min()) if kind == "minmax" else raw
        if kind == "minmax":
            assert float(w.min()) == 0.0 and float(w.max()) == 1.0
        else:
            assert float(w.min()) > 0.0
        out[f"{name}/pred"], out[f"{name}/targ"], out[f"{name}/w"] = pred.numpy(), targ.numpy(), w.numpy()
        w64 = w.numpy().astype(np.float64)
        for variant, weights in (("u", None), ("w", w64)):
            for term, fn in TERMS.items():
                p = pred.double().requires_grad_(True)
                value = fn(p, targ.double(), weights)
                assert value.dtype == torch.float64
                value.backward()
                out[f"{name}/{variant}/{term}/value"] = value.detach().numpy()
                if term == "cl2" and weights is not None and kind == "minmax":
                    assert bool(torch.isnan(p.grad).any())  # the reference's NaN at w_j * d_c == 0
                    continue
                out[f"{name}/{variant}/{term}/grad"] = p.grad.numpy()
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    path = os.path.join(HERE, "losses.npz")
    np.savez(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
