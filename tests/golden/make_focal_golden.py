"""Regenerates tests/golden/focal_losses.npz by driving the REFERENCE's own ``FocalLoss`` (utils/loss.py:13-28, loaded by file
path as make_kd_golden.py loads that file: it needs torch only).  Only arrays are stored; the inputs are the seeded ones of
make_kd_golden.unit_inputs, which the tests rebuild.

    python tests/golden/make_focal_golden.py          # writes focal_losses.npz next to this script (seconds)

For every shape of make_kd_golden.UNIT_SHAPES and every (gamma, alpha) of FOCAL: float64 low-resolution logits,
``F.interpolate(bilinear, align_corners=False)`` to the label size, ``FocalLoss(alpha, gamma, size_average=True,
ignore_index=255)``; stored are the loss and its gradient with respect to the LOW-resolution student logits, as float32 and
through make_goldens.compact() (the largest shape is stored as sums, row sums and samples).
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

FOCAL = ((2.0, 1.0), (0.5, 1.0), (1.0, 0.25), (3.5, 0.25))          # gamma, alpha


def focal_key(shape, gamma, alpha):
    return "x".join(str(v) for v in shape) + f"|{gamma:g}|{alpha:g}"


def unit(ref_loss):
    from make_goldens import compact
    from make_kd_golden import UNIT_SHAPES, unit_inputs
    out = {}
    for shape in UNIT_SHAPES:
        B, Ctot, K, h, H = shape
        sem, _, labels = unit_inputs(shape)
        for gamma, alpha in FOCAL:
            s = sem.double().requires_grad_(True)
            u = F.interpolate(s, size=(H, H), mode="bilinear", align_corners=False)
            loss = ref_loss.FocalLoss(alpha=alpha, gamma=gamma, size_average=True, ignore_index=255)(u, labels.clone())
            loss.backward()
            key = focal_key(shape, gamma, alpha)
            out[key + "|loss"] = np.array([loss.item()])
            out.update(compact(key + "|grad", s.grad.numpy().astype(np.float32)))
    return out


def main():
    import make_goldens as MG
    torch.set_num_threads(8)
    path = os.path.join(HERE, "focal_losses.npz")
    np.savez_compressed(path, **unit(MG.ref_loss))
    print("focal_losses.npz: %.1f KiB (kd_losses.npz: %.1f KiB)" % (os.path.getsize(path) / 1024,
                                                                   os.path.getsize(os.path.join(HERE, "kd_losses.npz")) / 1024))


if __name__ == "__main__":
    sys.exit(main())
