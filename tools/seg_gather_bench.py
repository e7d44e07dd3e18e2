"""GPU timing of the gather form of the fused logit losses (ucd_seg_losses_gather through ucd_amd.loss.fused_seg_losses, forward +
gradient to the low-resolution logits) at the per-rank ADE batch of an --output_stride 8 run, 3 x 512^2 <- 64^2, against the only
other way that arithmetic can run - the torch composition on up-sampled logits (F.interpolate of both logit tensors, the unbiased
cross entropy and distillation modules, backward) - and, for scale, the many-class tiled form at 3 x 512^2 <- 32^2
(--output_stride 16).  HIP-event times, warm, the paths alternating, median of N calls; the results are compared at the timed
size.  The numbers of profiles/seg_gather.md.

usage: python tools/seg_gather_bench.py [--calls 20]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from ucd_amd import synth
from ucd_amd.loss import UnbiasedCrossEntropy, UnbiasedKnowledgeDistillationLoss, fused_seg_losses, seg_losses_route

B, H = 3, 512
SPLITS = [(151, 101), (151, 141)]
CE_W, KD_W = 1.0, 10.0


def composition(sem, sem_old, labels, K):
    up = lambda t: F.interpolate(t, size=labels.shape[-2:], mode="bilinear", align_corners=False)
    u = up(sem)
    ce = UnbiasedCrossEntropy(old_cl=K, ignore_index=255, reduction="none")(u, labels).mean()
    kd = UnbiasedKnowledgeDistillationLoss(alpha=1.0)(u, up(sem_old))
    return CE_W * ce + KD_W * kd, ce, kd


def main(calls):
    dev = torch.device("cuda:0")
    for Ctot, K in SPLITS:
        labels = synth.seg_labels(7, B, H, H, range(K, Ctot)).to(dev)
        data = {}
        for h in (64, 32):
            data[h] = (synth.t_normal(11, (B, Ctot, h, h), stream=1, scale=2.0).to(dev).requires_grad_(True),
                       synth.t_normal(11, (B, K, h, h), stream=2, scale=2.0).to(dev))
        assert seg_losses_route(H, H, 64, 64, Ctot, K, True) == "gather" and seg_losses_route(H, H, 32, 32, Ctot, K, True) == "tiled"

        def run(h, fn):
            sem, sem_old = data[h]
            sem.grad = None
            total, ce, kd = fn(sem, sem_old)
            total.backward()
            return ce.detach(), kd.detach(), sem.grad

        paths = {
            "gather, 64^2 cells": (64, lambda s, t: fused_seg_losses(s, t, labels, K, CE_W, KD_W, form="gather")),
            "torch composition, 64^2 cells": (64, lambda s, t: composition(s, t, labels, K)),
            "tiled many-class form, 32^2 cells": (32, lambda s, t: fused_seg_losses(s, t, labels, K, CE_W, KD_W, form="tiled")),
            "gather, 32^2 cells": (32, lambda s, t: fused_seg_losses(s, t, labels, K, CE_W, KD_W, form="gather")),
        }
        for _ in range(3):
            res = {k: run(h, fn) for k, (h, fn) in paths.items()}
        torch.cuda.synchronize()
        rel = lambda x, y: ((x - y).abs().max() / y.abs().max().clamp_min(1e-30)).item()
        a, b = res["gather, 64^2 cells"], res["torch composition, 64^2 cells"]
        print(f"classes {Ctot}/{K}, B {B}, {H}^2: gather vs composition at 64^2 cells: ce {a[0].item():.6f} vs {b[0].item():.6f}, kd "
              f"{a[1].item():.6f} vs {b[1].item():.6f}, gradient max difference / max {rel(a[2], b[2]):.2e}", flush=True)
        times = {k: [] for k in paths}
        for _ in range(calls):                      # alternating: every path sees the same neighbours on the machine
            for key, (h, fn) in paths.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record(); run(h, fn); e.record()
                times[key].append((s, e))
        torch.cuda.synchronize()
        for key, v in times.items():
            t = sorted(s.elapsed_time(e) for s, e in v)
            print(f"    {key}: fwd + gradient median {t[len(t) // 2] * 1e3:.0f} us (min {t[0] * 1e3:.0f}, max {t[-1] * 1e3:.0f})  [{calls} calls]",
                  flush=True)
        del data, labels
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the tool measures on the GPU; there is nothing to report without one"
    main(max(args.calls, 20))
