"""GPU timing of ucd_seg_views (csrc/seg_views.hip) with the twelve default views - six scales (0.5 ... 1.75), each plain and mirrored -
at VOC 513^2, 21 classes and ADE 512^2, 151 classes, --output_stride 16, against the torch composition it replaces on the same GPU:
per view F.interpolate + flip + softmax, the rule over the views, argmax, bincount.  HIP-event times, warm, the paths alternating in
one process (5 rounds), median of the rounds; the predictions are compared at the timed size first.  The numbers of
profiles/seg_views.md.

usage: python tools/seg_views_bench.py [--out results.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ucd_amd import hip

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
SCALES = (1.0, 0.5, 0.75, 1.25, 1.5, 1.75)


def compose(sems, flips, labels, n, rule):
    H, W = labels.shape[-2:]
    score = None
    for sem, flip in zip(sems, flips):
        u = F.interpolate(sem, size=(H, W), mode="bilinear", align_corners=False)
        u = u.flip(-1) if flip else u
        if rule == "voting":
            p = torch.zeros_like(u).scatter_(1, u.argmax(1, keepdim=True), 1.0)
        else:
            p = u.softmax(1)
        score = p if score is None else (torch.maximum(score, p) if rule == "max" else score + p)
    pred = score.argmax(1)
    ok = (labels >= 0) & (labels < n)
    return pred, torch.bincount(n * labels[ok] + pred[ok], minlength=n * n).reshape(n, n)


def timeit(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3      # us


out = {}
for name, (B, H, Ctot) in {"voc_4x513_21": (4, 513, 21), "ade_2x512_151": (2, 512, 151)}.items():
    g = torch.Generator(dev).manual_seed(5)
    views = [((int(H * s + 0.5) + 15) // 16, f) for s in SCALES for f in (False, True)]
    sems = [torch.randn(B, Ctot, h, h, device=dev, generator=g) * 3 for h, _ in views]
    flips = [f for _, f in views]
    labels = torch.randint(0, Ctot, (B, H, H), device=dev, generator=g)
    rows = [s.permute(0, 2, 3, 1).reshape(-1, Ctot).contiguous() for s in sems]
    shapes = [(h, h) for h, _ in views]
    hist = torch.zeros(Ctot, Ctot, dtype=torch.int64, device=dev)
    pred = torch.empty(B, H, H, dtype=torch.int64, device=dev)
    plan = hip.seg_views_plan(H, H, [(h, h, f) for h, f in views], Ctot, Ctot)
    res = {"plan": plan}
    for rule in ("mean", "max", "voting"):
        kernel = lambda: hip.seg_views(rows, shapes, flips, labels, Ctot, Ctot, rule, hist, pred)
        torch_fn = lambda: compose(sems, flips, labels, Ctot, rule)
        hist.zero_(); kernel(); ref_pred, ref_hist = torch_fn(); torch.cuda.synchronize()
        agree = float((pred == ref_pred).float().mean())
        hist_diff = int((hist - ref_hist).abs().sum())
        for fn in (kernel, torch_fn):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        rounds = {"kernel": [], "torch": []}
        for r in range(5):                          # alternate the two in one process
            rounds["kernel"].append(timeit(kernel, 10))
            rounds["torch"].append(timeit(torch_fn, 3))
        res[rule] = {k: {"median_us": float(np.median(v)), "min_us": float(min(v)), "max_us": float(max(v))} for k, v in rounds.items()}
        res[rule].update(pred_agreement=agree, hist_abs_diff=hist_diff)
    out[name] = res
    print(name, json.dumps(res), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
