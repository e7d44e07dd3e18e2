"""GPU timing of ucd_seg_render (csrc/seg_render.hip) with all five outputs at the two benchmark batches - VOC 24 x 513^2 <- 33^2, 21
classes; ADE 24 x 512^2 <- 32^2, 150 classes - against the torch composition it replaces on the same GPU: F.interpolate + argmax +
palette indexing + de-normalise + .to(uint8), plus the interpolate of the attention map.  Also ucd_attn_energy on a [24, 2048, h, h]
bf16 body map.  HIP-event times, warm, the paths alternating in one process (7 rounds of 50 / 10 / 50 calls), median of the rounds;
the results are compared at the timed size first.  The numbers of profiles/seg_render.md.

usage: python tools/seg_render_bench.py [--out results.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ucd_amd import hip, visual

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
MEAN = torch.tensor(visual.MEAN, device=dev).view(1, 3, 1, 1)
STD = torch.tensor(visual.STD, device=dev).view(1, 3, 1, 1)


def compose(sem, labels, images, att_low, cm):
    H, W = labels.shape[-2:]
    up = F.interpolate(sem, size=(H, W), mode="bilinear", align_corners=False)
    pred = up.argmax(dim=1)
    pred_rgb = cm[pred]
    label_rgb = cm[labels & 255]
    img = ((images * STD + MEAN) * 255).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    att = F.interpolate(att_low.unsqueeze(1), size=(H, W), mode="bilinear", align_corners=False).squeeze(1)
    return pred.to(torch.uint8), pred_rgb, label_rgb, img, att


def timeit(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3      # us


out = {}
for name, (B, H, h, Ctot) in {"voc_24x513_33_21": (24, 513, 33, 21), "ade_24x512_32_150": (24, 512, 32, 150)}.items():
    g = torch.Generator(dev).manual_seed(5)
    sem = (torch.randn(B, Ctot, h, h, device=dev, generator=g) * 3).contiguous(memory_format=torch.channels_last)
    labels = torch.randint(0, Ctot, (B, H, H), device=dev, generator=g)
    images = torch.randn(B, 3, H, H, device=dev, generator=g).contiguous(memory_format=torch.channels_last)
    body = torch.randn(B, 2048, h, h, device=dev, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    att_low = visual.attn_energy(body)
    cm = torch.from_numpy(visual.color_map()).to(dev)
    s = sem.permute(0, 2, 3, 1).reshape(B * h * h, Ctot).float().contiguous()
    bufs = [torch.empty(B, H, H, dtype=torch.uint8, device=dev)] + [torch.empty(B, H, H, 3, dtype=torch.uint8, device=dev) for _ in range(3)] + \
        [torch.empty(B, H, H, device=dev)]
    lib = hip.load()

    def kernel():
        hip._check(lib.ucd_seg_render(hip.ptr(s), Ctot, hip.ptr(labels), hip.ptr(images), *images.stride(), *visual.MEAN, *visual.STD,
                                      hip.ptr(cm), hip.ptr(att_low), h, h, B, H, H, h, h, Ctot, *[hip.ptr(b) for b in bufs], hip.stream()),
                   "ucd_seg_render")

    def energy():
        visual.attn_energy(body)

    def torch_fn():
        compose(sem, labels, images, att_low, cm)

    # same results first
    kernel(); ref = compose(sem, labels, images, att_low, cm); torch.cuda.synchronize()
    agree = float((bufs[0] == ref[0]).float().mean())
    rgb_ok = bool((bufs[1] == cm[bufs[0].long()]).all()) and bool((bufs[2] == ref[2]).all())
    img_diff = int((bufs[3].int() - ref[3].int()).abs().max())
    att_diff = float((bufs[4] - ref[4]).abs().max())
    for fn in (kernel, torch_fn, energy):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    rounds = {"kernel": [], "torch": [], "energy": []}
    for r in range(7):                          # alternate the two in one process
        rounds["kernel"].append(timeit(kernel, 50))
        rounds["torch"].append(timeit(torch_fn, 10))
        rounds["energy"].append(timeit(energy, 50))
    nbytes = B * H * H * (8 + 12 + 1 + 9 + 4) + B * h * h * Ctot * 4
    res = {k: {"median_us": float(np.median(v)), "min_us": float(min(v)), "max_us": float(max(v))} for k, v in rounds.items()}
    res.update(pred_agreement=agree, rgb_exact=rgb_ok, image_max_diff=img_diff, att_max_diff=att_diff, algorithmic_bytes=nbytes,
               kernel_GBps=nbytes / res["kernel"]["median_us"] / 1e3)
    out[name] = res
    print(name, json.dumps(res), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
