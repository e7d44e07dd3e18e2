"""ucd_batch_path (one launch, csrc/batch_path.hip) against the pair it replaces for resident samples, ucd_image_path +
ucd_label_path, at the benchmark's batch: B = 24, S = 513, VOC-sized sources, RandomResizedCrop boxes drawn like the loader draws
them.  Same tensors, outputs compared bit for bit first.  Two numbers per arm:
  device  HIP-event time around the call(s), alternating the arms, median of the repeats;
  host    wall time of one DeviceBatcher.__call__ up to its return (enqueue cost: what the main process spends per batch), on
          cached (device) samples against host samples, with a device synchronise between calls that is not timed.
usage: python tools/batch_path_bench.py [--repeats N] -> profiles/datacache.md"""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ucd_amd import datapipe, hip  # noqa: E402
from ucd_amd.dataset import DeviceBatcher  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=50)
ap.add_argument("--batch", type=int, default=24)
ap.add_argument("--size", type=int, default=513)
args = ap.parse_args()
B, S, dev = args.batch, args.size, torch.device("cuda:0")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
rng = np.random.RandomState(0)
random.seed(0)
host = []
for k in range(B):
    H, W = (375, 500) if k % 3 else (500, 375)
    host.append((torch.from_numpy(rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)),
                 torch.from_numpy(rng.choice([0, 15, 16, 20, 255], size=(H, W)).astype(np.uint8))))
resident = [(i.to(dev), l.to(dev)) for i, l in host]
imgs, labs = [s[0] for s in resident], [s[1] for s in resident]
lut = datapipe.target_lut(list(range(16, 21)), list(range(1, 16))).to(dev)
boxes = [datapipe.random_resized_crop_params(i.shape[0], i.shape[1]) for i in imgs]
flips = [random.random() < 0.5 for _ in imgs]
image_path, label_path = datapipe.DeviceImagePath(S, MEAN, STD), datapipe.DeviceLabelPath(S, lut)


def pair():
    return image_path(imgs, boxes, flips), label_path(labs, boxes, flips)


def fused():
    return hip.batch_path(imgs, labs, boxes, flips, S, lut, MEAN, STD)


a, b = pair(), fused()
assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "ucd_batch_path differs from ucd_image_path + ucd_label_path"
print(f"# B {B}, S {S}, boxes h x w from {min(b[2] * b[3] for b in boxes)} to {max(b[2] * b[3] for b in boxes)} pixels; outputs equal bit for bit")


def device_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end)


for _ in range(5):
    pair(), fused()
times = {"pair": [], "fused": []}
for _ in range(args.repeats):                       # alternating: both arms see the same clock and neighbours
    times["pair"].append(device_ms(pair))
    times["fused"].append(device_ms(fused))
for name, label in (("pair", "ucd_image_path + ucd_label_path (events around both calls, their uploads included)"),
                    ("fused", "ucd_batch_path (events around the call, its upload included)")):
    t = sorted(times[name])
    print(f"device {label}: median {statistics.median(t) * 1e3:.0f} us, min {t[0] * 1e3:.0f}, max {t[-1] * 1e3:.0f}")
print(f"device ratio fused / pair: {statistics.median(times['fused']) / statistics.median(times['pair']):.2f}")

batcher = DeviceBatcher(dev, S, lut.cpu(), train=True)
wall = {"host samples": [], "cached samples": []}
for _ in range(5):
    batcher(host), batcher(resident)
for _ in range(args.repeats):
    for name, samples in (("host samples", host), ("cached samples", resident)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batcher(samples)
        wall[name].append(time.perf_counter() - t0)
        torch.cuda.synchronize()
for name, t in wall.items():
    t = sorted(t)
    print(f"host wall of DeviceBatcher.__call__ on {name}: median {statistics.median(t) * 1e6:.0f} us, min {t[0] * 1e6:.0f}, max {t[-1] * 1e6:.0f}")
print(f"host ratio cached / host samples: {statistics.median(wall['cached samples']) / statistics.median(wall['host samples']):.2f}")
