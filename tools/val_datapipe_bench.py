"""Throughput of the validation batch transform, DeviceBatcher(train=False), on the device (UCD_VAL_DEVICE=1: raw samples copied, one
ucd_val_image_path and one ucd_val_label_path call per batch) against the host form it replaces (UCD_VAL_DEVICE=0: Pillow resize + crop
per sample and a copy each, then the train path with the identity box; torch launches at full size), in ONE process: synthetic raw
pairs at VOC size 375 x 500, crop 513, batches of 24 for --crop_val and of 1 for full size.  Warm-up, then rounds that alternate the
two forms; every round is a host clock around its batches (the list of --batches repeated until a round lasts about
--min_seconds), ended by a device synchronisation.  The outputs of the two forms are
compared first.  The host form runs on the CPU, so the CPU model is part of the result.  The numbers of profiles/val_datapipe.md.

usage: python tools/val_datapipe_bench.py [--batches 20] [--rounds 5] [--min_seconds 0.5] [--out results.json]"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ucd_amd import datapipe, switches, tasks
from ucd_amd.dataset import DeviceBatcher

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, default=20, help="batches per timed round (at least 20)")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--min_seconds", type=float, default=0.5, help="a timed round repeats its batches until it lasts about this long")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.batches >= 20 and args.rounds >= 1
assert torch.cuda.is_available(), "this benchmark needs a GPU"

dev = torch.device("cuda:0")
H0, W0, S = 375, 500, 513


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def samples(n, seed):
    """raw pairs as the dataset hands them out: uint8 CPU tensors, blocky like decoded pictures and label maps"""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        img = rng.randint(0, 256, size=(H0 // 5 + 1, W0 // 5 + 1, 3)).astype(np.uint8).repeat(5, 0).repeat(5, 1)[:H0, :W0]
        lab = rng.randint(0, 21, size=(H0 // 25 + 1, W0 // 25 + 1)).astype(np.uint8).repeat(25, 0).repeat(25, 1)[:H0, :W0]
        out.append((torch.from_numpy(np.ascontiguousarray(img)), torch.from_numpy(np.ascontiguousarray(lab))))
    return out


def run(bt, batches, mode, passes=1):
    switches.set("UCD_VAL_DEVICE", mode)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(passes):
        for b in batches:
            bt(b)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


labels, labels_old, _ = tasks.get_task_labels("voc", "15-5", 1)
lut = datapipe.target_lut(labels, labels_old)
result = {"cpu": cpu_model(), "gpu": torch.cuda.get_device_name(0),
          "source": [H0, W0], "size": S, "rounds": args.rounds}
for name, crop, B in (("crop_val_batch24", True, 24), ("full_size_batch1", False, 1)):
    pool = samples(48, seed=3)
    batches = [[pool[(k * B + n) % len(pool)] for n in range(B)] for k in range(args.batches)]
    bt = DeviceBatcher(dev, S, lut, train=False, crop=crop)
    switches.set("UCD_VAL_DEVICE", "0"); x0, y0 = bt(batches[0])
    switches.set("UCD_VAL_DEVICE", "1"); x1, y1 = bt(batches[0])
    same = bool(torch.equal(x0, x1) and torch.equal(y0, y1))
    passes = {}
    for mode in ("0", "1"):                                    # warm-up of both forms at the timed shapes, then size the window
        run(bt, batches[:3], mode)
        passes[mode] = max(1, int(np.ceil(args.min_seconds / run(bt, batches, mode))))
    secs = {"0": [], "1": []}
    for _ in range(args.rounds):                               # alternate the two forms
        for mode in ("0", "1"):
            secs[mode].append(run(bt, batches, mode, passes[mode]))
    rate = {m: passes[m] * args.batches * B / float(np.median(v)) for m, v in secs.items()}
    result[name] = {"outputs_identical": same, "host_batches_per_round": passes["0"] * args.batches,
                    "device_batches_per_round": passes["1"] * args.batches,
                    "host_img_per_s": rate["0"], "device_img_per_s": rate["1"], "ratio": rate["1"] / rate["0"],
                    "host_ms_per_img": 1e3 / rate["0"], "device_ms_per_img": 1e3 / rate["1"],
                    "host_round_s": secs["0"], "device_round_s": secs["1"]}
    print(name, json.dumps(result[name]), flush=True)
switches.unset("UCD_VAL_DEVICE")
print(json.dumps({k: result[k] for k in ("cpu", "gpu")}), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
