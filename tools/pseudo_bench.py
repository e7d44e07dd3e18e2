#!/usr/bin/env python
"""Call-level timing of PLOP's pseudo-labelling (``--pseudo entropy``; csrc/pseudo_label.hip) at the benchmarked shape (B = 24,
513^2 labels, 33^2 teacher cells, K = 16): ``fused_pseudo_labels`` and ``pseudo_hist`` on the HIP kernels against the torch
composition on the same tensors and against their traffic floor (labels read once and, for the label call, written once: 16 or 8
bytes per pixel, plus the teacher rows), the fused cross entropy with a per-image weight against the call without one, and - with
``--step_time`` - the whole UCD step with ``--pseudo entropy --pseudo_adaptive`` on against off, in one process.

    python tools/pseudo_bench.py [--batch 24] [--crop 513] [--iters 10] [--no_torch] [--step_time]

Prints one JSON line per measurement.  Times are medians of HIP-event intervals over ``--iters`` calls after three warm-up calls.
The operands (50 MB of labels, 1.7 MB of teacher rows) fit the 256 MiB last-level cache: the rates are cache rates, not HBM rates."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.pod_bench import STREAM_TBS, timed        # noqa: E402


def call_level(args):
    from ucd_amd import switches, synth, tasks
    from ucd_amd.loss import fused_pseudo_labels, fused_seg_losses, pseudo_hist, pseudo_median
    dev = torch.device("cuda:0")
    B, H, K, Ctot = args.batch, args.crop, 16, 21
    h = (H - 1) // 16 + 1
    g = torch.Generator(device=dev).manual_seed(5)
    sem_old = 3.0 * torch.randn(B, K, h, h, device=dev, generator=g)
    new_ids, _, _ = tasks.get_task_labels("voc", "15-5", 1)
    labels = synth.seg_labels(1234, B, H, H, new_ids).to(dev)
    hist = torch.zeros(K, 100, dtype=torch.int64, device=dev)
    pseudo_hist(sem_old, labels, hist)
    thr = torch.from_numpy(pseudo_median(hist, 0.001)).float().to(dev)
    pix, rows = B * H * H, sem_old.numel() * 4
    for tag in ("hip", "torch"):
        if tag == "torch" and args.no_torch:
            continue
        switches.set("UCD_FUSED_PSEUDO", "1" if tag == "hip" else "0")
        try:
            t_lab = timed(lambda: fused_pseudo_labels(sem_old, labels, thr, 0.0), args.iters)
            t_hist = timed(lambda: pseudo_hist(sem_old, labels, hist), args.iters)
            _, factor, counts = fused_pseudo_labels(sem_old, labels, thr, 0.0)
        finally:
            switches.unset("UCD_FUSED_PSEUDO")
        for call, ms, floor in (("label", t_lab, 16 * pix + rows), ("hist", t_hist, 8 * pix + rows)):
            print(json.dumps({"call": call, "path": tag, "B": B, "H": H, "h": h, "K": K, "ms": round(ms, 4), "floor_MB": round(floor / 1e6, 1),
                              "floor_TBs": round(floor / ms / 1e9, 3), "fraction": round(floor / ms / 1e9 / STREAM_TBS, 3),
                              "kept": round((counts[:, 0].sum() / counts[:, 1].sum()).item(), 4)}), flush=True)
    # the weighted cross entropy against the call without a weight: the step's pair (unbiased CE + unbiased KD) and PLOP's (plain CE)
    sem = torch.randn(B, Ctot, h, h, device=dev, generator=g).requires_grad_(True)
    for name, teacher, old_cl, kd_w in (("unbiased CE + KD", sem_old, K, 10.0), ("plain CE", None, 1, 0.0)):
        for tag, sw in (("unweighted", None), ("weighted", factor)):
            ms = timed(lambda: fused_seg_losses(sem, teacher, labels, old_cl, 1.0, kd_w, sample_weight=sw), args.iters)
            print(json.dumps({"call": "seg_losses", "pair": name, "path": tag, "ms": round(ms, 4)}), flush=True)


def step_time(args):
    from ucd_amd import argparser, synth, tasks
    from ucd_amd.ddp import DistributedDataParallel
    from ucd_amd.run import build_models, load_step_checkpoint, make_optimizer
    from ucd_amd.scheduler import PolyLR
    from ucd_amd.train import Trainer
    dev = torch.device("cuda:0")
    for extra in ((), ("--pseudo", "entropy", "--pseudo_adaptive")):
        opts = argparser.modify_command_options(argparser.get_argparser().parse_args(
            ["--method", "UCD", "--task", "15-5", "--dataset", "voc", "--step", "1", "--lr", "0.001", "--batch_size", str(args.batch),
             "--crop_size", str(args.crop), "--no_pretrained", "--opt_level", "O1", "--norm_act", "iabn_sync", *extra]))
        classes = tasks.get_per_task_classes("voc", "15-5", 1)
        new_ids, _, _ = tasks.get_task_labels("voc", "15-5", 1)
        torch.manual_seed(opts.random_seed)
        model, model_old = build_models(opts, dev, classes)
        state = {"module." + k: v for k, v in synth.fill_state_dict(
            {k: v.cpu() for k, v in model_old.state_dict().items()}, 42, calibrated=True).items()}
        optim = make_optimizer(opts, model)
        sched = PolyLR(optim, max_iters=2681, power=opts.lr_power)
        model = DistributedDataParallel(model, delay_allreduce=True, bf16_weights=True)
        load_step_checkpoint(opts, model, model_old, state, dev)
        trainer = Trainer(model, model_old, device=dev, opts=opts, classes=classes)
        images = synth.images(1234, args.batch, args.crop).to(dev).contiguous(memory_format=torch.channels_last)
        labels = synth.seg_labels(1234, args.batch, args.crop, args.crop, new_ids).to(dev)
        pass_ms = None
        if trainer.pseudo_flag:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            trainer.find_pseudo_thresholds([(images, labels)])
            b.record()
            b.synchronize()
            pass_ms = round(a.elapsed_time(b), 3)
        model.train()
        for _ in range(6):                                       # eager warm-up, capture, first replays
            trainer.train_step(images, labels, optim, sched)
        ms = timed(lambda: trainer.train_step(images, labels, optim, sched), args.iters)
        print(json.dumps({"step": "pseudo on" if extra else "pseudo off", "batch": args.batch, "crop": args.crop, "step_ms": round(ms, 3),
                          "graph_steps": trainer.graph_steps, "graph_error": trainer.step_graph_error, "threshold_pass_ms": pass_ms,
                          "PSEUDO": trainer.last["pseudo_kept"].item() if "pseudo_kept" in trainer.last else None}), flush=True)
        del trainer, model, model_old, optim, sched
        torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--batch", type=int, default=24)
    p.add_argument("--crop", type=int, default=513)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--no_torch", action="store_true", help="skip the torch composition")
    p.add_argument("--step_time", action="store_true", help="also time the whole UCD step with the term on and off")
    args = p.parse_args()
    assert torch.cuda.is_available(), "pseudo_bench.py needs a GPU"
    call_level(args)
    if args.step_time:
        step_time(args)


if __name__ == "__main__":
    main()
