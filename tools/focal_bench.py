#!/usr/bin/env python
"""Call-level timing of the focal cross entropy (``--focal_loss``; ucd_seg_losses_focal / ucd_seg_losses_gather_focal) at the
benchmarked shape (B = 24, 513^2 labels, 33^2 cells): every form's focal call - gamma 2, which runs without exp2 / log, and a
general gamma - against the unmodulated call on the same tensors; the fused cross-entropy-only call against the torch composition
(up-sample, cross-entropy map, ``focal_modulate``, mean, backward), which decides the default of ``UCD_FUSED_FOCAL``; and - with
``--step_time`` - the whole UCD step with ``--focal_loss`` on against off, in one process.

    python tools/focal_bench.py [--batch 24] [--crop 513] [--iters 10] [--no_torch] [--step_time]

Prints one JSON line per measurement.  Times are medians of HIP-event intervals over ``--iters`` calls (forward + backward of the
Function: the kernels run in the forward, the backward scales the stored gradient) after three warm-up calls."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.pod_bench import timed        # noqa: E402

FOCAL = (("unmodulated", None), ("gamma 2", (2.0, 1.0)), ("gamma 3.5", (3.5, 0.25)))


def _form(H, h, Ctot, K, old_cl, teacher):
    import ctypes as C
    from ucd_amd import hip
    from ucd_amd.loss import seg_losses_route
    if seg_losses_route(H, H, h, h, Ctot, K if teacher else old_cl, teacher, old_cl) == "gather":
        return "gather"
    f = C.c_int()
    hip.load().ucd_seg_losses_plan_ex(H, H, h, h, Ctot, K, old_cl, hip.KD_UNBIASED, int(teacher), 1, -1, C.byref(f), None, None, None)
    return hip.SEG_FORMS[f.value]


def call_level(args):
    import torch.nn.functional as F
    from ucd_amd import synth
    from ucd_amd.loss import UnbiasedCrossEntropy, focal_modulate, fused_seg_losses
    dev = torch.device("cuda:0")
    B = args.batch
    g = torch.Generator(device=dev).manual_seed(5)
    # name, Ctot, K, crop, cells, teacher, old_cl, kd weight
    h16 = (args.crop - 1) // 16 + 1
    cases = (("unbiased CE + KD, 21 / 16", 21, 16, args.crop, h16, True, 16, 10.0),
             ("plain CE, 21, no teacher", 21, 16, args.crop, h16, False, 1, 0.0),
             ("unbiased CE + KD, 151 / 101", 151, 101, args.crop, h16, True, 101, 10.0),
             ("unbiased CE + KD, 151 / 101, stride 8", 151, 101, 512, 64, True, 101, 10.0))
    for name, Ctot, K, H, h, teacher, old_cl, kd_w in cases:
        sem = (2.0 * torch.randn(B, Ctot, h, h, device=dev, generator=g)).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        sem_old = 2.0 * torch.randn(B, K, h, h, device=dev, generator=g) if teacher else None
        labels = synth.seg_labels(1234, B, H, H, range(K, Ctot)).to(dev)
        form = _form(H, h, Ctot, K, old_cl, teacher)

        def fused(focal):
            total, _, _ = fused_seg_losses(sem, sem_old, labels, old_cl, 1.0, kd_w, focal=focal)
            total.backward()
            sem.grad = None

        for tag, focal in FOCAL:
            ms = timed(lambda: fused(focal), args.iters)
            print(json.dumps({"call": "seg_losses", "case": name, "form": form, "B": B, "H": H, "h": h, "path": tag, "ms": round(ms, 4)}),
                  flush=True)
        if teacher or args.no_torch:
            continue
        # the composition the Trainer runs under UCD_FUSED_FOCAL=0, cross entropy only
        crit = UnbiasedCrossEntropy(old_cl=old_cl, ignore_index=255, reduction="none")

        def composed(focal):
            up = F.interpolate(sem, size=(H, H), mode="bilinear", align_corners=False)
            focal_modulate(crit(up, labels), *focal).mean().backward()
            sem.grad = None

        for tag, focal in FOCAL[1:]:
            ms = timed(lambda: composed(focal), args.iters)
            print(json.dumps({"call": "composition", "case": name, "B": B, "H": H, "h": h, "path": tag, "ms": round(ms, 4)}), flush=True)
        del sem, sem_old, labels
        torch.cuda.empty_cache()


def step_time(args):
    from ucd_amd import argparser, synth, tasks
    from ucd_amd.ddp import DistributedDataParallel
    from ucd_amd.run import build_models, load_step_checkpoint, make_optimizer
    from ucd_amd.scheduler import PolyLR
    from ucd_amd.train import Trainer
    dev = torch.device("cuda:0")
    for extra in ((), ("--focal_loss",), ("--focal_loss", "--focal_loss_gamma", "3.5")):
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
        model.train()
        for _ in range(6):                                       # eager warm-up, capture, first replays
            trainer.train_step(images, labels, optim, sched)
        ms = timed(lambda: trainer.train_step(images, labels, optim, sched), args.iters)
        print(json.dumps({"step": " ".join(extra) or "focal off", "batch": args.batch, "crop": args.crop, "step_ms": round(ms, 3),
                          "graph_steps": trainer.graph_steps, "graph_error": trainer.step_graph_error,
                          "ce": trainer.last["ce"].item()}), flush=True)
        del trainer, model, model_old, optim, sched
        torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--batch", type=int, default=24)
    p.add_argument("--crop", type=int, default=513)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--no_torch", action="store_true", help="skip the torch composition")
    p.add_argument("--step_time", action="store_true", help="also time the whole UCD step with the flag on and off")
    args = p.parse_args()
    assert torch.cuda.is_available(), "focal_bench.py needs a GPU"
    call_level(args)
    if args.step_time:
        step_time(args)


if __name__ == "__main__":
    main()
