#!/usr/bin/env python
"""Call-level timing of SDR's class-prototype feature losses (``--sdr_match`` / ``--sdr_attract`` / ``--sdr_repel``; csrc/proto.hip)
on the pre-logits of the benchmarked step (B = 24, 256 channels, bf16) at 33 x 33 and 65 x 65, with 21 and 151 classes: the class
map, forward and backward of ``fused_proto_losses`` and of the torch composition ``proto_losses_torch`` on the same device and
operands, and - with ``--step_time`` - the whole UCD step without and with the three flags, alternating.

    python tools/proto_bench.py [--batch 24] [--iters 20] [--no_torch] [--step_time] [--crop 513] [--rounds 3]

Prints one JSON line per measurement.  Times are medians of HIP-event intervals over ``--iters`` calls after three warm-up calls."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((33, 513, 21, 16), (33, 513, 151, 101), (65, 1025, 21, 16), (65, 1025, 151, 101))        # (h = w, H = W, T, K)
SDR = ("--sdr_match", "0.01", "--sdr_attract", "0.001", "--sdr_repel", "0.001")


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def call_level(args):
    from ucd_amd import hip
    from ucd_amd.loss import fused_proto_losses, proto_classes, proto_classes_torch, proto_losses_torch
    dev = torch.device("cuda:0")
    B, Cc = args.batch, 256
    for hw, HW, T, K in SHAPES:
        g = torch.Generator(device=dev).manual_seed(5)
        x = torch.randn((B, Cc, hw, hw), device=dev, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        x.requires_grad_(True)
        # labels in blocks of 64 x 64 pixels: a few classes per image, a tenth of the blocks ignored
        blocks = torch.randint(0, T, (B, HW // 64 + 1, HW // 64 + 1), device=dev, generator=g)
        blocks[torch.rand(blocks.shape, device=dev, generator=g) < 0.1] = 255
        labels = blocks.repeat_interleave(64, 1).repeat_interleave(64, 2)[:, :HW, :HW].contiguous()
        sem_t = torch.randn((B, K, hw, hw), device=dev, generator=g)
        state = (torch.randn(T, Cc, device=dev, generator=g).double() * 40, torch.full((T,), 40, dtype=torch.int64, device=dev))
        old = (torch.randn(K, Cc, device=dev, generator=g), torch.ones(K, dtype=torch.bool, device=dev))
        weights = tuple(float(v) for v in SDR[1::2])
        nbytes = x.numel() * x.element_size()
        plan = hip.proto_plan(B * hw * hw, Cc, T, hip.BF16)
        for tag, classify, fn in (("hip", proto_classes, fused_proto_losses), ("torch", proto_classes_torch, proto_losses_torch)):
            if tag == "torch" and args.no_torch:
                continue
            t_cls = timed(lambda: classify(labels, sem_t, T, K, (hw, hw)), args.iters)
            cls = classify(labels, sem_t, T, K, (hw, hw))
            fwd = timed(lambda: fn(x, cls, state, old, weights), args.iters)
            val, parts = fn(x, cls, state, old, weights)

            def bwd():
                x.grad = None
                val.backward(retain_graph=True)
            t_bwd = timed(bwd, args.iters)
            print(json.dumps({"shape": [B, hw, hw, Cc], "T": T, "K": K, "path": tag, "map_MB": round(nbytes / 1e6, 1),
                              "classify_ms": round(t_cls, 4), "fwd_ms": round(fwd, 4), "bwd_ms": round(t_bwd, 4),
                              "present": int((parts["n"] > 0).sum()), "value": val.item(),
                              "workspace_MB": round(plan["workspace_bytes"] / 1e6, 1), "grid": plan["grid"]}), flush=True)
            del val, parts
        del x, labels, sem_t
        torch.cuda.empty_cache()


def build_trainer(args, extra):
    from ucd_amd import argparser, synth, tasks
    from ucd_amd.ddp import DistributedDataParallel
    from ucd_amd.run import build_models, load_step_checkpoint, make_optimizer
    from ucd_amd.scheduler import PolyLR
    from ucd_amd.train import Trainer
    dev = torch.device("cuda:0")
    opts = argparser.modify_command_options(argparser.get_argparser().parse_args(
        ["--method", "UCD", "--task", "15-5", "--dataset", "voc", "--step", "1", "--lr", "0.001", "--batch_size", str(args.batch),
         "--crop_size", str(args.crop), "--no_pretrained", "--opt_level", "O1", "--norm_act", "iabn_sync", *extra]))
    classes = tasks.get_per_task_classes("voc", "15-5", 1)
    torch.manual_seed(opts.random_seed)
    model, model_old = build_models(opts, dev, classes)
    state = {"module." + k: v for k, v in synth.fill_state_dict(
        {k: v.cpu() for k, v in model_old.state_dict().items()}, 42, calibrated=True).items()}
    optim = make_optimizer(opts, model)
    sched = PolyLR(optim, max_iters=100000, power=opts.lr_power)
    model = DistributedDataParallel(model, delay_allreduce=True, bf16_weights=True)
    load_step_checkpoint(opts, model, model_old, state, dev)
    trainer = Trainer(model, model_old, device=dev, opts=opts, classes=classes)
    if trainer.proto_flag and trainer.proto_w[0] > 0.:
        g = torch.Generator().manual_seed(5)                     # old prototypes as find_prototypes would leave them
        trainer._set_proto_old(torch.randn(trainer.old_classes, trainer.proto_sum.shape[1], generator=g) * 0.5,
                               torch.ones(trainer.old_classes, dtype=torch.bool))
    model.train()
    return trainer, optim, sched


def step_time(args):
    from ucd_amd import synth, tasks
    dev = torch.device("cuda:0")
    new_ids, _, _ = tasks.get_task_labels("voc", "15-5", 1)
    images = synth.images(1234, args.batch, args.crop).to(dev).contiguous(memory_format=torch.channels_last)
    labels = synth.seg_labels(1234, args.batch, args.crop, args.crop, new_ids).to(dev)
    runs = {tag: build_trainer(args, extra) for tag, extra in (("flags off", ()), ("flags on", SDR))}
    for trainer, optim, sched in runs.values():
        for _ in range(6):                                       # eager warm-up, capture, first replays
            trainer.train_step(images, labels, optim, sched)
    times = {tag: [] for tag in runs}
    for _ in range(args.rounds):                                 # alternating: the two steps share whatever else the machine does
        for tag, (trainer, optim, sched) in runs.items():
            times[tag].append(timed(lambda: trainer.train_step(images, labels, optim, sched), args.iters))
    for tag, (trainer, _, _) in runs.items():
        print(json.dumps({"step": tag, "batch": args.batch, "crop": args.crop, "step_ms": round(statistics.median(times[tag]), 3),
                          "rounds_ms": [round(t, 3) for t in times[tag]], "graph_steps": trainer.graph_steps,
                          "graph_error": trainer.step_graph_error,
                          "PROTO": trainer.last["PROTO"].item() if "PROTO" in trainer.last else None}), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--batch", type=int, default=24)
    p.add_argument("--crop", type=int, default=513)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--no_torch", action="store_true", help="skip the torch composition")
    p.add_argument("--step_time", action="store_true", help="also time the whole UCD step without and with the flags, alternating")
    p.add_argument("--only_step", action="store_true", help="only the step timing")
    args = p.parse_args()
    assert torch.cuda.is_available(), "proto_bench.py needs a GPU"
    if not args.only_step:
        call_level(args)
    if args.step_time or args.only_step:
        step_time(args)


if __name__ == "__main__":
    main()
