#!/usr/bin/env python
"""Call-level timing of Local POD (``--pod_factor``; csrc/pod.hip) at the levels of the benchmarked step (B = 24, 513^2, bf16):
forward and backward of ``fused_local_pod`` and of the torch composition ``local_pod_torch`` per level, against the traffic floor
of a fused level (forward: one read of each map; backward: one read of the student map and one write of its gradient), the level
on the logits (``--pod_logits``: ``fused_local_pod_logits`` against ``local_pod_logits_torch`` at VOC 15-5 and ADE 100-10 class
counts, both ``normalize`` settings) and - with ``--step_time`` - the whole UCD step with the term off, on, and on with the level
on the logits.

    python tools/pod_bench.py [--batch 24] [--crop 513] [--iters 10] [--no_torch] [--step_time] [--only features|logits]

Prints one JSON line per measurement.  Times are medians of HIP-event intervals over ``--iters`` calls after three warm-up calls.
The two maps of the first level (204 MB each at the default shape) exceed the 256 MiB last-level cache together; the other levels
fit into it, so their rates are cache rates, not HBM rates."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STREAM_TBS = 6.3            # achievable HBM stream rate of an MI355X, TB/s (8 TB/s peak)


def levels(batch, crop):
    s4, s8, s16 = (crop - 1) // 4 + 1, (crop - 1) // 8 + 1, (crop - 1) // 16 + 1
    return [("mod2", (batch, 256, s4, s4), 0.01), ("mod3", (batch, 512, s8, s8), 0.01), ("mod4", (batch, 1024, s16, s16), 0.01),
            ("mod5", (batch, 2048, s16, s16), 0.01), ("pre_logits", (batch, 256, s16, s16), 1.0)]


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
    from ucd_amd.loss import fused_local_pod, local_pod_torch
    dev = torch.device("cuda:0")
    for name, shape, slope in levels(args.batch, args.crop):
        g = torch.Generator(device=dev).manual_seed(5)
        mk = lambda: torch.randn(shape, device=dev, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        x_s, x_t = mk().requires_grad_(True), mk()
        nbytes = x_t.numel() * x_t.element_size()
        for tag, fn in (("hip", fused_local_pod), ("torch", local_pod_torch)):
            if tag == "torch" and args.no_torch:
                continue
            fwd = timed(lambda: fn(x_s, x_t, slope, (1, 2, 4), 0.01), args.iters)
            val = fn(x_s, x_t, slope, (1, 2, 4), 0.01)

            def bwd():
                x_s.grad = None
                val.backward(retain_graph=True)
            t_bwd = timed(bwd, args.iters)
            floor = 2 * nbytes                                   # forward: both maps once; backward: one read + one write
            print(json.dumps({"level": name, "shape": list(shape), "path": tag, "map_MB": round(nbytes / 1e6, 1),
                              "fwd_ms": round(fwd, 4), "bwd_ms": round(t_bwd, 4),
                              "fwd_floor_TBs": round(floor / fwd / 1e9, 3), "bwd_floor_TBs": round(floor / t_bwd / 1e9, 3),
                              "fwd_fraction": round(floor / fwd / 1e9 / STREAM_TBS, 3),
                              "bwd_fraction": round(floor / t_bwd / 1e9 / STREAM_TBS, 3)}), flush=True)
            del val
        del x_s, x_t
        torch.cuda.empty_cache()


LOGIT_SPLITS = (("voc 15-5", 21, 16), ("ade 100-10 step 1", 111, 101))


def logits_level(args):
    """The level on the logits at the stride-16 map of the benchmarked step: fp32 channels-last rows, as the head hands them out."""
    from ucd_amd.loss import fused_local_pod_logits, local_pod_logits_torch
    dev = torch.device("cuda:0")
    s16 = (args.crop - 1) // 16 + 1
    for name, Ctot, K in LOGIT_SPLITS:
        g = torch.Generator(device=dev).manual_seed(5)
        mk = lambda c: torch.randn((args.batch, c, s16, s16), device=dev, generator=g).contiguous(memory_format=torch.channels_last)
        x_s, x_t = mk(Ctot).requires_grad_(True), mk(K)
        for normalize in (1, 0):
            for tag, fn in (("hip", fused_local_pod_logits), ("torch", local_pod_logits_torch)):
                if tag == "torch" and args.no_torch:
                    continue
                fwd = timed(lambda: fn(x_s, x_t, (1, 2, 4), 0.0005, normalize), args.iters)
                val = fn(x_s, x_t, (1, 2, 4), 0.0005, normalize)

                def bwd():
                    x_s.grad = None
                    val.backward(retain_graph=True)
                t_bwd = timed(bwd, args.iters)
                print(json.dumps({"level": "logits", "split": name, "shape": [args.batch, Ctot, K, s16, s16], "normalize": normalize,
                                  "path": tag, "student_MB": round(x_s.numel() * 4 / 1e6, 2), "fwd_ms": round(fwd, 4),
                                  "bwd_ms": round(t_bwd, 4), "value": val.item()}), flush=True)
                del val


def step_time(args):
    from ucd_amd import argparser, synth, tasks
    from ucd_amd.ddp import DistributedDataParallel
    from ucd_amd.run import build_models, load_step_checkpoint, make_optimizer
    from ucd_amd.scheduler import PolyLR
    from ucd_amd.train import Trainer
    dev = torch.device("cuda:0")
    for tag, extra in (("pod off", ()), ("pod on", ("--pod_factor", "0.01")), ("pod on + logits", ("--pod_factor", "0.01", "--pod_logits"))):
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
        print(json.dumps({"step": tag, "batch": args.batch, "crop": args.crop, "step_ms": round(ms, 3),
                          "graph_steps": trainer.graph_steps, "graph_error": trainer.step_graph_error,
                          "LPOD": trainer.last["LPOD"].item() if "LPOD" in trainer.last else None}), flush=True)
        del trainer, model, model_old, optim, sched
        torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--batch", type=int, default=24)
    p.add_argument("--crop", type=int, default=513)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--no_torch", action="store_true", help="skip the torch composition")
    p.add_argument("--step_time", action="store_true", help="also time the whole UCD step with the term off, on, and on with --pod_logits")
    p.add_argument("--only", choices=["features", "logits"], default=None, help="call-level timing of the feature levels or of the logits only")
    args = p.parse_args()
    assert torch.cuda.is_available(), "pod_bench.py needs a GPU"
    if args.only != "logits":
        call_level(args)
    if args.only != "features":
        logits_level(args)
    if args.step_time:
        step_time(args)


if __name__ == "__main__":
    main()
