"""EWC / PI / RW regulariser (csrc/reg.hip): the kernel alone at the full model size, and the captured train step with and
without it.

    python tools/reg_probe.py [--steps 20] [--crop 513] [--batch 24]

1. ``ucd_reg_step`` per method over the VOC 15-5 step-1 student (~58 M trainable elements, channels-last): device-event time
   per launch (two launches: the pass + the fixed-order reduction), algorithmic bytes per element (EWC 28, PI 36, RW 44 on
   its every-`iterations` update, 28 on the others: it is timed with --reg_iterations 1, every update a score update) and the
   fraction of 8 TB/s.
2. The B = 24, 513^2, O1 step of bench.py (whole-step graph), A = UCD, B = UCD + EWC, run in the order ABAB in one process;
   each phase re-captures the step graph after its eager warm-up.  ms per step from device events around ``--steps`` steps.
Prints one JSON line; the box is named by its hostname and GPU.
"""
import argparse
import json
import os
import socket
import sys

os.environ.setdefault("UCD_MIOPEN_SEED", "1")       # bench.py seeds the committed MIOpen find-db when imported with it

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_GBS = 8000.0


def kernel_alone(name, steps):
    from ucd_amd import argparser
    from ucd_amd.ddp import DistributedDataParallel  # noqa: F401  (same import order as a run)
    from ucd_amd.regularizer import get_regularizer
    from ucd_amd.segmentation_module import make_model
    opts = argparser.modify_command_options(argparser.get_argparser().parse_args(
        ["--method", name.upper(), "--task", "15-5", "--step", "1", "--no_pretrained", "--reg_iterations", "1"]))
    dev = torch.device("cuda")
    torch.manual_seed(0)

    class Wrap(torch.nn.Module):
        def __init__(self, m):
            super().__init__()
            self.module = m
    student = Wrap(make_model(opts, classes=[16, 5])).to(dev).to(memory_format=torch.channels_last)
    teacher = make_model(opts, classes=[16]).to(dev).to(memory_format=torch.channels_last)
    arrays = ["fisher"] if name == "ewc" else ["score"] if name == "pi" else ["fisher", "score"]
    state = {"name": name}
    for a in arrays:
        state[a] = {"module." + n: torch.rand(q.shape, device=dev) for n, q in teacher.named_parameters()}
    for p in student.parameters():
        if p.requires_grad:
            p.grad = torch.randn_like(p) * 1e-3
    reg = get_regularizer(student, teacher, dev, opts, state)
    for _ in range(3):
        reg.step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        reg.step()
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / steps
    elements = reg._plan.elements
    bytes_ = reg.bytes_per_element * elements
    out = {"elements": elements, "bytes_per_element": reg.bytes_per_element, "ms": ms, "gbs": bytes_ / ms / 1e6,
           "frac_8tbs": bytes_ / ms / 1e6 / PEAK_GBS, "launch_blocks": reg._plan.n_blocks}
    del reg, student, teacher, state
    torch.cuda.empty_cache()
    return out


def step_ab(args):
    import bench
    from ucd_amd import argparser
    from ucd_amd.regularizer import get_regularizer
    saved = sys.argv
    sys.argv = ["bench.py", "--gpus", "1", "--crop", str(args.crop), "--global_batch", str(args.batch), "--no_miopen_find"]
    try:
        bargs = bench.parse()
    finally:
        sys.argv = saved
    dev = torch.device("cuda")
    trainer, optim, sched, images, labels, _ = bench.build(bargs, dev, args.batch, 0)
    opts = argparser.modify_command_options(argparser.get_argparser().parse_args(
        ["--method", "EWC", "--task", "15-5", "--step", "1", "--no_pretrained"]))
    state = {"name": "ewc", "fisher": {k: torch.rand(v.shape, device=dev) for k, v in trainer.model.named_parameters()
                                       if k.startswith("module.") and not k.startswith("module.cls.1")}}
    reg = get_regularizer(trainer.model, trainer.model_old, dev, opts, state)

    def phase(with_reg):
        trainer.regularizer, trainer.regularizer_flag = (reg, True) if with_reg else (None, False)
        trainer._sg, trainer._sg_seen = None, 0
        optim.device_hyper(False)
        for _ in range(trainer.step_graph_warmup + 2):
            trainer.train_step(images, labels, optim, sched)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.steps):
            trainer.train_step(images, labels, optim, sched)
        b.record()
        torch.cuda.synchronize()
        return {"ms_per_step": a.elapsed_time(b) / args.steps, "graph": trainer._sg is not None,
                "graph_error": trainer.step_graph_error}

    runs = []
    for with_reg in (False, True, False, True):
        runs.append(dict(phase(with_reg), reg=with_reg))
    a = [r["ms_per_step"] for r in runs if not r["reg"]]
    b = [r["ms_per_step"] for r in runs if r["reg"]]
    return {"order": "ABAB", "runs": runs, "delta_ms": sum(b) / len(b) - sum(a) / len(a)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--crop", type=int, default=513)
    p.add_argument("--batch", type=int, default=24)
    p.add_argument("--skip_step", action="store_true")
    args = p.parse_args()
    out = {"box": socket.gethostname(), "gpu": torch.cuda.get_device_name(0), "kernel": {}}
    for name in ("ewc", "pi", "rw"):
        out["kernel"][name] = kernel_alone(name, args.steps)
    if not args.skip_step:
        out["step"] = step_ab(args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
