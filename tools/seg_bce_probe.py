"""GPU probe of the fused BCE losses (ucd_seg_bce through ucd_amd.loss.fused_seg_bce, forward + backward to the low-resolution
logits) against the torch composition the reference runs, on the same GPU in the same process: F.interpolate of both logit
tensors, the criterion formula, sigmoid, BCEWithLogitsLoss, backward to the low-resolution logits.  HIP-event times, warm, the
two alternating, median of N calls; the two results are compared at the timed size.

usage: python tools/seg_bce_probe.py [--calls 20] [--steps]
  --steps   also time the --method LWF-MC and --method UCD iterations at batch 24 / 513^2 (bf16, synthetic checkpoint), eager and
            replayed from the whole-step graph
Shapes: 24 x 513^2 <- 33^2 with (21, 16) classes, with and without teacher; 3 x 512^2 <- 32^2 with (151, 101), with teacher."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from ucd_amd import synth
from ucd_amd.loss import fused_seg_bce

SHAPES = [("voc 15-5, teacher", 24, 513, 33, 21, 16, True), ("ade 100-50, teacher", 3, 512, 32, 151, 101, True),
          ("voc 15-5, no teacher", 24, 513, 33, 21, 16, False)]
HARD_W, SOFT_W = 1.0, 10.0


def composition(sem, sem_old, labels, soft_w):
    """What the reference runs (utils/loss.py:31-54 with reduction 'none' then .mean(); train.py:119-124)."""
    H, W = labels.shape[-2:]
    out = F.interpolate(sem, size=(H, W), mode="bilinear", align_corners=False)
    n_cl = out.shape[1]
    lab = torch.where(labels != 255, labels, torch.full_like(labels, n_cl))
    tgt = F.one_hot(lab, n_cl + 1).float().permute(0, 3, 1, 2)[:, :n_cl]
    loss = F.binary_cross_entropy_with_logits(out, tgt, reduction="none").sum(dim=1)
    bce = (loss * tgt.sum(dim=1)).mean()
    soft = torch.zeros((), device=sem.device)
    if sem_old is not None:
        out_old = F.interpolate(sem_old, size=(H, W), mode="bilinear", align_corners=False)
        K = out_old.shape[1]
        soft = K * F.binary_cross_entropy_with_logits(out.narrow(1, 0, K), torch.sigmoid(out_old))
    return HARD_W * bce + soft_w * soft, bce, soft


def loss_probe(calls):
    dev = torch.device("cuda:0")
    for name, B, H, h, Ctot, K, teacher in SHAPES:
        sem = synth.t_normal(11, (B, Ctot, h, h), stream=1, scale=2.0).to(dev).requires_grad_(True)
        sem_old = synth.t_normal(11, (B, K, h, h), stream=2, scale=2.0).to(dev) if teacher else None
        labels = synth.seg_labels(7, B, H, H, range(K, Ctot)).to(dev)
        soft_w = SOFT_W if teacher else 0.0

        def run(fn):
            sem.grad = None
            total, bce, soft = fn()
            total.backward()
            return bce.detach(), soft.detach(), sem.grad

        fused = lambda: fused_seg_bce(sem, sem_old, labels, HARD_W, soft_w)
        torch_ = lambda: composition(sem, sem_old, labels, soft_w)
        for _ in range(3):
            a, b = run(fused), run(torch_)
        torch.cuda.synchronize()
        rel = lambda x, y: ((x - y).abs().max() / y.abs().max().clamp_min(1e-30)).item()
        print(f"{name}: B {B}, {H}^2 <- {h}^2, classes {Ctot}/{K}: bce {a[0].item():.6f} vs {b[0].item():.6f}, soft {a[1].item():.6f} vs "
              f"{b[1].item():.6f}, gradient max difference / max {rel(a[2], b[2]):.2e}", flush=True)
        times = {"fused": [], "torch": []}
        for _ in range(calls):                      # alternating: both see the same neighbours on the machine
            for key, fn in (("fused", fused), ("torch", torch_)):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record(); run(fn); e.record()
                times[key].append((s, e))
        torch.cuda.synchronize()
        med = {k: sorted(s.elapsed_time(e) for s, e in v) for k, v in times.items()}
        f, t = med["fused"], med["torch"]
        print(f"    fused_seg_bce fwd + bwd: median {f[len(f) // 2] * 1e3:.0f} us (min {f[0] * 1e3:.0f}, max {f[-1] * 1e3:.0f});  torch composition: "
              f"median {t[len(t) // 2] * 1e3:.0f} us (min {t[0] * 1e3:.0f}, max {t[-1] * 1e3:.0f});  ratio {t[len(t) // 2] / f[len(f) // 2]:.1f}x  "
              f"[{calls} calls each]", flush=True)
        del sem, sem_old, labels
        torch.cuda.empty_cache()


def step_probe(steps=12, batch=24, crop=513):
    """Iteration times of --method LWF-MC next to --method UCD: VOC 15-5 step 1, O1, synthetic calibrated checkpoint; the eager
    iterations (UCD_STEP_GRAPH=0) and the replayed ones (after the three warm-up iterations and the capture)."""
    from ucd_amd import argparser, switches, tasks
    from ucd_amd.ddp import DistributedDataParallel
    from ucd_amd.run import build_models, load_step_checkpoint, make_optimizer
    from ucd_amd.train import Trainer
    dev = torch.device("cuda:0")
    img = synth.images(700, batch, crop)
    labels = synth.seg_labels(700, batch, crop, crop, range(16, 21))
    for method in ("UCD", "LWF-MC"):
        for graph in ("0", "1"):
            opts = argparser.modify_command_options(argparser.get_argparser().parse_args(
                ["--method", method, "--dataset", "voc", "--task", "15-5", "--step", "1", "--lr", "0.001", "--no_pretrained",
                 "--norm_act", "iabn_sync", "--opt_level", "O1"]))
            classes = tasks.get_per_task_classes("voc", "15-5", 1)
            torch.manual_seed(0)
            model, model_old = build_models(opts, dev, classes)
            state = synth.fill_state_dict({k: v.cpu() for k, v in model_old.state_dict().items()}, 42, calibrated=True)
            optim = make_optimizer(opts, model)
            model = DistributedDataParallel(model, delay_allreduce=True, bf16_weights=True)
            load_step_checkpoint(opts, model, model_old, state, dev)
            switches.set("UCD_STEP_GRAPH", graph)
            try:
                trainer = Trainer(model, model_old, device=dev, opts=opts, classes=classes)
                model.train()
                for _ in range(6):                                  # warm-up: solver search, the capture
                    trainer.train_step(img, labels, optim, None)
                torch.cuda.synchronize()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(steps):
                    r = trainer.train_step(img, labels, optim, None)
                e.record()
                torch.cuda.synchronize()
                print(f"--method {method}, batch {batch}, {crop}^2, O1, step graph {graph}: {s.elapsed_time(e) / steps:.1f} ms / iteration over "
                      f"{steps} (graph replays {trainer.graph_steps}, capture error {trainer.step_graph_error}); ce {r['ce'].item():.4f}",
                      flush=True)
            finally:
                switches.unset("UCD_STEP_GRAPH")
            del trainer, model, model_old, optim
            torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--steps", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is nothing to report without one"
    loss_probe(max(args.calls, 20))
    if args.steps:
        step_probe()
