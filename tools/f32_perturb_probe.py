"""GPU probe: is the fp32 student's train-mode logit error of the split-bf16 convolutions (csrc/conv_f32.hip) on a golden step
amplification of their ~4.5e-6 per-output error, or a defect?  Runs the golden's whole fp32 step (the setup of
tests/test_step_gpu.py::_run_golden_step) on the MIOpen path with every output of the layers the split kernels would take
multiplied by (1 + s * N(0, 1)) - an error of relative L2 s, the size tests/test_conv_f32_gpu.py measures for the split
kernels - for several noise seeds, next to the unperturbed MIOpen step and the step on the split kernels
(UCD_F32_OWN_CONV=1).  Prints the student's train-mode logit relative L2 against the golden and the loss errors per run.
usage: python tools/f32_perturb_probe.py [golden ...]   (default: ucd_step_513.npz ucd_step_513_cal.npz)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from conftest import load_golden  # noqa: E402
from ucd_amd import argparser, blocks, switches, synth, tasks  # noqa: E402

CASES = {"ucd_step_513.npz": ("voc", "15-5", range(16, 21), False),
         "ucd_step_513_cal.npz": ("voc", "15-5", range(16, 21), True)}
SPLIT_ERR = 4.5e-6      # relative L2 of one split-kernel output against float64 (tests/test_conv_f32_gpu.py, every shape)


def run(gname, perturb=0.0, noise_seed=0, split=False):
    from ucd_amd.run import build_models, load_step_checkpoint, make_optimizer
    from ucd_amd.train import Trainer
    dataset, task, ids, calibrated = CASES[gname]
    g = load_golden(gname)
    seed, B, S = [int(v) for v in g["cfg"]]
    dev = torch.device("cuda:0")
    if split:
        switches.set("UCD_F32_OWN_CONV", "1")
    else:
        switches.unset("UCD_F32_OWN_CONV")
    opts = argparser.modify_command_options(argparser.get_argparser().parse_args(
        ["--method", "UCD", "--dataset", dataset, "--task", task, "--step", "1", "--lr", "0.001", "--no_pretrained",
         "--norm_act", "iabn_sync"]))
    classes = tasks.get_per_task_classes(dataset, task, 1)
    torch.backends.cudnn.allow_tf32 = False
    model, model_old = build_models(opts, dev, classes)
    state = synth.fill_state_dict({k: v.cpu() for k, v in model_old.state_dict().items()}, 42, calibrated=calibrated)
    optim = make_optimizer(opts, model)
    load_step_checkpoint(opts, model, model_old, state, dev)
    gen = torch.Generator(device=dev).manual_seed(noise_seed)

    def noise(mod, args, out):
        x = args[0]
        taps = mod.kernel_size[0] * mod.kernel_size[1]
        if not blocks._own_f32_conv(x.shape[0] * x.shape[2] * x.shape[3], mod.in_channels, mod.out_channels, taps):
            return out
        e = torch.randn(out.shape, generator=gen, device=dev).contiguous(memory_format=torch.channels_last)
        return out * (1.0 + perturb * e)
    if perturb > 0:
        for m in (model, model_old):
            for mod in m.modules():
                if isinstance(mod, (blocks.Conv1x1, blocks.Conv3x3)):
                    mod.register_forward_hook(noise)
    trainer = Trainer(model, model_old, device=dev, opts=opts, classes=classes)
    img = synth.images(seed, B, S)
    labels = synth.seg_labels(seed, B, S, S, ids)
    model.train()
    box = {}
    h = model.register_forward_hook(lambda m, a, out: box.__setitem__("out", out))
    r = trainer.train_step(img, labels, optim, None)
    h.remove()
    torch.cuda.synchronize()
    sem = box["out"][1]["sem"].detach().float()
    logits = F.interpolate(sem, size=(S, S), mode="bilinear", align_corners=False)
    got = logits.flatten()[torch.from_numpy(g["sample_idx"]).to(dev)].cpu().numpy()
    err = np.linalg.norm(got - g["logits_sample"]) / np.linalg.norm(g["logits_sample"])
    losses = {k: abs(r[k].item() - float(g[k])) / abs(float(g[k])) for k in ("ce", "con", "loss", "lkd")}
    switches.unset("UCD_F32_OWN_CONV")
    return err, losses


def main():
    names = sys.argv[1:] or list(CASES)
    for gname in names:
        print(f"== {gname}: student train-mode logits, relative L2 against the golden (bar of the fp32 tests: 5e-3); loss errors")
        rows = [("MIOpen fp32", dict())]
        rows += [(f"MIOpen fp32 + conv-output noise {s:.1e}, seed {k}", dict(perturb=s, noise_seed=k))
                 for s in (SPLIT_ERR,) for k in range(4)]
        rows += [(f"MIOpen fp32 + conv-output noise {SPLIT_ERR / 10:.1e}, seed 0", dict(perturb=SPLIT_ERR / 10))]
        rows += [("split-bf16 kernels (UCD_F32_OWN_CONV=1)", dict(split=True))]
        for name, kw in rows:
            err, losses = run(gname, **kw)
            print(f"{name:>52}: logits {err:.2e}  losses " + " ".join(f"{k} {v:.1e}" for k, v in losses.items()), flush=True)


if __name__ == "__main__":
    main()
