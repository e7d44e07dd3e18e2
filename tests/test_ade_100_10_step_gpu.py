"""GPU: ADE 100-10 past its second step - heads of 101 + 10 s classes, a teacher of K = 111 .. 141 - through the two loss calls that
see those class counts and through one whole Trainer step.  The contrastive loss used to stop at 110 (fp32) / 112 (fp16) teacher
classes, which made steps 2 .. 5 of this task the one wired combination that could not train."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import losses as OL
from ucd_amd import argparser, synth, tasks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("Ctot,K", [(151, 141), (121, 111)])
def test_fused_logit_losses_at_the_step_5_and_step_2_heads(Ctot, K):
    """Unbiased CE + unbiased KD on the many-class form against float64, with the bounds tests/test_seglosses_gpu.py::_check holds
    that form to: losses within max(4 x the error of the fp32 torch composition, 1e-6 relative); gradient element-wise within
    A + R, A the fixed-point allowance of the form (quantum gmax / 2^17, half a quantum per tile and cell, (ceil(2 f / 32) + 1)
    (ceil(2 f / 64) + 1) tiles per cell at factor f) and R = 4 x the largest error of the fp32 composition."""
    from ucd_amd import hip
    from ucd_amd.loss import UnbiasedCrossEntropy, UnbiasedKnowledgeDistillationLoss, fused_seg_losses
    B, h, H, kd_w = 1, 8, 64, 10.0
    form = C.c_int()
    assert hip.load().ucd_seg_losses_plan(H, H, h, h, Ctot, K, 1, 1, -1, C.byref(form), None, None, None) == 0
    assert hip.SEG_FORMS[form.value] == "wide/fixed"
    seed = 7100 + Ctot
    sem = synth.t_normal(seed, (B, Ctot, h, h), stream=1, scale=2.0)
    sem_t = synth.t_normal(seed, (B, K, h, h), stream=2, scale=2.0)
    labels = synth.seg_labels(seed, B, H, H, range(K, Ctot), rects=4)
    up = lambda t: F.interpolate(t, size=(H, H), mode="bilinear", align_corners=False)
    s64 = sem.double().requires_grad_(True)
    ce64 = OL.unbiased_cross_entropy(up(s64), labels, K).mean()
    kd64 = OL.unbiased_kd(up(s64), up(sem_t.double()))
    (ce64 + kd_w * kd64).backward()
    dev = torch.device("cuda:0")
    s32 = sem.to(dev).requires_grad_(True)
    ce32 = UnbiasedCrossEntropy(old_cl=K, reduction="none")(up(s32), labels.to(dev)).mean()
    kd32 = UnbiasedKnowledgeDistillationLoss(alpha=1.0)(up(s32), up(sem_t.to(dev)))
    (ce32 + kd_w * kd32).backward()
    s_dev = sem.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    total, ce, kd = fused_seg_losses(s_dev, sem_t.to(dev), labels.to(dev), K, 1.0, kd_w)
    total.backward()
    g64, g32, g = s64.grad.numpy(), s32.grad.double().cpu().numpy(), s_dev.grad.double().cpu().numpy()
    gmax = (1.0 + 2.0 * kd_w / K) / (B * H * H)
    f = H / h
    A = gmax / 2.0 ** 17 / 2.0 * (int(np.ceil(2.0 * f / 32)) + 1) * (int(np.ceil(2.0 * f / 64)) + 1)
    R = 4.0 * float(np.abs(g32 - g64).max())
    err = float(np.abs(g - g64).max())
    print(f"Ctot {Ctot} K {K}: ce {ce64.item():.6e} comp32 {abs(ce32.item() - ce64.item()):.2e} kernel {abs(ce.item() - ce64.item()):.2e} | "
          f"kd {kd64.item():.6e} comp32 {abs(kd32.item() - kd64.item()):.2e} kernel {abs(kd.item() - kd64.item()):.2e} | "
          f"grad max {np.abs(g64).max():.3e} kernel {err:.2e} A {A:.2e} R {R:.2e}")
    assert abs(ce.item() - ce64.item()) <= max(4.0 * abs(ce32.item() - ce64.item()), 1e-6 * abs(ce64.item()))
    assert abs(kd.item() - kd64.item()) <= max(4.0 * abs(kd32.item() - kd64.item()), 1e-6 * abs(kd64.item()))
    assert np.isfinite(g).all() and err <= A + R, (err, A, R)


@pytest.mark.parametrize("opt_level", ["O1", "O0"])
def test_trainer_step_of_ade_100_10_step_5(opt_level):
    """Two eager iterations with the head layout [101, 10, 10, 10, 10, 10] and its 141-class teacher at the 129-pixel crop of
    tests/test_step_gpu.py::test_other_baseline_configs_step_runs (built the same way): every loss piece is finite, the
    contrastive term is positive, and the module that produces pre_logits (the student's head) receives a gradient.  O1 takes the
    fp16 fixed-split sweeps (K > 32), O0 the fp32 kernels with the anchor block's probability rows in global memory."""
    from test_step_gpu import _capture_features
    from ucd_amd import hip, switches
    from ucd_amd.run import build_models, load_step_checkpoint, make_optimizer
    from ucd_amd.train import Trainer
    dev = torch.device("cuda:0")
    classes = tasks.get_per_task_classes("ade", "100-10", 5)
    labels_new, labels_old, _ = tasks.get_task_labels("ade", "100-10", 5)
    assert classes == [101, 10, 10, 10, 10, 10] and sum(classes[:-1]) == 141
    extra = () if opt_level == "O0" else ("--opt_level", opt_level)
    opts = argparser.modify_command_options(argparser.get_argparser().parse_args(
        ["--method", "UCD", "--dataset", "ade", "--task", "100-10", "--step", "5", "--lr", "0.001", "--no_pretrained",
         "--norm_act", "iabn_sync", *extra]))
    torch.backends.cudnn.allow_tf32 = False
    model, model_old = build_models(opts, dev, classes)
    state = synth.fill_state_dict({k: v.cpu() for k, v in model_old.state_dict().items()}, 42)
    load_step_checkpoint(opts, model, model_old, state, dev)
    switches.set("UCD_STEP_GRAPH", "0")
    try:
        trainer = Trainer(model, model_old, device=dev, opts=opts, classes=classes)
        assert trainer.old_classes == 141 and trainer.pixcon_precision == ("f32" if opt_level == "O0" else "f16")
        optim = make_optimizer(opts, model)
        ids = [l for l in labels_new if l != 0][:8]
        img = synth.images(601, 2, 129)
        labels = synth.seg_labels(601, 2, 129, 129, ids)
        model.train()
        box, hook = _capture_features(model)
        for _ in range(2):
            r = trainer.train_step(img, labels, optim, None)
            assert all(torch.isfinite(v).item() for v in r.values()), {k: v.item() for k, v in r.items()}
        hook.remove()
    finally:
        switches.unset("UCD_STEP_GRAPH")
    assert getattr(trainer, "graph_steps", 0) == 0
    assert r["con"].item() > 0 and r["ce"].item() > 0
    sem = box["out"][1]["sem"]
    assert sem.shape[1] == 151 and trainer.model_old.cls is not None and sum(m.out_channels for m in trainer.model_old.cls) == 141
    bhw = sem.shape[0] * sem.shape[2] * sem.shape[3]
    assert hip.pixcon_loss_plan(bhw, 141, trainer.pixcon_precision)["path"] == ("f32/wide" if opt_level == "O0" else "f16/split")
    head = getattr(model, "module", model).head
    grads = [p.grad for p in head.parameters() if p.requires_grad]
    assert grads and all(g is not None and torch.isfinite(g).all().item() for g in grads)
    assert sum(g.float().abs().sum().item() for g in grads) > 0
