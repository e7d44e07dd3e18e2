"""GPU: the --method LWF and --method ILT iterations, and --method UCD at --alpha 0.5, with their logit losses on the fused HIP
kernel (ucd_seg_losses_ex): against the reference's train.py:95-151 loop (tests/golden/lwf_step.npz, ilt_step.npz, written by
tests/golden/make_kd_golden.py) and against this package's own unfused routing (UCD_SEG_KD_EX=0: the torch modules on the
up-sampled logits).  fp32 (--opt_level O0), eager; bounds: 1e-3 on the loss terms (tests/test_step_gpu.py's bar for its fp32
whole-step goldens), the SGD updates of sampled parameters as tests/test_regularizer_gpu.py compares them."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _model(method, extra=()):
    """The product at VOC 15-5 step 1 on the calibrated synthetic step-0 checkpoint, student in the gradient-bucket wrapper."""
    from ucd_amd import argparser, synth, tasks
    from ucd_amd.ddp import DistributedDataParallel
    from ucd_amd.run import build_models, load_step_checkpoint, make_optimizer
    dev = torch.device("cuda:0")
    opts = argparser.modify_command_options(argparser.get_argparser().parse_args(
        ["--method", method, "--task", "15-5", "--step", "1", "--lr", "0.001", "--no_pretrained", "--norm_act", "iabn_sync", *extra]))
    classes = tasks.get_per_task_classes("voc", "15-5", 1)
    torch.backends.cudnn.allow_tf32 = False
    torch.manual_seed(0)                     # the new head's random initial values: the same in every run of a comparison
    model, model_old = build_models(opts, dev, classes)
    state = synth.fill_state_dict({k: v.cpu() for k, v in model_old.state_dict().items()}, 42, calibrated=True)
    optim = make_optimizer(opts, model)
    model = DistributedDataParallel(model, delay_allreduce=True, bf16_weights=False)
    load_step_checkpoint(opts, model, model_old, state, dev)
    return opts, model, model_old, optim, classes, dev


def _run(method, extra=(), head=None, kd_ex="1", iters=3, fused_lde="1"):
    """``iters`` eager Trainer steps on the goldens' batch; (trainer, per-iteration terms, the first 16 elements of every
    parameter before and after)."""
    from ucd_amd import switches, synth
    from ucd_amd.train import Trainer
    opts, model, model_old, optim, classes, dev = _model(method, extra)
    net = model.module
    if head is not None:                     # --init_balanced is off for LWF / ILT: the reference's random new head
        with torch.no_grad():
            net.cls[1].weight.copy_(torch.from_numpy(head[0]))
            net.cls[1].bias.copy_(torch.from_numpy(head[1]))
    sample = lambda: {n: p.detach().flatten()[:16].cpu().double().numpy() for n, p in net.named_parameters()}
    before = sample()
    switches.set("UCD_STEP_GRAPH", "0")
    switches.set("UCD_SEG_KD_EX", kd_ex)
    switches.set("UCD_FUSED_LDE", fused_lde)
    # every lazy attention map a Features dict builds during the run (student or teacher), by key
    from ucd_amd.segmentation_module import Features
    built, missing = [], Features.__missing__

    def recording(self, key):
        built.append(key)
        return missing(self, key)

    Features.__missing__ = recording
    try:
        trainer = Trainer(model, model_old, device=dev, opts=opts, classes=classes)
        img = synth.images(501, 2, 129)
        labels = synth.seg_labels(501, 2, 129, 129, range(16, 21))
        model.train()
        rec = {"ce": [], "con": [], "lkd": [], "lde": []}
        for _ in range(iters):
            r = trainer.train_step(img, labels, optim, None)
            for k in rec:
                rec[k].append(r[k].item())
        torch.cuda.synchronize()
    finally:
        switches.unset("UCD_STEP_GRAPH")
        switches.unset("UCD_SEG_KD_EX")
        switches.unset("UCD_FUSED_LDE")
        Features.__missing__ = missing
    trainer.built_maps = built
    return trainer, rec, before, sample()


def _same_updates(params, ref_after, before, names):
    for n in names:
        p0 = before[n].astype(np.float64)
        up, ur = params[n] - p0, ref_after[n].astype(np.float64) - p0
        if np.linalg.norm(ur) > 1e-7:
            cos = float(up @ ur / (np.linalg.norm(up) * np.linalg.norm(ur) + 1e-30))
            assert cos > 0.9 and 0.5 < np.linalg.norm(up) / np.linalg.norm(ur) < 2.0, (n, cos)


@pytest.mark.parametrize("method", ["LWF", "ILT"])
def test_step_matches_reference_golden_fp32(method):
    """Three iterations against the reference's loop: ce / con / lkd / lde within 1e-3, the sampled parameters move like the
    reference's.  The logit losses come from the fused kernel (plain CE + plain KD at loss_kd = 100)."""
    g = dict(np.load(os.path.join(GOLDEN, f"{method.lower()}_step.npz")))
    trainer, rec, _, params = _run(method, head=(g["cls1_weight_init"], g["cls1_bias_init"]))
    assert trainer.fuse_logit_losses and trainer.lkd_flag and trainer.kd_mode == "plain" and not trainer.unce
    assert trainer.lde_flag == (method == "ILT") == trainer.fused_lde and not trainer.lde_lazy
    # neither loss reads the lazy Features dict: no attention-weighted map ("body", "pre_logits") was ever materialised
    assert trainer.built_maps == [], trainer.built_maps
    print(method, rec)
    for k in ("ce", "con", "lkd"):
        np.testing.assert_allclose(rec[k], g[k], rtol=1e-3, err_msg=k)
    if method == "ILT":
        np.testing.assert_allclose(rec["lde"], g["lde"], rtol=1e-3)
    else:
        assert rec["lde"] == [0.0, 0.0, 0.0]
    names = [k.split("|", 1)[1] for k in g if k.startswith("before|")]
    _same_updates(params, {n: g["after|" + n] for n in names}, {n: g["before|" + n] for n in names}, names)


@pytest.mark.parametrize("method,extra", [("LWF", ()), ("ILT", ()), ("UCD", ("--alpha", "0.5"))])
def test_switch_kd_ex_0_is_the_same_step(method, extra):
    """UCD_SEG_KD_EX=0 restores the unfused routing (torch modules on up-sampled logits) for these pairs; it is the reference of
    this comparison.  The default takes the fused kernel and gives the same three iterations: loss terms within 1e-3, the same
    parameter updates.  (--method UCD --alpha 0.5: unbiased CE + unbiased KD on scaled teacher logits.)"""
    old_t, old, start, old_p = _run(method, extra, kd_ex="0")
    new_t, new, start_new, new_p = _run(method, extra, kd_ex="1")
    assert not old_t.fuse_logit_losses and new_t.fuse_logit_losses and new_t.lkd_flag
    assert all(np.array_equal(start[n], start_new[n]) for n in start)
    print(method, extra, old, new)
    for k in ("ce", "con", "lkd", "lde"):
        np.testing.assert_allclose(new[k], old[k], rtol=1e-3, atol=1e-12, err_msg=k)
    _same_updates(new_p, old_p, start, [n for n in new_p if n.endswith("weight")][::12])


def test_switch_fused_lde_0_is_the_same_ilt_step():
    """UCD_FUSED_LDE=0 restores the torch composition of the encoder term (attention maps through the lazy Features dict, fp32
    copies, MSELoss) and keeps ILT outside the graphs; it is the reference of this comparison.  The default gives the same three
    iterations: loss terms within 1e-3, the same parameter updates."""
    old_t, old, start, old_p = _run("ILT", fused_lde="0")
    new_t, new, start_new, new_p = _run("ILT")
    assert not old_t.fused_lde and old_t.lde_lazy and "body" in old_t.built_maps and "pre_logits" in old_t.built_maps
    assert new_t.fused_lde and not new_t.lde_lazy and new_t.built_maps == []
    assert all(np.array_equal(start[n], start_new[n]) for n in start)
    print(old, new)
    for k in ("ce", "con", "lkd", "lde"):
        np.testing.assert_allclose(new[k], old[k], rtol=1e-3, err_msg=k)
    _same_updates(new_p, old_p, start, [n for n in new_p if n.endswith("weight")][::12])


def _ilt_scheduled(step_graph, steps=8, batch=3, crop=257):
    """tests/test_step_gpu.py's _scheduled_steps for --method ILT: ``steps`` iterations at O1 under a steep PolyLR on two alternating
    batches, with or without the whole-step graph."""
    from ucd_amd import argparser, switches, synth, tasks
    from ucd_amd.ddp import DistributedDataParallel
    from ucd_amd.run import build_models, load_step_checkpoint, make_optimizer
    from ucd_amd.scheduler import PolyLR
    from ucd_amd.train import Trainer
    dev = torch.device("cuda:0")
    opts = argparser.modify_command_options(argparser.get_argparser().parse_args(
        ["--method", "ILT", "--dataset", "voc", "--task", "15-5", "--step", "1", "--lr", "0.001", "--no_pretrained",
         "--norm_act", "iabn_sync", "--opt_level", "O1"]))
    classes = tasks.get_per_task_classes("voc", "15-5", 1)
    torch.manual_seed(0)
    model, model_old = build_models(opts, dev, classes)
    state = synth.fill_state_dict({k: v.cpu() for k, v in model_old.state_dict().items()}, 42, calibrated=True)
    optim = make_optimizer(opts, model)
    sched = PolyLR(optim, max_iters=steps + 2, power=0.9)
    net = model
    model = DistributedDataParallel(model, delay_allreduce=True, bf16_weights=True)
    load_step_checkpoint(opts, model, model_old, state, dev)
    switches.set("UCD_STEP_GRAPH", step_graph)
    switches.set("UCD_STAT_ATOMIC", "0")                  # the deterministic statistics path: the tight bounds of that test
    torch.backends.cudnn.deterministic = True
    try:
        trainer = Trainer(model, model_old, device=dev, opts=opts, classes=classes)
        model.train()
        rec = []
        for it in range(steps):
            img = synth.images(700 + it % 2, batch, crop)
            labels = synth.seg_labels(700 + it % 2, batch, crop, crop, range(16, 21))
            r = trainer.train_step(img, labels, optim, sched)
            rec.append([r[k].item() for k in ("ce", "con", "lkd", "lde", "loss")])
        torch.cuda.synchronize()
        params = dict(net.named_parameters())
        names = ["body.mod1.conv1.weight", "body.mod5.block3.convs.conv3.weight", "head.map_convs.2.weight", "cls.1.weight"]
        after = {n: params[n].detach().float().cpu().clone() for n in names}
        return np.asarray(rec), after, trainer
    finally:
        torch.backends.cudnn.deterministic = False
        switches.unset("UCD_STEP_GRAPH")
        switches.unset("UCD_STAT_ATOMIC")


def test_ilt_whole_step_graph_replays_the_eager_iteration():
    """With both losses fused an ILT iteration is captured like a UCD one: after the three eager warm-up iterations the step is
    replayed, and it is the eager iteration - the bounds of tests/test_step_gpu.py's replay test in its deterministic mode (losses
    2e-3, parameters 3e-4 in relative L2)."""
    eager, pe, t_e = _ilt_scheduled("0")
    graph, pg, t_g = _ilt_scheduled("1")
    assert t_g.step_graph_error is None, t_g.step_graph_error
    assert t_e.graph_steps == 0 and t_g.graph_steps == 8 - 3, (t_e.graph_steps, t_g.graph_steps)
    assert t_g.fused_lde and t_g.fuse_logit_losses and not t_g.lde_lazy
    print("eager vs graph losses, max rel:", np.abs(eager - graph).max(0) / np.abs(eager).max(0))
    assert np.all(np.isfinite(graph)) and np.all(graph[:, 3] > 0)
    np.testing.assert_allclose(graph, eager, rtol=2e-3)
    for n in pe:
        d = ((pe[n] - pg[n]).norm() / pe[n].norm()).item()
        assert d < 3e-4, (n, d)
