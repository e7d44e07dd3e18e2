"""GPU: ADE 100-50 step 1 at --output_stride 8 - 151 student / 101 teacher classes on 17 x 17 logits under a 129-pixel crop, the
geometry no tiled form of the fused logit-loss kernel serves (207 456 bytes of LDS at the 512-pixel crop).  The Trainer's loss
calls and its validation go to the gather form (ucd_seg_losses_gather): whole iterations, eager and as
the captured step graph, and a validation pass.  Built like tests/test_ade_100_10_step_gpu.py."""
import pytest
import torch

from ucd_amd import argparser, synth, tasks

pytestmark = pytest.mark.gpu

EUNSUPPORTED = -4
CLASSES = [101, 50]


def _refused():
    """What every test here stands on: no tiled form serves the call, and the route names the gather form."""
    from ucd_amd import hip
    from ucd_amd.loss import seg_losses_route
    lib = hip.load()
    assert lib.ucd_seg_losses_plan(129, 129, 17, 17, 151, 101, 1, 1, -1, None, None, None, None) == EUNSUPPORTED
    assert "no form of the kernel serves this factor" in lib.ucd_last_error().decode()
    assert lib.ucd_seg_losses_plan(129, 129, 17, 17, 151, 151, 0, 1, -1, None, None, None, None) == EUNSUPPORTED
    assert seg_losses_route(129, 129, 17, 17, 151, 101, True) == "gather"


def _build(method, opt_level, wrap=False):
    from ucd_amd.run import build_models, load_step_checkpoint, make_optimizer
    dev = torch.device("cuda:0")
    classes = tasks.get_per_task_classes("ade", "100-50", 1)
    assert classes == CLASSES
    extra = () if opt_level == "O0" else ("--opt_level", opt_level)
    opts = argparser.modify_command_options(argparser.get_argparser().parse_args(
        ["--method", method, "--dataset", "ade", "--task", "100-50", "--step", "1", "--output_stride", "8", "--lr", "0.001",
         "--no_pretrained", "--norm_act", "iabn_sync", *extra]))
    torch.backends.cudnn.allow_tf32 = False
    torch.manual_seed(0)
    model, model_old = build_models(opts, dev, classes)
    state = synth.fill_state_dict({k: v.cpu() for k, v in model_old.state_dict().items()}, 42)
    optim = make_optimizer(opts, model)
    if wrap:                                  # the gradient-bucket wrapper: what a capture of the whole step needs
        from ucd_amd.ddp import DistributedDataParallel
        model = DistributedDataParallel(model, delay_allreduce=True, bf16_weights=opt_level != "O0")
    load_step_checkpoint(opts, model, model_old, state, dev)
    return opts, model, model_old, optim, classes, dev


def _new_ids():
    labels_new, _, _ = tasks.get_task_labels("ade", "100-50", 1)
    return [l for l in labels_new if l != 0][:8]


@pytest.mark.parametrize("method,opt_level", [("UCD", "O0"), ("UCD", "O1"), ("LWF", "O1")])
def test_trainer_step_at_output_stride_8(method, opt_level):
    """Two eager iterations: every loss piece is finite, the cross entropy positive, UCD's contrastive term positive, and the
    classifier and the head receive finite gradients that are not all zero.  (UCD: the unbiased pair; LWF: plain cross entropy
    beside plain distillation, the ucd_seg_losses_ex arguments on the same kernel.)"""
    from test_step_gpu import _capture_features
    from ucd_amd import switches
    from ucd_amd.train import Trainer
    _refused()
    opts, model, model_old, optim, classes, dev = _build(method, opt_level)
    switches.set("UCD_STEP_GRAPH", "0")
    try:
        trainer = Trainer(model, model_old, device=dev, opts=opts, classes=classes)
        assert trainer.old_classes == 101
        img = synth.images(611, 2, 129)
        labels = synth.seg_labels(611, 2, 129, 129, _new_ids())
        model.train()
        box, hook = _capture_features(model)
        for _ in range(2):
            r = trainer.train_step(img, labels, optim, None)
            assert all(torch.isfinite(v).item() for v in r.values()), {k: v.item() for k, v in r.items()}
        hook.remove()
    finally:
        switches.unset("UCD_STEP_GRAPH")
    assert trainer.graph_steps == 0
    sem = box["out"][1]["sem"]
    assert tuple(sem.shape) == (2, 151, 17, 17)
    assert r["ce"].item() > 0
    if method == "UCD":
        assert r["con"].item() > 0
    net = getattr(model, "module", model)
    for part in (net.cls, net.head):
        grads = [p.grad for p in part.parameters() if p.requires_grad]
        assert grads and all(g is not None and torch.isfinite(g).all().item() for g in grads)
        assert sum(g.float().abs().sum().item() for g in grads) > 0


def test_validate_at_output_stride_8():
    """Trainer.validate on four images: the class loss (151 classes without a teacher: refused by the tiled forms, formed by the
    gather form with no gradient buffer) is finite and positive; the confusion matrix (ucd_seg_confusion serves the geometry)
    counts every labelled pixel once."""
    from ucd_amd.metrics import StreamSegMetrics
    from ucd_amd.run import SyntheticSegmentation
    from ucd_amd.train import Trainer
    _refused()
    opts, model, model_old, _, classes, dev = _build("UCD", "O1")
    trainer = Trainer(model, model_old, device=dev, opts=opts, classes=classes)
    loader = torch.utils.data.DataLoader(SyntheticSegmentation(4, 129, _new_ids(), seed=3), batch_size=2)
    metrics = StreamSegMetrics(151)
    assert trainer.fuse_logit_losses and hasattr(metrics, "update_from_logits")
    (class_loss, reg_loss), score, _ = trainer.validate(loader, metrics)
    assert torch.isfinite(class_loss).item() and class_loss.item() > 0
    labelled = sum(int(((lab >= 0) & (lab < 151)).sum()) for _, lab in loader)
    assert labelled > 0 and int(metrics.confusion_matrix.sum().item()) == labelled
    assert score["Total samples"] == 4 and 0.0 <= score["Mean IoU"] <= 1.0


def test_step_graph_at_output_stride_8():
    """The default whole-step graph (O1, UCD): three eager warm-up iterations, the capture and two replays; the gather kernel
    and its route are inside the captured iteration."""
    from ucd_amd.train import Trainer
    _refused()
    opts, model, model_old, optim, classes, dev = _build("UCD", "O1", wrap=True)
    trainer = Trainer(model, model_old, device=dev, opts=opts, classes=classes)
    assert trainer.step_graph
    img = synth.images(612, 2, 129)
    labels = synth.seg_labels(612, 2, 129, 129, _new_ids())
    model.train()
    rec = []
    for _ in range(5):
        r = trainer.train_step(img, labels, optim, None)
        rec.append({k: v.item() for k, v in r.items()})
    torch.cuda.synchronize()
    assert trainer.step_graph_error is None, trainer.step_graph_error
    assert trainer.graph_steps >= 1, trainer.graph_steps
    assert all(torch.isfinite(torch.tensor(list(r.values()))).all().item() for r in rec), rec
    assert all(r["ce"] > 0 and r["con"] > 0 for r in rec), rec
