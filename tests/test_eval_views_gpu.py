"""GPU: Trainer.test and evaluate.py with test-time views (--eval_scales, --eval_flip, --fusion-mode): the confusion matrix is that of
the float64 fusion of the per-view logits, the losses stay those of the plain view, the files show the prediction that was scored,
and the default flags run the single-view path of before.

Models and loader are those of tests/test_evaluate_gpu.py (built here again): VOC 15-5 step 1 with the calibrated synthetic weights,
129 x 129 synthetic images, fp32 activations (--opt_level O0).  The yardstick and its left-out rule are those of
tests/test_seg_views_gpu.py: float64 torch on the CPU from the per-view ``sem`` maps (the ones the trainer fused, recorded at
update_from_views and checked against the model called again on the scaled / mirrored images - two forward passes of this model do
not repeat their bits, see test_trainer_test_scores_the_fused_views); a pixel is left out where the two best float64 scores are closer than 1e-5 (mean, max) or any view's two
best up-sampled logits closer than 1e-4 (voting); at most 0.5 % may be left out."""
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ucd_amd import argparser, synth, tasks

pytestmark = pytest.mark.gpu

N_CLASSES = 21
VIEW_FLAGS = ["--eval_scales", "0.75", "1.0", "--eval_flip"]
CAP = 0.005


def _opts(extra=()):
    o = argparser.get_argparser().parse_args(["--task", "15-5", "--step", "1", "--lr", "0.001", "--no_pretrained", "--norm_act", "iabn_sync",
                                              "--opt_level", "O0", *extra])
    return argparser.modify_command_options(o)


@functools.lru_cache(maxsize=None)
def _models():
    """Student (16 + 5 classes) and teacher (16) with the calibrated synthetic fill, the student's heads and last block moved a
    little (tests/test_evaluate_gpu.py::_models)."""
    from ucd_amd.run import build_models, load_step_checkpoint
    dev = torch.device("cuda:0")
    opts = _opts(["--method", "UCD"])
    classes = tasks.get_per_task_classes("voc", "15-5", 1)
    torch.backends.cudnn.allow_tf32 = False
    model, model_old = build_models(opts, dev, classes)
    state = synth.fill_state_dict({k: v.cpu() for k, v in model_old.state_dict().items()}, 42, calibrated=True)
    load_step_checkpoint(opts, model, model_old, state, dev)
    with torch.no_grad():
        for i, head in enumerate(model.cls):
            head.weight.add_(synth.t_normal(90 + i, tuple(head.weight.shape), stream=1, scale=0.02).to(dev))
        for i, p in enumerate(list(model.body.parameters())[-6:]):
            p.mul_(1.0 + synth.t_normal(80 + i, tuple(p.shape), stream=1, scale=0.1).to(dev))
    return model, model_old, classes, dev


def _loader(n, batch_size):
    from ucd_amd.run import SyntheticSegmentation
    return torch.utils.data.DataLoader(SyntheticSegmentation(n, 129, list(range(16, 21)), seed=3), batch_size=batch_size)


def _yardstick(sems, flips, H, W, rule):
    """(float64 prediction, undecided mask) on the CPU from the per-view sem maps."""
    mean = mx = votes = gap = None
    for sem, flip in zip(sems, flips):
        u = F.interpolate(sem.detach().float().cpu().double(), size=(H, W), mode="bilinear", align_corners=False)
        u = u.flip(-1) if flip else u
        p = u.softmax(1)
        v = torch.zeros_like(p).scatter_(1, u.argmax(1, keepdim=True), 1.0)
        top = u.topk(2, dim=1).values
        g = top[:, 0] - top[:, 1]
        mean, mx, votes = (p, p, v) if mean is None else (mean + p, torch.maximum(mx, p), votes + v)
        gap = g if gap is None else torch.minimum(gap, g)
    score = {"mean": mean, "max": mx, "voting": votes}[rule]
    top = score.topk(2, dim=1).values
    undecided = (gap < 1e-4) if rule == "voting" else (top[:, 0] - top[:, 1] < 1e-5)
    return score.argmax(1), undecided


def _hist(labels, pred, mask):
    ok = mask & (labels >= 0) & (labels < N_CLASSES) & (pred < N_CLASSES)
    return torch.bincount(N_CLASSES * labels[ok] + pred[ok], minlength=N_CLASSES ** 2).reshape(N_CLASSES, N_CLASSES)


def _record_views(monkeypatch):
    """Every update_from_views call of the test: (sems on the host, flips, fusion)."""
    from ucd_amd.metrics import StreamSegMetrics
    calls = []
    real = StreamSegMetrics.update_from_views

    def recording(self, label_trues, sems, flips, fusion="mean", pred=None):
        calls.append(([s.detach().float().cpu() for s in sems], list(flips), fusion))
        return real(self, label_trues, sems, flips, fusion=fusion, pred=pred)
    monkeypatch.setattr(StreamSegMetrics, "update_from_views", recording)
    return calls


@pytest.mark.parametrize("rule", ["mean", "max", "voting"])
def test_trainer_test_scores_the_fused_views(rule, monkeypatch):
    """--eval_scales 0.75 1.0 --eval_flip: four views, (1.0, plain) first.  Confusion matrix and returned predictions against the float64
    fusion of the per-view sem maps.

    Two forward passes of this model on the same batch do not give the same bits (measured on an MI355X: sem differs by up to 5.5e-6
    between identical calls, the single-view class loss of Trainer.test by +-2 ulp from run to run), so the maps that are fused are
    the ones the trainer handed to update_from_views; that they ARE the model on the scaled / mirrored images, in the order of
    eval_views, is checked by calling the model again on those images: within 1e-4, twenty times the forward's own spread and a
    thousandth of what a wrong scale, order or mirror changes (logits of order 10).
    Losses: the class loss and the Reg loss (a teacher under --method UCD: the KD term) come from the plain view as in the single-view
    run - recomputed here from the recorded plain-view maps with the same fused call they must give the trainer's bits; against a
    separate single-view run they are held to rel 1e-4, the bound tests/test_evaluate_gpu.py holds these terms to (two runs differ
    by the forward's spread; 2 ulp observed)."""
    from ucd_amd.loss import fused_seg_losses
    from ucd_amd.metrics import StreamSegMetrics
    from ucd_amd.train import Trainer
    model, model_old, classes, dev = _models()
    opts = _opts(["--method", "UCD", "--fusion-mode", rule, *VIEW_FLAGS])
    views = argparser.eval_views(opts)
    assert views == [(1.0, False), (1.0, True), (0.75, False), (0.75, True)]
    trainer = Trainer(model, model_old, device=dev, opts=opts, classes=classes)
    calls = _record_views(monkeypatch)
    teacher, teacher_eager = [], trainer._teacher_eager

    def recording_teacher(images, up):
        out = teacher_eager(images, up)
        teacher.append((tuple(images.shape), out[1]["sem"].detach().clone()))
        return out
    trainer._teacher_eager = recording_teacher
    metrics = StreamSegMetrics(N_CLASSES)
    (class_loss, reg_loss), score, samples = trainer.test(_loader(3, 2), metrics)
    assert score["Total samples"] == 3 and len(samples) == 3 and len(calls) == 2 and len(teacher) == 2
    got = torch.from_numpy(np.stack([s[2] for s in samples]))
    model.eval()
    want = torch.zeros(N_CLASSES, N_CLASSES, dtype=torch.int64)
    class_ref = torch.zeros((), device=dev)
    reg_ref = torch.zeros((), device=dev)
    k = left = 0
    for (images, labels), (sems, flips, fusion), (t_shape, t_sem) in zip(_loader(3, 2), calls, teacher):
        assert fusion == rule and flips == [f for _, f in views] and t_shape == tuple(images.shape)
        assert [tuple(s.shape[-2:]) for s in sems] == [(9, 9), (9, 9), (7, 7), (7, 7)]
        images = images.to(dev, dtype=torch.float32)
        with torch.no_grad():
            for sem, (scale, flip) in zip(sems, views):
                x = images if scale == 1.0 else F.interpolate(images, size=(int(129 * scale + 0.5),) * 2, mode="bilinear",
                                                              align_corners=False)
                again = model(x.flip(-1) if flip else x, ret_intermediate=False, upsample=False)[1]["sem"].float().cpu()
                torch.testing.assert_close(sem, again, rtol=0, atol=1e-4)
        ref, undecided = _yardstick(sems, flips, 129, 129, rule)
        g = got[k:k + len(labels)]
        assert torch.equal(g[~undecided], ref[~undecided])
        want += _hist(labels, ref, ~undecided) + _hist(labels, g, undecided)
        k += len(labels)
        left += int(undecided.sum())
        plain, lab = sems[0].to(dev), labels.to(dev)
        with torch.no_grad():
            class_ref += fused_seg_losses(plain, None, lab, trainer.old_classes, 1.0, 0.0)[1]
            reg_ref += fused_seg_losses(plain, t_sem, lab, trainer.old_classes, 0.0, 1.0, kd=trainer.kd_mode, alpha=trainer.alpha)[2]
    print(f"Trainer.test / {rule}: {100 * left / got.numel():.4f} % of {got.numel()} pixels left out")
    assert left <= CAP * got.numel()
    assert torch.equal(metrics.confusion_matrix.cpu().long(), want)
    assert class_loss.item() == (class_ref / 2).item() and reg_loss.item() == (reg_ref / 2).item()
    single = Trainer(model, model_old, device=dev, opts=_opts(["--method", "UCD"]), classes=classes)
    (class_1, reg_1), _, _ = single.test(_loader(3, 2), StreamSegMetrics(N_CLASSES))
    assert len(calls) == 2 and reg_1.item() > 0
    print(f"class loss {class_loss.item():.9f} (single view {class_1.item():.9f}), Reg loss {reg_loss.item():.9f} ({reg_1.item():.9f})")
    assert class_loss.item() == pytest.approx(class_1.item(), rel=1e-4) and reg_loss.item() == pytest.approx(reg_1.item(), rel=1e-4)


def test_default_flags_run_the_single_view_path(monkeypatch):
    """No view flags: Trainer.test goes through update_from_logits once per batch, as before, and never through update_from_views;
    its predictions are the ones its matrix counts.  validate stays single-view even on a trainer whose options name views, unless
    views are passed."""
    from ucd_amd.metrics import StreamSegMetrics
    from ucd_amd.train import Trainer
    model, model_old, classes, dev = _models()
    calls = _record_views(monkeypatch)
    plain_calls = []
    real = StreamSegMetrics.update_from_logits
    monkeypatch.setattr(StreamSegMetrics, "update_from_logits",
                        lambda self, labels, sem, pred=None: plain_calls.append(pred is not None) or real(self, labels, sem, pred=pred))
    trainer = Trainer(model, None, device=dev, opts=_opts(["--method", "UCD"]), classes=classes)
    assert trainer.eval_views == [(1.0, False)]
    m_test = StreamSegMetrics(N_CLASSES)
    (cl_t, rg_t), score, samples = trainer.test(_loader(3, 2), m_test)
    assert calls == [] and plain_calls == [True, True] and score["Total samples"] == 3 and rg_t.item() == 0.0 and cl_t.item() > 0
    hist = torch.zeros(N_CLASSES, N_CLASSES, dtype=torch.int64)
    for _, lab, prd, _ in samples:
        lab, prd = torch.from_numpy(lab), torch.from_numpy(prd)
        hist += _hist(lab, prd, torch.ones_like(lab, dtype=torch.bool))
    assert torch.equal(hist, m_test.confusion_matrix.cpu().long())
    # a trainer with view flags: validate is single-view unless asked
    viewed = Trainer(model, None, device=dev, opts=_opts(["--method", "UCD", *VIEW_FLAGS]), classes=classes)
    m2 = StreamSegMetrics(N_CLASSES)
    (cl_v, _), _, _ = viewed.validate(_loader(3, 2), m2)
    assert calls == [] and plain_calls == [True, True, False, False] and m2.total_samples == 3
    assert cl_v.item() == pytest.approx(cl_t.item(), rel=1e-4)          # two runs of one path: the forward's own spread
    viewed.validate(_loader(3, 2), m2, views=viewed.eval_views)
    assert len(calls) == 2 and len(plain_calls) == 4 and m2.total_samples == 3

    # views without the fused logit path are refused, not served by a fall-back
    class Plain:
        def reset(self):
            pass

        def update(self, *a):
            pass
    with pytest.raises(RuntimeError, match="update_from_views"):
        viewed.test(_loader(1, 1), Plain())


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def test_evaluate_writes_the_fused_prediction(tmp_path, monkeypatch):
    """ucd_amd.evaluate.main on --data_root synthetic with the view flags: NNNNpre.png holds the fused map the confusion matrix was
    built from (recorded at update_from_views), NNNNpre_clo.png its colours."""
    from PIL import Image
    from ucd_amd import evaluate, visual
    from ucd_amd.metrics import StreamSegMetrics
    model, _, classes, dev = _models()
    monkeypatch.chdir(tmp_path)
    for k, v in (("MASTER_ADDR", "127.0.0.1"), ("RANK", "0"), ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0")):
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("MASTER_PORT", _free_port())
    ckpt = tmp_path / "student.pth"
    torch.save({"model_state": {k: v.cpu() for k, v in model.state_dict().items()}}, ckpt)
    preds = []
    real = StreamSegMetrics.update_from_views

    def recording(self, label_trues, sems, flips, fusion="mean", pred=None):
        assert pred is not None and fusion == "max" and list(flips) == [False, True, False, True]
        real(self, label_trues, sems, flips, fusion=fusion, pred=pred)
        preds.append(pred.cpu().numpy().copy())
    monkeypatch.setattr(StreamSegMetrics, "update_from_views", recording)
    opts = _opts(["--method", "UCD", "--data_root", "synthetic", "--crop_size", "129", "--batch_size", "2", "--fusion-mode", "max",
                  "--logdir", str(tmp_path / "logs"), "--name", "views", "--step_ckpt", str(ckpt), *VIEW_FLAGS])
    _, score = evaluate.main(opts)
    fused = np.concatenate(preds)
    assert score["Total samples"] == fused.shape[0] == 4
    out = tmp_path / "logs" / "15-5-voc" / "views" / "predictions"
    assert len(os.listdir(out)) == 5 * fused.shape[0]
    cmap = visual.color_map("voc")
    for k in range(fused.shape[0]):
        pre = np.asarray(Image.open(out / f"{k:04d}pre.png"))
        assert pre.dtype == np.uint8 and pre.shape == (129, 129)
        np.testing.assert_array_equal(pre, fused[k].astype(np.uint8))
        np.testing.assert_array_equal(np.asarray(Image.open(out / f"{k:04d}pre_clo.png")), cmap[pre])
    assert 0.0 <= score["Mean IoU"] <= 1.0
