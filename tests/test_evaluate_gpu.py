"""GPU: what a run produces at its end - the teacher-side terms of Trainer.validate, its returned samples, Trainer.test with a
rendering sink, and the two drivers (run.py with --lr_policy step and --sample_num, evaluate.py on the checkpoint it wrote).

Models and loader are those of tests/test_step_gpu.py::test_validation_loop_device_metrics: VOC 15-5 step 1 with synthetic weights,
129 x 129 synthetic images; fp32 activations (--opt_level O0) wherever values are compared."""
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


def _opts(extra=()):
    o = argparser.get_argparser().parse_args(["--task", "15-5", "--step", "1", "--lr", "0.001", "--no_pretrained", "--norm_act", "iabn_sync",
                                              "--opt_level", "O0", *extra])
    return argparser.modify_command_options(o)


@functools.lru_cache(maxsize=None)
def _models():
    """Student (16 + 5 classes) and teacher (16), built once for the module; evaluation changes neither.  The weights are the
    CALIBRATED synthetic fill: evaluation-mode logits of order 10 (the plain fill gives 1e5, soft-maxes that are one-hot in fp32 and
    distillation terms that vanish).  After the balanced initialisation the student's distribution over the old classes IS the
    teacher's, so its heads are then moved a little: the distillation terms compare two different networks."""
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
        for i, p in enumerate(list(model.body.parameters())[-6:]):          # the last block: the body maps differ too
            p.mul_(1.0 + synth.t_normal(80 + i, tuple(p.shape), stream=1, scale=0.1).to(dev))
    return model, model_old, classes, dev


def _loader(n, batch_size):
    from ucd_amd.run import SyntheticSegmentation
    return torch.utils.data.DataLoader(SyntheticSegmentation(n, 129, list(range(16, 21)), seed=3), batch_size=batch_size)


def _torch_terms(loader, kd_module, with_encoder):
    """Mean over the batches of the reference's unscaled terms (train.py:228-233), from the torch modules on up-sampled logits of the
    same eval-mode models."""
    model, model_old, _, dev = _models()
    model.eval()

    def att(x):                                     # segmentation_module.py:86-94 of the reference
        a = (x.float() ** 2).sum(dim=1)
        a = a / a.flatten(1).norm(dim=1)[:, None, None]
        return a.unsqueeze(1) * x.float()

    total, n = 0.0, 0
    with torch.no_grad():
        for images, labels in loader:
            images = images.to(dev, dtype=torch.float32)
            _, f = model(images, upsample=False)
            _, fo = model_old(images, upsample=False)
            up = lambda t: F.interpolate(t.float(), size=images.shape[-2:], mode="bilinear", align_corners=False)
            term = kd_module(up(f["sem"]), up(fo["sem"])).item() if kd_module is not None else 0.0
            if with_encoder:
                term += torch.nn.MSELoss()(att(f.raw("body")), att(fo.raw("body"))).item()
            total, n = total + term, n + 1
    return total / n


def test_validate_evaluates_the_kd_term_with_a_teacher():
    """--method UCD: Reg Loss > 0 and equal to the mean over batches of UnbiasedKnowledgeDistillationLoss(alpha)(up(sem), up(sem_old))
    within rel 1e-4, the bound tests/test_kd_losses_gpu.py (check) holds the fused KD value to against that composition."""
    from ucd_amd.loss import UnbiasedKnowledgeDistillationLoss
    from ucd_amd.metrics import StreamSegMetrics
    from ucd_amd.train import Trainer
    model, model_old, classes, dev = _models()
    opts = _opts(["--method", "UCD"])
    trainer = Trainer(model, model_old, device=dev, opts=opts, classes=classes)
    assert trainer.lkd_flag and not trainer.lde_flag
    loader = _loader(4, 2)
    (class_loss, reg_loss), score, samples = trainer.validate(loader, StreamSegMetrics(N_CLASSES))
    ref = _torch_terms(loader, UnbiasedKnowledgeDistillationLoss(alpha=opts.alpha), False)
    print(f"UCD validate: class {class_loss.item():.6f} reg {reg_loss.item():.6f} torch {ref:.6f}")
    assert reg_loss.is_cuda and reg_loss.item() > 0 and class_loss.item() > 0
    assert reg_loss.item() == pytest.approx(ref, rel=1e-4)
    assert samples == [] and score["Total samples"] == 4
    # no teacher: exactly 0, as before
    (_, reg0), _, _ = Trainer(model, None, device=dev, opts=opts, classes=classes).validate(loader, StreamSegMetrics(N_CLASSES))
    assert reg0.item() == 0.0


def test_validate_adds_the_encoder_term_under_ilt():
    """--method ILT: the plain KD value plus the encoder term on the body maps, MSE(att(body), att(body_old)), each within rel 1e-4
    of the torch composition (tests/test_kd_losses_gpu.py holds the KD value and the fused_attn_mse loss to rel 1e-4 each; both terms
    are positive, so their sum is within 1e-4 too).  The encoder term is much the smaller of the two, so it is also held to rel
    1e-4 on its own, in a run with --loss_de alone."""
    from ucd_amd.loss import KnowledgeDistillationLoss
    from ucd_amd.metrics import StreamSegMetrics
    from ucd_amd.train import Trainer
    model, model_old, classes, dev = _models()
    opts = _opts(["--method", "ILT"])
    trainer = Trainer(model, model_old, device=dev, opts=opts, classes=classes)
    assert trainer.lkd_flag and trainer.lde_flag and trainer.fused_lde
    loader = _loader(4, 2)
    (_, reg_loss), _, _ = trainer.validate(loader, StreamSegMetrics(N_CLASSES))
    kd_only = _torch_terms(loader, KnowledgeDistillationLoss(alpha=opts.alpha), False)
    ref = _torch_terms(loader, KnowledgeDistillationLoss(alpha=opts.alpha), True)
    print(f"ILT validate: reg {reg_loss.item():.6f} torch {ref:.6f} (KD alone {kd_only:.6f})")
    assert ref > kd_only > 0
    assert reg_loss.item() == pytest.approx(ref, rel=1e-4)
    trainer = Trainer(model, model_old, device=dev, opts=_opts(["--loss_de", "100"]), classes=classes)
    assert trainer.lde_flag and not trainer.lkd_flag
    (_, reg_de), _, _ = trainer.validate(loader, StreamSegMetrics(N_CLASSES))
    de_only = _torch_terms(loader, None, True)
    print(f"encoder term alone: {reg_de.item():.6e} torch {de_only:.6e}")
    assert de_only > 0
    assert reg_de.item() == pytest.approx(de_only, rel=1e-4)


def test_validate_returns_the_requested_samples():
    """Batch size 1, ret_samples_ids = [0, 1] on a two-image loader: two (image, label, prediction) tuples of the documented shapes
    and dtypes, and bincount(n * label + prediction) over them IS the confusion matrix (the predictions are the kernel's own)."""
    from ucd_amd.metrics import StreamSegMetrics
    from ucd_amd.train import Trainer
    model, model_old, classes, dev = _models()
    trainer = Trainer(model, model_old, device=dev, opts=_opts(["--method", "UCD"]), classes=classes)
    metrics = StreamSegMetrics(N_CLASSES)
    _, _, samples = trainer.validate(_loader(2, 1), metrics, ret_samples_ids=[0, 1])
    assert len(samples) == 2
    hist = np.zeros(N_CLASSES * N_CLASSES, dtype=np.int64)
    for (img, lab, prd), (img_ref, lab_ref) in zip(samples, _loader(2, 1)):
        assert img.dtype == np.float32 and img.shape == (3, 129, 129)
        assert lab.dtype == np.int64 and lab.shape == (129, 129) and prd.dtype == np.int64 and prd.shape == (129, 129)
        np.testing.assert_array_equal(img, img_ref[0].numpy())
        np.testing.assert_array_equal(lab, lab_ref[0].numpy())
        mask = (lab >= 0) & (lab < N_CLASSES)
        hist += np.bincount(N_CLASSES * lab[mask] + prd[mask], minlength=N_CLASSES * N_CLASSES)
    np.testing.assert_array_equal(hist.reshape(N_CLASSES, N_CLASSES), metrics.confusion_matrix.cpu().numpy().astype(np.int64))
    _, _, none = trainer.validate(_loader(2, 1), metrics, ret_samples_ids=[5])
    assert none == []


def test_trainer_test_renders_into_a_sink(tmp_path):
    """Trainer.test with a save_samples sink: five files per image; NNNNpre.png read back, with NNNNgt.png, gives the confusion matrix
    (it is the map the matrix was built from); NNNNpre_clo.png is cmap[pre]; NNNNgt.png is the labels.  Without a sink: the
    reference's 4-tuples, one per image."""
    from PIL import Image
    from ucd_amd import visual
    from ucd_amd.metrics import StreamSegMetrics
    from ucd_amd.train import Trainer
    model, model_old, classes, dev = _models()
    trainer = Trainer(model, None, device=dev, opts=_opts(["--method", "UCD"]), classes=classes)
    metrics = StreamSegMetrics(N_CLASSES)
    sink = visual.SampleWriter(str(tmp_path / "predictions"))
    (class_loss, reg_loss), score, samples = trainer.test(_loader(3, 2), metrics, sink=sink)
    assert samples == [] and sink.count == 3 and score["Total samples"] == 3 and reg_loss.item() == 0.0 and class_loss.item() > 0
    names = sorted(os.listdir(tmp_path / "predictions"))
    assert names == sorted(f"{k:04d}{s}" for k in range(3) for s in ("pre.png", "gt.png", "pre_clo.png", "gt_clo.png", "rgb.jpg"))
    cmap = visual.color_map("voc")
    read = lambda k, s: np.asarray(Image.open(tmp_path / "predictions" / f"{k:04d}{s}"))
    labels = torch.cat([lab for _, lab in _loader(3, 2)]).numpy()
    hist = np.zeros(N_CLASSES * N_CLASSES, dtype=np.int64)
    for k in range(3):
        pre, gt = read(k, "pre.png"), read(k, "gt.png")
        assert pre.dtype == np.uint8 and pre.shape == (129, 129)
        np.testing.assert_array_equal(gt, labels[k].astype(np.uint8))
        np.testing.assert_array_equal(read(k, "pre_clo.png"), cmap[pre])
        np.testing.assert_array_equal(read(k, "gt_clo.png"), cmap[gt])
        assert read(k, "rgb.jpg").shape == (129, 129, 3)
        mask = gt < N_CLASSES
        hist += np.bincount(N_CLASSES * gt[mask].astype(np.int64) + pre[mask], minlength=N_CLASSES * N_CLASSES)
    np.testing.assert_array_equal(hist.reshape(N_CLASSES, N_CLASSES), metrics.confusion_matrix.cpu().numpy().astype(np.int64))
    # no sink: (image, label, prediction, att) per image, the predictions again those of the confusion matrix
    _, _, tuples = trainer.test(_loader(3, 2), metrics)
    assert len(tuples) == 3
    hist[:] = 0
    for k, (img, lab, prd, att) in enumerate(tuples):
        assert img.shape == (3, 129, 129) and img.dtype == np.float32 and att.shape == (129, 129) and att.dtype == np.float32
        assert lab.dtype == np.int64 and prd.dtype == np.int64 and prd.shape == (129, 129)
        np.testing.assert_array_equal(lab, labels[k])
        assert np.isfinite(att).all() and att.min() >= 0
        mask = (lab >= 0) & (lab < N_CLASSES)
        hist += np.bincount(N_CLASSES * lab[mask] + prd[mask], minlength=N_CLASSES * N_CLASSES)
    np.testing.assert_array_equal(hist.reshape(N_CLASSES, N_CLASSES), metrics.confusion_matrix.cpu().numpy().astype(np.int64))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def test_drivers_step_policy_samples_and_evaluate(tmp_path, monkeypatch):
    """ucd_amd.run.main with --lr_policy step --lr_decay_step 1 on the synthetic data: one epoch of 8 iterations ends with
    lr = lr0 * factor^8 in every parameter group; --sample_num 2 leaves two image | target | prediction strips of the epoch; the
    checkpoint it wrote goes through ucd_amd.evaluate.main, which leaves five files per test image and a score table."""
    from PIL import Image
    from ucd_amd import evaluate, run
    monkeypatch.chdir(tmp_path)
    for k, v in (("MASTER_ADDR", "127.0.0.1"), ("RANK", "0"), ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0")):
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("MASTER_PORT", _free_port())
    args = ["--method", "FT", "--task", "15-5", "--step", "0", "--no_pretrained", "--norm_act", "iabn_sync", "--opt_level", "O1",
            "--data_root", "synthetic", "--lr", "0.01", "--lr_policy", "step", "--lr_decay_step", "1", "--lr_decay_factor", "0.5",
            "--epochs", "1", "--batch_size", "24", "--crop_size", "129", "--sample_num", "2", "--logdir", str(tmp_path / "logs"),
            "--name", "drv"]
    opts = argparser.modify_command_options(argparser.get_argparser().parse_args(args))
    assert opts.sample_num == 2
    made = []
    make = run.make_optimizer
    monkeypatch.setattr(run, "make_optimizer", lambda o, m: made.append(make(o, m)) or made[-1])
    run.main(opts)
    iters = 24 * 8 // 24
    assert len(made) == 1
    for group in made[0].param_groups:
        assert group["lr"] == pytest.approx(0.01 * 0.5 ** iters, rel=1e-6)
    strips = sorted(os.listdir(tmp_path / "logs" / "15-5-voc" / "drv" / "samples" / "epoch_0"))
    assert strips == ["sample_0.png", "sample_1.png"]
    assert np.asarray(Image.open(tmp_path / "logs" / "15-5-voc" / "drv" / "samples" / "epoch_0" / strips[0])).shape == (129, 3 * 129, 3)
    ckpt = tmp_path / "checkpoints" / "step" / "15-5-voc_drv_0.pth"
    assert ckpt.exists()
    monkeypatch.setenv("MASTER_PORT", _free_port())
    opts = argparser.modify_command_options(argparser.get_argparser().parse_args(args + ["--step_ckpt", str(ckpt)]))
    _, score = evaluate.main(opts)
    assert 0.0 <= score["Mean IoU"] <= 1.0 and score["Total samples"] == 48
    files = os.listdir(tmp_path / "logs" / "15-5-voc" / "drv" / "predictions")
    assert len(files) == 5 * 48 and "0047pre_clo.png" in files
