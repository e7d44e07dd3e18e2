"""Regenerates tests/golden/kd_losses.npz, lwf_step.npz and ilt_step.npz by driving the REFERENCE's own distillation losses
(utils/loss.py, loaded by file path: it needs torch only) and, for the whole-step files, its model classes (imported as
make_goldens.py does).  Only arrays are stored; the inputs come from ucd_amd.synth, seeded, and the tests rebuild them.

    python tests/golden/make_kd_golden.py          # writes the .npz files next to this script
    python tests/golden/make_kd_golden.py unit     # kd_losses.npz only (seconds; the whole-step ones take minutes)

kd_losses.npz (:func:`unit`).  For every shape of UNIT_SHAPES, KD in {plain, unbiased}, alpha in ALPHAS and CE in {plain,
unbiased}: float64 low-resolution logits, ``F.interpolate(bilinear, align_corners=False)`` to the label size, the reference's
``nn.CrossEntropyLoss`` / ``UnbiasedCrossEntropy`` (reduction 'none', then ``.mean()``: train.py:116) and
``KnowledgeDistillationLoss`` / ``UnbiasedKnowledgeDistillationLoss``; stored are (ce, kd) and the gradient of
``UNIT_CE_W * ce + UNIT_KD_W * kd`` with respect to the LOW-resolution student logits, as float32 (the comparison bounds are
1e-6 and looser; float64 would double a file that has to stay small) and through make_goldens.compact(): the largest shape
is stored as sums, row sums and samples (conftest.assert_matches_compact compares either kind).

lwf_step.npz / ilt_step.npz (:func:`whole_step`): VOC 15-5 step 1 on 2 x 129^2, three iterations of the reference's
train.py:95-151 loop on one batch with the ``--method LWF`` / ``--method ILT`` presets (argparser.py:18-25: loss_kd = 100,
ILT also loss_de = 100; plain cross entropy, plain KD, alpha 1); the contrastive term is part of every step with a teacher
(train.py:116).  Recorded like regularizer_step_*.npz: per-iteration ce / con / lkd / lde and the first 16 elements of the
WS_NAMES parameters before and after, plus the new head's random initial values.
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

UNIT_SHAPES = [(2, 21, 16, 9, 129), (2, 20, 14, 12, 190), (2, 41, 27, 11, 173)]       # B, Ctot, K, h, H
ALPHAS = (1.0, 0.5, 2.0)
UNIT_CE_W, UNIT_KD_W = 1.0, 10.0
PRESETS = {"lwf": (100.0, 0.0), "ilt": (100.0, 100.0)}          # loss_kd, loss_de


def unit_key(shape, kd, alpha, ce):
    return "x".join(str(v) for v in shape) + f"|{kd}|{alpha:g}|{ce}"


def unit_inputs(shape):
    """(student logits [B, Ctot, h, h], teacher logits [B, K, h, h], labels [B, H, H]) of one shape, float32 / int64."""
    from ucd_amd import synth
    B, Ctot, K, h, H = shape
    seed = 8100 + Ctot + h
    sem = synth.t_normal(seed, (B, Ctot, h, h), stream=1, scale=2.0)
    sem_t = synth.t_normal(seed, (B, K, h, h), stream=2, scale=2.0)
    labels = synth.seg_labels(seed, B, H, H, range(K, Ctot), rects=4)
    # old-class ids as well: the plain cross entropy scores them as themselves, the unbiased one as background
    old = torch.from_numpy(synth.randint(seed, (B, H, H), 1, K, stream=7))
    pick = torch.from_numpy(synth.randint(seed, (B, H // 8 + 1, H // 8 + 1), 0, 4, stream=8))
    pick = pick.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :H]
    labels = torch.where((pick == 0) & (labels == 0), old, labels)
    return sem, sem_t, labels


def unit(ref_loss):
    from make_goldens import compact
    out = {}
    for shape in UNIT_SHAPES:
        B, Ctot, K, h, H = shape
        sem, sem_t, labels = unit_inputs(shape)
        up = lambda t: F.interpolate(t, size=(H, H), mode="bilinear", align_corners=False)
        t_up = up(sem_t.double())
        for kd in ("plain", "unbiased"):
            for alpha in ALPHAS:
                for ce in ("plain", "unbiased"):
                    s = sem.double().requires_grad_(True)
                    u = up(s)
                    crit = (nn.CrossEntropyLoss(ignore_index=255, reduction="none") if ce == "plain" else
                            ref_loss.UnbiasedCrossEntropy(old_cl=K, ignore_index=255, reduction="none"))
                    l_ce = crit(u, labels.clone()).mean()
                    mod = ref_loss.KnowledgeDistillationLoss if kd == "plain" else ref_loss.UnbiasedKnowledgeDistillationLoss
                    l_kd = mod(alpha=alpha)(u, t_up)
                    (UNIT_CE_W * l_ce + UNIT_KD_W * l_kd).backward()
                    key = unit_key(shape, kd, alpha, ce)
                    out[key + "|loss"] = np.array([l_ce.item(), l_kd.item()])
                    out.update(compact(key + "|grad", s.grad.numpy().astype(np.float32)))
    return out


def whole_step(ref_loss, name):
    from functools import partial
    import make_goldens as MG
    from make_regularizer_golden import WS_CROP, WS_ITERS, WS_NAMES, WS_SEED
    from ucd_amd import synth
    models, modules, segm = MG.import_reference_model()
    norm = partial(MG.ShimInPlaceABN, activation="leaky_relu", activation_param=0.01)
    loss_kd, loss_de = PRESETS[name]

    def build(cls):
        body = models.net_resnet101(norm_act=norm, output_stride=16)
        head = modules.DeeplabV3(body.out_channels, 256, 256, norm_act=norm, out_stride=16, pooling_size=32)
        return segm.IncrementalSegmentationModule(body, head, 256, classes=cls)

    torch.manual_seed(0)
    student, teacher = build([16, 5]), build([16])
    sd = synth.fill_state_dict(teacher.state_dict(), 42, calibrated=True)
    teacher.load_state_dict(sd)
    student.load_state_dict(sd, strict=False)
    for p in teacher.parameters():
        p.requires_grad = False
    teacher.eval(); student.train()
    params = dict(student.named_parameters())
    out = {"cls1_weight_init": params["cls.1.weight"].detach().numpy().copy(),
           "cls1_bias_init": params["cls.1.bias"].detach().numpy().copy()}
    groups = [{"params": [p for p in m.parameters() if p.requires_grad], "weight_decay": 1e-4}
              for m in (student.body, student.head, student.cls)]
    opt = torch.optim.SGD(groups, lr=1e-3, momentum=0.9, nesterov=True)
    img = synth.images(WS_SEED, 2, WS_CROP)
    labels = synth.seg_labels(WS_SEED, 2, WS_CROP, WS_CROP, range(16, 21))
    before = {n: params[n].detach().flatten()[:16].numpy().copy() for n in WS_NAMES}
    with torch.no_grad():
        out_old, feat_old = teacher(img, ret_intermediate=True)
    mse = nn.MSELoss()
    rec = {"ce": [], "con": [], "lkd": [], "lde": []}
    for it in range(WS_ITERS):
        opt.zero_grad()
        outp, feat = student(img, x_b_old=feat_old["body"], x_pl_old=feat_old["pre_logits"], ret_intermediate=True)
        a, c, la, lc, P = ref_loss.pre_contrastive_pixel(feat["pre_logits"], labels.clone(), l_po=feat_old["sem"],
                                                         f_o=feat_old["pre_logits"])
        ce = nn.CrossEntropyLoss(ignore_index=255, reduction="none")(outp, labels.clone()).mean()
        con = ref_loss.PixelConLossV2(temperature=0.07)(a, c, la, lc, P)
        lkd = loss_kd * ref_loss.KnowledgeDistillationLoss(alpha=1.0)(outp, out_old)
        lde = torch.zeros(())
        if loss_de > 0:
            lde = loss_de * (mse(feat["body"], feat_old["body"]) + mse(feat["pre_logits"], feat_old["pre_logits"]))
        (ce + con / 100 + lkd + lde).backward()
        opt.step()
        for k, v in (("ce", ce), ("con", con), ("lkd", lkd), ("lde", lde)):
            rec[k].append(v.item())
        print(f"{name} step {it}: " + " ".join(f"{k} {v[-1]:.6f}" for k, v in rec.items()), flush=True)
    out.update({k: np.array(v) for k, v in rec.items()})
    for n in WS_NAMES:
        out["before|" + n] = before[n]
        out["after|" + n] = params[n].detach().flatten()[:16].numpy().copy()
    return out


def main():
    import make_goldens as MG
    torch.set_num_threads(8)
    np.savez_compressed(os.path.join(HERE, "kd_losses.npz"), **unit(MG.ref_loss))
    print("kd_losses.npz: %.1f KiB" % (os.path.getsize(os.path.join(HERE, "kd_losses.npz")) / 1024))
    if len(sys.argv) > 1 and sys.argv[1] == "unit":
        return
    for name in PRESETS:
        np.savez(os.path.join(HERE, f"{name}_step.npz"), **whole_step(MG.ref_loss, name))
        print(f"{name}_step.npz written")


if __name__ == "__main__":
    sys.exit(main())
