"""Regenerates tests/golden/bce_losses.npz and lwfmc_step.npz by driving the REFERENCE's own BCE losses (utils/loss.py, loaded by
file path: it needs torch only) and, for the whole-step file, its model classes (imported as make_goldens.py does).  Only arrays
are stored; the inputs come from ucd_amd.synth, seeded, and the tests rebuild them.

    python tests/golden/make_bce_golden.py          # writes both .npz files next to this script
    python tests/golden/make_bce_golden.py unit     # bce_losses.npz only (seconds; the whole-step one takes minutes)

bce_losses.npz (:func:`unit`).  For every shape of make_kd_golden.UNIT_SHAPES, on make_kd_golden.unit_inputs with about 10 % of
the labels set to 255 (:func:`unit_labels`): float64 low-resolution logits, ``F.interpolate(bilinear, align_corners=False)`` to the
label size, the reference's ``BCEWithLogitsLossWithIgnoreIndex(reduction='none')(u, y).mean()`` (train.py:112/116) and
``K * nn.BCEWithLogitsLoss()(u[:, :K], sigmoid(t_up))`` (train.py:119-124 without icarl_importance); stored are the two values and
the gradient of ``UNIT_HARD_W * bce + UNIT_SOFT_W * soft`` with respect to the LOW-resolution student logits, as float32 and
through make_goldens.compact() (the largest shape is stored as sums, row sums and samples).  The reference casts its one-hot
targets to float32 (``.float()``) inside a float64 evaluation: that cast is the floor of any comparison with these numbers.

lwfmc_step.npz (:func:`whole_step`): VOC 15-5 step 1 on 2 x 129^2, three iterations of the reference's train.py:95-151 loop on one
batch with the ``--method LWF-MC`` preset (argparser.py: icarl, icarl_importance 10; BCE criterion, no KD) at ``--lr`` WS_LR: make_kd_golden's
restatement of the loop plus train.py:119-124.  Recorded like lwf_step.npz: per-iteration ce / con / icarl and the first 16
elements of the WS_NAMES parameters before and after, plus the new head's random initial values.
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

UNIT_HARD_W, UNIT_SOFT_W = 1.0, 10.0
ICARL_IMPORTANCE = 10.0
# The learning rate of the whole-step run.  lwf_step.npz uses 1e-3 on a total loss of ~20; the LWF-MC total is ~119 (the iCaRL term
# alone 106), so the same rate moves the parameters ~6 times as far per iteration, and a three-iteration trajectory on 2 x 81
# low-resolution cells of batch statistics then amplifies the summation-order noise of ANY two fp32 implementations to about the
# 1e-3 the comparison allows.  1e-3 * 20 / 119, rounded up: the per-iteration movement of the LWF golden.
WS_LR = 2e-4


def unit_key(shape):
    return "x".join(str(v) for v in shape)


def unit_labels(shape, labels):
    """make_kd_golden.unit_inputs' labels with 255 in 8 x 8 blocks over about a tenth of the map."""
    from ucd_amd import synth
    B, Ctot, K, h, H = shape
    pick = torch.from_numpy(synth.randint(8100 + Ctot + h, (B, H // 8 + 1, H // 8 + 1), 0, 10, stream=9))
    pick = pick.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :H]
    return torch.where(pick == 0, torch.full_like(labels, 255), labels)


def unit(ref_loss):
    from make_goldens import compact
    from make_kd_golden import UNIT_SHAPES, unit_inputs
    out = {}
    for shape in UNIT_SHAPES:
        B, Ctot, K, h, H = shape
        sem, sem_t, labels = unit_inputs(shape)
        labels = unit_labels(shape, labels)
        up = lambda t: F.interpolate(t, size=(H, H), mode="bilinear", align_corners=False)
        t_up = up(sem_t.double())
        s = sem.double().requires_grad_(True)
        u = up(s)
        l_bce = ref_loss.BCEWithLogitsLossWithIgnoreIndex(reduction="none")(u, labels.clone()).mean()
        l_soft = K * nn.BCEWithLogitsLoss(reduction="mean")(u.narrow(1, 0, K), torch.sigmoid(t_up))
        (UNIT_HARD_W * l_bce + UNIT_SOFT_W * l_soft).backward()
        key = unit_key(shape)
        out[key + "|loss"] = np.array([l_bce.item(), l_soft.item()])
        out[key + "|ignored"] = np.array((labels == 255).double().mean().item())
        out.update(compact(key + "|grad", s.grad.numpy().astype(np.float32)))
        print(f"{key}: bce {l_bce.item():.6f} soft {l_soft.item():.6f} ignored {out[key + '|ignored']:.3f}", flush=True)
    return out


def whole_step(ref_loss):
    from functools import partial
    import make_goldens as MG
    from make_regularizer_golden import WS_CROP, WS_ITERS, WS_NAMES, WS_SEED
    from ucd_amd import synth
    models, modules, segm = MG.import_reference_model()
    norm = partial(MG.ShimInPlaceABN, activation="leaky_relu", activation_param=0.01)

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
    opt = torch.optim.SGD(groups, lr=WS_LR, momentum=0.9, nesterov=True)
    img = synth.images(WS_SEED, 2, WS_CROP)
    labels = synth.seg_labels(WS_SEED, 2, WS_CROP, WS_CROP, range(16, 21))
    before = {n: params[n].detach().flatten()[:16].numpy().copy() for n in WS_NAMES}
    with torch.no_grad():
        out_old, feat_old = teacher(img, ret_intermediate=False)
    criterion = ref_loss.BCEWithLogitsLossWithIgnoreIndex(reduction="none")
    licarl = nn.BCEWithLogitsLoss(reduction="mean")
    rec = {"ce": [], "con": [], "icarl": []}
    for it in range(WS_ITERS):
        opt.zero_grad()
        outp, feat = student(img, x_b_old=feat_old["body"], x_pl_old=feat_old["pre_logits"], ret_intermediate=False)
        a, c, la, lc, P = ref_loss.pre_contrastive_pixel(feat["pre_logits"], labels.clone(), l_po=feat_old["sem"],
                                                         f_o=feat_old["pre_logits"])
        ce = criterion(outp, labels.clone()).mean()
        con = ref_loss.PixelConLossV2(temperature=0.07)(a, c, la, lc, P)
        n_cl_old = out_old.shape[1]
        icarl = ICARL_IMPORTANCE * n_cl_old * licarl(outp.narrow(1, 0, n_cl_old), torch.sigmoid(out_old))
        (ce + con / 100 + icarl).backward()
        opt.step()
        for k, v in (("ce", ce), ("con", con), ("icarl", icarl)):
            rec[k].append(v.item())
        print(f"lwfmc step {it}: " + " ".join(f"{k} {v[-1]:.6f}" for k, v in rec.items()), flush=True)
    out.update({k: np.array(v) for k, v in rec.items()})
    for n in WS_NAMES:
        out["before|" + n] = before[n]
        out["after|" + n] = params[n].detach().flatten()[:16].numpy().copy()
    return out


def main():
    import make_goldens as MG
    torch.set_num_threads(8)
    np.savez_compressed(os.path.join(HERE, "bce_losses.npz"), **unit(MG.ref_loss))
    print("bce_losses.npz: %.1f KiB" % (os.path.getsize(os.path.join(HERE, "bce_losses.npz")) / 1024))
    if len(sys.argv) > 1 and sys.argv[1] == "unit":
        return
    np.savez(os.path.join(HERE, "lwfmc_step.npz"), **whole_step(MG.ref_loss))
    print("lwfmc_step.npz written")


if __name__ == "__main__":
    sys.exit(main())
