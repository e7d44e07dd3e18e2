"""Regenerates tests/golden/regularizer_{ewc,pi,rw}.npz by driving the REFERENCE's own regularisers
(utils/regularizer.py, loaded by file path: it needs torch only) on a small seeded model.  Only arrays are stored.

    python tests/golden/make_regularizer_golden.py          # writes the .npz files next to this script
    python tests/golden/make_regularizer_golden.py unit     # the unit goldens only (seconds; the whole-step ones take minutes)

The model is wrapped like the reference's DistributedDataParallel student (``module.`` keys): a 4-D convolution weight,
an ABN weight and bias of odd size (13: the kernel's scalar tail), a frozen parameter and a "new head" absent from the old
model.  The inputs (parameters, previous-step state, gradients and parameter moves) come from :func:`inputs`, seeded, which
the tests call as well; the files hold the outputs.  Two scenarios per method:

* ``s1``: step > 0 - a teacher (the old model; the student starts at teacher + noise) and a seeded previous-step state;
* ``s0``: step 0 - no teacher, no previous state (no penalty; the state is still updated).

Each of ITERS iterations follows train.py:135-145: seeded ``p.grad``, ``update()``, ``reg_importance * penalty()``
back-propagated when non-zero, then a seeded move of the parameters.  Recorded: the penalty, every gradient after the
penalty's backward, every state array, and the final ``state_dict()``.  RW runs with iterations = 2 so its score branch
fires more than once.  The reference's EWC.update raises TypeError on a parameter without a gradient (``p.grad ** 2``);
it is driven through a view of the model that lists only parameters with a gradient, which is the behaviour this
project implements (frozen parameters are skipped).

Whole-step goldens, regularizer_step_{ewc,pi,rw}.npz (:func:`whole_step`): VOC 15-5 step 1 on 2 x 129^2, three iterations
of the reference's train.py:95-151 loop on one batch through its own model classes (imported as make_goldens.py does), the
previous-step state closed-form from ucd_amd.synth (:func:`prev_state`).  Stored: per-iteration ce / con / l_reg, the first
16 elements and the abs-sum of the state of a few parameters, the first 16 elements of those parameters before and after,
and the new head's random initial values.
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
ITERS = 6
LAMBDA = {"ewc": 500.0, "pi": 500.0, "rw": 100.0}          # the --method presets (argparser.py)
SEP = "|"


def load_reference_regularizer():
    spec = importlib.util.spec_from_file_location("ref_regularizer", os.path.join(REF, "utils/regularizer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SHAPES = {"conv.weight": (8, 8, 3, 3), "abn.weight": (13,), "abn.bias": (13,), "frozen.weight": (3, 13),
          "head.weight": (5, 13, 1, 1)}
OLD_KEYS = ["conv.weight", "abn.weight", "abn.bias", "frozen.weight"]          # the new head is absent from the old model


def make_net(values, with_head):
    net = nn.Module()
    for key, shape in SHAPES.items():
        if key == "head.weight" and not with_head:
            continue
        mod_name, attr = key.split(".")
        if not hasattr(net, mod_name):
            net.add_module(mod_name, nn.Module())
        p = nn.Parameter(values[key].clone(), requires_grad=key != "frozen.weight")
        getattr(net, mod_name).register_parameter(attr, p)
    return net


class Wrapped(nn.Module):
    def __init__(self, net):
        super().__init__()
        self.module = net


class WithGrad:
    """The model as the reference's EWC.update sees it, minus parameters without a gradient."""

    def __init__(self, model):
        self.m = model

    def named_parameters(self):
        return ((n, p) for n, p in self.m.named_parameters() if p.grad is not None)

    def state_dict(self):
        return self.m.state_dict()


class Opts:
    def __init__(self, name):
        self.regularizer, self.reg_importance, self.reg_alpha = name, LAMBDA[name], 0.9
        self.reg_no_normalize, self.reg_iterations = False, 2      # RW: score updates at iterations 2, 4, ...


def inputs(name, scen):
    """Seeded inputs of one scenario: teacher / student values, previous-step state ({array: {"module." key: tensor}} or
    None), per-iteration gradients of the trainable parameters and parameter moves (keys without the prefix)."""
    gen = torch.Generator().manual_seed(1234 + 10 * ["ewc", "pi", "rw"].index(name) + (scen == "s1"))
    teacher_vals = {k: torch.randn(SHAPES[k], generator=gen) * 0.1 for k in SHAPES}
    student_vals = {k: (teacher_vals[k] + torch.randn(SHAPES[k], generator=gen) * 0.01) if scen == "s1" else teacher_vals[k]
                    for k in SHAPES}
    old_state = None
    if scen == "s1":
        old_state = {"name": name}
        for a in (["fisher"] if name == "ewc" else ["score"] if name == "pi" else ["fisher", "score"]):
            old_state[a] = {"module." + k: torch.randn(SHAPES[k], generator=gen).abs() * (3.0 if a == "score" else 0.5)
                            for k in OLD_KEYS}
    grads = [{k: torch.randn(SHAPES[k], generator=gen) * 0.1 for k in SHAPES if k != "frozen.weight"} for _ in range(ITERS)]
    steps = [{k: torch.randn(SHAPES[k], generator=gen) * 0.01 for k in SHAPES} for _ in range(ITERS)]
    return teacher_vals, student_vals, old_state, grads, steps


def scenario(ref, name, scen, out):
    pre = f"{scen}{SEP}"
    teacher_vals, student_vals, old_state, grads, steps = inputs(name, scen)
    student = Wrapped(make_net(student_vals, True))
    teacher = Wrapped(make_net(teacher_vals, False)) if scen == "s1" else None
    # the reference's objects take the old state by reference and modify it: hand them copies
    state_arg = None if old_state is None else {a: ({k: v.clone() for k, v in d.items()} if isinstance(d, dict) else d)
                                                 for a, d in old_state.items()}
    reg = ref.get_regularizer(student, teacher, torch.device("cpu"), Opts(name), state_arg)
    if name == "ewc":
        reg.model = WithGrad(student)
    lam = LAMBDA[name]
    for t in range(ITERS):
        for n, p in student.named_parameters():
            p.grad = grads[t][n[len("module."):]].clone() if p.requires_grad else None
        reg.update()
        l_reg = lam * reg.penalty()
        if l_reg != 0.:
            l_reg.backward()
        out[pre + "penalty" + SEP + str(t)] = np.float64(float(l_reg.detach()) if torch.is_tensor(l_reg) else l_reg)
        for n, p in student.named_parameters():
            if p.grad is not None:
                out[pre + f"grad{t}" + SEP + n[len("module."):]] = p.grad.numpy().copy()
        states = {"fisher": reg.fisher} if name == "ewc" else {"delta": reg.delta} if name == "pi" else \
            {"fisher": reg.fisher, "score": reg.score}
        for a, d in states.items():
            for n, v in d.items():
                out[pre + f"{a}{t}" + SEP + n[len("module."):]] = v.detach().numpy().copy()
        with torch.no_grad():
            for n, p in student.named_parameters():
                p.add_(steps[t][n[len("module."):]])
    sd = reg.state_dict()
    for a, v in sd.items():
        if isinstance(v, dict):
            out[pre + "sdkeys" + SEP + a] = np.array(sorted(v.keys()))
            for n, x in v.items():
                out[pre + "sd" + SEP + a + SEP + n] = x.detach().numpy().copy()
        else:
            out[pre + "sd" + SEP + a] = np.array(v)


# ---- whole-step goldens: the reference's train.py:95-151 loop with the regulariser -------------------------------------
WS_ITERS = 3
WS_SEED, WS_CROP = 501, 129
WS_NAMES = ["body.mod1.conv1.weight", "body.mod3.block2.convs.bn2.weight", "body.mod5.block3.convs.conv3.weight",
            "head.map_convs.2.weight", "head.red_bn.bias", "cls.1.weight", "cls.1.bias"]
WS_ARRAYS = {"ewc": ("fisher",), "pi": ("delta",), "rw": ("fisher", "score")}


def prev_state(name, shapes, prefix="module."):
    """Closed-form previous-step regulariser state over the teacher's parameters ``shapes`` ({name: shape}): |N(0, 1)| * 0.5
    (Fisher) or * 3 (score), from ucd_amd.synth, keyed ``prefix + name`` (the reference's checkpoints carry ``module.``)."""
    import zlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from ucd_amd import synth
    arrays = {"ewc": ["fisher"], "pi": ["score"], "rw": ["fisher", "score"]}[name]
    state = {"name": name}
    for a in arrays:
        scale, stream = (0.5, 3000) if a == "fisher" else (3.0, 5000)
        state[a] = {prefix + k: torch.from_numpy(np.abs(synth.normal(7, tuple(shp), stream=stream + (zlib.crc32(k.encode()) & 0xFFFF)))
                                                 .astype(np.float32) * np.float32(scale)).reshape(tuple(shp))
                    for k, shp in shapes.items()}
    return state


def whole_step(ref, name):
    """VOC 15-5 step 1, 2 x 129^2, WS_ITERS iterations on one batch: CE + contrastive / 100, backward, update(),
    reg_importance * penalty() back-propagated when non-zero, SGD-Nesterov (lr 1e-3, wd 1e-4) in the three groups.  The
    teacher / student come from the CALIBRATED synthetic step-0 checkpoint (synth.fill_state_dict, seed 42: the uncalibrated one
    has teacher logits of order 1e5, on which two fp32 implementations part by percent after one SGD step); --init_balanced is off for
    these methods, so the new head keeps its random initial values, which are stored."""
    from functools import partial
    sys.path.insert(0, HERE)
    import make_goldens as MG
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
    state = prev_state(name, {k: v.shape for k, v in teacher.named_parameters()}, prefix="")   # the models are not wrapped here
    reg = ref.get_regularizer(student, teacher, torch.device("cpu"), Opts(name), state)
    if name == "ewc":
        reg.model = WithGrad(student)
    groups = [{"params": [p for p in m.parameters() if p.requires_grad], "weight_decay": 1e-4}
              for m in (student.body, student.head, student.cls)]
    opt = torch.optim.SGD(groups, lr=1e-3, momentum=0.9, nesterov=True)
    img = synth.images(WS_SEED, 2, WS_CROP)
    labels = synth.seg_labels(WS_SEED, 2, WS_CROP, WS_CROP, range(16, 21))
    before = {n: params[n].detach().flatten()[:16].numpy().copy() for n in WS_NAMES}
    with torch.no_grad():
        _, feat_old = teacher(img)
    rec = {"ce": [], "con": [], "l_reg": []}
    for it in range(WS_ITERS):
        opt.zero_grad()
        outp, feat = student(img)
        a, c, la, lc, P = MG.ref_loss.pre_contrastive_pixel(feat["pre_logits"], labels.clone(), l_po=feat_old["sem"],
                                                            f_o=feat_old["pre_logits"])
        ce = nn.CrossEntropyLoss(ignore_index=255, reduction="none")(outp, labels.clone()).mean()
        con = MG.ref_loss.PixelConLossV2(temperature=0.07)(a, c, la, lc, P)
        (ce + con / 100).backward()
        reg.update()
        l_reg = LAMBDA[name] * reg.penalty()
        if l_reg != 0.:
            l_reg.backward()
        opt.step()
        rec["ce"].append(ce.item()); rec["con"].append(con.item())
        rec["l_reg"].append(float(l_reg.detach()) if torch.is_tensor(l_reg) else float(l_reg))
        print(f"{name} step {it}: ce {rec['ce'][-1]:.6f} con {rec['con'][-1]:.6f} l_reg {rec['l_reg'][-1]:.6f}", flush=True)
    out.update({k: np.array(v) for k, v in rec.items()})
    for n in WS_NAMES:
        out["before|" + n] = before[n]
        out["after|" + n] = params[n].detach().flatten()[:16].numpy().copy()
        for a in WS_ARRAYS[name]:
            v = getattr(reg, a)[n].detach()
            out[f"{a}|{n}"] = v.flatten()[:16].numpy().copy()
            out[f"{a}_abs|{n}"] = np.float64(v.double().abs().sum())
    return out


def main():
    torch.set_num_threads(1)
    ref = load_reference_regularizer()
    for name in ["ewc", "pi", "rw"]:
        out = {}
        for scen in ("s1", "s0"):
            scenario(ref, name, scen, out)
        np.savez(os.path.join(HERE, f"regularizer_{name}.npz"), **out)
        print(f"regularizer_{name}.npz: {len(out)} arrays")
    if len(sys.argv) > 1 and sys.argv[1] == "unit":
        return
    torch.set_num_threads(8)
    for name in ["ewc", "pi", "rw"]:
        np.savez(os.path.join(HERE, f"regularizer_step_{name}.npz"), **whole_step(ref, name))
        print(f"regularizer_step_{name}.npz written")


if __name__ == "__main__":
    sys.exit(main())
