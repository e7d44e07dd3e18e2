"""CPU: the host half of Local POD feature distillation (``--pod_factor``; csrc/pod.hip, ucd_amd.loss.fused_local_pod) - the plan,
the library's refusals on host buffers, the torch composition against the float64 reference (tests/pod_ref.py), the command line
and a Trainer step on a small CPU network."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import pod_ref
from ucd_amd import argparser, hip, switches
from ucd_amd.loss import fused_local_pod, local_pod_torch

GEOMETRIES = [((33, 33, 256), (1, 2, 4)), ((129, 129, 256), (1, 2, 4)), ((9, 9, 64), (1, 2, 4)), ((7, 11, 72), (1, 2, 4)),
              ((9, 9, 64), (1, 3))]


def test_names_are_registered():
    assert {"ucd_pod_plan", "ucd_pod_forward", "ucd_pod_backward"} <= set(hip.SIGNATURES)
    assert switches.DEFAULTS["UCD_FUSED_POD"] == "1" and "UCD_FUSED_POD" in switches.snapshot()


@pytest.mark.parametrize("geom,scales", GEOMETRIES)
def test_plan_counts_the_embedding(geom, scales):
    h, w, Cc = geom
    plan = hip.pod_plan(h, w, Cc, scales, B=2)
    assert plan["n_E"] == sum(s * s * Cc * (h // s + w // s) for s in scales) == pod_ref.n_embed(Cc, h, w, scales)
    tiles, chunks, nrs, ncs = plan["grid"]
    # every row / column piece lies inside one region of every scale and is at most 8 rows / 16 columns long
    assert nrs >= math.ceil(h / 8) and ncs >= math.ceil(w / 16)
    assert tiles == math.ceil(2 * nrs * ncs * (Cc // 8) / 256) and 1 <= chunks <= 256
    # the workspace holds at least the two sets of pooled strips
    assert plan["workspace_bytes"] >= 2 * 2 * plan["n_E"] * 4


def test_plan_of_the_non_nested_geometry():
    # (7, 11): kh = 7, 3, 1 and kw = 11, 5, 2 - row 6 is outside scale 2, columns 10 / 8.. outside scales 2 / 4
    plan = hip.pod_plan(7, 11, 72, (1, 2, 4))
    assert plan["n_E"] == 72 * (1 * (7 + 11) + 4 * (3 + 5) + 16 * (1 + 2))
    # row pieces: cut at 0,1,2,3,4,6,7 (scale 4: every row up to 4; scale 2: 3 and 6)
    assert plan["grid"][2] == 6
    # column pieces: cut at 0,2,4,5,6,8,10,11
    assert plan["grid"][3] == 7


def _host(n, dtype=np.float32):
    return np.zeros(n, dtype=dtype)


def _forward_rc(x_s="ok", x_t="ok", ld=8, dtype=hip.F32, B=1, Cc=8, h=4, w=4, slope=1.0, scales=(1, 2, 4), n=None, out="ok", g="ok",
                ws="ok", ws_bytes=None):
    lib = hip.load()
    buf = _host(4096)                       # host memory: a call that got past its checks would fault, a refusal never touches it
    p = lambda v: buf.ctypes.data if isinstance(v, str) else v
    arr = (C.c_int * 8)(*scales) if scales is not None else None
    nb = (1 << 20) if ws_bytes is None else ws_bytes
    return lib.ucd_pod_forward(p(x_s), ld, p(x_t), ld, dtype, B, Cc, h, w, slope, C.cast(arr, C.c_void_p) if arr is not None else None,
                               len(scales) if n is None else n, 1.0, p(out), p(g), p(ws), nb, None)


def _backward_rc(x="ok", ld=8, dtype=hip.F32, B=1, Cc=8, h=4, w=4, slope=1.0, scales=(1, 2, 4), g="ok", go="ok", d="ok"):
    lib = hip.load()
    buf = _host(4096)
    p = lambda v: buf.ctypes.data if isinstance(v, str) else v
    arr = (C.c_int * 8)(*scales)
    return lib.ucd_pod_backward(p(x), ld, dtype, B, Cc, h, w, slope, C.cast(arr, C.c_void_p), len(scales), p(g), p(go), p(d), ld, None)


@pytest.mark.parametrize("kwargs,code", [
    (dict(x_s=None), hip.EINVAL), (dict(x_t=None), hip.EINVAL), (dict(out=None), hip.EINVAL), (dict(g=None), hip.EINVAL),
    (dict(scales=None, n=3), hip.EINVAL),
    (dict(B=0), hip.EINVAL), (dict(Cc=0), hip.EINVAL), (dict(h=3), hip.EINVAL), (dict(w=3), hip.EINVAL),
    (dict(scales=()), hip.EINVAL), (dict(scales=(1, 2, 3, 4, 5), h=8, w=8), hip.EINVAL), (dict(scales=(0, 2)), hip.EINVAL),
    (dict(scales=(1, 9), h=16, w=16), hip.EINVAL), (dict(scales=(2, 2)), hip.EINVAL), (dict(scales=(4, 2)), hip.EINVAL),
    (dict(slope=0.0), hip.EINVAL), (dict(slope=1.5), hip.EINVAL), (dict(dtype=7), hip.EINVAL), (dict(ld=4), hip.EINVAL),
    (dict(Cc=12, ld=12), hip.EUNSUPPORTED), (dict(Cc=4, ld=4), hip.EUNSUPPORTED), (dict(h=2048), hip.EUNSUPPORTED),
    (dict(ld=10), hip.EALIGN),
    (dict(ws=None), hip.EWORKSPACE), (dict(ws_bytes=64), hip.EWORKSPACE),
])
def test_forward_refuses_on_the_host(kwargs, code):
    assert _forward_rc(**kwargs) == code
    assert hip.load().ucd_last_error()                     # a message was recorded


@pytest.mark.parametrize("kwargs,code", [
    (dict(x=None), hip.EINVAL), (dict(g=None), hip.EINVAL), (dict(go=None), hip.EINVAL), (dict(d=None), hip.EINVAL),
    (dict(B=0), hip.EINVAL), (dict(Cc=-8), hip.EINVAL), (dict(h=1), hip.EINVAL), (dict(scales=(3, 1)), hip.EINVAL),
    (dict(slope=-0.01), hip.EINVAL), (dict(Cc=20, ld=20), hip.EUNSUPPORTED),
])
def test_backward_refuses_on_the_host(kwargs, code):
    assert _backward_rc(**kwargs) == code


def test_plan_refuses_like_the_calls():
    with pytest.raises(RuntimeError, match="multiple of 8"):
        hip.pod_plan(9, 9, 12)
    with pytest.raises(RuntimeError, match="largest scale"):
        hip.pod_plan(3, 9, 64)
    with pytest.raises(RuntimeError, match="increase strictly"):
        hip.pod_plan(9, 9, 64, (2, 1))
    with pytest.raises(RuntimeError, match="scales"):
        hip.pod_plan(9, 9, 64, ())


def _maps(seed, B, Cc, h, w):
    rng = np.random.RandomState(seed)
    return rng.randn(B, Cc, h, w) * 2.0, rng.randn(B, Cc, h, w) * 2.0


@pytest.mark.parametrize("geom,scales", GEOMETRIES)
def test_torch_composition_matches_the_reference_fp64(geom, scales):
    """The plan's geometries with a = 0.01 and mixed signs: value and gradient to 1e-12 (relative to the largest entry)."""
    h, w, Cc = geom
    xs, xt = _maps(3, 1 if h > 100 else 2, Cc, h, w)
    ts = torch.from_numpy(xs).requires_grad_(True)
    val = local_pod_torch(ts, torch.from_numpy(xt), 0.01, scales, 0.7)
    val.backward()
    ref = 0.7 * pod_ref.level(xs, xt, 0.01, scales)
    assert abs(val.item() - ref) <= 1e-12 * max(1.0, abs(ref))
    gref = pod_ref.level_grad(xs, xt, 0.01, scales, 0.7)
    assert np.abs(ts.grad.numpy() - gref).max() <= 1e-12 * max(1.0, np.abs(gref).max())


def test_gradcheck():
    xs, xt = _maps(5, 2, 8, 5, 6)
    ts = torch.from_numpy(xs).requires_grad_(True)
    tt = torch.from_numpy(xt)
    assert torch.autograd.gradcheck(lambda x: local_pod_torch(x, tt, 0.01, (1, 2, 4), 1.3), (ts,), eps=1e-6, atol=1e-6)
    # fused_local_pod on a CPU tensor IS the composition
    assert torch.equal(fused_local_pod(ts, tt, 0.01, (1, 2, 4), 1.3), local_pod_torch(ts, tt, 0.01, (1, 2, 4), 1.3))


def test_degenerate_cases_are_exactly_zero():
    xs, _ = _maps(7, 2, 8, 5, 6)
    same = torch.from_numpy(xs).requires_grad_(True)
    val = local_pod_torch(same, torch.from_numpy(xs.copy()), 0.01)
    val.backward()
    assert val.item() == 0.0 and torch.isfinite(same.grad).all() and not same.grad.any()
    zero = torch.zeros(2, 8, 5, 6, dtype=torch.float64, requires_grad=True)
    val = local_pod_torch(zero, torch.zeros(2, 8, 5, 6, dtype=torch.float64), 0.01)
    val.backward()
    assert val.item() == 0.0 and torch.isfinite(zero.grad).all() and not zero.grad.any()
    assert pod_ref.level(xs, xs, 0.01, (1, 2, 4)) == 0.0 and not pod_ref.level_grad(xs, xs, 0.01, (1, 2, 4)).any()


def test_argument_rules():
    x = torch.zeros(1, 8, 4, 4)
    for bad in ((), (1, 2, 3, 4, 5), (0, 1), (1, 9), (2, 2), (4, 2)):
        with pytest.raises(ValueError):
            local_pod_torch(x, x, 1.0, bad)
    with pytest.raises(ValueError):
        local_pod_torch(x, x, 1.0, (1, 2, 8))               # 4 x 4 is below scale 8
    with pytest.raises(ValueError):
        local_pod_torch(x, x, 0.0)
    with pytest.raises(ValueError):
        local_pod_torch(x, torch.zeros(1, 8, 4, 5))


# ---- command line and trainer ------------------------------------------------------------------------------------------------
def _opts(extra=()):
    return argparser.modify_command_options(argparser.get_argparser().parse_args(
        ["--method", "UCD", "--task", "15-5", "--step", "1", "--no_pretrained"] + list(extra)))


def test_parser_defaults_and_validation():
    o = _opts()
    assert (o.pod_factor, o.pod_last_factor, o.pod_scales) == (0.0, 0.0005, [1, 2, 4])
    o = _opts(["--pod_factor", "0.01", "--pod_scales", "1", "3"])
    assert o.pod_factor == 0.01 and o.pod_scales == [1, 3]
    assert (o.loss_kd, o.unce, o.unkd) == (10, True, True)              # no preset changed
    for bad in (["0", "1"], ["2", "2"], ["1", "2", "3", "4", "5"], ["1", "9"]):
        with pytest.raises(SystemExit):
            _opts(["--pod_scales"] + bad)


class _ToyNet(nn.Module):
    """Four stage maps, a head map and logits, with the model interface the Trainer uses."""

    def __init__(self, classes, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        chans = (3, 8, 8, 16, 16)
        self.stages = nn.ModuleList([nn.Conv2d(a, b, 3, stride=2 if i < 2 else 1, padding=1) for i, (a, b) in
                                     enumerate(zip(chans, chans[1:]))])
        self.head = nn.Conv2d(16, 8, 1)
        self.cls = nn.Conv2d(8, classes, 1)
        for p in self.parameters():
            with torch.no_grad():
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
        self.calls = []

    def pod_slope(self):
        return 0.01

    def forward(self, x, x_b_old=None, x_pl_old=None, ret_intermediate=False, upsample=True, taps=False):
        from ucd_amd.segmentation_module import Features
        self.calls.append(taps)
        maps = []
        y = x
        for conv in self.stages:
            y = F.leaky_relu(conv(y), 0.01)
            maps.append(y)
        x_pl = self.head(y)
        sem = self.cls(x_pl)
        logits = F.interpolate(sem, size=x.shape[-2:], mode="bilinear", align_corners=False)
        return logits, Features(y, x_pl, sem, tuple(maps) if taps else None)


def _toy_trainer(extra):
    from ucd_amd.train import Trainer
    opts = _opts(extra)
    opts.pixcon_weight = 0.0                    # the contrastive kernels exist on the GPU only
    student, teacher = _ToyNet(21, 1), _ToyNet(16, 2)
    teacher.eval()
    trainer = Trainer(student, teacher, torch.device("cpu"), opts, classes=[16, 5])
    return trainer, student, teacher


def _toy_batch():
    g = torch.Generator().manual_seed(11)
    return torch.randn(2, 3, 36, 44, generator=g), torch.randint(0, 21, (2, 36, 44), generator=g)


def test_pod_factor_zero_requests_no_taps():
    trainer, student, teacher = _toy_trainer([])
    assert trainer.pod_flag is False
    images, labels = _toy_batch()
    out = trainer.train_step(images, labels, torch.optim.SGD(student.parameters(), lr=0.0))
    assert student.calls == [False] and teacher.calls == [False] and "LPOD" not in out
    # and without a teacher the flag stays off whatever the factor
    from ucd_amd.train import Trainer
    assert Trainer(student, None, torch.device("cpu"), _opts(["--pod_factor", "0.01"]), classes=[16, 5]).pod_flag is False


def test_cpu_trainer_step_adds_the_term_composed_by_hand():
    plain, student0, _ = _toy_trainer([])
    trainer, student, teacher = _toy_trainer(["--pod_factor", "0.01", "--pod_last_factor", "0.0005"])
    assert trainer.pod_flag and trainer.pod_slope == 0.01
    images, labels = _toy_batch()
    r0 = plain.train_step(images, labels, torch.optim.SGD(student0.parameters(), lr=0.0))
    r = trainer.train_step(images, labels, torch.optim.SGD(student.parameters(), lr=0.0))
    assert student.calls == [True] and teacher.calls == [True]
    with torch.no_grad():
        _, fs = student(images, taps=True)
        _, ft = teacher(images, taps=True)
    gamma = math.sqrt(21 / 5)
    by_hand = sum(0.01 * pod_ref.level(s.numpy(), t.numpy(), 0.01, (1, 2, 4)) for s, t in zip(fs.stages, ft.stages))
    by_hand += 0.0005 * pod_ref.level(fs.raw("pre_logits").numpy(), ft.raw("pre_logits").numpy(), 1.0, (1, 2, 4))
    by_hand *= gamma / 5
    assert by_hand > 0 and abs(r["LPOD"].item() - by_hand) <= 1e-5 * by_hand
    # the other terms are the plain step's, and the gradient of the first stage moved by the term
    for k in ("loss", "lkd", "ce"):
        assert r[k].item() == r0[k].item()
    assert not torch.equal(student.stages[0].weight.grad, student0.stages[0].weight.grad)
    assert torch.equal(student.cls.weight.grad, student0.cls.weight.grad)          # the classifier sits behind every tapped map


def test_refused_activation():
    from ucd_amd.segmentation_module import IncrementalSegmentationModule

    class _M:
        pass
    m = _M()
    m.body = _M(); m.body.mod2 = _M(); m.body.mod2.block1 = _M(); m.body.mod2.block1.convs = _M()
    bn = _M(); bn.activation, bn.activation_param = "elu", 1.0
    m.body.mod2.block1.convs.bn1 = bn
    with pytest.raises(ValueError, match="leaky_relu or identity"):
        IncrementalSegmentationModule.pod_slope(m)
    bn.activation = "identity"
    assert IncrementalSegmentationModule.pod_slope(m) == 1.0
    bn.activation, bn.activation_param = "leaky_relu", 0.01
    assert IncrementalSegmentationModule.pod_slope(m) == 0.01
