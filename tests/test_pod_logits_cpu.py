"""CPU: the host half of Local POD on the logits (``--pod_logits``; csrc/pod.hip, ucd_amd.loss.fused_local_pod_logits) - the plan,
the library's refusals on host buffers, the torch composition against the float64 reference (tests/pod_logits_ref.py), the command
line and a Trainer step on a small CPU network."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pod_logits_ref as ref
import pod_ref
from test_pod_cpu import _opts, _toy_batch, _toy_trainer
from ucd_amd import hip
from ucd_amd.loss import fused_local_pod_logits, local_pod_logits_torch

# (B, Ctot, K, h, w), scales: the cases of tests/test_pod_logits_gpu.py
CASES = [((2, 21, 16, 9, 9), (1, 2, 4)), ((3, 21, 20, 7, 11), (1, 2, 4)), ((1, 6, 1, 4, 4), (1, 2, 4)),
         ((1, 111, 101, 33, 33), (1, 2, 4)), ((2, 17, 16, 9, 9), (1, 3)), ((2, 16, 16, 5, 5), (1, 2, 4))]


def test_names_are_registered():
    assert {"ucd_pod_logits_plan", "ucd_pod_logits_forward", "ucd_pod_logits_backward"} <= set(hip.SIGNATURES)


@pytest.mark.parametrize("case,scales", CASES)
def test_plan_counts_the_embedding(case, scales):
    B, Ctot, K, h, w = case
    for normalize in (0, 1):
        plan = hip.pod_logits_plan(h, w, Ctot, K, scales, B, normalize)
        assert plan["n_E"] == sum(s * s * K * (h // s + w // s) for s in scales) == ref.n_embed(K, h, w, scales)
        tiles, chunks, nrs, ncs = plan["grid"]
        assert tiles >= 1 and 1 <= chunks <= 256 and nrs >= math.ceil(h / 8) and ncs >= math.ceil(w / 16)
        assert plan["workspace_bytes"] >= 2 * B * plan["n_E"] * 4          # at least the pooled strips of both maps
    # the pieces are those of a feature level on the same map
    assert plan["grid"][2:] == hip.pod_plan(h, w, 8, scales)["grid"][2:]


def _forward_rc(x_s="ok", x_t="ok", ld_s=21, ld_t=16, dtype=hip.F32, B=1, Ctot=21, K=16, h=4, w=4, scales=(1, 2, 4), n=None,
                normalize=1, out="ok", g="ok", ws="ok", ws_bytes=None):
    lib = hip.load()
    buf = np.zeros(8192, dtype=np.float32)       # host memory: a refusal never touches it
    p = lambda v: buf.ctypes.data + (v if isinstance(v, int) else 0) if v is not None else None
    arr = (C.c_int * 8)(*scales) if scales is not None else None
    nb = (1 << 20) if ws_bytes is None else ws_bytes
    return lib.ucd_pod_logits_forward(p(x_s), ld_s, p(x_t), ld_t, dtype, B, Ctot, K, h, w,
                                      C.cast(arr, C.c_void_p) if arr is not None else None, len(scales) if n is None else n, normalize,
                                      1.0, p(out), p(g), p(ws), nb, None)


def _backward_rc(x="ok", ld_s=21, ld_d=21, dtype=hip.F32, B=1, Ctot=21, K=16, h=4, w=4, scales=(1, 2, 4), g="ok", go="ok", d="ok"):
    lib = hip.load()
    buf = np.zeros(8192, dtype=np.float32)
    p = lambda v: buf.ctypes.data + (v if isinstance(v, int) else 0) if v is not None else None
    arr = (C.c_int * 8)(*scales)
    return lib.ucd_pod_logits_backward(p(x), ld_s, dtype, B, Ctot, K, h, w, C.cast(arr, C.c_void_p), len(scales), p(g), p(go), p(d), ld_d,
                                       None)


@pytest.mark.parametrize("kwargs,code,word", [
    (dict(x_s=None), hip.EINVAL, "NULL"), (dict(x_t=None), hip.EINVAL, "NULL"), (dict(out=None), hip.EINVAL, "NULL"),
    (dict(g=None), hip.EINVAL, "NULL"), (dict(scales=None, n=3), hip.EINVAL, "scales"),
    (dict(K=0), hip.EINVAL, "K = 0"), (dict(K=22), hip.EINVAL, "K = 22"), (dict(B=0), hip.EINVAL, "B = 0"),
    (dict(ld_s=20), hip.EINVAL, "x_s"), (dict(ld_t=15), hip.EINVAL, "x_t"),
    (dict(scales=()), hip.EINVAL, "scales"), (dict(scales=(0, 2)), hip.EINVAL, "scale"), (dict(scales=(2, 2)), hip.EINVAL, "strictly"),
    (dict(scales=(1, 9), h=16, w=16), hip.EINVAL, "scale"), (dict(h=3), hip.EINVAL, "largest scale"),
    (dict(normalize=2), hip.EINVAL, "normalize"), (dict(normalize=-1), hip.EINVAL, "normalize"),
    (dict(Ctot=300, ld_s=300), hip.EUNSUPPORTED, "Ctot = 300"), (dict(dtype=hip.BF16), hip.EUNSUPPORTED, "dtype"),
    (dict(h=2048), hip.EUNSUPPORTED, "2048"), (dict(w=1025), hip.EUNSUPPORTED, "1025"),
    (dict(x_s=2), hip.EALIGN, "x_s"), (dict(x_t=1), hip.EALIGN, "x_t"), (dict(g=2), hip.EALIGN, "g_E"),
    (dict(ws=None), hip.EWORKSPACE, "workspace"), (dict(ws_bytes=64), hip.EWORKSPACE, "workspace"),
])
def test_forward_refuses_on_the_host(kwargs, code, word):
    assert _forward_rc(**kwargs) == code
    assert word in hip.load().ucd_last_error().decode()             # the message names the argument


@pytest.mark.parametrize("kwargs,code,word", [
    (dict(x=None), hip.EINVAL, "NULL"), (dict(g=None), hip.EINVAL, "NULL"), (dict(go=None), hip.EINVAL, "NULL"),
    (dict(d=None), hip.EINVAL, "NULL"), (dict(K=0), hip.EINVAL, "K = 0"), (dict(K=30), hip.EINVAL, "K = 30"),
    (dict(ld_s=16), hip.EINVAL, "x_s"), (dict(ld_d=20), hip.EINVAL, "d_x"), (dict(scales=(3, 1)), hip.EINVAL, "strictly"),
    (dict(Ctot=257, ld_s=257, ld_d=257), hip.EUNSUPPORTED, "Ctot = 257"), (dict(dtype=hip.BF16), hip.EUNSUPPORTED, "dtype"),
    (dict(h=1025), hip.EUNSUPPORTED, "1025"), (dict(x=2), hip.EALIGN, "x_s"), (dict(d=3), hip.EALIGN, "d_x"),
])
def test_backward_refuses_on_the_host(kwargs, code, word):
    assert _backward_rc(**kwargs) == code
    assert word in hip.load().ucd_last_error().decode()


def test_plan_refuses_like_the_calls():
    with pytest.raises(RuntimeError, match="K = 22"):
        hip.pod_logits_plan(9, 9, 21, 22)
    with pytest.raises(RuntimeError, match="K = 0"):
        hip.pod_logits_plan(9, 9, 21, 0)
    with pytest.raises(RuntimeError, match="Ctot = 300"):
        hip.pod_logits_plan(9, 9, 300, 16)
    with pytest.raises(RuntimeError, match="normalize"):
        hip.pod_logits_plan(9, 9, 21, 16, normalize=2)
    with pytest.raises(RuntimeError, match="largest scale"):
        hip.pod_logits_plan(3, 9, 21, 16)
    with pytest.raises(RuntimeError, match="above 1024"):
        hip.pod_logits_plan(9, 1025, 21, 16)
    assert hip.pod_logits_plan(1024, 1024, 256, 1)["n_E"] == ref.n_embed(1, 1024, 1024, (1, 2, 4))


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("case,scales", CASES)
def test_torch_composition_matches_the_reference_fp64(case, scales, normalize):
    """Integer logits and Gaussian ones: value and gradient to 1e-12 (relative to the largest entry)."""
    B, Ctot, K, h, w = case
    rng = np.random.RandomState(3)
    for s, t in (ref.integer_logits(5, *case), (rng.randn(B, Ctot, h, w) * 2.0, rng.randn(B, K, h, w) * 2.0)):
        ts = torch.from_numpy(s).requires_grad_(True)
        val = local_pod_logits_torch(ts, torch.from_numpy(t), scales, 0.7, normalize)
        val.backward()
        want = 0.7 * ref.level(s, t, scales, normalize)
        assert val.dtype == torch.float64 and abs(val.item() - want) <= 1e-12 * max(1.0, abs(want))
        gref = ref.level_grad(s, t, scales, normalize, 0.7)
        assert np.abs(ts.grad.numpy() - gref).max() <= 1e-12 * max(1.0, np.abs(gref).max())
        # channel 0 and the new-class channels share one gradient
        for c in range(K, Ctot):
            assert np.array_equal(gref[:, c], gref[:, 0])


@pytest.mark.parametrize("normalize", [0, 1])
def test_gradcheck(normalize):
    rng = np.random.RandomState(9)
    ts = torch.from_numpy(rng.randn(2, 7, 5, 6) * 2.0).requires_grad_(True)
    tt = torch.from_numpy(rng.randn(2, 4, 5, 6) * 2.0)
    assert torch.autograd.gradcheck(lambda x: local_pod_logits_torch(x, tt, (1, 2, 4), 1.3, normalize), (ts,), eps=1e-6, atol=1e-6)
    # fused_local_pod_logits on a CPU tensor IS the composition
    assert torch.equal(fused_local_pod_logits(ts, tt, (1, 2, 4), 1.3, normalize), local_pod_logits_torch(ts, tt, (1, 2, 4), 1.3, normalize))


def test_without_new_channels_it_is_the_feature_level_at_slope_one():
    s, t = ref.integer_logits(7, 2, 16, 16, 5, 5)
    assert ref.level(s, t, (1, 2, 4), 1) == pod_ref.level(s, t, 1.0, (1, 2, 4))
    assert np.array_equal(ref.level_grad(s, t, (1, 2, 4), 1, 0.7), pod_ref.level_grad(s, t, 1.0, (1, 2, 4), 0.7))
    val = local_pod_logits_torch(torch.from_numpy(s), torch.from_numpy(t), (1, 2, 4), 1.0, 1)
    assert abs(val.item() - pod_ref.level(s, t, 1.0, (1, 2, 4))) <= 1e-12


def test_degenerate_cases_and_argument_rules():
    s, t = ref.integer_logits(11, 2, 9, 6, 5, 6)
    s[:, 0] = t[:, 0] - s[:, 6:].sum(1)                     # M == T
    s[:, 1:6] = t[:, 1:]
    for normalize in (0, 1):
        ts = torch.from_numpy(s).requires_grad_(True)
        val = local_pod_logits_torch(ts, torch.from_numpy(t), (1, 2, 4), 1.0, normalize)
        val.backward()
        assert val.item() == 0.0 and torch.isfinite(ts.grad).all() and not ts.grad.any()
        assert ref.level(s, t, (1, 2, 4), normalize) == 0.0 and not ref.level_grad(s, t, (1, 2, 4), normalize).any()
    x = torch.zeros(1, 8, 4, 4)
    with pytest.raises(ValueError):
        local_pod_logits_torch(x, torch.zeros(1, 9, 4, 4))          # K above Ctot
    with pytest.raises(ValueError):
        local_pod_logits_torch(x, torch.zeros(1, 4, 4, 5))
    with pytest.raises(ValueError):
        local_pod_logits_torch(x, x, (2, 2))
    with pytest.raises(ValueError):
        local_pod_logits_torch(x, x, (1, 2, 4), 1.0, 2)


# ---- command line and trainer ------------------------------------------------------------------------------------------------
def test_parser_defaults():
    o = _opts()
    assert o.pod_logits is False and o.pod_logits_norm == 1
    o = _opts(["--pod_logits", "--pod_logits_norm", "0"])
    assert o.pod_logits is True and o.pod_logits_norm == 0 and o.pod_factor == 0.0
    with pytest.raises(SystemExit):
        _opts(["--pod_logits_norm", "2"])
    # the PLOP preset stays as it is; --pod_logits completes it
    from ucd_amd import argparser
    plop = lambda extra: argparser.modify_command_options(argparser.get_argparser().parse_args(
        ["--method", "PLOP", "--task", "15-5", "--step", "1", "--no_pretrained"] + extra))
    assert plop([]).pod_logits is False and plop([]).pod_factor == 0.01
    assert plop(["--pod_logits"]).pod_logits is True and plop(["--pod_logits"]).pod_last_factor == 0.0005


def test_pod_logits_alone_requests_nothing():
    trainer, student, teacher = _toy_trainer(["--pod_logits"])
    assert trainer.pod_flag is False and trainer.pod_logits is False
    images, labels = _toy_batch()
    out = trainer.train_step(images, labels, torch.optim.SGD(student.parameters(), lr=0.0))
    assert student.calls == [False] and teacher.calls == [False] and "LPOD" not in out


def _by_hand(student, teacher, images, logits, normalize=1):
    with torch.no_grad():
        _, fs = student(images, taps=True)
        _, ft = teacher(images, taps=True)
    gamma = math.sqrt(21 / 5)
    total = sum(0.01 * pod_ref.level(s.numpy(), t.numpy(), 0.01, (1, 2, 4)) for s, t in zip(fs.stages, ft.stages))
    pl = pod_ref.level(fs.raw("pre_logits").numpy(), ft.raw("pre_logits").numpy(), 1.0, (1, 2, 4))
    if not logits:
        return (total + 0.0005 * pl) * gamma / 5
    return (total + 0.01 * pl + 0.0005 * ref.level(fs["sem"].numpy(), ft["sem"].numpy(), (1, 2, 4), normalize)) * gamma / 6


@pytest.mark.parametrize("normalize", [1, 0])
def test_cpu_trainer_step_sums_six_levels(normalize):
    five, student5, teacher5 = _toy_trainer(["--pod_factor", "0.01", "--pod_logits_norm", str(normalize)])
    six, student6, teacher6 = _toy_trainer(["--pod_factor", "0.01", "--pod_logits", "--pod_logits_norm", str(normalize)])
    assert five.pod_flag and not five.pod_logits and six.pod_flag and six.pod_logits
    images, labels = _toy_batch()
    r5 = five.train_step(images, labels, torch.optim.SGD(student5.parameters(), lr=0.0))
    r6 = six.train_step(images, labels, torch.optim.SGD(student6.parameters(), lr=0.0))
    want5 = _by_hand(student5, teacher5, images, False)
    want6 = _by_hand(student6, teacher6, images, True, normalize)
    assert want5 > 0 and abs(r5["LPOD"].item() - want5) <= 1e-5 * want5
    assert want6 > 0 and abs(r6["LPOD"].item() - want6) <= 1e-5 * want6 and want6 != want5
    for k in ("loss", "lkd", "ce"):
        assert r6[k].item() == r5[k].item()
    # the level on the logits reaches the classifier, which sits behind every other tapped map
    assert not torch.equal(student6.cls.weight.grad, student5.cls.weight.grad)
