"""GPU: Local POD feature distillation (``--pod_factor``) - the kernels of csrc/pod.hip against the float64 reference
(tests/pod_ref.py) on exact operands, and the term inside the UCD step: eager, under the A/B switch, replayed from the whole-step
graph, and from the command line."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pod_ref
from ucd_amd import argparser, synth, tasks
from ucd_amd.loss import fused_local_pod, local_pod_torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"

# (B, C, h, w), scales: uncovered last row / column at scales 2 and 4; non-square with non-nested regions; the smallest map the
# default scales take; more than one workgroup in every launch; another scale list
CASES = [((2, 64, 9, 9), (1, 2, 4)), ((3, 72, 7, 11), (1, 2, 4)), ((1, 64, 4, 4), (1, 2, 4)), ((1, 256, 33, 33), (1, 2, 4)),
         ((2, 64, 9, 9), (1, 3))]
WEIGHT, UPSTREAM = 0.7, 1.5


@functools.lru_cache(maxsize=None)
def _case(shape, scales, a):
    """Operands and the float64 reference of one case, computed once and shared (read-only) by the tests that need them."""
    xs, xt = pod_ref.integer_maps(17, shape, a)
    value = pod_ref.level(xs, xt, a, scales)
    grad = pod_ref.level_grad(xs, xt, a, scales, WEIGHT * UPSTREAM)
    for arr in (xs, xt, grad):
        arr.setflags(write=False)
    return xs, xt, value, grad


def _pitched(x, dtype):
    """The map as a channel slice of a channels-last tensor with 8 more channels: row pitch C + 8."""
    B, Cc, h, w = x.shape
    wide = torch.full((B, Cc + 8, h, w), 77.0, dtype=dtype, device=DEV).contiguous(memory_format=torch.channels_last)
    host = torch.from_numpy(np.array(x, dtype=np.float64))          # a copy: the shared operands are read-only
    wide[:, :Cc] = host.to(DEV, dtype)
    view = wide[:, :Cc]
    assert view.stride()[3] == Cc + 8 and torch.equal(view.double().cpu(), host)      # the operands are exact in the map dtype
    return view


def _run(xs, xt, a, scales, dtype):
    s = _pitched(xs, dtype).detach().requires_grad_(True)
    t = _pitched(xt, dtype)
    val = fused_local_pod(s, t, a, scales, WEIGHT)
    (val * UPSTREAM).backward()
    torch.cuda.synchronize()
    return val.detach(), s.grad


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("a", [0.01, 1.0, 0.5])         # 0.5: the one slope whose negative entries are stored scaled, exactly
@pytest.mark.parametrize("shape,scales", CASES)
def test_kernels_match_the_reference(shape, scales, a, dtype):
    """Small-integer operands (exact in bf16; every strip sum of a = 1 exact in fp32).  Level value within 1e-5 ref + 1e-6 (fp32
    rounding of the normalised entries, fp64 reductions); dX relative L2 within 1e-5 (fp32 maps) or 4e-3 (bf16 maps: the one output
    rounding, 2^-9, with 2x headroom)."""
    xs, xt, ref, gref = _case(shape, scales, a)
    val, grad = _run(xs, xt, a, scales, dtype)
    got = val.item() / WEIGHT
    print(f"level {got!r} reference {ref!r} diff {abs(got - ref):.3e}")
    assert grad.dtype == dtype and grad.shape == tuple(shape)
    g = grad.double().cpu().numpy()
    rel = np.linalg.norm(g - gref) / np.linalg.norm(gref)
    print(f"dX relative L2 {rel:.3e}")
    assert abs(got - ref) <= 1e-5 * ref + 1e-6
    assert rel <= (1e-5 if dtype == torch.float32 else 4e-3)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_torch_composition_on_the_same_operands(dtype):
    """The A/B partner of the kernels (UCD_FUSED_POD=0) is held to the same reference on the device."""
    for shape, scales in CASES[:2]:
        xs, xt, ref, gref = _case(shape, scales, 0.01)
        s = _pitched(xs, dtype).detach().requires_grad_(True)
        val = local_pod_torch(s, _pitched(xt, dtype), 0.01, scales, WEIGHT)
        (val * UPSTREAM).backward()
        assert abs(val.item() / WEIGHT - ref) <= 1e-5 * ref + 1e-6
        rel = np.linalg.norm(s.grad.double().cpu().numpy() - gref) / np.linalg.norm(gref)
        assert rel <= (1e-5 if dtype == torch.float32 else 4e-3), rel


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_degenerate_maps_and_reproducibility(dtype):
    shape, scales = CASES[1]
    xs, xt, _, _ = _case(shape, scales, 0.01)
    # student == teacher: exactly zero loss and gradient
    val, grad = _run(xs, xs, 0.01, scales, dtype)
    assert val.item() == 0.0 and not grad.any()
    # an all-zero student (and both all-zero): finite
    zero = np.zeros(shape)
    for teacher in (xt, zero):
        val, grad = _run(zero, teacher, 0.01, scales, dtype)
        assert torch.isfinite(val).all() and torch.isfinite(grad).all()
    val, grad = _run(zero, zero, 0.01, scales, dtype)
    assert val.item() == 0.0 and not grad.any()
    # two runs: the same bits
    a = _run(xs, xt, 0.01, scales, dtype)
    b = _run(xs, xt, 0.01, scales, dtype)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_refused_geometry_runs_the_composition():
    x = torch.randn(2, 12, 6, 6, device=DEV, requires_grad=True)            # C = 12: not a multiple of 8
    t = torch.randn(2, 12, 6, 6, device=DEV)
    assert torch.equal(fused_local_pod(x, t, 0.01), local_pod_torch(x, t, 0.01))


# ---- the term inside the UCD step ------------------------------------------------------------------------------------------------
NAMES = ("body.mod1.conv1.weight", "body.mod2.block1.convs.conv1.weight", "body.mod2.block3.convs.conv3.weight",
         "body.mod3.block2.convs.conv2.weight", "body.mod4.block10.convs.conv3.weight", "body.mod5.block3.convs.conv3.weight",
         "head.red_conv.weight", "cls.1.weight")


def _steps(extra_args=(), step_graph="0", steps=1, flips=None, batch=2, crop=65):
    """``steps`` scheduled UCD iterations (bf16, 15-5 step 1, synthetic calibrated checkpoint, as tests/test_step_gpu.py builds
    them) at 2 x 65^2: stage maps 17^2, 9^2, 5^2, 5^2.  Returns the losses per step, the accumulated update of a few parameters, the
    number of replayed iterations and the capture error."""
    from ucd_amd import switches
    from ucd_amd.ddp import DistributedDataParallel
    from ucd_amd.run import build_models, load_step_checkpoint, make_optimizer
    from ucd_amd.scheduler import PolyLR
    from ucd_amd.train import Trainer
    dev = torch.device(DEV)
    opts = argparser.modify_command_options(argparser.get_argparser().parse_args(
        ["--method", "UCD", "--dataset", "voc", "--task", "15-5", "--step", "1", "--lr", "0.001", "--no_pretrained",
         "--norm_act", "iabn_sync", "--opt_level", "O1"] + list(extra_args)))
    classes = tasks.get_per_task_classes("voc", "15-5", 1)
    flips = dict(flips or {}, UCD_STEP_GRAPH=step_graph)
    for k, v in flips.items():
        switches.set(k, v)
    torch.backends.cudnn.deterministic = True
    try:
        model, model_old = build_models(opts, dev, classes)
        state = synth.fill_state_dict({k: v.cpu() for k, v in model_old.state_dict().items()}, 42, calibrated=True)
        optim = make_optimizer(opts, model)
        sched = PolyLR(optim, max_iters=steps + 2, power=0.9)
        net = model
        model = DistributedDataParallel(model, delay_allreduce=True, bf16_weights=True)
        load_step_checkpoint(opts, model, model_old, state, dev)
        trainer = Trainer(model, model_old, device=dev, opts=opts, classes=classes)
        model.train()
        params = dict(net.named_parameters())
        before = {n: params[n].detach().float().cpu().clone() for n in NAMES}
        rec = []
        for it in range(steps):
            img = synth.images(700 + it % 2, batch, crop)
            labels = synth.seg_labels(700 + it % 2, batch, crop, crop, range(16, 21))
            r = trainer.train_step(img, labels, optim, sched)
            rec.append([r[k].item() for k in ("ce", "con", "lkd", "loss")] + [r["LPOD"].item() if "LPOD" in r else 0.0])
        torch.cuda.synchronize()
        upd = {n: params[n].detach().float().cpu() - before[n] for n in NAMES}
        return np.asarray(rec), upd, trainer.graph_steps, trainer.step_graph_error, trainer
    finally:
        torch.backends.cudnn.deterministic = False
        for k in flips:
            switches.unset(k)


POD = ("--pod_factor", "0.01")


@pytest.mark.usefixtures("deterministic_stats")
def test_step_with_pod_against_the_torch_composition():
    """One UCD step with --pod_factor 0.01 on the default switches: the three tapped stage boundaries left their block link
    unclaimed, so the backward raises no "second consumer"; against the same step under UCD_FUSED_POD=0 UCD_BWD_LINK=0 the losses
    keep the bars of tests/test_step_gpu.py::test_switch_combinations_give_the_same_step and the first update of eight parameters
    across the network those of its bf16 update comparison (cosine above 0.78 in the body, 0.98 elsewhere; length within
    0.85 .. 1.25)."""
    from ucd_amd import hip
    calls = hip.enable_call_timing()
    try:
        got, up, _, _, trainer = _steps(POD)
        fused_calls = (len(calls.get("ucd_pod_forward", ())), len(calls.get("ucd_pod_backward", ())))
        calls.clear()
        ref, up_ref, _, _, _ = _steps(POD, flips={"UCD_FUSED_POD": "0", "UCD_BWD_LINK": "0"})
        assert "ucd_pod_forward" not in calls and "ucd_pod_backward" not in calls
    finally:
        hip.disable_call_timing()
    assert fused_calls == (5, 5), fused_calls                   # five levels, each on its own kernels
    assert trainer.pod_flag and got[0, 4] > 0 and np.isfinite(got).all()
    print("fused:", got, "composition:", ref)
    np.testing.assert_allclose(got[:, 3], ref[:, 3], rtol=1e-2)
    np.testing.assert_allclose(got[:, 0], ref[:, 0], rtol=1e-2)
    np.testing.assert_allclose(got[:, 1:3], ref[:, 1:3], rtol=5e-2, atol=1e-3)
    np.testing.assert_allclose(got[:, 4], ref[:, 4], rtol=1e-2)                    # the term itself: both paths pool in fp32
    for n in NAMES:
        a, b = up_ref[n].flatten().double(), up[n].flatten().double()
        cos = float(a @ b / (a.norm() * b.norm() + 1e-300))
        ratio = float(b.norm() / (a.norm() + 1e-300))
        print(f"first update, fused vs composition: {n}: cosine {cos:.4f} length ratio {ratio:.3f}")
        assert cos > (0.78 if n.startswith("body.") else 0.98) and 0.85 < ratio < 1.25, (n, cos, ratio)


@pytest.mark.usefixtures("deterministic_stats")
def test_whole_step_graph_replays_the_eager_step_with_pod():
    """The five Local POD levels (taps of both networks, four launches forward and one backward each) inside the captured
    iteration, on the deterministic statistics path: three eager warm-up iterations and three replays give the bits of six eager
    iterations - every loss, the POD term among them, at every step, and every compared parameter afterwards."""
    eager, pe, n_e, _, _ = _steps(POD, "0", steps=6)
    graph, pg, n_g, err, _ = _steps(POD, "1", steps=6)
    assert err is None, err
    assert n_e == 0 and n_g == 6 - 3, (n_e, n_g)
    print("eager", eager, "graph", graph, "max abs difference", np.abs(eager - graph).max())
    for n in pe:
        print(n, "relative difference", ((pe[n] - pg[n]).norm() / pe[n].norm()).item())
    assert np.array_equal(eager, graph), (eager, graph)
    for n in pe:
        assert torch.equal(pe[n], pg[n]), n


@pytest.mark.usefixtures("deterministic_stats")
def test_pod_factor_zero_is_the_plain_step():
    """--pod_factor 0 requests no taps: the same launches, the same bits as a Trainer built without the flags."""
    plain, pp, _, _, t0 = _steps((), steps=2)
    zero, pz, _, _, t1 = _steps(("--pod_factor", "0", "--pod_last_factor", "0.0005", "--pod_scales", "1", "2"), steps=2)
    assert not t0.pod_flag and not t1.pod_flag
    assert np.array_equal(plain, zero), (plain, zero)
    for n in pp:
        assert torch.equal(pp[n], pz[n]), n


def test_run_py_logs_the_term(tmp_path):
    """run.py --method UCD --pod_factor 0.01 on synthetic batches, two iterations at the smallest crop whose stage maps take the
    default scales (65: 5 x 5 at stride 16)."""
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), "--data_root", "synthetic", "--method", "UCD", "--pod_factor", "0.01",
           "--task", "15-5", "--step", "1", "--crop_size", "65", "--batch_size", "96", "--epochs", "1", "--no_pretrained",
           "--opt_level", "O1", "--lr", "0.001", "--debug", "--print_interval", "1", "--val_interval", "100", "--name", "pod"]
    r = subprocess.run(cmd, cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    import re
    terms = [float(v) for v in re.findall(r"LPOD ([-+0-9.eE]+)", log)]
    assert len(terms) == 2 and all(np.isfinite(v) and v > 0 for v in terms), log[-3000:]
