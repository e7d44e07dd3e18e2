"""GPU: the fp32 split-bf16 convolutions (csrc/conv_f32.hip, ``UCD_F32_OWN_CONV=1``).

Kernel level: exact on integer operands that need the lo parts (a bf16-only kernel fails), within 5e-5 relative L2 and
2^-14 |A| |B|^T elementwise of a float64 reference on random data, bit-reproducible.  Layer level: ``Conv1x1`` / ``Conv3x3``
route to them only with the switch on.  Network level: the fp32 whole steps against the reference goldens at 1e-3 with every
eligible layer of student and teacher on the new kernels, and the 20-step trajectory (eager and replayed from a graph)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ucd_amd import blocks, hip, switches

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CL = torch.channels_last


@pytest.fixture
def f32_switch():
    switches.set("UCD_F32_OWN_CONV", "1")
    yield
    switches.unset("UCD_F32_OWN_CONV")


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(t.shape[0] * t.shape[2] * t.shape[3], t.shape[1])


def _wmat(w):
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def _fwd(x, w, d, y=None, accumulate=False):
    """The kernel on a [B, K, H, W] map and an [N, K, k, k] weight (d = 0: 1x1)."""
    B, K, H, W = x.shape
    if y is None:
        y = torch.empty((B, w.shape[0], H, W), dtype=torch.float32, device=DEV, memory_format=CL)
    hip.conv_f32(_rows(x.contiguous(memory_format=CL)), _wmat(w), _rows(y), conv3=(H, W, d) if d else None, accumulate=accumulate)
    return y


def _wgrad(dy, x, d):
    B, K, H, W = x.shape
    N = dy.shape[1]
    k = 3 if d else 1
    dw = torch.empty((N, k * k * K), dtype=torch.float32, device=DEV)
    hip.conv_f32_wgrad(_rows(dy.contiguous(memory_format=CL)), _rows(x.contiguous(memory_format=CL)), dw,
                       conv3=(H, W, d) if d else None)
    return dw.view(N, k, k, K).permute(0, 3, 1, 2)


def _conv64(x, w, d):
    return F.conv2d(x.double(), w.double(), None, 1, d, max(d, 1))


def _wgrad64(dy, x, w_shape, d):
    return torch.ops.aten.convolution_backward(dy.double(), x.double(), torch.empty(w_shape, dtype=torch.float64, device=x.device),
                                               None, [1, 1], [d, d], [max(d, 1)] * 2, False, [0, 0], 1, [False, True, False])[1]


def _ints(shape, lo, hi, gen):
    """Integers with |v| in [lo, hi] and random signs (lo = 0: the plain range [-hi, hi])."""
    mag = torch.randint(lo, hi + 1, shape, generator=gen)
    sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    return (mag * sign).float()


DILATIONS = [0, 1, 2, 6, 12, 18]       # 0: 1x1


@pytest.mark.parametrize("d", DILATIONS)
@pytest.mark.parametrize("wide", ["x", "w"])
def test_forward_is_exact_on_integers_that_need_the_lo_parts(d, wide):
    """One operand in {-2..2} (its lo part is 0), the other with 9-11 significant bits (needs its lo part): every product and
    partial sum is an integer below 2^24, so any summation order is exact and the result must equal the float64 reference bit
    for bit.  ``wide = "w"`` is the operand role of the input gradient (the weight carries the bits)."""
    gen = torch.Generator().manual_seed(7 + d)
    B, H, W, K, N = (2, 33, 33, 256, 128) if d else (1, 25, 40, 512, 192)
    x = _ints((B, K, H, W), 256, 2047, gen) if wide == "x" else _ints((B, K, H, W), 0, 2, gen)
    w = _ints((N, K, 3 if d else 1, 3 if d else 1), 0, 2, gen) if wide == "x" else _ints((N, K, 3 if d else 1, 3 if d else 1), 256, 2047, gen)
    ref = F.conv2d(x.double(), w.double(), None, 1, d, max(d, 1))
    got = _fwd(x.to(DEV).contiguous(memory_format=CL), w.to(DEV).contiguous(memory_format=CL), d).cpu()
    assert torch.equal(got.double(), ref), (got.double() - ref).abs().max().item()


@pytest.mark.parametrize("d", DILATIONS)
def test_weight_gradient_is_exact_on_integers(d):
    gen = torch.Generator().manual_seed(11 + d)
    B, H, W, K, N = (2, 33, 33, 128, 256) if d else (3, 33, 33, 192, 64)       # M = 2178 / 3267 rows: sums below 2^24
    dy = _ints((B, N, H, W), 0, 2, gen)
    x = _ints((B, K, H, W), 256, 2047, gen)
    k = 3 if d else 1
    ref = _wgrad64(dy, x, (N, K, k, k), d)
    got = _wgrad(dy.to(DEV), x.to(DEV), d).cpu()
    assert torch.equal(got.double(), ref), (got.double() - ref).abs().max().item()


def _check_close(got, ref, bound, what):
    got = got.double().cpu()
    ref = ref.cpu()
    rel = ((got - ref).norm() / ref.norm()).item()
    worst = ((got - ref).abs() / bound.cpu().clamp_min(1e-30)).max().item()
    print(f"{what}: rel-L2 {rel:.2e}, max |err| / (|A||B|) {worst * 2 ** -14:.2e}")
    assert rel <= 5e-5, (what, rel)
    assert torch.all((got - ref).abs() <= 2 ** -14 * bound.cpu()), (what, worst)


SHAPES_1X1 = [(1, 25, 40, 64, 256), (2, 33, 33, 1024, 256), (24, 33, 33, 2048, 512), (24, 33, 33, 512, 2048),
              (24, 33, 33, 2048, 256), (24, 33, 33, 256, 64), (24, 33, 33, 64, 64), (24, 33, 33, 256, 1024)]
SHAPES_3X3 = [(2, 7, 9, 256, 256, 1), (3, 7, 9, 64, 128, 2), (2, 65, 65, 64, 64, 1), (2, 65, 65, 128, 128, 1),
              (2, 33, 33, 256, 256, 2), (2, 33, 33, 512, 512, 4), (2, 33, 33, 2048, 256, 12), (24, 33, 33, 256, 256, 1)]


@pytest.mark.parametrize("shape", SHAPES_1X1 + SHAPES_3X3, ids=lambda s: "x".join(map(str, s)))
def test_forward_input_and_weight_gradient_against_float64(shape):
    B, H, W, K, N = shape[:5]
    d = shape[5] if len(shape) > 5 else 0
    k = 3 if d else 1
    gen = torch.Generator(device=DEV).manual_seed(sum(shape))
    x = torch.randn((B, K, H, W), device=DEV, generator=gen).contiguous(memory_format=CL)
    w = (torch.randn((N, K, k, k), device=DEV, generator=gen) / (K * k * k) ** 0.5).contiguous(memory_format=CL)
    dy = torch.randn((B, N, H, W), device=DEV, generator=gen).contiguous(memory_format=CL)
    _check_close(_fwd(x, w, d), _conv64(x, w, d), _conv64(x.abs(), w.abs(), d), f"forward {shape}")
    # input gradient: the forward call on the rearranged weight
    wt = (w.transpose(0, 1) if not d else w.flip(2, 3).transpose(0, 1)).contiguous(memory_format=CL)
    _check_close(_fwd(dy, wt, d), _conv64(dy, wt, d), _conv64(dy.abs(), wt.abs(), d), f"input gradient {shape}")
    _check_close(_wgrad(dy, x, d), _wgrad64(dy, x, w.shape, d), _wgrad64(dy.abs(), x.abs(), w.shape, d), f"weight gradient {shape}")


def test_accumulate_adds_to_the_output():
    gen = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn((2, 256, 33, 33), device=DEV, generator=gen).contiguous(memory_format=CL)
    w = torch.randn((128, 256, 1, 1), device=DEV, generator=gen).contiguous(memory_format=CL)
    y0 = torch.randn((2, 128, 33, 33), device=DEV, generator=gen).contiguous(memory_format=CL)
    y = _fwd(x, w, 0, y=y0.clone(), accumulate=True)
    ref = _conv64(x, w, 0) + y0.double()
    _check_close(y, ref, _conv64(x.abs(), w.abs(), 0) + y0.double().abs(), "accumulate")


@pytest.mark.parametrize("d", [0, 2])
def test_every_entry_point_is_bit_reproducible(d):
    gen = torch.Generator(device=DEV).manual_seed(5)
    k = 3 if d else 1
    x = torch.randn((24, 256, 33, 33), device=DEV, generator=gen).contiguous(memory_format=CL)
    w = torch.randn((256, 256, k, k), device=DEV, generator=gen).contiguous(memory_format=CL)
    dy = torch.randn((24, 256, 33, 33), device=DEV, generator=gen).contiguous(memory_format=CL)
    assert torch.equal(_fwd(x, w, d), _fwd(x, w, d))
    assert torch.equal(_wgrad(dy, x, d), _wgrad(dy, x, d))


def _count_calls(monkeypatch):
    calls = {"conv_f32": 0, "conv_f32_wgrad": 0}
    for name in calls:
        orig = getattr(hip, name)

        def shim(*a, _orig=orig, _name=name, **kw):
            calls[_name] += 1
            return _orig(*a, **kw)
        monkeypatch.setattr(hip, name, shim)
    return calls


@pytest.mark.parametrize("kind", ["1x1", "3x3"])
def test_layers_with_the_switch_against_float64(kind, f32_switch, monkeypatch):
    torch.manual_seed(0)
    if kind == "1x1":
        conv, d = blocks.Conv1x1(512, 256), 0
    else:
        conv, d = blocks.Conv3x3(256, 128, 3, stride=1, padding=6, dilation=6, bias=False), 6
    conv = conv.to(DEV).to(memory_format=CL)
    x = torch.randn((3, conv.in_channels, 33, 33), device=DEV).contiguous(memory_format=CL).requires_grad_(True)
    calls = _count_calls(monkeypatch)
    y = conv(x)
    dy = torch.randn_like(y)
    y.backward(dy)
    assert calls == {"conv_f32": 2, "conv_f32_wgrad": 1}
    w = conv.weight.detach()
    _check_close(y.detach(), _conv64(x.detach(), w, d), _conv64(x.detach().abs(), w.abs(), d), f"{kind} layer forward")
    xr = x.detach().double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    F.conv2d(xr, wr, None, 1, d, max(d, 1)).backward(dy.double())
    xa = x.detach().abs().double().requires_grad_(True)
    wa = w.abs().double().requires_grad_(True)
    F.conv2d(xa, wa, None, 1, d, max(d, 1)).backward(dy.abs().double())
    _check_close(x.grad, xr.grad, xa.grad, f"{kind} layer input gradient")
    _check_close(conv.weight.grad, wr.grad, wa.grad, f"{kind} layer weight gradient")
    # the frozen teacher's call (no autograd) takes the kernel too
    with torch.no_grad():
        assert torch.equal(conv(x), y)
    assert calls["conv_f32"] == 3


def test_switch_off_never_calls_the_kernels(monkeypatch):
    switches.unset("UCD_F32_OWN_CONV")
    calls = _count_calls(monkeypatch)
    for conv in (blocks.Conv1x1(256, 128), blocks.Conv3x3(128, 128, 3, stride=1, padding=2, dilation=2, bias=False)):
        conv = conv.to(DEV).to(memory_format=CL)
        x = torch.randn((2, conv.in_channels, 33, 33), device=DEV).contiguous(memory_format=CL).requires_grad_(True)
        conv(x).sum().backward()
        with torch.no_grad():
            conv(x)
    assert calls == {"conv_f32": 0, "conv_f32_wgrad": 0}


# ---- whole steps against the reference goldens ---------------------------------------------------------------------------------
# The uncalibrated VOC golden (teacher logits of 1e5) amplifies ANY conv-output error of the split kernels' size into its student
# train-mode logits: MIOpen fp32 itself, with every output of the same layers multiplied by (1 + 4.5e-6 N(0, 1)) - the relative
# L2 the split kernels measure against float64 on every shape above - lands at 4.7e-3 / 6.4e-3 / 6.6e-3 / 7.4e-3 for four noise
# seeds, 8.7e-4 at a tenth of that noise, 7.0e-4 without it; on the calibrated golden the same noise gives 3-4e-5
# (tools/f32_perturb_probe.py, profiles/r07_f32_perturb_probe.txt).  So that one quantity of that one golden gets an explicit bar
# calibrated on that spread (1e-2 relative L2, 1.35x its largest draw) in place of 5 tol; every other check of the step keeps the
# fp32 bars (losses and teacher logits 1e-3, running mean, gradient abs-sums 10 %) and the call counts below.
UNCAL_513_STUDENT_LOGITS_L2 = 1e-2
STEP_CASES = [("ucd_step_513.npz", "voc", "15-5", 513, range(16, 21), False, UNCAL_513_STUDENT_LOGITS_L2),
              ("ucd_step_513_cal.npz", "voc", "15-5", 513, range(16, 21), True, None),
              ("ucd_step_ade_512.npz", "ade", "100-50", 512, range(101, 151), True, None),
              ("ucd_step_city_768.npz", "city", "13-6", 768, range(14, 20), True, None)]


@pytest.mark.parametrize("gname,dataset,task,crop,ids,cal,logits_l2", STEP_CASES,
                         ids=["ucd_step_513", "ucd_step_513_cal", "ucd_step_ade_512", "ucd_step_city_768"])
def test_whole_fp32_step_on_the_split_kernels_matches_the_reference_golden(gname, dataset, task, crop, ids, cal, logits_l2, f32_switch,
                                                                         monkeypatch):
    """The arguments and bars of test_step_gpu's fp32 golden tests (losses and teacher logits 1e-3, student logits 5e-3 - on the
    uncalibrated golden the calibrated UNCAL_513_STUDENT_LOGITS_L2 - running mean, body gradient abs-sums 10 %) with the switch on; every Conv1x1 / Conv3x3 call of student and teacher that the gate accepts - counted
    by forward pre-hooks on the model's modules - went through the new kernels, forward, input gradient and weight gradient."""
    from test_step_gpu import _run_golden_step
    import ucd_amd.run as run
    calls = _count_calls(monkeypatch)
    expect = {"fwd": 0, "dgrad": 0, "wgrad": 0, "layers": 0, "seen": set()}
    orig_build = run.build_models

    def hook(mod, args):
        x = args[0]
        if blocks._f32_conv_ok(mod, x):
            expect["seen"].add(id(mod))
            expect["fwd"] += 1
            if torch.is_grad_enabled():
                expect["dgrad"] += int(x.requires_grad)
                M, taps = x.shape[0] * x.shape[2] * x.shape[3], mod.kernel_size[0] * mod.kernel_size[1]
                expect["wgrad"] += int(mod.weight.requires_grad and blocks._own_f32_wgrad(M, mod.in_channels, mod.out_channels, taps))

    def build(*a, **kw):
        models = orig_build(*a, **kw)
        for m in models:
            for mod in m.modules():
                if isinstance(mod, (blocks.Conv1x1, blocks.Conv3x3)):
                    mod.register_forward_pre_hook(hook)
                    # every map of these networks has >= 1024 rows: the gate's verdict on the layer's channels alone
                    if blocks._own_f32_conv(4096, mod.in_channels, mod.out_channels, mod.kernel_size[0] * mod.kernel_size[1]):
                        expect["layers"] += 1
        return models
    monkeypatch.setattr(run, "build_models", build)
    _run_golden_step(gname, dataset, task, 1, 42, crop, ids, calibrated=cal, train_logits_l2=logits_l2)
    print(gname, "conv_f32 calls", calls, "expected", {k: v for k, v in expect.items() if k != "seen"})
    assert expect["layers"] > 100 and len(expect["seen"]) == expect["layers"]      # every aligned layer of both networks
    assert calls["conv_f32"] == expect["fwd"] + expect["dgrad"]
    assert calls["conv_f32_wgrad"] == expect["wgrad"] > 0


def _o0_trajectory(steps, step_graph):
    """test_step_gpu._trajectory("O0", ...); for step_graph = "1" with the model behind the gradient-bucket wrapper the way bench.py
    runs the fp32 mode (fp32 weights, no bf16 working copies) - the whole-step graph needs the wrapper's fixed gradient addresses."""
    import test_step_gpu as T
    import ucd_amd.train as train
    from ucd_amd.ddp import DistributedDataParallel
    if step_graph == "0":
        return T._trajectory("O0", steps, step_graph=step_graph)
    orig_trainer = train.Trainer

    class WrappedTrainer(orig_trainer):
        def __init__(self, model, *a, **kw):
            if not hasattr(model, "finish_grad_sync"):
                model = DistributedDataParallel(model, delay_allreduce=True, bf16_weights=False)
            super().__init__(model, *a, **kw)
    train.Trainer = WrappedTrainer
    try:
        return T._trajectory("O0", steps, step_graph=step_graph)
    finally:
        train.Trainer = orig_trainer


def _trajectory_on_split_kernels(step_graph):
    from conftest import load_golden
    from test_step_gpu import TRAJ_UPDATE_NAMES
    g = load_golden("ucd_traj_513_cal.npz")
    steps = int(g["cfg"][3])
    f32, up32, ex32 = _o0_trajectory(steps, step_graph)
    for k in ("ce", "con", "lkd"):
        rel = np.abs(f32[k] - g[k]) / np.abs(g[k])
        print(k, "split kernels vs reference: first 5 max %.2e, all max %.2e" % (rel[:5].max(), rel.max()))
        assert rel[:5].max() < 1e-3, (k, rel)
        assert rel.max() < 5e-3, (k, rel)
    np.testing.assert_allclose(ex32["cls1_bias"], g["cls1_bias_after"], rtol=1e-3, atol=1e-6)
    np.testing.assert_allclose(ex32["running_mean"], g["running_mean_after"], rtol=1e-3, atol=1e-6)
    for i, n in enumerate(TRAJ_UPDATE_NAMES):
        ref = torch.from_numpy(g["upd"][i])
        idx = torch.from_numpy(np.linspace(0, up32[n].numel() - 1, ref.numel()).astype(np.int64))
        mine = up32[n].flatten()[idx]
        cos = float(mine @ ref / (mine.norm() * ref.norm() + 1e-300))
        ratio = float(up32[n].norm() / float(g["upd_norm"][i]))
        print(f"update over {steps} steps vs the reference: {n}: cosine {cos:.4f} length ratio {ratio:.3f}")
        assert cos > 0.99 and abs(ratio - 1.0) < 0.03, (n, cos, ratio)
    return ex32


def test_twenty_step_trajectory_on_the_split_kernels_against_the_reference(f32_switch, monkeypatch):
    calls = _count_calls(monkeypatch)
    _trajectory_on_split_kernels("0")
    assert calls["conv_f32"] > 0 and calls["conv_f32_wgrad"] > 0


def test_twenty_step_trajectory_replayed_from_a_graph_on_the_split_kernels(f32_switch, monkeypatch):
    calls = _count_calls(monkeypatch)
    ex = _trajectory_on_split_kernels("1")
    assert ex["graph_steps"] > 0
    assert calls["conv_f32"] > 0 and calls["conv_f32_wgrad"] > 0
