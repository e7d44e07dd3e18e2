"""GPU: weight gradients that the C++ autograd nodes leave non-final (a deferred slab sum, a product queued on the library's side
stream; include/ucd_hip.h ucd_conv_wgrad_ex flags) are correct only if nothing reads them before ucd_conv_wgrad_flush.  Every
entry point that passes such flags (conv_stride1, gemm1x1, gemm1x1_skip, conv_abn_train) is run under every deferral mode with
one early reader at a time - a preset ``.grad`` that AccumulateGrad adds into, ``create_graph=True``, a weight whose layout
AccumulateGrad re-strides, a tensor hook, a post-accumulate-grad hook - and what each reader saw is compared with a float64 CPU
weight gradient of the same operands (sparse small integers: every value is exact in bf16, so the comparison is bit for bit) or
with the same graph at mode 0.  ``node.wgrad_calls()`` shows which calls were issued deferred: every reader case must run
exactly as at mode 0, the plain case (nothing reads before the flush) must keep deferring.  The wrapper-level tests cover the
public-API trigger (bf16 layers under the default gradient-bucket wrapper, whose ``.grad`` views are pre-attached) and the
benchmarked step, which must keep deferring every own weight-gradient call."""
import pytest
import torch

from ucd_amd import switches, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = (1, 2, 3)
READERS = ("R0", "R1", "R2", "R4", "R5")


def _node():
    from ucd_amd import abn
    node = abn._abn_node()
    if node is None or not hasattr(node, "wgrad_calls"):
        pytest.skip("C++ autograd nodes not built")
    return node


def _ints(g, shape, hi, dens):
    """bf16 CPU tensor of small integers in [-hi, hi], a fraction ``dens`` of them nonzero."""
    return (torch.randint(-hi, hi + 1, shape, generator=g) * (torch.rand(shape, generator=g) < dens)).bfloat16()


def _rel(x, ref):
    return ((x.double() - ref).norm() / ref.norm()).item()


def _backward(reader, mode, forward, weights, dys, g0=None):
    """One forward + backward pass under deferral mode ``mode`` with the early reader ``reader`` on every weight of ``weights``.
    Returns ({weight index: [what the reader saw, .grad after the pass, .grad after a flush]}, (own weight-gradient calls of the
    pass, those issued deferred / for the side stream))."""
    from ucd_amd import hip
    node = _node()
    seen = {i: [] for i in range(len(weights))}
    hooks = []
    for i, w in enumerate(weights):
        w.grad = None
        if reader == "R1":
            w.grad = g0[i].clone()
        elif reader == "R4":
            hooks.append(w.register_hook(lambda g, i=i: seen[i].append(g.detach().clone())))
        elif reader == "R5":
            hooks.append(w.register_post_accumulate_grad_hook(lambda t, i=i: seen[i].append(t.grad.detach().clone())))
    torch.cuda.synchronize()
    assert hip.wgrad_defer(mode) == 0
    try:
        c0 = node.wgrad_calls()
        outs = forward()
        torch.autograd.backward(outs, dys, create_graph=reader == "R2")
        c1 = node.wgrad_calls()
        for i, w in enumerate(weights):
            seen[i].append(w.grad.detach().clone())
        hip.wgrad_flush()
        torch.cuda.synchronize()
        for i, w in enumerate(weights):
            seen[i].append(w.grad.detach().clone())
    finally:
        hip.wgrad_drop()
        hip.wgrad_defer(0)
        for h in hooks:
            h.remove()
        for w in weights:
            w.grad = None                          # (create_graph: the gradient references the graph of its own weight)
    return seen, (c1[0] - c0[0], c1[1] - c0[1])


def _check_calls(reader, mode, calls, n):
    """n own weight-gradient calls in the pass; deferred: all of them with nothing reading early, none otherwise."""
    assert calls[0] == n, (reader, mode, calls)
    assert calls[1] == (n if reader == "R0" else 0), (reader, mode, calls)


def _poison(*likes):
    """Fill free blocks of the allocator with NaN: an unsummed gradient then cannot inherit the right bits of an earlier case."""
    for t in [torch.full(x.shape, float("nan"), device=DEV, dtype=x.dtype) for x in likes for _ in range(3)]:
        del t


# ---- conv_stride1 (StrideOneConvNode: 1x1, 3x3 at dilation 1 and 2) ------------------------------------------------------------
STRIDE1 = [(1, 1, 128, 64), (3, 1, 64, 128), (3, 2, 64, 64)]          # kernel size, dilation, K (in), N (out)


def _stride1_case(k, d, K, N, seed, layout="cl", random=False):
    g = torch.Generator().manual_seed(seed)
    B, H, W = 2, 17, 19
    if random:
        x = torch.randn(B, K, H, W, generator=g).bfloat16()
        dy = torch.randn(B, N, H, W, generator=g).bfloat16()
    else:
        dens = (24.0 / (B * H * W)) ** 0.5
        x, dy = _ints(g, (B, K, H, W), 1, dens), _ints(g, (B, N, H, W), 2, dens)
    w = (torch.randn(N, K, k, k, generator=g) * 0.05).bfloat16()
    ref = torch.nn.grad.conv2d_weight(x.double(), w.shape, dy.double(), padding=d * (k // 2), dilation=d)
    g0 = _ints(g, (N, K, k, k), 3, 0.5)
    cl = torch.channels_last
    wd = w.to(DEV).contiguous(memory_format=cl if layout == "cl" else torch.contiguous_format).requires_grad_()
    return x.to(DEV).contiguous(memory_format=cl), dy.to(DEV).contiguous(memory_format=cl), wd, ref, g0.to(DEV).contiguous(memory_format=cl)


def _stride1_forward(x, w, d):
    from ucd_amd import hip
    node = _node()
    own_fwd = w.shape[2] == 3 and w.is_contiguous(memory_format=torch.channels_last)
    return lambda: [node.conv_stride1(x, w, d, None, own_fwd, False, hip.stream(), True)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,d,K,N,reader", [c + (r,) for c in STRIDE1 for r in READERS + (("R3",) if c[0] == 3 else ())])
def test_conv_stride1_weight_gradient_every_reader_sees_the_final_value(k, d, K, N, reader, mode):
    """(R3 only for the 3x3 layers: a 1x1 weight has one memory order in either format.)"""
    x, dy, w, ref, g0 = _stride1_case(k, d, K, N, 1000 * k + 100 * d + 10 * mode + (READERS + ("R3",)).index(reader),
                                      layout="nchw" if reader == "R3" else "cl")
    assert ref.abs().max().item() <= 64
    _poison(w)
    seen, calls = _backward(reader, mode, _stride1_forward(x, w, d), [w], [dy], [g0])
    want = ref + (g0.cpu().double() if reader == "R1" else 0)
    for v in seen[0]:
        assert torch.equal(v.cpu().double(), want), (reader, mode, (v.cpu().double() - want).abs().max().item())
    # R3: the node takes a 3x3 weight in NCHW order with the library's weight-gradient solver, never the own kernel
    _check_calls(reader, mode, calls, 0 if reader == "R3" else 1)


@pytest.mark.parametrize("reader", ("R0", "R1"))
@pytest.mark.parametrize("k,d,K,N", STRIDE1)
def test_conv_stride1_weight_gradient_on_random_operands(k, d, K, N, reader):
    x, dy, w, ref, g0 = _stride1_case(k, d, K, N, 31 + k + d, random=True)
    g0 = (torch.randn(g0.shape, device=DEV) * ref.abs().max().item()).bfloat16().contiguous(memory_format=torch.channels_last)
    for mode in MODES:
        _poison(w)
        seen, calls = _backward(reader, mode, _stride1_forward(x, w, d), [w], [dy], [g0])
        want = ref.to(DEV) + (g0.double() if reader == "R1" else 0)
        for v in seen[0]:
            assert _rel(v, want) < 3e-3, (reader, mode, _rel(v, want))
        _check_calls(reader, mode, calls, 1)


# ---- gemm1x1 / gemm1x1_skip (Gemm1x1Node, Gemm1x1SkipNode: own_wgrad_rows) -------------------------------------------------------
def _gemm_node():
    from ucd_amd import hip
    node = _node()
    if not hip.gemm_available():
        pytest.skip("ucd_gemm_load failed: no library GEMM")
    return node


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("reader", READERS)
@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("M,Ci,Co", [(1000, 128, 64), (8450, 64, 256)])
def test_gemm1x1_weight_gradient_every_reader_sees_the_final_value(M, Ci, Co, skip, reader, mode):
    from ucd_amd import hip
    node = _gemm_node()
    g = torch.Generator().manual_seed(M + Ci + 10 * mode + READERS.index(reader) + (500 if skip else 0))
    dens = (24.0 / M) ** 0.5
    rows, dy = _ints(g, (M, Ci), 1, dens), _ints(g, (M, Co), 2, dens)
    ref = (dy.double().t() @ rows.double()).view(Co, Ci, 1, 1)
    assert ref.abs().max().item() <= 64
    g0 = _ints(g, (Co, Ci, 1, 1), 3, 0.5).to(DEV)
    w = (torch.randn(Co, Ci, 1, 1, generator=g) * 0.05).bfloat16().to(DEV).requires_grad_()
    rows, dy = rows.to(DEV), dy.to(DEV)
    if skip:
        fwd = lambda: [node.gemm1x1_skip(rows, w, hip.stream(), True)[0]]
    else:
        fwd = lambda: [node.gemm1x1(rows, w, hip.stream(), True)]
    _poison(w)
    seen, calls = _backward(reader, mode, fwd, [w], [dy], [g0])
    want = ref + (g0.cpu().double() if reader == "R1" else 0)
    for v in seen[0]:
        assert torch.equal(v.cpu().double(), want), (reader, mode, (v.cpu().double() - want).abs().max().item())
    _check_calls(reader, mode, calls, 1)


@pytest.mark.parametrize("reader", ("R0", "R1"))
def test_gemm1x1_weight_gradient_on_random_operands(reader):
    from ucd_amd import hip
    node = _gemm_node()
    g = torch.Generator().manual_seed(3)
    M, Ci, Co = 8450, 128, 256
    rows, dy = torch.randn(M, Ci, generator=g).bfloat16(), torch.randn(M, Co, generator=g).bfloat16()
    ref = (dy.double().t() @ rows.double()).view(Co, Ci, 1, 1).to(DEV)
    g0 = (torch.randn(Co, Ci, 1, 1, device=DEV) * ref.abs().max().item()).bfloat16()
    w = (torch.randn(Co, Ci, 1, 1, generator=g) * 0.05).bfloat16().to(DEV).requires_grad_()
    rows, dy = rows.to(DEV), dy.to(DEV)
    for mode in MODES:
        _poison(w)
        seen, calls = _backward(reader, mode, lambda: [node.gemm1x1(rows, w, hip.stream(), True)], [w], [dy], [g0])
        want = ref + (g0.double() if reader == "R1" else 0)
        for v in seen[0]:
            assert _rel(v, want) < 3e-3, (reader, mode, _rel(v, want))
        _check_calls(reader, mode, calls, 1)


# ---- conv_abn_train through ResidualBlock (ConvABNTrainNode: the 1x1, 3x3 and strided weight gradients) ------------------------
BLOCKS = [(256, (64, 64, 256), 1, 1, 33), (256, (128, 128, 512), 2, 1, 33), (128, (64, 64, 128), 1, 2, 33)]


def _block(cin, chans, stride, dil):
    """A bottleneck block whose convolution weights are bf16 leaves (the ABN parameters stay fp32): every own weight-gradient call
    of its conv + ABN nodes sees the parameter itself."""
    from functools import partial
    from ucd_amd import abn, blocks
    norm = partial(abn.InPlaceABNSync, activation="leaky_relu", activation_param=0.01)
    blk = blocks.ResidualBlock(cin, chans, norm_act=norm, stride=stride, dilation=dil)
    blk.load_state_dict(synth.fill_state_dict(blk.state_dict(), 5))
    for m in blk.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.bfloat16()
    return blk.to(DEV).to(memory_format=torch.channels_last).train()


@pytest.mark.usefixtures("deterministic_stats")
@pytest.mark.parametrize("cin,chans,stride,dil,hw", BLOCKS)
def test_conv_abn_weight_gradients_every_reader_sees_the_mode0_bits(cin, chans, stride, dil, hw):
    blk = _block(cin, chans, stride, dil)
    ws = [p for n, p in blk.named_parameters() if p.dim() == 4]
    B = 4
    x = (synth.t_normal(9, (B, cin, hw, hw), stream=1)).to(DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    oh = (hw - 1) // stride + 1
    dy = synth.t_normal(10, (B, chans[2], oh, oh), stream=1).to(DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(11)
    g0 = [_ints(g, tuple(w.shape), 3, 0.5).to(DEV).contiguous(memory_format=torch.channels_last) for w in ws]
    fwd = lambda: [blk(x.clone().requires_grad_(True))]
    keep = []                                          # every result stays referenced: no later buffer inherits its bits
    torch.backends.cudnn.deterministic = True          # (the strided block's input gradient stays with the library's solver)
    try:
        for reader in ("R0", "R1", "R4", "R5"):
            want, n0 = _backward(reader, 0, fwd, ws, [dy], g0)
            keep.append(want)
            assert n0[0] >= (2 if stride == 1 else 3), n0      # the 1x1 layers (+ the strided 3x3 and projection) on the own kernel
            for mode in MODES:
                _poison(*ws)
                got, calls = _backward(reader, mode, fwd, ws, [dy], g0)
                keep.append(got)
                for i in want:
                    for a in got[i]:
                        assert torch.equal(a, want[i][-1]), (reader, mode, i)
                _check_calls(reader, mode, calls, n0[0])
    finally:
        torch.backends.cudnn.deterministic = False


# ---- the gradient-bucket wrapper ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero_where", ["before", "after"])
def test_bf16_layers_under_the_default_wrapper_follow_the_plain_model(zero_where):
    """bf16 channels-last Conv3x3 / Conv1x1 layers under ``DistributedDataParallel(model)`` (default: no working copies): each weight
    is its own leaf parameter, and its ``.grad`` a bucket view the wrapper attached before the backward - AccumulateGrad adds the
    nodes' weight gradients into it the moment they arrive, before any flush.  Three steps of the reference's plain loop follow the
    unwrapped model (which never defers) bit for bit, and the first step's weight gradients agree with a float64 run."""
    from ucd_amd import blocks
    from ucd_amd.ddp import DistributedDataParallel

    def net():
        torch.manual_seed(0)
        m = torch.nn.Sequential(blocks.Conv3x3(64, 64, 3, padding=1, dilation=1, bias=False),
                                blocks.Conv3x3(64, 64, 3, padding=2, dilation=2, bias=False), blocks.Conv1x1(64, 128))
        for c in m:
            torch.nn.init.normal_(c.weight, std=0.05)
        return m.to(DEV).bfloat16().to(memory_format=torch.channels_last).train()

    B, H, W = 2, 65, 65                                              # M = 8450 >= 8192
    x = synth.t_normal(31, (B, 64, H, W), stream=1).to(DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    dy = synth.t_normal(32, (B, 128, H, W), stream=1).to(DEV).contiguous(memory_format=torch.channels_last)
    node = _gemm_node()
    plain, wrapped = net(), DistributedDataParallel(net())
    opts = [torch.optim.SGD(m.parameters(), lr=0.05, momentum=0.9) for m in (plain, wrapped)]
    for step in range(3):
        grads = []
        for m, opt in zip((plain, wrapped), opts):
            c0 = node.wgrad_calls()
            if zero_where == "before":
                opt.zero_grad()
                y = m(x)
            else:
                y = m(x)
                opt.zero_grad()
            (y.float() * dy).sum().backward()
            c1 = node.wgrad_calls()
            assert c1[0] - c0[0] == 3, (c0, c1)                       # every layer on the own weight-gradient kernel
            grads.append([p.grad.detach().clone() for p in m.parameters()])
            opt.step()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(*grads)):
            assert torch.equal(a, b), (step, i, (a.float() - b.float()).abs().max().item())
        for (n, p), (_, q) in zip(plain.named_parameters(), wrapped.module.named_parameters()):
            assert torch.equal(q, p), (n, step)
        if step == 0:
            ref = net().cpu().double()                              # the same bf16 weights, every product in float64
            (ref(x.cpu().double()) * dy.cpu().double()).sum().backward()
            for a, r in zip(grads[1], ref.parameters()):
                assert _rel(a.cpu(), r.grad) < 1e-2, _rel(a.cpu(), r.grad)


# own weight-gradient calls of one eager step of the benchmarked model at this size, every one of them deferred - the count measured
# before deferral was gated on the early readers (the gate must not change it)
BENCH_STEP_CALLS = 108


def test_the_benchmarked_step_keeps_deferring_every_weight_gradient():
    """One eager step of the model bench.py measures (working copies, default switches, a small crop): every own weight-gradient call
    of the pass is issued deferred / for the side stream - the working copies' only post-accumulate-grad hook is the wrapper's,
    which reads no values before its flush."""
    from ucd_amd import argparser, tasks
    from ucd_amd.ddp import DistributedDataParallel
    from ucd_amd.run import build_models, load_step_checkpoint, make_optimizer
    from ucd_amd.train import Trainer
    node = _node()
    opts = argparser.modify_command_options(argparser.get_argparser().parse_args(
        ["--method", "UCD", "--dataset", "voc", "--task", "15-5", "--step", "1", "--lr", "0.001", "--no_pretrained",
         "--norm_act", "iabn_sync", "--opt_level", "O1"]))
    classes = tasks.get_per_task_classes("voc", "15-5", 1)
    dev = torch.device(DEV)
    model, model_old = build_models(opts, dev, classes)
    state = synth.fill_state_dict({k: v.cpu() for k, v in model_old.state_dict().items()}, 42, calibrated=True)
    optim = make_optimizer(opts, model)
    model = DistributedDataParallel(model, delay_allreduce=True, bf16_weights=True)
    load_step_checkpoint(opts, model, model_old, state, dev)
    switches.set("UCD_STEP_GRAPH", "0")
    try:
        trainer = Trainer(model, model_old, device=dev, opts=opts, classes=classes)
        model.train()
        counts = []
        for it in range(2):
            img = synth.images(700 + it, 2, 129)
            labels = synth.seg_labels(700 + it, 2, 129, 129, range(16, 21))
            c0 = node.wgrad_calls()
            trainer.train_step(img, labels, optim)
            torch.cuda.synchronize()
            c1 = node.wgrad_calls()
            counts.append((c1[0] - c0[0], c1[1] - c0[1]))
    finally:
        switches.unset("UCD_STEP_GRAPH")
    print("own weight-gradient calls per step (all, deferred):", counts)
    for n, deferred in counts:
        assert n == BENCH_STEP_CALLS and deferred == n, counts
