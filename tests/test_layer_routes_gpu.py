"""GPU: the host path of the convolution layers decides and launches what it did when tests/golden/layer_routes.json was recorded
(tests/golden/make_layer_routes_golden.py, run at the commit in front of the one that retired the layers' library arms).  Three
records of the 2 x 129^2 bf16 (--opt_level O1) student + teacher step of tests/test_step_gpu.py, compared for exact equality:

* routes: what ``blocks._conv_abn_route`` decided for every conv + ABN pair of one training forward, in call order;
* calls: with the C++ nodes switched off the way bench.py's instrumented pass does it, every ``hip._timed`` entry
  (call name, work, flops) of one whole training step and of one teacher forward under ``no_grad``, in launch order - the values
  bench.py's kernel table and roofline classification are computed from;
* gate: the autograd node a ``Conv1x1(256, 21)`` (off the 64-channel grid) builds on either side of its 8192-row bound.
"""
import json
import os

import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "layer_routes.json")
GATE_SHAPES = ((2, 256, 64, 64), (2, 256, 63, 64))          # M = 8192 and M = 8064


def _route_entry(r):
    if r is None:
        return None
    return {"is3": bool(r.is3), "stride": int(r.stride), "dilation": int(r.dilation), "own_dgrad": bool(r.own_dgrad),
            "wflip": r.wflip is not None, "wgrad_conv": int(r.wgrad_conv), "link": None if r.link is None else int(r.link.kind),
            "make_link": bool(r.make_link)}


def record_step(on_route=None):
    """{"routes": [...], "step_calls": [...], "teacher_calls": [...]} of the step described in the module docstring.  ``on_route``
    sees every route as ``_conv_abn_route`` returned it (the recording script checks the field this test cannot know about)."""
    from test_step_gpu import _build, _opts
    from ucd_amd import abn, blocks, hip, synth
    from ucd_amd.ddp import DistributedDataParallel
    from ucd_amd.run import make_optimizer
    from ucd_amd.train import Trainer
    dev = torch.device("cuda:0")
    opts = _opts(["--opt_level", "O1"])
    opts.graph_teacher = False
    model, model_old, classes = _build(opts, dev)
    optim = make_optimizer(opts, model)
    ddp = DistributedDataParallel(model, bf16_weights=True)
    trainer = Trainer(ddp, model_old, device=dev, opts=opts, classes=classes)
    img = synth.images(501, 2, 129)
    labels = synth.seg_labels(501, 2, 129, 129, range(16, 21))
    ddp.train()

    routes, calls = [], []
    route_fn, timed_fn = blocks._conv_abn_route, hip._timed

    def route(*args, **kwargs):
        r = route_fn(*args, **kwargs)
        if on_route is not None:
            on_route(r)
        routes.append(_route_entry(r))
        return r

    def timed(name, work, flops=None, staged=None):
        calls.append([name, work, flops])
        return timed_fn(name, work, flops, staged)

    blocks._conv_abn_route = route
    try:
        trainer.train_step(img, labels, optim, None)              # the first iteration is eager: one training forward
    finally:
        blocks._conv_abn_route = route_fn
    torch.cuda.synchronize()

    # bench.py::kernel_timing: no C++ nodes (their Python twins issue the same library calls), no graphs, no side stream
    saved = (abn._node_mod, trainer.graph_teacher, trainer._side, blocks._node_cache[0], trainer.step_graph)
    abn._abn_node()
    abn._node_mod, trainer.graph_teacher, trainer._side, trainer.step_graph = None, False, None, False
    blocks._node_cache[0] = None
    try:
        trainer.train_step(img, labels, optim, None)              # the twins' first run (tuning, caches) stays unrecorded
        torch.cuda.synchronize()
        hip.enable_call_timing()
        hip._timed = timed
        try:
            trainer.train_step(img, labels, optim, None)
            torch.cuda.synchronize()
            step_calls = list(calls)
            del calls[:]
            trainer._teacher_eager(img.to(dev).contiguous(memory_format=torch.channels_last),
                                   {"upsample": False} if trainer.fuse_logit_losses else {})
            torch.cuda.synchronize()
            teacher_calls = list(calls)
        finally:
            hip._timed = timed_fn
            hip.disable_call_timing()
    finally:
        abn._node_mod, trainer.graph_teacher, trainer._side, blocks._node_cache[0], trainer.step_graph = saved
    return {"routes": routes, "step_calls": step_calls, "teacher_calls": teacher_calls}


def record_gate():
    """grad_fn type name of a ``Conv1x1(256, 21)`` under autocast for each of GATE_SHAPES, keyed by the row count M."""
    from ucd_amd.blocks import Conv1x1
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    conv = Conv1x1(256, 21).to(dev).to(memory_format=torch.channels_last)
    out = {}
    for shape in GATE_SHAPES:
        x = torch.randn(shape, device=dev, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = conv(x)
        assert tuple(y.shape) == (shape[0], 21, shape[2], shape[3])
        out[str(shape[0] * shape[2] * shape[3])] = type(y.grad_fn).__name__
    return out


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def step():
    return json.loads(json.dumps(record_step()))          # tuples / ints as the fixture file holds them


def _assert_same(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{what} #{i}: got {a}, recorded {b}"
    assert len(got) == len(want), f"{what}: {len(got)} entries, recorded {len(want)}"


def test_every_conv_abn_pair_takes_its_recorded_route(step, golden):
    assert len(golden["routes"]) > 100 and all(golden["routes"])        # 103 pairs, none of them on the module path
    _assert_same(step["routes"], golden["routes"], "route")


def test_the_twins_issue_the_recorded_calls_in_order(step, golden):
    assert len(golden["step_calls"]) > 500 and len(golden["teacher_calls"]) > 50
    _assert_same(step["step_calls"], golden["step_calls"], "call of the training step")
    _assert_same(step["teacher_calls"], golden["teacher_calls"], "call of the teacher forward")


def test_off_grid_1x1_layer_keeps_its_row_count_gate(golden):
    assert sorted(golden["gate"]) == ["8064", "8192"] and golden["gate"]["8064"] != golden["gate"]["8192"]
    assert record_gate() == golden["gate"]
