"""CPU: the host half of the fused BCE losses (ucd_seg_bce, csrc/seg_gather.hip) - the exported symbols, every host-side rejection
(decided before any device call: no GPU is needed to hear them), the float64 restatement of the formulas (seg_bce_ref.py) against
the reference's own numbers (tests/golden/bce_losses.npz), and the Trainer's refusals: the BCE family exists on the GPU only,
--icarl_disjoint with a teacher not at all."""
import ctypes as C
import types

import pytest
import torch

from conftest import load_golden
import seg_bce_ref as R

EINVAL, EWORKSPACE = -1, -3


def test_symbols_are_exported():
    from ucd_amd import hip
    assert "ucd_seg_bce" in hip.SIGNATURES and "ucd_seg_bce_workspace_bytes" in hip.SIGNATURES
    lib = hip.load()
    assert lib.ucd_seg_bce is not None and lib.ucd_seg_bce_workspace_bytes is not None
    assert lib.ucd_seg_bce_workspace_bytes(2, 9, 9) == 2 * 9 * 9 * 2 * 4
    assert lib.ucd_version() == 100


def _call(lib, **over):
    """ucd_seg_bce on host buffers that no accepted call would take: every case here is refused before a device call."""
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    a = dict(sem_s=p, ld_s=21, sem_t=p, ld_t=16, labels=p, B=2, H=129, W=129, h=9, w=9, Ctot=21, K=16, ignore=255, hard=1.0, soft=10.0,
             loss_out=p, d_sem=p, ld_d=21, workspace=p, workspace_bytes=lib.ucd_seg_bce_workspace_bytes(2, 9, 9))
    a.update(over)
    rc = lib.ucd_seg_bce(a["sem_s"], a["ld_s"], a["sem_t"], a["ld_t"], a["labels"], a["B"], a["H"], a["W"], a["h"], a["w"], a["Ctot"],
                         a["K"], a["ignore"], a["hard"], a["soft"], a["loss_out"], a["d_sem"], a["ld_d"], a["workspace"],
                         a["workspace_bytes"], None)
    return rc, lib.ucd_last_error().decode()


REJECTIONS = [
    ("sem_s NULL", dict(sem_s=None), EINVAL), ("labels NULL", dict(labels=None), EINVAL), ("loss_out NULL", dict(loss_out=None), EINVAL),
    ("workspace NULL", dict(workspace=None), EINVAL),
    ("B 0", dict(B=0), EINVAL), ("H -1", dict(H=-1), EINVAL), ("W 0", dict(W=0), EINVAL), ("h 0", dict(h=0), EINVAL),
    ("w 0", dict(w=0), EINVAL), ("Ctot 0", dict(Ctot=0), EINVAL),
    ("K 0", dict(K=0), EINVAL), ("K > Ctot", dict(K=22), EINVAL),
    ("ld_s < Ctot", dict(ld_s=20), EINVAL), ("ld_t < K", dict(ld_t=15), EINVAL), ("ld_d < Ctot", dict(ld_d=20), EINVAL),
    ("H < h", dict(H=8), EINVAL), ("W < w", dict(W=8), EINVAL),
    ("short workspace", dict(workspace_bytes=2 * 9 * 9 * 2 * 4 - 1), EWORKSPACE),
]


@pytest.mark.parametrize("what,over,code", REJECTIONS, ids=[r[0] for r in REJECTIONS])
def test_host_side_rejections(what, over, code):
    from ucd_amd import hip
    rc, msg = _call(hip.load(), **over)
    assert rc == code, (what, rc, msg)
    assert msg.startswith("ucd_seg_bce:") and len(msg) > len("ucd_seg_bce: "), msg


def test_leading_dimensions_of_absent_operands_are_not_checked():
    """ld_t only counts with a teacher, ld_d only with d_sem: the call gets past them to the next check (the short workspace)."""
    from ucd_amd import hip
    rc, msg = _call(hip.load(), sem_t=None, ld_t=0, d_sem=None, ld_d=0, workspace_bytes=1)
    assert rc == EWORKSPACE, (rc, msg)


@pytest.mark.parametrize("shape", R.GOLDEN_SHAPES, ids=R.golden_key)
def test_restatement_reproduces_the_reference(shape):
    """The three formulas in float64 against the reference's modules in float64: losses rel 1e-6, gradients 1e-5 of the largest
    element (the reference casts its one-hot targets to float32, and the golden stores the gradient as float32)."""
    gold = load_golden("bce_losses.npz")
    sem, sem_t, labels = R.golden_inputs(shape)
    assert float(gold[R.golden_key(shape) + "|ignored"]) == pytest.approx((labels == 255).double().mean().item(), abs=1e-12)
    l_bce, l_soft, grad = R.restatement(sem, sem_t, labels, R.HARD_W, R.SOFT_W)
    ref = gold[R.golden_key(shape) + "|loss"]
    print(shape, "bce", l_bce, ref[0], "soft", l_soft, ref[1])
    assert l_bce == pytest.approx(ref[0], rel=1e-6) and l_soft == pytest.approx(ref[1], rel=1e-6)
    err, gmax = R.golden_grad_errors(gold, R.golden_key(shape) + "|grad", grad.numpy())
    print("gradient: max error", err, "of", gmax)
    assert err <= 1e-5 * gmax


@pytest.mark.parametrize("args", [["--bce"], ["--method", "LWF-MC"], ["--icarl"]], ids=lambda a: " ".join(a))
def test_trainer_on_a_cpu_device_raises(args):
    from ucd_amd import argparser
    from ucd_amd.train import Trainer
    opts = argparser.modify_command_options(argparser.get_argparser().parse_args(
        [*args, "--task", "15-5", "--step", "1", "--no_pretrained"]))
    with pytest.raises(NotImplementedError, match="BCE / iCaRL.*GPU only"):
        Trainer(torch.nn.Linear(2, 2), torch.nn.Linear(2, 2), torch.device("cpu"), opts, classes=[16, 5])


def test_icarl_disjoint_with_a_teacher_is_refused():
    """Decided before anything touches the device: a stand-in device object of type "cuda" is enough to reach the refusal.  At step
    0 (no teacher) the same options are plain BCE and are not refused for being disjoint."""
    from ucd_amd import argparser
    from ucd_amd.train import Trainer
    opts = argparser.modify_command_options(argparser.get_argparser().parse_args(
        ["--icarl", "--icarl_disjoint", "--task", "15-5", "--step", "1", "--no_pretrained"]))
    gpu = types.SimpleNamespace(type="cuda")
    with pytest.raises(NotImplementedError, match=r"BCE / iCaRL.*train\.py:110-116"):
        Trainer(torch.nn.Linear(2, 2), torch.nn.Linear(2, 2), gpu, opts, classes=[16, 5])
    with pytest.raises(NotImplementedError, match="BCE / iCaRL.*GPU only"):
        Trainer(torch.nn.Linear(2, 2), None, torch.device("cpu"), opts, classes=[16])


def test_fused_seg_bce_has_no_cpu_path():
    from ucd_amd.loss import fused_seg_bce
    with pytest.raises(RuntimeError, match="GPU only"):
        fused_seg_bce(torch.zeros(1, 5, 2, 2), None, torch.zeros(1, 8, 8, dtype=torch.long))
