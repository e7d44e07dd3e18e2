"""CPU: the loss pairs of the reference's --method table behind the fused logit-loss kernel.  (1) the torch modules of
ucd_amd/loss.py - the twin the GPU tests use at sizes the goldens do not cover - reproduce the reference's own numbers
(tests/golden/kd_losses.npz, tests/golden/make_kd_golden.py); (2) the argument rules of ucd_seg_losses_ex, which run on the
host before any device call; (3) ucd_seg_losses_plan_ex: form, cells and LDS bytes do not depend on the distillation mode;
(4) the argument rules of ucd_attn_mse."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import assert_matches_compact, load_golden
from ucd_amd import hip

EINVAL = -1


def test_torch_modules_reproduce_the_reference_golden():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_kd_golden as MK
    from ucd_amd.loss import KnowledgeDistillationLoss, UnbiasedCrossEntropy, UnbiasedKnowledgeDistillationLoss
    gold = load_golden("kd_losses.npz")
    seen = 0
    for shape in MK.UNIT_SHAPES:
        B, Ctot, K, h, H = shape
        sem, sem_t, labels = MK.unit_inputs(shape)
        assert int((labels == 255).sum()) and int(((labels > 0) & (labels < K)).sum()) and int((labels >= K).sum())
        up = lambda t: F.interpolate(t, size=(H, H), mode="bilinear", align_corners=False)
        t_up = up(sem_t.double())
        for kd in ("plain", "unbiased"):
            for alpha in MK.ALPHAS:
                for ce in ("plain", "unbiased"):
                    s = sem.double().requires_grad_(True)
                    u = up(s)
                    crit = (nn.CrossEntropyLoss(ignore_index=255, reduction="none") if ce == "plain" else
                            UnbiasedCrossEntropy(old_cl=K, ignore_index=255, reduction="none"))
                    l_ce = crit(u, labels.clone()).mean()
                    l_kd = (KnowledgeDistillationLoss if kd == "plain" else UnbiasedKnowledgeDistillationLoss)(alpha=alpha)(u, t_up)
                    assert l_ce.dtype == torch.float64 and l_kd.dtype == torch.float64
                    (MK.UNIT_CE_W * l_ce + MK.UNIT_KD_W * l_kd).backward()
                    key = MK.unit_key(shape, kd, alpha, ce)
                    np.testing.assert_allclose([l_ce.item(), l_kd.item()], gold[key + "|loss"], rtol=1e-6, err_msg=key)
                    # gradients are stored as float32 (2^-24 relative): 1e-6 of an element plus 1e-6 of the largest one
                    g = s.grad.numpy()
                    assert_matches_compact(gold, key + "|grad", g, rtol=1e-6, atol=1e-6 * float(np.abs(g).max()))
                    seen += 1
    assert seen == 36


def _ex(**kw):
    """ucd_seg_losses_ex on host buffers, no stream: an argument error returns before anything touches a device."""
    lib = hip.load()
    buf = np.zeros(4096, dtype=np.float32)
    p = buf.ctypes.data
    a = dict(sem_t=p, Ctot=21, K=16, ce_old_cl=16, kd_mode=hip.KD_UNBIASED, alpha=1.0)
    a.update(kw)
    rc = lib.ucd_seg_losses_ex(p, a["Ctot"], a["sem_t"], a["K"], p, 1, 64, 64, 4, 4, a["Ctot"], a["K"], a["ce_old_cl"], a["kd_mode"],
                               a["alpha"], 255, 1.0, 1.0, p, p, a["Ctot"], p, 0, None)
    assert not buf.any()
    return rc, lib.ucd_last_error().decode()


@pytest.mark.parametrize("kw,names", [
    (dict(kd_mode=2), "kd_mode"), (dict(kd_mode=-1), "kd_mode"),
    (dict(alpha=0.0), "alpha"), (dict(alpha=float("nan")), "alpha"), (dict(alpha=float("inf")), "alpha"),
    (dict(alpha=float("-inf")), "alpha"),
    (dict(ce_old_cl=5), "ce_old_cl"), (dict(ce_old_cl=15, kd_mode=1), "ce_old_cl"),
    (dict(ce_old_cl=22), "ce_old_cl"), (dict(ce_old_cl=22, sem_t=None), "ce_old_cl"), (dict(ce_old_cl=0), "ce_old_cl"),
])
def test_ex_argument_errors_need_no_device(kw, names):
    rc, msg = _ex(**kw)
    assert rc == EINVAL and names in msg and "ucd_seg_losses_ex" in msg, (kw, rc, msg)


def test_ex_legal_arguments_pass_the_argument_checks():
    """The legal pairs get past the argument rules: what stops them here is the workspace of 0 bytes (still no device call)."""
    for kw in (dict(), dict(ce_old_cl=1), dict(kd_mode=1), dict(kd_mode=1, ce_old_cl=1, alpha=0.5), dict(alpha=-2.0),
               dict(sem_t=None, ce_old_cl=7)):
        rc, msg = _ex(**kw)
        assert rc == -3 and "workspace too small" in msg, (kw, rc, msg)


def _plans(H, W, h, w, Ctot, K, ce_old_cl, kd_mode, teacher, aligned, pk):
    lib = hip.load()
    f, ny, nx, lds = C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
    rc = lib.ucd_seg_losses_plan_ex(H, W, h, w, Ctot, K, ce_old_cl, kd_mode, teacher, aligned, pk, C.byref(f), C.byref(ny), C.byref(nx),
                                    C.byref(lds))
    ex = (rc, f.value, ny.value, nx.value, lds.value) if rc == 0 else (rc,)
    rc = lib.ucd_seg_losses_plan(H, W, h, w, Ctot, K, teacher, aligned, pk, C.byref(f), C.byref(ny), C.byref(nx), C.byref(lds))
    return ex, ((rc, f.value, ny.value, nx.value, lds.value) if rc == 0 else (rc,))


def test_plan_ex_does_not_depend_on_the_mode():
    """The benchmark pins of tests/test_seglosses_cpu.py and a sweep of class splits, aligned or not, packed forms allowed or
    not: the same answer for plain and unbiased distillation and for either cross entropy, equal to ucd_seg_losses_plan."""
    assert _plans(513, 513, 33, 33, 21, 16, 1, hip.KD_PLAIN, 1, 1, 1)[0] == (0, 1, 6, 6, 65544)
    assert _plans(512, 512, 32, 32, 21, 16, 1, hip.KD_PLAIN, 1, 1, 1)[0] == (0, 1, 6, 6, 65544)
    assert _plans(512, 512, 32, 32, 151, 101, 1, hip.KD_PLAIN, 1, 1, 1)[0] == (0, 6, 4, 6, 83040)
    n = 0
    for H, h in ((513, 33), (512, 32), (512, 64), (190, 12)):
        for Ctot in (2, 17, 20, 21, 24, 25, 41, 151):
            for K in sorted({1, 2, Ctot // 2, Ctot - 5, Ctot - 1, Ctot} & set(range(1, Ctot + 1))):
                for aligned in (0, 1):
                    for pk in (0, 1):
                        base = _plans(H, H, h, h, Ctot, K, K, hip.KD_UNBIASED, 1, aligned, pk)
                        assert base[0] == base[1], (H, h, Ctot, K, aligned, pk, base)
                        for ce_old_cl in (1, K):
                            for mode in (hip.KD_UNBIASED, hip.KD_PLAIN):
                                assert _plans(H, H, h, h, Ctot, K, ce_old_cl, mode, 1, aligned, pk)[0] == base[0]
                                n += 1
    assert n > 1000


def test_plan_ex_without_a_teacher_splits_at_the_cross_entropy_count():
    ex, _ = _plans(513, 513, 33, 33, 21, 21, 16, hip.KD_UNBIASED, 0, 1, 1)
    _, bare = _plans(513, 513, 33, 33, 21, 16, 16, hip.KD_UNBIASED, 0, 1, 1)
    assert ex == bare and ex[1] == 1
    lib = hip.load()
    assert lib.ucd_seg_losses_plan_ex(513, 513, 33, 33, 21, 16, 5, 0, 1, 1, 1, None, None, None, None) == EINVAL
    assert "ce_old_cl" in lib.ucd_last_error().decode()
    assert lib.ucd_seg_losses_plan_ex(513, 513, 33, 33, 21, 16, 16, 2, 1, 1, 1, None, None, None, None) == EINVAL
    assert "kd_mode" in lib.ucd_last_error().decode()


def _attn(**kw):
    """ucd_attn_mse on host buffers (16-byte aligned), no stream: an argument error returns before anything touches a device."""
    lib = hip.load()
    buf = np.zeros(8192 + 4, dtype=np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    B, HW, C = 2, 9, 16
    need = lib.ucd_attn_mse_workspace_bytes(B, HW)
    a = dict(x_s=p, x_t=p, out=p, d=p, ws=p, nbytes=need, dtype=hip.F32, B=B, HW=HW, C=C, ld=C)
    a.update(kw)
    rc = lib.ucd_attn_mse(a["x_s"], a["ld"], a["x_t"], a["ld"], a["dtype"], a["B"], a["HW"], a["C"], 1.0, a["out"], a["d"], a["ld"],
                          a["ws"], a["nbytes"], None)
    assert not buf.any()
    return rc, lib.ucd_last_error().decode(), need


@pytest.mark.parametrize("kw,code,text", [
    (dict(x_s=None), EINVAL, "NULL"), (dict(x_t=None), EINVAL, "NULL"), (dict(out=None), EINVAL, "NULL"), (dict(d=None), EINVAL, "NULL"),
    (dict(C=0), EINVAL, "C = 0"), (dict(C=-3), EINVAL, "C = -3"), (dict(dtype=2), EINVAL, "dtype"), (dict(dtype=-1), EINVAL, "dtype"),
    (dict(B=0), EINVAL, "bad sizes"), (dict(HW=0), EINVAL, "bad sizes"), (dict(C=20, ld=16), EINVAL, "leading dimension"),
    (dict(C=3, ld=3), -2, "16-byte"),
    (dict(ws=None), -3, "workspace"), (dict(nbytes=0), -3, "workspace"),
])
def test_attn_mse_argument_errors_need_no_device(kw, code, text):
    rc, msg, need = _attn(**kw)
    assert rc == code and text in msg and "ucd_attn_mse" in msg, (kw, rc, msg)
    if "nbytes" not in kw and "ws" not in kw:
        return
    assert need > 0 and _attn(nbytes=need - 1)[0] == -3
