"""CPU: the host half of the gather form of the fused logit losses (ucd_seg_losses_gather, csrc/seg_gather.hip; DESIGN.md
section 3.5.5) - which geometries ``seg_losses_route`` sends to it (exactly those ucd_seg_losses_plan_ex refuses as unsupported) and
every host-side rejection of the entry point (decided before any device call: no GPU is needed to hear them)."""
import ctypes as C

import pytest
import torch

EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -3, -4

# (H, W, h, w), Ctot, K, has_teacher
GATHER = [((512, 512, 64, 64), 151, 101, True), ((512, 512, 64, 64), 111, 101, True), ((512, 512, 64, 64), 151, 101, False),
          ((512, 512, 64, 64), 151, 151, False), ((129, 129, 17, 17), 151, 141, True), ((64, 64, 16, 16), 21, 16, True),
          ((48, 48, 16, 16), 21, 16, True)]
TILED = [((513, 513, 33, 33), 21, 16, True), ((192, 192, 24, 24), 21, 16, True), ((512, 512, 32, 32), 151, 101, True),
         ((512, 512, 64, 64), 101, 51, True)]


def _id(case):
    (H, W, h, w), Ctot, K, teacher = case
    return f"{H}x{W}-{h}x{w}-{Ctot}-{K}" + ("" if teacher else "-no_teacher")


def test_symbols_are_exported():
    from ucd_amd import hip
    assert "ucd_seg_losses_gather" in hip.SIGNATURES and "ucd_seg_losses_gather_workspace_bytes" in hip.SIGNATURES
    lib = hip.load()
    assert lib.ucd_seg_losses_gather_workspace_bytes(2, 17, 17) == 2 * 17 * 17 * 2 * 4
    assert lib.ucd_seg_losses_gather_workspace_bytes(0, 17, 17) == 0


@pytest.mark.parametrize("case", GATHER, ids=_id)
def test_route_is_gather_where_the_plan_refuses(case):
    from ucd_amd import hip
    from ucd_amd.loss import seg_losses_route
    geom, Ctot, K, teacher = case
    assert seg_losses_route(*geom, Ctot, K, teacher) == "gather"
    assert hip.load().ucd_seg_losses_plan(*geom, Ctot, K, int(teacher), 1, -1, None, None, None, None) == EUNSUPPORTED


@pytest.mark.parametrize("case", TILED, ids=_id)
def test_route_is_tiled_where_the_plan_serves(case):
    from ucd_amd import hip
    from ucd_amd.loss import seg_losses_route
    geom, Ctot, K, teacher = case
    assert seg_losses_route(*geom, Ctot, K, teacher) == "tiled"
    assert hip.load().ucd_seg_losses_plan(*geom, Ctot, K, int(teacher), 1, -1, None, None, None, None) == 0


def test_route_takes_the_cross_entropy_split_and_is_cached():
    from ucd_amd.loss import seg_losses_route
    # the EX pairs (plain cross entropy beside a teacher of K classes) are planned on the teacher's split
    assert seg_losses_route(512, 512, 64, 64, 151, 101, True, 1) == "gather"
    assert seg_losses_route(513, 513, 33, 33, 21, 16, True, 1) == "tiled"
    before = seg_losses_route.cache_info().hits
    seg_losses_route(513, 513, 33, 33, 21, 16, True, 1)
    assert seg_losses_route.cache_info().hits == before + 1


def test_route_leaves_illegal_arguments_to_the_call():
    """"gather" means UCD_EUNSUPPORTED and nothing else: what the plan calls illegal stays on the tiled call, which reports it."""
    from ucd_amd.loss import seg_losses_route
    assert seg_losses_route(8, 8, 16, 16, 21, 16, True) == "tiled"                 # H < h
    assert seg_losses_route(513, 513, 33, 33, 21, 16, True, 5) == "tiled"          # ce_old_cl neither 1 nor K


def test_fused_seg_losses_checks_form_before_the_device():
    from ucd_amd.loss import fused_seg_losses
    with pytest.raises(RuntimeError, match="GPU only"):
        fused_seg_losses(torch.zeros(1, 5, 2, 2), None, torch.zeros(1, 8, 8, dtype=torch.long), 1, form="gather")


def _call(lib, **over):
    """ucd_seg_losses_gather on host buffers that no accepted call would take: every case here is refused before a device call."""
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    a = dict(sem_s=p, ld_s=151, sem_t=p, ld_t=101, labels=p, B=2, H=129, W=129, h=17, w=17, Ctot=151, K=101, ce_old_cl=101, kd_mode=0,
             alpha=1.0, ignore=255, ce_w=1.0, kd_w=10.0, loss_out=p, d_sem=p, ld_d=151, workspace=p,
             workspace_bytes=lib.ucd_seg_losses_gather_workspace_bytes(2, 17, 17))
    a.update(over)
    rc = lib.ucd_seg_losses_gather(a["sem_s"], a["ld_s"], a["sem_t"], a["ld_t"], a["labels"], a["B"], a["H"], a["W"], a["h"], a["w"],
                                   a["Ctot"], a["K"], a["ce_old_cl"], a["kd_mode"], a["alpha"], a["ignore"], a["ce_w"], a["kd_w"],
                                   a["loss_out"], a["d_sem"], a["ld_d"], a["workspace"], a["workspace_bytes"], None)
    return rc, lib.ucd_last_error().decode()


# what, overrides, code, the argument the message must name
REJECTIONS = [
    ("sem_s NULL", dict(sem_s=None), EINVAL, "sem_s"), ("labels NULL", dict(labels=None), EINVAL, "labels"),
    ("loss_out NULL", dict(loss_out=None), EINVAL, "loss_out"), ("workspace NULL", dict(workspace=None), EINVAL, "workspace"),
    ("B 0", dict(B=0), EINVAL, "B"), ("H -1", dict(H=-1), EINVAL, "H"), ("w 0", dict(w=0), EINVAL, "w"),
    ("Ctot 0", dict(Ctot=0), EINVAL, "Ctot"), ("K 0", dict(K=0), EINVAL, "K"), ("K > Ctot", dict(K=152), EINVAL, "K"),
    ("ld_s < Ctot", dict(ld_s=150), EINVAL, "ld_s"), ("ld_t < K", dict(ld_t=100), EINVAL, "ld_t"),
    ("ld_d < Ctot", dict(ld_d=150), EINVAL, "ld_d"),
    ("H < h", dict(H=16), EINVAL, "H x W"), ("W < w", dict(W=16), EINVAL, "H x W"),
    ("kd_mode 2", dict(kd_mode=2), EINVAL, "kd_mode"), ("kd_mode -1", dict(kd_mode=-1), EINVAL, "kd_mode"),
    ("alpha 0", dict(alpha=0.0), EINVAL, "alpha"), ("alpha nan", dict(alpha=float("nan")), EINVAL, "alpha"),
    ("alpha inf", dict(alpha=float("inf")), EINVAL, "alpha"),
    ("ce_old_cl 0", dict(ce_old_cl=0), EINVAL, "ce_old_cl"), ("ce_old_cl > Ctot", dict(ce_old_cl=152), EINVAL, "ce_old_cl"),
    ("ce_old_cl neither 1 nor K", dict(ce_old_cl=50), EINVAL, "ce_old_cl"),
    ("short workspace", dict(workspace_bytes=2 * 17 * 17 * 2 * 4 - 1), EWORKSPACE, "workspace"),
    ("2000 classes", dict(Ctot=2000, ld_s=2000, ld_d=2000, sem_t=None, ce_old_cl=1), EUNSUPPORTED, "72000 bytes"),
    ("1000 + 900 classes", dict(Ctot=1000, ld_s=1000, ld_d=1000, K=900, ld_t=900, ce_old_cl=900), EUNSUPPORTED, "68400 bytes"),
]


@pytest.mark.parametrize("what,over,code,names", REJECTIONS, ids=[r[0] for r in REJECTIONS])
def test_host_side_rejections(what, over, code, names):
    from ucd_amd import hip
    rc, msg = _call(hip.load(), **over)
    assert rc == code, (what, rc, msg)
    assert msg.startswith("ucd_seg_losses_gather: ") and names in msg, msg


def test_absent_operands_are_not_checked():
    """d_sem = NULL is legal (losses only); ld_t only counts with a teacher, ld_d only with d_sem, and without a teacher any
    ce_old_cl in [1, Ctot] is a split: the call gets past all of them to the next check (the short workspace)."""
    from ucd_amd import hip
    rc, msg = _call(hip.load(), sem_t=None, ld_t=0, d_sem=None, ld_d=0, ce_old_cl=50, workspace_bytes=1)
    assert rc == EWORKSPACE, (rc, msg)
