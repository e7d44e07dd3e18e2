"""GPU: focal cross entropy inside the fused logit-loss kernels (ucd_seg_losses_focal / ucd_seg_losses_gather_focal, through
fused_seg_losses(focal=...)) on every tiled form and the gather form against the float64 definition of tests/focal_ref.py, against
the reference's own numbers (tests/golden/focal_losses.npz), the identity focal=(0, 1), saturated / ignored / out-of-range pixels,
and the Trainer's step with --focal_loss.

Bars: the project's own for these kernels (tests/test_seglosses_gpu.py:47-53, tests/test_kd_losses_gpu.py): losses rel 1e-4,
gradient max error / max 1e-3, gradient L2-relative 1e-4."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import focal_ref as R
import test_pod_gpu as PG
import test_seglosses_gpu as T
from conftest import assert_matches_compact, load_golden
from oracle import losses as OL
from ucd_amd import argparser, hip, synth, tasks
from ucd_amd.loss import fused_seg_losses

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

FOCAL = ((2.0, 1.0), (0.5, 0.25), (3.5, 1.0))          # gamma, alpha
WEIGHTS = (None, (0.25, 1.0), (0.0, 0.5))
TILED_SPLITS = ("pk16", "pk20", "pk12", "reg24", "wide")
UNALIGNED_GEO = (2, 190, 129, 12, 9)


def _plan_ex(case, old_cl, teacher, aligned=True):
    """The form ucd_seg_losses_plan_ex names for the call (host only)."""
    import ctypes as C
    Ctot, K, _ = T.SPLITS[case.split]
    B, H, W, h, w = case.geo
    f = C.c_int()
    lib = hip.load()
    rc = lib.ucd_seg_losses_plan_ex(H, W, h, w, Ctot, K, old_cl, hip.KD_UNBIASED, int(teacher), int(aligned), -1, C.byref(f), None, None, None)
    assert rc == 0, lib.ucd_last_error().decode()
    return f.value


def _reference(inputs, K, old_cl, teacher, focal, weight, ce_w, kd_w, ignore=255):
    """(focal loss, kd, gradient of ce_w * focal + kd_w * kd w.r.t. the low-resolution logits) in float64 on the CPU."""
    sem, sem_t, labels = inputs
    s = sem.double().requires_grad_(True)
    loss, _ = R.focal_loss(s, labels, focal[0], focal[1], old_cl=old_cl, weight=weight, ignore_index=ignore)
    kd = torch.zeros((), dtype=torch.float64)
    if teacher:
        up = lambda t: F.interpolate(t, size=labels.shape[-2:], mode="bilinear", align_corners=False)
        kd = OL.unbiased_kd(up(s), up(sem_t.double()))
    (ce_w * loss + kd_w * kd).backward()
    return loss.item(), kd.item(), s.grad.numpy()


def _run(inputs, K, old_cl, teacher, focal, weight, ce_w, kd_w, form="auto", ignore=255):
    sem, sem_t, labels = inputs
    s = sem.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    sw = None if weight is None else torch.tensor(weight, device=DEV)
    total, ce, kd = fused_seg_losses(s, sem_t.to(DEV) if teacher else None, labels.to(DEV), old_cl, ce_w, kd_w if teacher else 0.0,
                                     ignore_index=ignore, form=form, sample_weight=sw, focal=focal)
    total.backward()
    return ce.item(), kd.item(), s.grad.double().cpu().numpy()


def _check(tag, got, ref, teacher):
    (ce, kd, g), (ce_r, kd_r, g_r) = got, ref
    e_max = np.abs(g - g_r).max() / np.abs(g_r).max()
    e_l2 = np.linalg.norm(g - g_r) / np.linalg.norm(g_r)
    print(f"{tag}: focal {ce:.6f} ref {ce_r:.6f} | kd {kd:.6f} ref {kd_r:.6f} | grad max-rel {e_max:.2e} L2-rel {e_l2:.2e}")
    assert np.isfinite(g).all()
    assert ce == pytest.approx(ce_r, rel=1e-4), tag
    if teacher:
        assert kd == pytest.approx(kd_r, rel=1e-4), tag
    assert e_max < 1e-3 and e_l2 < 1e-4, (tag, e_max, e_l2)


def _all_calls():
    for split in TILED_SPLITS:
        case = T.Case("focal", split, T.SMALL)
        K = T.SPLITS[split][1]
        for teacher in (True, False):
            for old_cl in (1, K):
                yield case, teacher, old_cl


def test_the_cases_reach_every_tiled_form():
    """pk<16,8>, pk<20,4>, pk<12,12>, reg<24,16>, reg<24,24> and the many-class form through fused_seg_losses at the small geometry
    (without a teacher the cross entropy's split picks the form: plain CE on 21 classes is reg<24,16>), the two fp32-atomic forms
    again and wide/f32 through the C ABI with a d_sem off the 16-byte grid."""
    forms = {_plan_ex(case, old_cl, teacher) for case, teacher, old_cl in _all_calls()}
    assert forms == {T.PK16, T.PK20, T.PK12, T.REG16, T.REG24, T.WIDE_FX}, forms
    un = {_plan_ex(T.Case("focal_unaligned", s, UNALIGNED_GEO), T.SPLITS[s][1], True, aligned=False) for s in ("pk16", "wide")}
    assert un == {T.REG16, T.WIDE_F32}, un


@pytest.mark.parametrize("split", TILED_SPLITS)
def test_tiled_forms_against_float64(split):
    """Every call the issue names on the split's forms: with and without a teacher, ce_old_cl in {1, K}, three (gamma, alpha), no
    weight, [0.25, 1] and [0, 0.5]."""
    case = T.Case("focal", split, T.SMALL)
    Ctot, K, _ = T.SPLITS[split]
    inputs = T._inputs(case)
    seen = set()
    for teacher in (True, False):
        for old_cl in (1, K):
            form = _plan_ex(case, old_cl, teacher)
            seen.add(form)
            for focal in FOCAL:
                for weight in WEIGHTS:
                    tag = f"{T.FORM_NAMES[form]} teacher={teacher} old_cl={old_cl} focal={focal} weight={weight}"
                    got = _run(inputs, K, old_cl, teacher, focal, weight, case.ce_w, case.kd_w)
                    _check(tag, got, _reference(inputs, K, old_cl, teacher, focal, weight, case.ce_w, case.kd_w if teacher else 0.0), teacher)
    assert T.SPLITS[split][2] in seen


def _launch_abi(case, inputs, focal, weight, entry="ucd_seg_losses_focal"):
    """The C entry on a d_sem one float off the 16-byte grid; NaN around the block."""
    lib = hip.load()
    Ctot, K, _ = T.SPLITS[case.split]
    B, H, W, h, w = case.geo
    sem, sem_t, labels = inputs
    rows = B * h * w
    s_buf = sem.permute(0, 2, 3, 1).reshape(rows, Ctot).contiguous().to(DEV)
    t_buf = sem_t.permute(0, 2, 3, 1).reshape(rows, K).contiguous().to(DEV)
    store = torch.full((rows * Ctot + 8,), float("nan"), device=DEV)
    d = store[1:1 + rows * Ctot].view(rows, Ctot)
    assert d.data_ptr() % 16 == 4
    out = torch.full((2,), float("nan"), device=DEV)
    nbytes = lib.ucd_seg_losses_workspace_bytes(B, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    lab = labels.to(DEV)
    sw = None if weight is None else torch.tensor(weight, device=DEV)
    hip._check(getattr(lib, entry)(hip.ptr(s_buf), Ctot, hip.ptr(t_buf), K, hip.ptr(lab), B, H, W, h, w, Ctot, K, K, hip.KD_UNBIASED, 1.0,
                                   case.ignore, case.ce_w, case.kd_w, hip.ptr(sw), focal[0], focal[1], hip.ptr(out), hip.ptr(d), Ctot,
                                   hip.ptr(ws), nbytes, hip.stream()), entry)
    torch.cuda.synchronize()
    assert bool(torch.isnan(store[:1]).all()) and bool(torch.isnan(store[1 + rows * Ctot:]).all())
    g = d.reshape(B, h, w, Ctot).permute(0, 3, 1, 2)
    return out[0].item(), out[1].item(), g.double().cpu().numpy()


@pytest.mark.parametrize("split", ["pk16", "wide"])
def test_unaligned_d_sem_pair(split):
    """reg<24,16> and wide/f32 as an unaligned d_sem reaches them, through the C entry."""
    case = T.Case("focal_unaligned", split, UNALIGNED_GEO, unaligned=True)
    Ctot, K, _ = T.SPLITS[split]
    assert _plan_ex(case, K, True, aligned=False) == (T.REG16 if split == "pk16" else T.WIDE_F32)
    inputs = T._inputs(case)
    for focal, weight in ((FOCAL[0], None), (FOCAL[1], (0.25, 1.0)), (FOCAL[2], (0.0, 0.5))):
        got = _launch_abi(case, inputs, focal, weight)
        _check(f"unaligned {split} focal={focal} weight={weight}", got,
               _reference(inputs, K, K, True, focal, weight, case.ce_w, case.kd_w), True)


@pytest.mark.parametrize("geo", [(2, 129, 129, 17, 17), (2, 129, 129, 9, 9)], ids=["s8_129", "small"])
def test_gather_form(geo):
    """ucd_seg_losses_gather_focal through fused_seg_losses(form="gather"): the same bars; a weight of ones gives the bits of the
    call without one; the same inputs give the same bits twice."""
    case = T.Case("focal_gather", "pk16", geo)
    Ctot, K, _ = T.SPLITS[case.split]
    inputs = T._inputs(case)
    for teacher, old_cl in ((True, K), (True, 1), (False, 1), (False, K)):
        for focal in FOCAL:
            for weight in WEIGHTS:
                got = _run(inputs, K, old_cl, teacher, focal, weight, case.ce_w, case.kd_w, form="gather")
                _check(f"gather teacher={teacher} old_cl={old_cl} focal={focal} weight={weight}", got,
                       _reference(inputs, K, old_cl, teacher, focal, weight, case.ce_w, case.kd_w if teacher else 0.0), teacher)
    for focal in FOCAL:
        plain = _run(inputs, K, K, True, focal, None, case.ce_w, case.kd_w, form="gather")
        ones = _run(inputs, K, K, True, focal, (1.0, 1.0), case.ce_w, case.kd_w, form="gather")
        again = _run(inputs, K, K, True, focal, None, case.ce_w, case.kd_w, form="gather")
        assert plain[:2] == ones[:2] and np.array_equal(plain[2], ones[2])
        assert plain[:2] == again[:2] and np.array_equal(plain[2], again[2])


def test_against_reference_golden():
    """fused_seg_losses(old_cl=1, focal=...) on the inputs of tests/golden/make_focal_golden.py against the numbers its run of the
    reference's FocalLoss stored, at the bars tests/test_kd_losses_gpu.py::test_against_reference_golden holds kd_losses.npz to."""
    import make_focal_golden as MF
    import make_kd_golden as MK
    gold = load_golden("focal_losses.npz")
    for shape in MK.UNIT_SHAPES:
        B, Ctot, K, h, H = shape
        sem, _, labels = MK.unit_inputs(shape)
        for gamma, alpha in MF.FOCAL:
            key = MF.focal_key(shape, gamma, alpha)
            s = sem.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            total, ce, _ = fused_seg_losses(s, None, labels.to(DEV), 1, 1.0, 0.0, focal=(gamma, alpha))
            total.backward()
            ref = float(gold[key + "|loss"][0])
            print(f"{key}: focal {ce.item():.7f} reference {ref:.7f}")
            assert ce.item() == pytest.approx(ref, rel=1e-4), key
            assert total.item() == pytest.approx(ref, rel=1e-4), key
            g = s.grad.cpu().numpy()
            if key + "|grad" in gold:
                g_r = gold[key + "|grad"].astype(np.float64)
                assert np.abs(g - g_r).max() / np.abs(g_r).max() < 1e-3, key
                assert np.linalg.norm(g - g_r) / np.linalg.norm(g_r) < 1e-4, key
            else:
                gmax = float(np.abs(gold[key + "|grad::samples"]).max())
                assert_matches_compact(gold, key + "|grad", g, rtol=1e-4, atol=1e-3 * gmax)


@pytest.mark.parametrize("split", TILED_SPLITS + ("gather",))
def test_gamma_0_alpha_1_is_the_call_without_focal(split):
    """focal=(0, 1) is routed on the host to the unmodulated launch: the bits of focal=None in the losses on every form, in the
    gradient on the fixed-point forms and the gather form (the fp32-atomic forms have no fixed order of their adds)."""
    form_arg = "gather" if split == "gather" else "auto"
    case = T.Case("focal_identity", "pk16" if split == "gather" else split, T.SMALL)
    Ctot, K, _ = T.SPLITS[case.split]
    inputs = T._inputs(case)
    for teacher, old_cl in ((True, K), (False, 1)):
        form = _plan_ex(case, old_cl, teacher)
        for weight in (None, (0.25, 1.0)):
            a = _run(inputs, K, old_cl, teacher, None, weight, case.ce_w, case.kd_w, form=form_arg)
            b = _run(inputs, K, old_cl, teacher, (0.0, 1.0), weight, case.ce_w, case.kd_w, form=form_arg)
            assert a[:2] == b[:2], (split, teacher, weight)
            if split == "gather" or form in (T.PK16, T.PK20, T.PK12, T.WIDE_FX):
                assert np.array_equal(a[2], b[2]), (split, teacher, weight)
            else:
                assert np.abs(a[2] - b[2]).max() <= 1e-5 * np.abs(a[2]).max()


def _saturated(split):
    """CE-only inputs: in the left half of the map the label is the first new class and its logit stands 40 above the rest in every
    cell (fp32: ce rounds to 0 away from the seam), 8 x 8 blocks of it ignored; the right half is the mixed case."""
    case = T.Case("focal_saturated", split, T.SMALL, teacher=False, kd_w=0.0)
    Ctot, K, _ = T.SPLITS[split]
    B, H, W, h, w = case.geo
    sem, _, labels = T._inputs(case)
    sem, labels = sem.clone(), labels.clone()
    half = w // 2
    sem[:, :, :, :half] = 0.0
    sem[:, K, :, :half] = 40.0
    xs = int(half * W / w)
    ign = labels[:, :, :xs] == case.ignore
    labels[:, :, :xs] = torch.where(ign, labels[:, :, :xs], torch.full_like(labels[:, :, :xs], K))
    return case, (sem, None, labels), half


@pytest.mark.parametrize("split", ["pk16", "reg24", "wide", "gather"])
def test_saturated_ignored_and_out_of_range_pixels(split):
    form_arg = "gather" if split == "gather" else "auto"
    case, inputs, half = _saturated("pk16" if split == "gather" else split)
    Ctot, K, _ = T.SPLITS[case.split]
    assert bool((inputs[2][:, :, :8] == case.ignore).any()) and bool((inputs[2][:, :, :8] == K).any())
    plain = _run(inputs, K, K, False, None, None, 1.0, 0.0, form=form_arg)
    for gamma in (0.5, 2.0):
        ce, _, g = _run(inputs, K, K, False, (gamma, 1.0), None, 1.0, 0.0, form=form_arg)
        ce_r, _, g_r = _reference(inputs, K, K, False, (gamma, 1.0), None, 1.0, 0.0)
        assert np.isfinite(ce) and np.isfinite(g).all()
        assert ce == pytest.approx(ce_r, rel=1e-4)
        # cells whose whole bilinear support lies in the saturated half: every pixel under them has u = 0, their gradient is 0
        assert not g[:, :, :, :half - 2].any(), np.abs(g[:, :, :, :half - 2]).max()
        assert np.abs(g - g_r).max() / np.abs(g_r).max() < 1e-3
    # the gamma == 0 rule: alpha times the unmodulated call, saturated pixels included
    ce0, _, g0 = _run(inputs, K, K, False, (0.0, 0.5), None, 1.0, 0.0, form=form_arg)
    assert ce0 == pytest.approx(0.5 * plain[0], rel=1e-6)
    if split in ("gather", "pk16", "wide"):
        assert np.array_equal(g0, 0.5 * plain[2])                # a power of two through every product, and through the fixed point
    else:
        assert np.abs(g0 - 0.5 * plain[2]).max() <= 1e-5 * np.abs(plain[2]).max()
    # an all-ignored batch: exactly 0
    sem, _, labels = inputs
    for gamma in (0.5, 2.0):
        ce, _, g = _run((sem, None, torch.full_like(labels, case.ignore)), K, K, False, (gamma, 1.0), None, 1.0, 0.0, form=form_arg)
        assert ce == 0.0 and not g.any()
    # labels that are no class (beyond every form's padding): the clamp on u keeps a negative LSE(z) out of the power
    lab = labels.clone()
    lab[:, ::3, ::5] = 254
    for focal in ((0.5, 1.0), (2.0, 1.0), (0.0, 0.5)):
        for s in (sem, sem - 60.0):                               # LSE(z) positive, and negative
            ce, _, g = _run((s, None, lab), K, K, False, focal, None, 1.0, 0.0, form=form_arg)
            assert np.isfinite(ce) and np.isfinite(g).all(), focal


# ---- the step ------------------------------------------------------------------------------------------------------------------------
NAMES = PG.NAMES
CROP = 129


def _batch(it):
    return synth.images(700 + it % 2, 2, CROP), synth.seg_labels(700 + it % 2, 2, CROP, CROP, range(16, 21))


def _steps(extra_args=(), step_graph="0", steps=1, flips=None):
    """tests/test_pseudo_gpu.py::_steps at 2 x 129^2 (bf16, VOC 15-5 step 1, synthetic calibrated checkpoint; the threshold pass of
    a pseudo-labelling run in front of the first iteration).  Returns the losses per step (ce, con, lkd, loss, LPOD), the
    accumulated update of a few parameters, the replayed iterations, the capture error and the trainer."""
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
        if trainer.pseudo_flag:
            trainer.find_pseudo_thresholds([_batch(0), _batch(1)])
        model.train()
        params = dict(net.named_parameters())
        before = {n: params[n].detach().float().cpu().clone() for n in NAMES}
        rec = []
        for it in range(steps):
            r = trainer.train_step(*_batch(it), optim, sched)
            rec.append([r[k].item() for k in ("ce", "con", "lkd", "loss")] + [r["LPOD"].item() if "LPOD" in r else 0.0])
        torch.cuda.synchronize()
        upd = {n: params[n].detach().float().cpu() - before[n] for n in NAMES}
        return np.asarray(rec), upd, trainer.graph_steps, trainer.step_graph_error, trainer
    finally:
        torch.backends.cudnn.deterministic = False
        for k in flips:
            switches.unset(k)


FLAG = ("--focal_loss",)


@pytest.mark.usefixtures("deterministic_stats")
def test_step_with_focal_against_the_torch_composition():
    """One UCD step with --focal_loss against the same step under UCD_FUSED_FOCAL=0 (up-sampled logits, the cross-entropy map,
    focal_modulate, the torch KD module): losses and first updates at the bars of
    tests/test_pseudo_gpu.py::test_step_with_pseudo_labels_against_the_torch_composition; the criterion differs from the plain one."""
    calls = hip.enable_call_timing()
    try:
        got, up, _, _, trainer = _steps(FLAG)
        fused_calls = len(calls.get("ucd_seg_losses", ()))
        calls.clear()
        ref, up_ref, _, _, t_ref = _steps(FLAG, flips={"UCD_FUSED_FOCAL": "0"})
        assert "ucd_seg_losses" not in calls
    finally:
        hip.disable_call_timing()
    plain = _steps(())[0]
    assert fused_calls == 1 and trainer.focal == (2.0, 1.0) and trainer.fuse_logit_losses and not t_ref.fuse_logit_losses
    print("fused:", got, "composition:", ref, "without the flag:", plain)
    assert np.isfinite(got).all() and got[0, 0] < plain[0, 0]                    # (1 - p)^2 <= 1 on every pixel
    np.testing.assert_allclose(got[:, 3], ref[:, 3], rtol=1e-2)
    np.testing.assert_allclose(got[:, 0], ref[:, 0], rtol=1e-2)
    np.testing.assert_allclose(got[:, 1:3], ref[:, 1:3], rtol=5e-2, atol=1e-3)
    for n in NAMES:
        a, b = up_ref[n].flatten().double(), up[n].flatten().double()
        cos = float(a @ b / (a.norm() * b.norm() + 1e-300))
        ratio = float(b.norm() / (a.norm() + 1e-300))
        print(f"first update, fused vs composition: {n}: cosine {cos:.4f} length ratio {ratio:.3f}")
        assert cos > (0.78 if n.startswith("body.") else 0.98) and 0.85 < ratio < 1.25, (n, cos, ratio)


@pytest.mark.usefixtures("deterministic_stats")
def test_whole_step_graph_replays_the_eager_step_with_focal():
    """The focal launch inside the captured iteration: three eager warm-up iterations and three replays give the bits of six eager
    iterations - every loss at every step, every compared parameter afterwards."""
    eager, pe, n_e, _, _ = _steps(FLAG, "0", steps=6)
    graph, pg, n_g, err, _ = _steps(FLAG, "1", steps=6)
    assert err is None, err
    assert n_e == 0 and n_g == 6 - 3, (n_e, n_g)
    print("eager", eager, "graph", graph, "max abs difference", np.abs(eager - graph).max())
    assert np.array_equal(eager, graph), (eager, graph)
    for n in pe:
        assert torch.equal(pe[n], pg[n]), n


@pytest.mark.usefixtures("deterministic_stats")
def test_without_the_flag_it_is_the_plain_step():
    """--focal_loss_gamma / --focal_loss_alpha without --focal_loss request nothing: the launches and the bits of a Trainer built
    without them."""
    calls = hip.enable_call_timing()
    try:
        plain, pp, _, _, t0 = PG._steps((), steps=2, crop=CROP)
        n_plain = {k: len(v) for k, v in calls.items()}
        calls.clear()
        off, po, _, _, t1 = _steps(("--focal_loss_gamma", "3.5", "--focal_loss_alpha", "0.25"), steps=2)
        n_off = {k: len(v) for k, v in calls.items()}
    finally:
        hip.disable_call_timing()
    assert t0.focal is None and t1.focal is None and n_plain == n_off, (n_plain, n_off)
    assert np.array_equal(plain[:, :4], off[:, :4]), (plain, off)
    for n in pp:
        assert torch.equal(pp[n], po[n]), n


def test_plop_with_pod_logits_and_focal_builds_and_steps():
    got, _, _, _, trainer = _steps(("--method", "PLOP", "--pod_logits") + FLAG)
    assert trainer.pod_flag and trainer.pod_logits and trainer.pseudo_flag and trainer.pseudo_adaptive and trainer.focal == (2.0, 1.0)
    assert np.isfinite(got).all() and got[0, 0] > 0 and got[0, 4] > 0


def test_validate_reports_the_focal_class_loss():
    """Trainer.validate with --focal_loss (fp32 activations): the class loss is the mean over the batches of the focal criterion on
    the up-sampled logits of the same eval-mode model - the fused path and the UCD_FUSED_FOCAL=0 composition both, at the kernels'
    loss bar - and it is not the unmodulated one."""
    import test_evaluate_gpu as EV
    from ucd_amd import switches
    from ucd_amd.loss import UnbiasedCrossEntropy, focal_modulate
    from ucd_amd.metrics import StreamSegMetrics
    from ucd_amd.train import Trainer
    model, model_old, classes, dev = EV._models()
    loader = EV._loader(4, 2)
    args = ["--method", "UCD", "--focal_loss", "--focal_loss_gamma", "0.5", "--focal_loss_alpha", "0.25"]
    trainer = Trainer(model, model_old, device=dev, opts=EV._opts(args), classes=classes)
    (fused, _), _, _ = trainer.validate(loader, StreamSegMetrics(EV.N_CLASSES))
    switches.set("UCD_FUSED_FOCAL", "0")
    try:
        t_comp = Trainer(model, model_old, device=dev, opts=EV._opts(args), classes=classes)
        assert trainer.fuse_logit_losses and not t_comp.fuse_logit_losses
        (comp, _), _, _ = t_comp.validate(loader, StreamSegMetrics(EV.N_CLASSES))
    finally:
        switches.unset("UCD_FUSED_FOCAL")
    (plain, _), _, _ = Trainer(model, model_old, device=dev, opts=EV._opts(["--method", "UCD"]), classes=classes).validate(
        loader, StreamSegMetrics(EV.N_CLASSES))
    model.eval()
    total, n = 0.0, 0
    crit = UnbiasedCrossEntropy(old_cl=16, ignore_index=255, reduction="none")
    with torch.no_grad():
        for images, labels in loader:
            _, f = model(images.to(dev, dtype=torch.float32), upsample=False)
            up = F.interpolate(f["sem"].double(), size=labels.shape[-2:], mode="bilinear", align_corners=False)
            total, n = total + focal_modulate(crit(up, labels.to(dev)), 0.5, 0.25).mean().item(), n + 1
    print(f"validate: fused {fused.item():.6f} composition {comp.item():.6f} by hand {total / n:.6f} without the flag {plain.item():.6f}")
    assert fused.item() == pytest.approx(total / n, rel=1e-4) and comp.item() == pytest.approx(total / n, rel=1e-4)
    assert abs(fused.item() - plain.item()) > 1e-2 * plain.item()
