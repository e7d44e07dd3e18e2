"""GPU: PLOP's pseudo-labelling (``--pseudo entropy``) - the kernels of csrc/pseudo_label.hip against the float64 reference
(tests/pseudo_ref.py) off its loose set, the per-image weight on the fused cross entropy on every tiled form and the gather form
(inputs, references and bars of tests/test_seglosses_gpu.py, by import), and the step: under the A/B switch, replayed from the
whole-step graph, with the PLOP preset, and from the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pseudo_ref as R
import test_seglosses_gpu as T
from oracle import losses as OL
from ucd_amd import argparser, hip, synth, tasks
from ucd_amd.loss import fused_seg_losses

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"

KS = (1, 2, 16, 21, 101)
# h, w, H, W: a non-integer factor 13; factors below 4, not square, odd; factor 1
GEOS = {"f13": (5, 5, 65, 65), "f3.7x3.9": (9, 12, 33, 47), "f1": (32, 32, 32, 32)}
BINS, F_MIN = 100, 0.0


def _call(rows, labels, K, geo, thresholds, f_min=F_MIN, B=2):
    """ucd_pseudo_label through the C ABI on rows with a padded pitch: (labels_out, counts, factor, uncertainty) on the host."""
    h, w, H, W = geo
    lib = hip.load()
    t, lab = rows.to(DEV), labels.to(DEV)
    thr = torch.as_tensor(thresholds, dtype=torch.float32).to(DEV)
    out = torch.full_like(lab, -7)
    counts = torch.full((B, 2), -7, dtype=torch.int32, device=DEV)
    factor = torch.full((B,), float("nan"), device=DEV)
    unc = torch.full((B, H, W), float("nan"), device=DEV)
    hip._check(lib.ucd_pseudo_label(hip.ptr(t), t.shape[1], hip.ptr(lab), B, H, W, h, w, K, R.IGNORE, hip.ptr(thr), f_min, hip.ptr(out),
                                    hip.ptr(counts), hip.ptr(factor), hip.ptr(unc), hip.stream()), "ucd_pseudo_label")
    torch.cuda.synchronize()
    return out.cpu(), counts.cpu(), factor.cpu(), unc.cpu()


def _hist(rows, labels, K, geo, hist, B=2):
    h, w, H, W = geo
    t, lab = rows.to(DEV), labels.to(DEV)
    hip._check(hip.load().ucd_pseudo_hist(hip.ptr(t), t.shape[1], hip.ptr(lab), B, H, W, h, w, K, R.IGNORE, hist.shape[1], hip.ptr(hist),
                                          hip.stream()), "ucd_pseudo_hist")
    torch.cuda.synchronize()
    return hist


@pytest.mark.parametrize("geo", sorted(GEOS))
@pytest.mark.parametrize("K", KS)
def test_labels_counts_factor_and_uncertainty(K, geo):
    """Off the loose set (a decision within 1e-5 of flipping; at most 1 % of the pixels, asserted on the reference first) the
    labels are the reference's exactly; u is within 1e-5 everywhere; the counts differ from the reference's by at most the image's
    loose pixels; the factor is max(num / (den + 1e-6), f_min) of the kernel's own counts to 1 ulp; a second run gives the same
    bits in every output."""
    c = R.case(K, *GEOS[geo])
    n = c.labels.numel()
    print(f"loose share {c.loose.sum().item() / n:.4%}")
    assert c.loose.sum().item() <= 0.01 * n
    out, counts, factor, unc = _call(c.rows, c.labels, K, GEOS[geo], c.thresholds)
    du = (unc.double() - c.unc).abs().max().item()
    wrong = ((out != c.labels_out) & ~c.loose).sum().item()
    print(f"max |u - u64| {du:.3e}, labels wrong off the loose set {wrong}, counts {counts.tolist()} reference "
          f"{list(zip(c.num.tolist(), c.den.tolist()))}")
    assert wrong == 0
    assert torch.equal(out[~c.cand], c.labels[~c.cand])
    assert du <= 1e-5
    loose_b = c.loose.flatten(1).sum(1)
    assert torch.equal(counts[:, 1].long(), c.den)
    assert bool(((counts[:, 0].long() - c.num).abs() <= loose_b).all())
    want = np.maximum(counts[:, 0].double().numpy() / (counts[:, 1].double().numpy() + 1e-6), F_MIN)
    want = np.where(counts[:, 1].numpy() == 0, max(0.0, F_MIN), want)
    assert np.all(np.abs(factor.double().numpy() - want) <= np.spacing(want.astype(np.float32)))
    again = _call(c.rows, c.labels, K, GEOS[geo], c.thresholds)
    assert all(torch.equal(a, b) for a, b in zip((out, counts, factor, unc), again))


@pytest.mark.parametrize("geo", sorted(GEOS))
@pytest.mark.parametrize("K", KS)
def test_histogram(K, geo):
    """Cell by cell: a bin of a class row differs from the reference's by at most the loose pixels that can sit in that cell
    (pseudo_ref.hist_allowance: a tie moves a pixel between the rows of its tied classes, in its bin; a pixel at a bin edge moves
    between the edge's two bins) - a cell no loose pixel can reach is exact; a row total differs by at most the tie pixels of that
    class; the grand total is exact; a second call doubles the histogram."""
    c = R.case(K, *GEOS[geo])
    hist = _hist(c.rows, c.labels, K, GEOS[geo], torch.zeros(K, BINS, dtype=torch.int64, device=DEV))
    got = hist.cpu()
    assert got.sum().item() == c.cand.sum().item()
    cells, rows = R.hist_allowance(c, BINS)
    diff = (got - c.hist).abs()
    print(f"bins that differ {int((diff > 0).sum())}, largest difference {int(diff.max())}; cells a loose pixel can reach "
          f"{int((cells > 0).sum())} of {int((c.hist > 0).sum())} occupied, largest allowance {int(cells.max())}")
    assert bool(((got.sum(1) - c.hist.sum(1)).abs() <= rows).all())
    assert bool((diff <= cells).all())
    twice = _hist(c.rows, c.labels, K, GEOS[geo], hist.clone()).cpu()
    assert torch.equal(twice, 2 * got)


def test_histogram_summed_per_wave_where_lds_has_no_room():
    """K x bins words that do not fit beside the cells (K = 21 at factor 1 on 32 x 32 tiles: 103 KB of cells, 8 KB of histogram
    at 100 bins, 86 KB at 1024 - the plan says so): the per-wave form gives the histogram of the LDS form, rebinned."""
    K, geo = 21, GEOS["f1"]
    assert not hip.pseudo_plan(geo[2], geo[3], geo[0], geo[1], K, 1024)["lds_hist"] and hip.pseudo_plan(geo[2], geo[3], geo[0], geo[1], K, BINS)["lds_hist"]
    c = R.case(K, *geo)
    fine = _hist(c.rows, c.labels, K, geo, torch.zeros(K, 1024, dtype=torch.int64, device=DEV)).cpu()
    coarse = _hist(c.rows, c.labels, K, geo, torch.zeros(K, 2, dtype=torch.int64, device=DEV)).cpu()
    assert fine.sum().item() == c.cand.sum().item()
    assert torch.equal(fine.view(K, 2, 512).sum(2), coarse)


def test_constant_cells_k1_and_an_image_without_candidates():
    """All classes equal: c* = 0 and u = 1 exactly, the last bin, every candidate becomes 255.  K = 1 passes every candidate as 0.
    An image without candidates gets factor = f_min."""
    geo, K = GEOS["f13"], 16
    h, w, H, W = geo
    c = R.case(K, *geo)
    rows = torch.full_like(c.rows, float("nan"))
    rows[:, :K] = 1.375
    labels = c.labels.clone()
    labels[1] = torch.where(c.cand[1], torch.full_like(labels[1], K + 1), labels[1])          # image 1: no candidates
    hist = _hist(rows, labels, K, geo, torch.zeros(K, BINS, dtype=torch.int64, device=DEV)).cpu()
    assert hist[0, BINS - 1].item() == c.cand[0].sum().item() == hist.sum().item()
    out, counts, factor, unc = _call(rows, labels, K, geo, R.median(hist.numpy(), 0.001), f_min=0.25)
    assert bool((unc[0][c.cand[0]] == 1.0).all()) and bool((out[0][c.cand[0]] == R.IGNORE).all())
    assert torch.equal(out[1], labels[1]) and counts.tolist() == [[0, int(c.cand[0].sum())], [0, 0]]
    assert factor.tolist() == [0.25, 0.25]
    one = R.case(1, *geo)
    out, counts, factor, unc = _call(one.rows, one.labels, 1, geo, [0.001])
    assert bool((out[one.cand] == 0).all()) and torch.equal(counts[:, 0], counts[:, 1]) and not unc.any()
    assert bool((factor > 0.999).all())


# ---- the per-image weight on the fused cross entropy ---------------------------------------------------------------------------------
GEO_W = (2, 190, 129, 12, 9)
W_CASES = [T.Case("w", s, T.SMALL) for s in ("pk16", "pk20", "pk12", "reg24", "wide")] + [
    T.Case("w_unaligned", "pk16", GEO_W, unaligned=True, pad=(0, 0, 3)), T.Case("w_unaligned", "wide", GEO_W, unaligned=True, pad=(0, 0, 3))]
WEIGHTS = ([0.25, 1.0], [0.0, 0.5])


def _launch_w(case, inputs, sw, ce_w=None, entry="ucd_seg_losses_ex_w"):
    """(ce, kd, gradient [B, Ctot, h, w] float64 numpy) of a tiled entry through the C ABI; sw None: ucd_seg_losses_ex."""
    lib = hip.load()
    Ctot, K, _ = T.SPLITS[case.split]
    B, H, W, h, w = case.geo
    sem, sem_t, labels = inputs
    rows = B * h * w
    ld_d = Ctot + case.pad[2]
    s_buf = sem.permute(0, 2, 3, 1).reshape(rows, Ctot).contiguous().to(DEV)
    t_buf = None if sem_t is None else sem_t.permute(0, 2, 3, 1).reshape(rows, K).contiguous().to(DEV)
    off = 1 if case.unaligned else 0
    store = torch.full((rows * ld_d + 8,), float("nan"), device=DEV)
    d = store[off:off + rows * ld_d].view(rows, ld_d)
    out = torch.full((2,), float("nan"), device=DEV)
    nbytes = lib.ucd_seg_losses_workspace_bytes(B, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    lab = labels.to(DEV)
    weight = () if sw is None else (hip.ptr(sw),)
    name = "ucd_seg_losses_ex" if sw is None else entry
    hip._check(getattr(lib, name)(hip.ptr(s_buf), Ctot, hip.ptr(t_buf), K, hip.ptr(lab), B, H, W, h, w, Ctot, K, K, hip.KD_UNBIASED, 1.0,
                                  case.ignore, case.ce_w if ce_w is None else ce_w, case.kd_w, *weight, hip.ptr(out), hip.ptr(d), ld_d,
                                  hip.ptr(ws), nbytes, hip.stream()), name)
    torch.cuda.synchronize()
    g = d[:, :Ctot].reshape(B, h, w, Ctot).permute(0, 3, 1, 2)
    return out[0].item(), out[1].item(), g.double().cpu().numpy()


_WREF = {}


def _weighted_references(case, inputs, sw):
    """test_seglosses_gpu._references with the cross entropy of image b weighed sw[b]: float64 on the CPU, fp32 composition on
    the GPU.  Computed once per (case, weights)."""
    key = (case.id, case.geo, tuple(sw))
    if key in _WREF:
        return _WREF[key]
    from ucd_amd.loss import UnbiasedCrossEntropy, UnbiasedKnowledgeDistillationLoss
    Ctot, K, _ = T.SPLITS[case.split]
    B, H, W, h, w = case.geo
    sem, sem_t, labels = inputs
    up = lambda t: F.interpolate(t, size=(H, W), mode="bilinear", align_corners=False)
    f64 = torch.tensor(sw, dtype=torch.float64).view(B, 1, 1)
    s64 = sem.double().requires_grad_(True)
    u = up(s64)
    ce64 = (f64 * OL.unbiased_cross_entropy(u, labels, K, ignore_index=case.ignore)).mean()
    kd64 = OL.unbiased_kd(u, up(sem_t.double()))
    (case.ce_w * ce64 + case.kd_w * kd64).backward()
    s32 = sem.to(DEV).requires_grad_(True)
    u = up(s32)
    ce32 = (f64.float().to(DEV) * UnbiasedCrossEntropy(old_cl=K, ignore_index=case.ignore, reduction="none")(u, labels.to(DEV))).mean()
    kd32 = UnbiasedKnowledgeDistillationLoss(alpha=1.0)(u, up(sem_t.to(DEV)))
    (case.ce_w * ce32 + case.kd_w * kd32).backward()
    _WREF[key] = ((ce64.item(), kd64.item(), s64.grad.numpy()), (ce32.item(), kd32.item(), s32.grad.double().cpu().numpy()))
    return _WREF[key]


def test_the_weighted_cases_reach_every_tiled_form():
    assert {T._expected_form(c) for c in W_CASES} == set(T.FORM_NAMES)


@pytest.mark.parametrize("case", W_CASES, ids=[c.id for c in W_CASES])
def test_weighted_tiled_forms(case):
    """On the form the case is named for: a weight of ones gives the bits of the unweighted call (losses on every form, the
    gradient on the fixed-point forms; on the fp32-atomic forms, which have no fixed order, the gradient within the reordering
    bound of its sums); [0.25, 1] and [0, 0.5] meet the float64 composition at
    the bars of test_seglosses_gpu._check, unchanged; under a weight of 0 the image's rows of d_sem are its KD-only gradient
    (the call with ce_weight 0) up to the two calls' fixed-point quanta and fp32 rounding of the same sums."""
    inputs = T._inputs(case)
    form = T._expected_form(case)
    assert T._plan(case, hip.load()) == form
    plain = _launch_w(case, inputs, None)
    ones = _launch_w(case, inputs, torch.ones(2, device=DEV))
    assert plain[:2] == ones[:2]
    if form not in (T.REG16, T.REG24, T.WIDE_F32):
        assert np.array_equal(plain[2], ones[2])
    else:
        # fp32 atomics: two launches of ONE kernel already differ in their last bits (the order of the adds).  An element is the sum
        # of at most n = (2 f_y + 2)(2 f_x + 2) weighted pixel gradients, each at most gmax, the bilinear weights of one cell summing
        # to at most (f_y + 1)(f_x + 1): two orders of that sum differ by at most 2 (n - 1) eps32 (f_y + 1)(f_x + 1) gmax
        B, H, W, h, w = case.geo
        fy, fx = H / h, W / w
        gmax = (abs(case.ce_w) + 2.0 * abs(case.kd_w) / T.SPLITS[case.split][1]) / (B * H * W)
        bound = 2 * ((2 * fy + 2) * (2 * fx + 2) - 1) * np.finfo(np.float32).eps * (fy + 1) * (fx + 1) * gmax
        err = np.abs(plain[2] - ones[2]).max()
        print(f"ones against unweighted, fp32 atomics: {err:.3e}, bound {bound:.3e}, largest gradient {np.abs(plain[2]).max():.3e}")
        assert err <= bound
    for sw in WEIGHTS:
        got = _launch_w(case, inputs, torch.tensor(sw, device=DEV))
        T._check(case, form, got, *_weighted_references(case, inputs, sw))
    kd_only = _launch_w(case, inputs, None, ce_w=0.0)
    A = T._fixed_point_allowance(case, form) + T._fixed_point_allowance(T.dataclasses.replace(case, ce_w=0.0), form)
    err = np.abs(got[2][0] - kd_only[2][0]).max()
    print(f"weight 0: image 0 against its KD-only gradient {err:.3e}, allowance {A:.3e}")
    assert err <= A + 8 * np.finfo(np.float32).eps * np.abs(kd_only[2][0]).max()


@pytest.mark.parametrize("geo", [(2, 129, 129, 17, 17), (2, 129, 129, 9, 9)], ids=["s8_129", "small"])
def test_weighted_gather_form(geo):
    """ucd_seg_losses_gather_w through fused_seg_losses(form="gather"): ones give the bits of the call without a weight, the
    weighted pairs meet the float64 composition at _check's bars (A = 0: no fixed point), and a weight of 0 leaves exactly the
    KD-only gradient in the image's rows (one store per element, a fixed order: 0 * CE adds exact zeros)."""
    case = T.Case("wg", "pk16", geo)
    inputs = T._inputs(case)
    K = T.SPLITS[case.split][1]
    sem, sem_t, labels = (x.to(DEV) for x in inputs)

    def run(sw, ce_w=case.ce_w):
        s = sem.clone().requires_grad_(True)
        total, ce, kd = fused_seg_losses(s, sem_t, labels, K, ce_w, case.kd_w, form="gather",
                                         sample_weight=None if sw is None else torch.tensor(sw, device=DEV))
        total.backward()
        return ce.item(), kd.item(), s.grad.double().cpu().numpy()

    plain, ones = run(None), run([1.0, 1.0])
    assert plain[:2] == ones[:2] and np.array_equal(plain[2], ones[2])
    for sw in WEIGHTS:
        got = run(sw)
        T._check(case, T.WIDE_F32, got, *_weighted_references(case, inputs, sw))
    assert np.array_equal(got[2][0], run(None, ce_w=0.0)[2][0])


# ---- the step ------------------------------------------------------------------------------------------------------------------------
import test_pod_gpu as PG

NAMES = PG.NAMES
PSEUDO = ("--pseudo", "entropy", "--pseudo_adaptive")


def _batch(it, batch=2, crop=65):
    return synth.images(700 + it % 2, batch, crop), synth.seg_labels(700 + it % 2, batch, crop, crop, range(16, 21))


def _steps(extra_args=(), step_graph="0", steps=1, flips=None, method="UCD"):
    """tests/test_pod_gpu.py::_steps (2 x 65^2, bf16, 15-5 step 1, synthetic calibrated checkpoint) with the threshold pass of a
    pseudo-labelling run in front of the first iteration: find_pseudo_thresholds over the two synthetic batches the steps cycle
    through.  Returns the losses per step (ce, con, lkd, loss, LPOD, PSEUDO), the accumulated update of a few parameters, the
    replayed iterations, the capture error and the trainer."""
    from ucd_amd import switches
    from ucd_amd.ddp import DistributedDataParallel
    from ucd_amd.run import build_models, load_step_checkpoint, make_optimizer
    from ucd_amd.scheduler import PolyLR
    from ucd_amd.train import Trainer
    dev = torch.device(DEV)
    opts = argparser.modify_command_options(argparser.get_argparser().parse_args(
        ["--method", method, "--dataset", "voc", "--task", "15-5", "--step", "1", "--lr", "0.001", "--no_pretrained",
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
            rec.append([r[k].item() for k in ("ce", "con", "lkd", "loss")] + [r[k].item() if k in r else 0.0 for k in ("LPOD", "pseudo_kept")])
        torch.cuda.synchronize()
        upd = {n: params[n].detach().float().cpu() - before[n] for n in NAMES}
        return np.asarray(rec), upd, trainer.graph_steps, trainer.step_graph_error, trainer
    finally:
        torch.backends.cudnn.deterministic = False
        for k in flips:
            switches.unset(k)


@pytest.mark.usefixtures("deterministic_stats")
def test_step_with_pseudo_labels_against_the_torch_composition():
    """One UCD step with --pseudo entropy --pseudo_adaptive against the same step under UCD_FUSED_PSEUDO=0 (thresholds, labels and
    factor from the torch composition): losses and first updates at the bars of
    tests/test_pod_gpu.py::test_step_with_pod_against_the_torch_composition; the share of kept candidates lies strictly inside
    (0, 1)."""
    calls = hip.enable_call_timing()
    try:
        got, up, _, _, trainer = _steps(PSEUDO)
        fused_calls = (len(calls.get("ucd_pseudo_hist", ())), len(calls.get("ucd_pseudo_label", ())))
        calls.clear()
        ref, up_ref, _, _, t_ref = _steps(PSEUDO, flips={"UCD_FUSED_PSEUDO": "0"})
        assert "ucd_pseudo_hist" not in calls and "ucd_pseudo_label" not in calls
    finally:
        hip.disable_call_timing()
    assert fused_calls == (2, 1), fused_calls
    assert trainer.pseudo_flag and np.isfinite(got).all() and 0.0 < got[0, 5] < 1.0
    print("fused:", got, "composition:", ref, "thresholds", trainer.pseudo_thresholds.tolist(), t_ref.pseudo_thresholds.tolist())
    np.testing.assert_allclose(got[:, 3], ref[:, 3], rtol=1e-2)
    np.testing.assert_allclose(got[:, 0], ref[:, 0], rtol=1e-2)
    np.testing.assert_allclose(got[:, 1:3], ref[:, 1:3], rtol=5e-2, atol=1e-3)
    np.testing.assert_allclose(got[:, 5], ref[:, 5], rtol=1e-2)
    for n in NAMES:
        a, b = up_ref[n].flatten().double(), up[n].flatten().double()
        cos = float(a @ b / (a.norm() * b.norm() + 1e-300))
        ratio = float(b.norm() / (a.norm() + 1e-300))
        print(f"first update, fused vs composition: {n}: cosine {cos:.4f} length ratio {ratio:.3f}")
        assert cos > (0.78 if n.startswith("body.") else 0.98) and 0.85 < ratio < 1.25, (n, cos, ratio)


@pytest.mark.usefixtures("deterministic_stats")
def test_whole_step_graph_replays_the_eager_step_with_pseudo_labels():
    """The label launch, the factor launch and the weighted loss inside the captured iteration: three eager warm-up iterations
    and three replays give the bits of six eager iterations - every loss and the kept share at every step, every compared
    parameter afterwards."""
    eager, pe, n_e, _, _ = _steps(PSEUDO, "0", steps=6)
    graph, pg, n_g, err, _ = _steps(PSEUDO, "1", steps=6)
    assert err is None, err
    assert n_e == 0 and n_g == 6 - 3, (n_e, n_g)
    print("eager", eager, "graph", graph, "max abs difference", np.abs(eager - graph).max())
    assert np.array_equal(eager, graph), (eager, graph)
    for n in pe:
        assert torch.equal(pe[n], pg[n]), n


@pytest.mark.usefixtures("deterministic_stats")
def test_without_the_flag_it_is_the_plain_step():
    """The other pseudo flags without --pseudo request nothing: the bits of a Trainer built without them."""
    plain, pp, _, _, t0 = PG._steps((), steps=2)
    off, po, _, _, t1 = _steps(("--pseudo_adaptive", "--pseudo_threshold", "0.5", "--pseudo_nb_bins", "10"), steps=2)
    assert not t0.pseudo_flag and not t1.pseudo_flag
    assert np.array_equal(plain[:, :4], off[:, :4]), (plain, off)
    for n in pp:
        assert torch.equal(pp[n], po[n]), n


def test_the_plop_preset_builds_and_steps():
    got, _, _, _, trainer = _steps((), method="PLOP")
    assert trainer.pod_flag and trainer.pseudo_flag and trainer.pseudo_adaptive and not trainer.lkd_flag and trainer.pixcon_weight == 0.0
    assert np.isfinite(got).all() and got[0, 4] > 0 and 0.0 < got[0, 5] <= 1.0


def test_run_py_logs_thresholds_and_resumes_without_the_pass(tmp_path):
    """run.py --method PLOP on synthetic batches, two iterations: the K = 16 thresholds and PSEUDO are logged; a second run resumed
    from its checkpoint takes the thresholds from it."""
    import re
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), "--data_root", "synthetic", "--method", "PLOP", "--task", "15-5", "--step", "1",
           "--crop_size", "65", "--batch_size", "96", "--epochs", "1", "--no_pretrained", "--opt_level", "O1", "--lr", "0.001", "--debug",
           "--print_interval", "1", "--val_interval", "100", "--name", "plop"]
    r = subprocess.run(cmd, cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    found = re.search(r"Pseudo-label thresholds of the 16 old classes: ((?:[0-9.]+ ?){16})", log)
    assert found, log[-3000:]
    kept = [float(v) for v in re.findall(r"PSEUDO ([-+0-9.eE]+)", log)]
    assert len(kept) == 2 and all(0.0 <= v <= 1.0 for v in kept), log[-3000:]
    ckpt = os.path.join(tmp_path, "checkpoints", "step", "15-5-voc_plop_1.pth")
    assert os.path.isfile(ckpt), os.listdir(tmp_path)
    cmd[cmd.index("--epochs") + 1] = "2"
    r = subprocess.run(cmd + ["--ckpt", ckpt], cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    log2 = r.stdout + r.stderr
    assert r.returncode == 0, log2[-3000:]
    again = re.search(r"Pseudo-label thresholds from the checkpoint: ((?:[0-9.]+ ?){16})", log2)
    assert again and "Pseudo-label thresholds of the" not in log2, log2[-3000:]
    assert again.group(1).split() == found.group(1).split()
