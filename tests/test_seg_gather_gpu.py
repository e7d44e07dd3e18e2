"""GPU: the gather form of the fused logit losses (ucd_seg_losses_gather, csrc/seg_gather.hip) at the
geometries no tiled form serves (ADE at --output_stride 8, small factors, factor 1) and - forced with form="gather" - at geometries
the tiled forms serve too.  Inputs, float64 references and bounds are those of tests/test_seglosses_gpu.py (unbiased pair) and
tests/test_kd_losses_gpu.py (the loss pairs of ucd_seg_losses_ex), by import; the gather form has no fixed point: A = 0."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

import test_kd_losses_gpu as KD
import test_seglosses_gpu as T
from conftest import assert_matches_compact, load_golden

pytestmark = pytest.mark.gpu

# B, H, W, h, w.  No tiled form serves these with 151 classes (ucd_seg_losses_plan; the few-class splits from the fourth on)
REFUSED = {
    "s8_129": (2, 129, 129, 17, 17), "s8_128": (1, 128, 128, 16, 16), "s8_ragged": (1, 57, 83, 9, 12), "f4": (2, 64, 64, 16, 16),
    "f3": (1, 48, 48, 16, 16), "f1.5x1.25": (1, 24, 20, 16, 16), "f1": (1, 16, 16, 16, 16),
}
# the tiled forms serve these: the gather form is forced
SERVED = {"small": (2, 129, 129, 9, 9), "nonsquare": (1, 190, 321, 12, 21), "f64x8": (2, 128, 72, 2, 9), "h1": (1, 64, 100, 1, 20)}
GEOS = {**REFUSED, **SERVED}
# a split test_seglosses_gpu.py does not list (its _inputs / _references look a case's split up in its table; its own cases, built
# at import, do not see the addition): ADE 100-10 at its last step, 141 teacher classes
T.SPLITS.setdefault("ade141", (151, 141, T.WIDE_FX))
SPLITS = ("ade", "ade141", "wide", "pk16", "pk20")          # (151, 101), (151, 141), (41, 27), (21, 16), (21, 20)
NO_FIXED_POINT = T.WIDE_F32                                   # _check's allowance A is 0 for the forms without fixed-point words
MAIN = REFUSED["s8_129"]


def _launch(case, inputs, form="gather", grad=True):
    """(ce, kd, gradient [B, Ctot, h, w] float64 numpy or None) through fused_seg_losses."""
    from ucd_amd.loss import fused_seg_losses
    dev = torch.device("cuda:0")
    K = T.SPLITS[case.split][1]
    sem, sem_t, labels = inputs
    s = sem.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(grad)
    total, ce, kd = fused_seg_losses(s, None if sem_t is None else sem_t.to(dev), labels.to(dev), K, case.ce_w, case.kd_w,
                                     ignore_index=case.ignore, form=form)
    if not grad:
        return ce.item(), kd.item(), None
    total.backward()
    return ce.item(), kd.item(), s.grad.double().cpu().numpy()


def _parity_cases():
    out = []
    for g, geo in GEOS.items():
        for split in SPLITS:
            out.append(T.Case("gather_" + g, split, geo))
            out.append(T.Case("gather_" + g + "_no_teacher", split, geo, teacher=False, kd_w=0.0))
    for split in SPLITS:
        out.append(T.Case("gather_all_ignored", split, MAIN, labels="all_ignored"))
        out.append(T.Case("gather_one_new", split, MAIN, labels="one_new"))
        out.append(T.Case("gather_no_ignored", split, MAIN, labels="no_ignored"))
        out.append(T.Case("gather_ignore250", split, MAIN, ignore=250))
        for regime in ("n12", "trained", "pm80"):
            out.append(T.Case("gather_" + regime, split, MAIN, regime=regime))
        out.append(T.Case("gather_ce0", split, MAIN, ce_w=0.0))
        out.append(T.Case("gather_kd0", split, MAIN, kd_w=0.0))
        out.append(T.Case("gather_both0", split, MAIN, ce_w=0.0, kd_w=0.0))
    return out


PARITY = _parity_cases()


def test_the_plan_refuses_what_this_file_calls_refused():
    from ucd_amd.loss import seg_losses_route
    for (B, H, W, h, w) in REFUSED.values():
        assert seg_losses_route(H, W, h, w, 151, 101, True) == "gather" and seg_losses_route(H, W, h, w, 151, 151, False) == "gather"
    for (B, H, W, h, w) in SERVED.values():
        for split in SPLITS:
            Ctot, K, _ = T.SPLITS[split]
            assert seg_losses_route(H, W, h, w, Ctot, K, True) == "tiled"


@pytest.mark.parametrize("case", PARITY, ids=[c.id for c in PARITY])
def test_unbiased_pair_vs_float64(case):
    """The unbiased pair against float64 (F.interpolate of float64 logits + the oracle's losses + autograd), bounds of
    test_seglosses_gpu._check with A = 0: losses within max(4 |fp32 composition - float64|, 1e-6 relative), gradient
    element-wise within 4 max |fp32 composition - float64|; an all-ignored map gives CE exactly 0, two zero weights a gradient
    that is exactly zero."""
    inputs = T._inputs(case)
    T._check(case, NO_FIXED_POINT, _launch(case, inputs), *T._references(case, inputs))


EX_GEOS = ("s8_129", "f3")


@pytest.mark.parametrize("geo", EX_GEOS)
@pytest.mark.parametrize("split", [(151, 101), (21, 16)], ids=["151-101", "21-16"])
def test_every_mode_vs_float64(split, geo):
    """{plain, unbiased} cross entropy x {plain, unbiased} distillation x alpha in {1, 0.5} at two refused geometries; reference
    and bounds of test_kd_losses_gpu (losses 1e-4, gradient 1e-3 max-relative and 1e-4 L2-relative)."""
    from ucd_amd.loss import fused_seg_losses
    Ctot, K = split
    dev = torch.device("cuda:0")
    sem, sem_t, labels = KD._inputs(f"gather-{geo}-{Ctot}", Ctot, K, REFUSED[geo])
    for kd, ce, alpha in KD.MODES:
        ref = KD.reference(sem.double(), sem_t.double(), labels, K, kd, ce, alpha, KD.CE_W, KD.KD_W)
        s = sem.to(dev).requires_grad_(True)
        total, ce_v, kd_v = fused_seg_losses(s, sem_t.to(dev), labels.to(dev), K if ce == "unbiased" else 1, KD.CE_W, KD.KD_W, kd=kd,
                                             alpha=alpha, form="gather")
        total.backward()
        KD.check(f"gather {geo} {Ctot} kd={kd} ce={ce} alpha={alpha}", (ce_v.item(), kd_v.item(), s.grad), ref)


@pytest.mark.parametrize("regime", ["n12", "pm80"])
@pytest.mark.parametrize("split", [(151, 101), (21, 16)], ids=["151-101", "21-16"])
def test_wide_logit_ranges_of_the_modes(split, regime):
    """test_kd_losses_gpu.test_wide_logit_ranges on the gather form: logits of scale 12, and one class at +80 over the others at
    -80 (the subset sums are taken again around the subset's own maximum), for three of the loss pairs."""
    from ucd_amd.loss import fused_seg_losses
    Ctot, K = split
    geo = REFUSED["s8_129"]
    dev = torch.device("cuda:0")
    sem, sem_t, labels = KD._inputs(f"gather-{regime}-{Ctot}", Ctot, K, geo, scale=12.0)
    if regime == "pm80":
        B, _, _, h, w = geo
        top = torch.from_numpy(KD.synth.randint(11, (B, 1, h, w), 0, Ctot, stream=6))
        sem = torch.full((B, Ctot, h, w), -80.0).scatter_(1, top, 80.0)
        sem_t = torch.full((B, K, h, w), -80.0).scatter_(1, (top + 3) % K, 80.0)
    for kd, ce, alpha in (("plain", "plain", 1.0), ("plain", "unbiased", 0.5), ("unbiased", "plain", 0.5)):
        ref = KD.reference(sem.double(), sem_t.double(), labels, K, kd, ce, alpha, KD.CE_W, KD.KD_W)
        s = sem.to(dev).requires_grad_(True)
        total, ce_v, kd_v = fused_seg_losses(s, sem_t.to(dev), labels.to(dev), K if ce == "unbiased" else 1, KD.CE_W, KD.KD_W, kd=kd,
                                             alpha=alpha, form="gather")
        total.backward()
        assert np.isfinite(ce_v.item()) and np.isfinite(kd_v.item()) and bool(torch.isfinite(s.grad).all())
        KD.check(f"gather {regime} {Ctot} kd={kd} ce={ce} alpha={alpha}", (ce_v.item(), kd_v.item(), s.grad), ref)


def test_against_reference_golden():
    """test_kd_losses_gpu.test_against_reference_golden with form="gather": the numbers the reference's utils/loss.py gave
    (tests/golden/kd_losses.npz), all 36 combinations, at that test's tolerances."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_kd_golden as MK
    from ucd_amd.loss import fused_seg_losses
    gold = load_golden("kd_losses.npz")
    dev = torch.device("cuda:0")
    n = 0
    for shape in MK.UNIT_SHAPES:
        B, Ctot, K, h, H = shape
        sem, sem_t, labels = MK.unit_inputs(shape)
        for kd in ("plain", "unbiased"):
            for alpha in MK.ALPHAS:
                for ce in ("plain", "unbiased"):
                    key = MK.unit_key(shape, kd, alpha, ce)
                    s = sem.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
                    total, l_ce, l_kd = fused_seg_losses(s, sem_t.to(dev), labels.to(dev), K if ce == "unbiased" else 1, MK.UNIT_CE_W,
                                                         MK.UNIT_KD_W, kd=kd, alpha=alpha, form="gather")
                    total.backward()
                    ce_r, kd_r = gold[key + "|loss"]
                    assert l_ce.item() == pytest.approx(ce_r, rel=1e-4), key
                    assert l_kd.item() == pytest.approx(kd_r, rel=1e-4), key
                    assert total.item() == pytest.approx(MK.UNIT_CE_W * ce_r + MK.UNIT_KD_W * kd_r, rel=1e-4), key
                    g = s.grad.cpu().numpy()
                    if key + "|grad" in gold:
                        g_r = gold[key + "|grad"].astype(np.float64)
                        assert np.abs(g - g_r).max() / np.abs(g_r).max() < 1e-3, key
                        assert np.linalg.norm(g - g_r) / np.linalg.norm(g_r) < 1e-4, key
                    else:
                        gmax = float(np.abs(gold[key + "|grad::samples"]).max())
                        assert_matches_compact(gold, key + "|grad", g, rtol=1e-4, atol=1e-3 * gmax)
                    n += 1
    assert n == 36


@pytest.mark.parametrize("split,geo", [("ade", "s8_129"), ("pk16", "f4")], ids=["151-101", "21-16"])
def test_the_same_inputs_give_the_same_bits(split, geo):
    """Forty calls on one input with unrelated kernels of varying length in between: total and gradient bit for bit; and the
    call that forms no gradient (d_sem = NULL) returns the same loss bits."""
    from ucd_amd.loss import fused_seg_losses
    dev = torch.device("cuda:0")
    case = T.Case("gather_bits", split, REFUSED[geo])
    K = T.SPLITS[split][1]
    sem, sem_t, labels = (t.to(dev) for t in T._inputs(case))
    junk = torch.empty(1 << 24, device=dev)

    def once():
        s = sem.clone().requires_grad_(True)
        total, ce, kd = fused_seg_losses(s, sem_t, labels, K, 1.0, 10.0, form="gather")
        total.backward()
        return torch.stack((total.detach(), ce, kd)), s.grad.clone()

    l0, g0 = once()
    for i in range(40):
        if i % 2:
            junk.normal_()
            (junk[: 1 << (12 + i % 12)] * 2).sum()
        l1, g1 = once()
        assert torch.equal(l1, l0) and torch.equal(g1, g0), i
    with torch.no_grad():
        total, ce, kd = fused_seg_losses(sem, sem_t, labels, K, 1.0, 10.0, form="gather")
    assert torch.equal(torch.stack((total, ce, kd)), l0)
    total, ce, kd = fused_seg_losses(sem, sem_t, labels, K, 1.0, 10.0, form="gather")        # a sem that needs no gradient
    assert not total.requires_grad and torch.equal(torch.stack((total, ce, kd)), l0)


@pytest.mark.parametrize("split", ["ade", "pk16"])
@pytest.mark.parametrize("grad", [True, False], ids=["d_sem", "losses_only"])
def test_buffer_hygiene_through_the_c_abi(split, grad):
    """Padded ld_s / ld_t / ld_d on NaN-filled buffers: every element of d_sem[:, :Ctot] is written (finite, and inside the
    float64 bound: nothing read from a padding column), the columns past Ctot are still NaN, nothing outside the block is
    written; with d_sem = NULL the losses have the same bits."""
    from ucd_amd import hip
    lib = hip.load()
    dev = torch.device("cuda:0")
    case = T.Case("gather_ld_padded", split, (2, 57, 83, 9, 12), pad=(3, 5, 7))
    Ctot, K, _ = T.SPLITS[split]
    B, H, W, h, w = case.geo
    inputs = T._inputs(case)
    sem, sem_t, labels = inputs
    rows = B * h * w
    ld_s, ld_t, ld_d = Ctot + case.pad[0], K + case.pad[1], Ctot + case.pad[2]
    nan = float("nan")
    s_buf = torch.full((rows, ld_s), nan, device=dev)
    s_buf[:, :Ctot] = sem.permute(0, 2, 3, 1).reshape(rows, Ctot).to(dev)
    t_buf = torch.full((rows, ld_t), nan, device=dev)
    t_buf[:, :K] = sem_t.permute(0, 2, 3, 1).reshape(rows, K).to(dev)
    store = torch.full((rows * ld_d + 16,), nan, device=dev)
    d = store[8:8 + rows * ld_d].view(rows, ld_d)
    lab = labels.to(dev)
    nbytes = lib.ucd_seg_losses_gather_workspace_bytes(B, h, w)
    assert nbytes == rows * 8
    ws = torch.full((rows * 2 + 8,), nan, device=dev)

    def call(d_ptr):
        out = torch.full((4,), nan, device=dev)
        hip._check(lib.ucd_seg_losses_gather(hip.ptr(s_buf), ld_s, hip.ptr(t_buf), ld_t, hip.ptr(lab), B, H, W, h, w, Ctot, K, K,
                                             hip.KD_UNBIASED, 1.0, case.ignore, case.ce_w, case.kd_w, hip.ptr(out), d_ptr, ld_d,
                                             hip.ptr(ws), nbytes, hip.stream()), "ucd_seg_losses_gather")
        torch.cuda.synchronize()
        assert bool(torch.isnan(out[2:]).all()) and bool(torch.isnan(ws[rows * 2:]).all()) and bool(torch.isfinite(ws[:rows * 2]).all())
        return out[:2].clone()

    out = call(hip.ptr(d) if grad else None)
    assert bool(torch.isnan(store[:8]).all()) and bool(torch.isnan(store[8 + rows * ld_d:]).all())
    assert bool(torch.isnan(d[:, Ctot:]).all())
    ref64, ref32 = T._references(case, inputs)
    if grad:
        assert bool(torch.isfinite(d[:, :Ctot]).all())
        g = d[:, :Ctot].reshape(B, h, w, Ctot).permute(0, 3, 1, 2).double().cpu().numpy()
        T._check(case, NO_FIXED_POINT, (out[0].item(), out[1].item(), g), ref64, ref32)
        assert torch.equal(call(None), out)
    else:
        assert bool(torch.isnan(d).all())
        for got, l64, l32 in zip(out.tolist(), ref64[:2], ref32[:2]):
            assert abs(got - l64) <= max(4.0 * abs(l32 - l64), 1e-6 * abs(l64)), (got, l64, l32)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("geo", sorted(SERVED))
def test_gather_and_tiled_agree(split, geo):
    """At a geometry both serve: each is inside its own bound of float64 (A + R for the tiled form, R for the gather form), so the
    two are within A + 2 R of each other; the losses within the sum of their two loss bounds."""
    from ucd_amd import hip
    case = T.Case("gather_" + geo, split, SERVED[geo])
    inputs = T._inputs(case)
    (ce64, kd64, g64), (ce32, kd32, g32) = T._references(case, inputs)
    a, b = _launch(case, inputs, "gather"), _launch(case, inputs, "tiled")
    R = 4.0 * float(np.abs(g32 - g64).max())
    A = T._fixed_point_allowance(case, T._plan(case, hip.load()))
    err = float(np.abs(a[2] - b[2]).max())
    print(f"{case.id}: gather vs tiled gradient {err:.2e}, bound {A + 2 * R:.2e}; ce {abs(a[0] - b[0]):.2e} kd {abs(a[1] - b[1]):.2e}")
    assert err <= A + 2 * R
    assert abs(a[0] - b[0]) <= 2 * max(4.0 * abs(ce32 - ce64), 1e-6 * abs(ce64))
    assert abs(a[1] - b[1]) <= 2 * max(4.0 * abs(kd32 - kd64), 1e-6 * abs(kd64))


def test_auto_follows_the_route():
    """form="auto" is the gather form where the plan refuses and - bit for bit in the losses - the tiled call where it serves;
    form="tiled" keeps the refusal and its message."""
    from ucd_amd.loss import fused_seg_losses
    dev = torch.device("cuda:0")
    case = T.Case("gather_auto", "ade", MAIN)
    sem, sem_t, labels = (t.to(dev) for t in T._inputs(case))
    auto = fused_seg_losses(sem, sem_t, labels, 101, 1.0, 10.0)
    forced = fused_seg_losses(sem, sem_t, labels, 101, 1.0, 10.0, form="gather")
    assert all(torch.equal(x, y) for x, y in zip(auto, forced))
    with pytest.raises(RuntimeError, match="no form of the kernel serves this factor"):
        fused_seg_losses(sem, sem_t, labels, 101, 1.0, 10.0, form="tiled")
    case = T.Case("gather_auto", "ade", (1, 128, 128, 8, 8))
    sem, sem_t, labels = (t.to(dev) for t in T._inputs(case))
    auto = fused_seg_losses(sem, sem_t, labels, 101, 1.0, 10.0)
    tiled = fused_seg_losses(sem, sem_t, labels, 101, 1.0, 10.0, form="tiled")
    assert all(torch.equal(x, y) for x, y in zip(auto, tiled))


@pytest.mark.parametrize("split", [(300, 200), (700, 450)], ids=["8_rounds", "29_rounds"])
def test_more_than_192_classes(split):
    """The instantiations of more class rounds than any dataset of the reference needs (up to 512 and up to 1820 classes), at one
    small geometry against the float64 formulas of test_kd_losses_gpu."""
    from ucd_amd.loss import fused_seg_losses
    Ctot, K = split
    dev = torch.device("cuda:0")
    sem, sem_t, labels = KD._inputs(f"gather-many-{Ctot}", Ctot, K, (1, 40, 56, 5, 7))
    for kd, ce, alpha in (("unbiased", "unbiased", 1.0), ("plain", "plain", 0.5)):
        ref = KD.reference(sem.double(), sem_t.double(), labels, K, kd, ce, alpha, KD.CE_W, KD.KD_W)
        s = sem.to(dev).requires_grad_(True)
        total, ce_v, kd_v = fused_seg_losses(s, sem_t.to(dev), labels.to(dev), K if ce == "unbiased" else 1, KD.CE_W, KD.KD_W, kd=kd,
                                             alpha=alpha, form="gather")
        total.backward()
        KD.check(f"gather {Ctot} classes kd={kd} ce={ce} alpha={alpha}", (ce_v.item(), kd_v.item(), s.grad), ref)


def test_labels_that_are_no_class_read_as_in_the_tiled_forms():
    """include/ucd_hip.h: a negative label is the background, a label in [Ctot, ...) other than ignore_index matches no class
    (the tiled forms: beyond the padding of their class rows, which is where the labels of this test lie).
    Both forms on a label map with such values: the gradients within A + 2 R of each other (R, A of the regular map of the same
    inputs, as in test_gather_and_tiled_agree), the losses within 1e-5 relative - some hundred ulps of two fp32 evaluations of the
    same sums, where reading one of the three label blocks differently moves the cross entropy by more than 1e-2."""
    case = T.Case("gather_small", "wide", SERVED["small"])
    sem, sem_t, labels = T._inputs(case)
    (_, _, g64), (_, _, g32) = T._references(case, (sem, sem_t, labels))
    labels = labels.clone()
    labels[:, 8:24, 8:40] = -3
    labels[:, 40:56, 16:48] = 1000
    labels[:, 64:80, 0:32] = 200
    a, b = _launch(case, (sem, sem_t, labels), "gather"), _launch(case, (sem, sem_t, labels), "tiled")
    R = 4.0 * float(np.abs(g32 - g64).max())
    A = T._fixed_point_allowance(case, T.WIDE_FX)
    assert np.isfinite(a[2]).all() and abs(a[0] - b[0]) <= 1e-5 * abs(b[0]) and abs(a[1] - b[1]) <= 1e-5 * abs(b[1])
    assert float(np.abs(a[2] - b[2]).max()) <= A + 2 * R


def _recorded_bits():
    import importlib.util
    import json
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_seg_gather_bits_golden", os.path.join(golden, "make_seg_gather_bits_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(golden, "seg_gather_bits.json")) as f:
        return gen, json.load(f)["cases"]


def test_the_kernel_reproduces_the_recorded_bits():
    """The kernel takes its cell walk - staging, scan ranges, a pixel's weights, owner and corner rows, the four-corner
    interpolation - from csrc/seg_cell.h, which it shares with the BCE kernel.  The walk is the arithmetic each kernel carried in
    a copy of its own, expression for expression (the library is built without fp contraction), so every output must be
    BIT-identical to that build's.  tests/golden/seg_gather_bits.json holds the SHA-256 of loss_out, d_sem and the per-cell pairs
    as that build wrote them (tests/golden/make_seg_gather_bits_golden.py): factor 1, ragged non-square factors, h = 1, factor
    64 x 8; one class split per instantiation (NR 1, 2, 3, 8, 29); no teacher, plain KD, alpha 0.5, plain cross entropy, no d_sem,
    padded leading dimensions, labels that are no class, the rescue branch.  The same calls are replayed here."""
    gen, recorded = _recorded_bits()
    assert set(recorded) == set(gen.CASES)
    bad = []
    for case in gen.SM_CASES:
        got = gen.run_case(case)
        assert set(got) == set(recorded[case]), f"{case}: outputs {sorted(set(got) ^ set(recorded[case]))}"
        bad += [f"{case}: {name}" for name in got if got[name] != recorded[case][name]]
    assert not bad, "outputs whose bits differ from the recorded build's: " + ", ".join(bad)
