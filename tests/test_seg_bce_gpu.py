"""GPU: the fused BCE losses (ucd_seg_bce, csrc/seg_gather.hip; ucd_amd.loss.fused_seg_bce) against the float64 restatement of their
formulas (seg_bce_ref.py) and the reference's own numbers (tests/golden/bce_losses.npz).

Bounds: the project's own for the fused logit losses (tests/test_seglosses_gpu.py:47-53, tests/test_kd_losses_gpu.py): losses rel
1e-4, gradient max error / max 1e-3, gradient L2-relative 1e-4."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
import seg_bce_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.0


def launch(sem, sem_t, labels, hard_w=1.0, soft_w=0.0, ld_s=None, ld_t=None, ld_d=None, want_grad=True, ignore=255):
    """Through the C ABI on cuda:0.  Returns (loss_out [2] on the host, d_sem rows [B*h*w, ld_d] on the device or None); the padding
    columns of every buffer hold SENTINEL."""
    from ucd_amd import hip
    lib = hip.load()
    dev = torch.device("cuda:0")
    B, Ctot, h, w = sem.shape
    H, W = labels.shape[-2:]
    rows = B * h * w
    K = sem_t.shape[1] if sem_t is not None else 1
    ld_s, ld_t, ld_d = ld_s or Ctot, ld_t or K, ld_d or Ctot

    def padded(t, ld):
        buf = torch.full((rows, ld), SENTINEL, device=dev)
        buf[:, :t.shape[1]] = t.to(dev).float().permute(0, 2, 3, 1).reshape(rows, t.shape[1])
        return buf

    s_buf = padded(sem, ld_s)
    t_buf = padded(sem_t, ld_t) if sem_t is not None else None
    d = torch.full((rows, ld_d), SENTINEL, device=dev) if want_grad else None
    out = torch.full((2,), float("nan"), device=dev)
    nbytes = lib.ucd_seg_bce_workspace_bytes(B, h, w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lab = labels.to(dev).contiguous()
    hip._check(lib.ucd_seg_bce(hip.ptr(s_buf), ld_s, hip.ptr(t_buf), ld_t, hip.ptr(lab), B, H, W, h, w, Ctot, K, ignore, hard_w, soft_w,
                               hip.ptr(out), hip.ptr(d), ld_d, hip.ptr(ws), nbytes, hip.stream()), "ucd_seg_bce")
    torch.cuda.synchronize()
    return out.cpu(), d


def as_map(d, B, Ctot, h, w):
    return d[:, :Ctot].reshape(B, h, w, Ctot).permute(0, 3, 1, 2).cpu().double()


def check(out, d, ref, shape4, soft=True, tag=""):
    """The three bounds, against (L_bce, soft, gradient) of the restatement."""
    l_bce, l_soft, grad = ref
    B, Ctot, h, w = shape4
    g = as_map(d, B, Ctot, h, w)
    gmax, gerr, l2 = grad.abs().max().item(), (g - grad).abs().max().item(), ((g - grad).norm() / grad.norm()).item()
    print(tag, "bce", out[0].item(), l_bce, "soft", out[1].item(), l_soft, "grad max err / max", gerr / gmax, "L2 rel", l2)
    assert torch.isfinite(out).all() and torch.isfinite(g).all()
    assert out[0].item() == pytest.approx(l_bce, rel=1e-4)
    if soft:
        assert out[1].item() == pytest.approx(l_soft, rel=1e-4)
    else:
        assert out[1].item() == 0.0
    assert gerr / gmax < 1e-3
    assert l2 < 1e-4


@pytest.mark.parametrize("teacher", [True, False], ids=["teacher", "no_teacher"])
@pytest.mark.parametrize("shape", R.GOLDEN_SHAPES, ids=R.golden_key)
def test_golden_shapes(shape, teacher):
    """The three golden shapes with teacher and weights (1, 10) against the restatement AND the reference's numbers; the same
    without teacher against the restatement (the golden's gradient holds the soft term)."""
    B, Ctot, K, h, H = shape
    sem, sem_t, labels = R.golden_inputs(shape)
    t = sem_t if teacher else None
    out, d = launch(sem, t, labels, R.HARD_W, R.SOFT_W if teacher else 0.0)
    check(out, d, R.restatement(sem, t, labels, R.HARD_W, R.SOFT_W if teacher else 0.0), sem.shape, soft=teacher, tag=str(shape))
    gold = load_golden("bce_losses.npz")
    ref = gold[R.golden_key(shape) + "|loss"]
    assert out[0].item() == pytest.approx(ref[0], rel=1e-4)
    if teacher:
        assert out[1].item() == pytest.approx(ref[1], rel=1e-4)
        err, gmax = R.golden_grad_errors(gold, R.golden_key(shape) + "|grad", as_map(d, *sem.shape).numpy())
        print("against the golden gradient: max error / max", err / gmax)
        assert err / gmax < 1e-3


GEOMETRIES = {
    "one_cell": (1, 5, 3, 1, 1, 16, 16),                # every pixel clamps to one cell
    "nonsquare": (1, 20, 14, 12, 7, 190, 97),           # non-integer factors
    "factor1": (1, 7, 3, 8, 8, 8, 8),                   # factors 1 and 2, which ucd_seg_losses refuses
    "factor2": (1, 7, 3, 8, 8, 16, 16),
    "factor64_5": (1, 21, 16, 2, 2, 129, 129),
    "many_classes": (1, 151, 101, 4, 4, 64, 64),        # the class-chunk loop
}


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_edge_geometry_and_many_classes(name):
    B, Ctot, K, h, w, H, W = GEOMETRIES[name]
    sem, sem_t, labels = R.random_case(4200 + Ctot + h, B, Ctot, K, h, w, H, W)
    out, d = launch(sem, sem_t, labels, 1.0, 10.0)
    check(out, d, R.restatement(sem, sem_t, labels, 1.0, 10.0), sem.shape, tag=name)


def test_leading_dimensions_and_untouched_padding():
    """Ctot = 21 in rows of 24 (student, gradient) and K = 16 in rows of 20: the padding columns are never read (they hold a
    sentinel that would wreck the sums) and those of d_sem still hold it afterwards."""
    B, Ctot, K, h, w, H, W = 2, 21, 16, 5, 6, 40, 52
    sem, sem_t, labels = R.random_case(4301, B, Ctot, K, h, w, H, W)
    out, d = launch(sem, sem_t, labels, 1.0, 10.0, ld_s=24, ld_t=20, ld_d=24)
    check(out, d, R.restatement(sem, sem_t, labels, 1.0, 10.0), sem.shape, tag="ld")
    assert (d[:, Ctot:] == SENTINEL).all()
    out2, d2 = launch(sem, sem_t, labels, 1.0, 10.0)
    assert torch.equal(out, out2) and torch.equal(d[:, :Ctot], d2)


def test_labels_all_ignored_one_class_and_out_of_range():
    B, Ctot, K, h, w, H, W = 1, 21, 16, 4, 5, 50, 61
    sem, sem_t, labels = R.random_case(4302, B, Ctot, K, h, w, H, W)
    # all ignored: the hard loss is exactly 0 and the gradient is the soft term's alone
    ign = torch.full_like(labels, 255)
    out, d = launch(sem, sem_t, ign, 1.0, 10.0)
    assert out[0].item() == 0.0
    _, _, soft_grad = R.restatement(sem, sem_t, ign, 0.0, 10.0)
    check(out, d, (0.0, R.restatement(sem, sem_t, ign, 1.0, 10.0)[1], soft_grad), sem.shape, tag="all ignored")
    out_s, d_s = launch(sem, sem_t, ign, 0.0, 10.0)
    assert torch.equal(d, d_s) and torch.equal(out, out_s)
    # all one class
    one = torch.full_like(labels, 17)
    out, d = launch(sem, sem_t, one, 1.0, 10.0)
    check(out, d, R.restatement(sem, sem_t, one, 1.0, 10.0), sem.shape, tag="one class")
    # a label of 200 with Ctot = 21 behaves as ignored: the same bits as 255 in its place
    odd = labels.clone()
    odd[:, 10:30, 5:40] = 200
    as_ign = torch.where(odd == 200, torch.full_like(odd, 255), odd)
    out_a, d_a = launch(sem, sem_t, odd, 1.0, 10.0)
    out_b, d_b = launch(sem, sem_t, as_ign, 1.0, 10.0)
    assert torch.equal(out_a, out_b) and torch.equal(d_a, d_b)
    check(out_a, d_a, R.restatement(sem, sem_t, odd, 1.0, 10.0), sem.shape, tag="label 200")


def test_logits_of_90_are_finite_and_within_the_bounds():
    B, Ctot, K, h, w, H, W = 1, 21, 16, 5, 5, 64, 64
    sem, sem_t, labels = R.random_case(4303, B, Ctot, K, h, w, H, W)
    sem = sem * (90.0 / sem.abs().max())
    sem_t = sem_t * (90.0 / sem_t.abs().max())
    assert sem.abs().max().item() == pytest.approx(90.0) and sem_t.abs().max().item() == pytest.approx(90.0)
    out, d = launch(sem, sem_t, labels, 1.0, 10.0)
    check(out, d, R.restatement(sem, sem_t, labels, 1.0, 10.0), sem.shape, tag="+-90")


def test_same_inputs_same_bits_and_losses_only():
    B, Ctot, K, h, H = R.GOLDEN_SHAPES[0]
    sem, sem_t, labels = R.golden_inputs(R.GOLDEN_SHAPES[0])
    out1, d1 = launch(sem, sem_t, labels, 1.0, 10.0)
    out2, d2 = launch(sem, sem_t, labels, 1.0, 10.0)
    assert torch.equal(out1, out2) and torch.equal(d1, d2)
    out3, d3 = launch(sem, sem_t, labels, 1.0, 10.0, want_grad=False)          # d_sem = NULL: the same loss bits
    assert d3 is None and torch.equal(out1, out3)


def test_autograd_function_and_no_grad():
    """fused_seg_bce: the gradient arrives through autograd in the layout and dtype of ``sem``; without a gradient to form (no_grad,
    a ``sem`` that requires none) the losses are the same bits."""
    from ucd_amd.loss import fused_seg_bce
    dev = torch.device("cuda:0")
    shape = R.GOLDEN_SHAPES[1]
    sem, sem_t, labels = R.golden_inputs(shape)
    s = sem.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    total, bce, soft = fused_seg_bce(s, sem_t.to(dev), labels.to(dev), 1.0, 10.0)
    assert not bce.requires_grad and not soft.requires_grad
    (2.0 * total).backward()
    l_bce, l_soft, grad = R.restatement(sem, sem_t, labels, 1.0, 10.0)
    assert total.item() == pytest.approx(l_bce + 10.0 * l_soft, rel=1e-4)
    g = s.grad.cpu().double() / 2.0
    assert ((g - grad).norm() / grad.norm()).item() < 1e-4 and (g - grad).abs().max().item() / grad.abs().max().item() < 1e-3
    with torch.no_grad():
        _, bce2, soft2 = fused_seg_bce(s, sem_t.to(dev), labels.to(dev), 1.0, 10.0)
    _, bce3, soft3 = fused_seg_bce(s.detach(), sem_t.to(dev), labels.to(dev), 1.0, 10.0)
    assert torch.equal(bce, bce2) and torch.equal(soft, soft2) and torch.equal(bce, bce3) and torch.equal(soft, soft3)


def test_with_kd_the_gradients_add():
    """--method LWF --bce: fused_seg_bce + fused_seg_losses(ce_weight=0, kd_weight=100, kd="plain", old_cl 1) on the same logits; the
    summed autograd gradient is that of the float64 BCE + 100 * KD (plain KD: -mean_p sum_{c<K} softmax(zt)_c log_softmax(z[:K])_c / K)."""
    from ucd_amd.loss import fused_seg_bce, fused_seg_losses
    dev = torch.device("cuda:0")
    shape = R.GOLDEN_SHAPES[0]
    B, Ctot, K, h, H = shape
    sem, sem_t, labels = R.golden_inputs(shape)
    s = sem.to(dev).requires_grad_(True)
    t_bce, bce, _ = fused_seg_bce(s, None, labels.to(dev), 1.0, 0.0)
    t_kd, _, kd = fused_seg_losses(s, sem_t.to(dev), labels.to(dev), 1, 0.0, 100.0, kd="plain", alpha=1.0)
    (t_bce + t_kd).backward()
    l_bce, _, g_bce = R.restatement(sem, None, labels, 1.0, 0.0)
    sd = sem.double().requires_grad_(True)
    up = lambda x: F.interpolate(x, size=(H, H), mode="bilinear", align_corners=False)
    l_kd = -(torch.log_softmax(up(sd)[:, :K], dim=1) * torch.softmax(up(sem_t.double()), dim=1)).sum(dim=1).mean() / K
    (100.0 * l_kd).backward()
    grad = g_bce + sd.grad
    assert bce.item() == pytest.approx(l_bce, rel=1e-4) and kd.item() == pytest.approx(l_kd.item(), rel=1e-4)
    assert (t_bce + t_kd).item() == pytest.approx(l_bce + 100.0 * l_kd.item(), rel=1e-4)
    g = s.grad.cpu().double()
    print("BCE + 100 KD: grad max err / max", (g - grad).abs().max().item() / grad.abs().max().item(), "L2", ((g - grad).norm() / grad.norm()).item())
    assert (g - grad).abs().max().item() / grad.abs().max().item() < 1e-3
    assert ((g - grad).norm() / grad.norm()).item() < 1e-4


def test_the_kernel_reproduces_the_recorded_bits():
    """The kernel takes its cell walk from csrc/seg_cell.h, which it shares with the soft-max gather kernel: the arithmetic it
    carried in a copy of its own, expression for expression, so every output must be BIT-identical to that build's.
    tests/golden/seg_gather_bits.json holds the SHA-256 of loss_out, d_sem and the per-cell pairs as that build wrote them
    (tests/golden/make_seg_gather_bits_golden.py): Ctot 24, 25 and 49 (one, two and three register chunks), K = 7 and K = Ctot, on
    factor 1, ragged non-square factors, h = 1 and factor 64 x 8; no teacher, no d_sem, padded leading dimensions, labels outside
    [0, Ctot), logits of +-90.  The same calls are replayed here."""
    import importlib.util
    import json
    import os
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_seg_gather_bits_golden", os.path.join(golden, "make_seg_gather_bits_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(golden, "seg_gather_bits.json")) as f:
        recorded = json.load(f)["cases"]
    assert set(recorded) == set(gen.CASES)
    bad = []
    for case in gen.BCE_CASES:
        got = gen.run_case(case)
        assert set(got) == set(recorded[case]), f"{case}: outputs {sorted(set(got) ^ set(recorded[case]))}"
        bad += [f"{case}: {name}" for name in got if got[name] != recorded[case][name]]
    assert not bad, "outputs whose bits differ from the recorded build's: " + ", ".join(bad)
