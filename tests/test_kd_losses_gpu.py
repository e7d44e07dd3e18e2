"""GPU: the fused logit-loss kernels on every loss pair of the reference's --method table (ucd_seg_losses_ex): {plain, unbiased}
cross entropy x {plain, unbiased} distillation x alpha, on every kernel form, against float64 built here from the formulas
of include/ucd_hip.h on the up-sampled logits; against the reference's own numbers (tests/golden/kd_losses.npz); and the
unbiased / alpha 1 / ce_old_cl = K call against ucd_seg_losses bit for bit.

Bounds: the project's own for this kernel (tests/test_seglosses_gpu.py:47-53): losses rel 1e-4, gradient max error / max 1e-3,
gradient L2-relative 1e-4."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_matches_compact, load_golden
from ucd_amd import synth

pytestmark = pytest.mark.gpu

PK16, PK20, PK12, REG16, REG24, WIDE_FX, WIDE_F32 = 1, 2, 3, 4, 5, 6, 7
FORM_NAMES = {PK16: "pk<16,8>", PK20: "pk<20,4>", PK12: "pk<12,12>", REG16: "reg<24,16>", REG24: "reg<24,24>",
              WIDE_FX: "wide/fixed", WIDE_F32: "wide/f32"}
FIXED_POINT = (PK16, PK20, PK12, WIDE_FX)
# form -> (Ctot, K, d_sem 4 bytes off the 16-byte grid): the splits and the unaligned route of tests/test_seglosses_gpu.py
FORMS = {PK16: (21, 16, False), PK20: (21, 20, False), PK12: (21, 11, False), REG16: (21, 16, True), REG24: (24, 18, False),
         WIDE_FX: (41, 27, False), WIDE_F32: (41, 27, True)}
# B, H, W, h, w: the per-form geometries of tests/test_seglosses_gpu.py (its GEOMETRIES, SMALL and the benchmark crop)
GEOMETRIES = {
    "bench": (3, 513, 513, 33, 33),
    "nonsquare": (1, 190, 321, 12, 21),
    "f64x8": (2, 128, 72, 2, 9),
    "f16": (2, 96, 160, 6, 10),
    "subtile": (2, 24, 40, 3, 5),
    "h1": (1, 64, 100, 1, 20),
    "w1": (2, 48, 64, 3, 1),
    "r513": (1, 513, 129, 33, 9),
    "small": (2, 129, 129, 9, 9),
}
MODES = [(kd, ce, alpha) for kd in ("plain", "unbiased") for ce in ("plain", "unbiased") for alpha in (1.0, 0.5)]
CE_W, KD_W = 1.0, 10.0


def _inputs(tag, Ctot, K, geo, scale=2.0):
    """Student / teacher logits and a label map in 8 x 8 blocks of background, OLD-class ids (a plain cross entropy scores them
    as themselves), new classes and ignored pixels; deterministic in the tag."""
    B, H, W, h, w = geo
    seed = zlib.crc32(tag.encode()) % 100000
    blocks = lambda lo, hi, s: np.repeat(np.repeat(synth.randint(seed, (B, -(-H // 8), -(-W // 8)), lo, hi, stream=s), 8, 1), 8, 2)[:, :H, :W]
    kind, old, new = blocks(0, 10, 3), blocks(1, max(K, 2), 4), blocks(K, Ctot, 5)
    lab = np.where(kind < 3, 0, np.where(kind < 5, old, new))
    lab = np.where(kind == 9, 255, lab)
    sem = synth.t_normal(seed, (B, Ctot, h, w), stream=1, scale=scale)
    sem_t = synth.t_normal(seed, (B, K, h, w), stream=2, scale=scale)
    return sem, sem_t, torch.from_numpy(lab.astype(np.int64))


def reference(sem, sem_t, labels, K, kd, ce, alpha, ce_w, kd_w, ignore=255):
    """(ce, kd, gradient w.r.t. the low-resolution logits) in the dtype / on the device of ``sem``, from the formulas:
    CE_p = -log softmax(z)_label, the classes below ce_old_cl pooled into the background (ce_old_cl = K, or 1: plain), mean over
    ALL pixels with ignored ones at 0; plain KD = -mean_p sum_{c<K} softmax(alpha t)_c log_softmax(z[:K])_c / K; unbiased KD =
    -mean_p [q_0 (LSE(z_0, z_K..) - LSE(z)) + sum_{1<=c<K} q_c (z_c - LSE(z))] / K."""
    H, W = labels.shape[-2:]
    s = sem.detach().clone().requires_grad_(True)
    z = F.interpolate(s, size=(H, W), mode="bilinear", align_corners=False)
    t = alpha * F.interpolate(sem_t, size=(H, W), mode="bilinear", align_corners=False)
    den = torch.logsumexp(z, dim=1)
    kce = K if ce == "unbiased" else 1
    lab = torch.where(labels < kce, torch.zeros_like(labels), labels)
    ign = labels == ignore
    idx = torch.where(ign, torch.zeros_like(lab), lab)
    picked = z.gather(1, idx.unsqueeze(1)).squeeze(1) - den
    logp = torch.where(idx == 0, torch.logsumexp(z[:, :kce], dim=1) - den, picked)
    l_ce = torch.where(ign, torch.zeros_like(logp), -logp).mean()
    q = torch.softmax(t, dim=1)
    if kd == "plain":
        l_kd = -(torch.log_softmax(z[:, :K], dim=1) * q).sum(dim=1).mean() / K
    else:
        bn = torch.logsumexp(torch.cat((z[:, :1], z[:, K:]), dim=1), dim=1) - den
        l_kd = -((q[:, 0] * bn + (q[:, 1:] * (z[:, 1:K] - den.unsqueeze(1))).sum(dim=1)) / K).mean()
    (ce_w * l_ce + kd_w * l_kd).backward()
    return l_ce.item(), l_kd.item(), s.grad


def launch(entry, sem, sem_t, labels, K, kd, ce, alpha, ce_w, kd_w, unaligned=False, want_form=None):
    """Through the C ABI on cuda:0: ``entry`` "ex" (ucd_seg_losses_ex) or "bare" (ucd_seg_losses); the plan is asked first which
    form the call gets.  Returns (ce, kd, d_sem as a [B, Ctot, h, w] device tensor)."""
    from ucd_amd import hip
    lib = hip.load()
    dev = torch.device("cuda:0")
    B, Ctot, h, w = sem.shape
    H, W = labels.shape[-2:]
    kce, mode = (K if ce == "unbiased" else 1), (hip.KD_PLAIN if kd == "plain" else hip.KD_UNBIASED)
    f = C.c_int()
    rc = lib.ucd_seg_losses_plan_ex(H, W, h, w, Ctot, K, kce, mode, 1, int(not unaligned), -1, C.byref(f), None, None, None)
    assert rc == 0, lib.ucd_last_error().decode()
    if want_form is not None:
        assert f.value == want_form, f"planned {FORM_NAMES[f.value]}, the case is written for {FORM_NAMES[want_form]}"
    rows = B * h * w
    s_buf = sem.to(dev).permute(0, 2, 3, 1).reshape(rows, Ctot).contiguous()
    t_buf = sem_t.to(dev).permute(0, 2, 3, 1).reshape(rows, K).contiguous()
    off = 1 if unaligned else 0
    store = torch.full((rows * Ctot + 8,), float("nan"), device=dev)
    d = store[off:off + rows * Ctot].view(rows, Ctot)
    assert d.data_ptr() % 16 == 4 * off
    out = torch.full((2,), float("nan"), device=dev)
    nbytes = lib.ucd_seg_losses_workspace_bytes(B, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lab = labels.to(dev)
    if entry == "bare":
        assert kd == "unbiased" and ce == "unbiased" and alpha == 1.0
        hip._check(lib.ucd_seg_losses(hip.ptr(s_buf), Ctot, hip.ptr(t_buf), K, hip.ptr(lab), B, H, W, h, w, Ctot, K, 255, ce_w, kd_w,
                                      hip.ptr(out), hip.ptr(d), Ctot, hip.ptr(ws), nbytes, hip.stream()), "ucd_seg_losses")
    else:
        hip._check(lib.ucd_seg_losses_ex(hip.ptr(s_buf), Ctot, hip.ptr(t_buf), K, hip.ptr(lab), B, H, W, h, w, Ctot, K, kce, mode,
                                         alpha, 255, ce_w, kd_w, hip.ptr(out), hip.ptr(d), Ctot, hip.ptr(ws), nbytes, hip.stream()),
                   "ucd_seg_losses_ex")
    torch.cuda.synchronize()
    assert bool(torch.isnan(store[:off]).all()) and bool(torch.isnan(store[off + rows * Ctot:]).all())
    return out[0].item(), out[1].item(), d.reshape(B, h, w, Ctot).permute(0, 3, 1, 2).clone(), f.value


def check(tag, got, ref, with_ce=True):
    (ce, kd, g), (ce_r, kd_r, g_r) = got, ref
    g, g_r = g.double().cpu(), g_r.double().cpu()
    e_max = ((g - g_r).abs().max() / g_r.abs().max()).item()
    e_l2 = ((g - g_r).norm() / g_r.norm()).item()
    print(f"{tag}: ce {ce:.6f} ref {ce_r:.6f} | kd {kd:.6f} ref {kd_r:.6f} | grad max-rel {e_max:.2e} L2-rel {e_l2:.2e}")
    if with_ce:
        assert ce == pytest.approx(ce_r, rel=1e-4)
    assert kd == pytest.approx(kd_r, rel=1e-4)
    assert e_max < 1e-3 and e_l2 < 1e-4, (e_max, e_l2)


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
@pytest.mark.parametrize("form", sorted(FORMS), ids=[FORM_NAMES[f] for f in sorted(FORMS)])
def test_every_form_and_mode_vs_float64(form, geo):
    Ctot, K, unaligned = FORMS[form]
    sem, sem_t, labels = _inputs(f"{geo}-{form}", Ctot, K, GEOMETRIES[geo])
    for kd, ce, alpha in MODES:
        ref = reference(sem.double(), sem_t.double(), labels, K, kd, ce, alpha, CE_W, KD_W)
        ce_v, kd_v, g, _ = launch("ex", sem, sem_t, labels, K, kd, ce, alpha, CE_W, KD_W, unaligned, want_form=form)
        check(f"{FORM_NAMES[form]} {geo} kd={kd} ce={ce} alpha={alpha}", (ce_v, kd_v, g), ref)


@pytest.mark.parametrize("kd,ce,alpha", [("plain", "plain", 0.5), ("unbiased", "plain", 1.0)])
def test_ade_split_at_full_size_vs_float64(kd, ce, alpha):
    """151 student / 101 teacher classes at 2 x 512^2: the many-class form at its benchmark shape."""
    sem, sem_t, labels = _inputs("ade", 151, 101, (2, 512, 512, 32, 32))
    ref = reference(sem.double(), sem_t.double(), labels, 101, kd, ce, alpha, CE_W, KD_W)
    ce_v, kd_v, g, _ = launch("ex", sem, sem_t, labels, 101, kd, ce, alpha, CE_W, KD_W, want_form=WIDE_FX)
    check(f"ade kd={kd} ce={ce} alpha={alpha}", (ce_v, kd_v, g), ref)


@pytest.mark.parametrize("regime", ["n12", "pm80"])
@pytest.mark.parametrize("form", [PK16, REG24, WIDE_FX], ids=["pk", "reg", "wide"])
def test_wide_logit_ranges(form, regime):
    """Logits of scale 12, and one class at +80 with the others at -80 (a class subset far below the leader: the sums of the
    old classes are taken again around their own maximum), plain distillation with plain and unbiased cross entropy."""
    Ctot, K, unaligned = FORMS[form]
    geo = GEOMETRIES["small"]
    sem, sem_t, labels = _inputs(f"{regime}-{form}", Ctot, K, geo, scale=12.0)
    if regime == "pm80":
        B, _, _, h, w = geo
        top = torch.from_numpy(synth.randint(11, (B, 1, h, w), 0, Ctot, stream=6))
        sem = torch.full((B, Ctot, h, w), -80.0).scatter_(1, top, 80.0)
        sem_t = torch.full((B, K, h, w), -80.0).scatter_(1, (top + 3) % K, 80.0)
    for kd, ce, alpha in (("plain", "plain", 1.0), ("plain", "unbiased", 0.5), ("unbiased", "plain", 0.5)):
        ref = reference(sem.double(), sem_t.double(), labels, K, kd, ce, alpha, CE_W, KD_W)
        ce_v, kd_v, g, _ = launch("ex", sem, sem_t, labels, K, kd, ce, alpha, CE_W, KD_W, unaligned, want_form=form)
        assert np.isfinite(ce_v) and np.isfinite(kd_v) and bool(torch.isfinite(g).all())
        check(f"{FORM_NAMES[form]} {regime} kd={kd} ce={ce} alpha={alpha}", (ce_v, kd_v, g), ref)


def test_against_reference_golden():
    """fused_seg_losses on the inputs of tests/golden/make_kd_golden.py against the numbers its run of the reference's
    utils/loss.py stored (float64 through F.interpolate), all 36 combinations."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_kd_golden as MK
    from ucd_amd.loss import fused_seg_losses
    gold = load_golden("kd_losses.npz")
    dev = torch.device("cuda:0")
    for shape in MK.UNIT_SHAPES:
        B, Ctot, K, h, H = shape
        sem, sem_t, labels = MK.unit_inputs(shape)
        for kd in ("plain", "unbiased"):
            for alpha in MK.ALPHAS:
                for ce in ("plain", "unbiased"):
                    key = MK.unit_key(shape, kd, alpha, ce)
                    s = sem.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
                    total, l_ce, l_kd = fused_seg_losses(s, sem_t.to(dev), labels.to(dev), K if ce == "unbiased" else 1, MK.UNIT_CE_W,
                                                         MK.UNIT_KD_W, kd=kd, alpha=alpha)
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
                        # stored as sums, row sums and samples: 1e-3 of the largest element on each sample, 1e-4 on the sums
                        gmax = float(np.abs(gold[key + "|grad::samples"]).max())
                        assert_matches_compact(gold, key + "|grad", g, rtol=1e-4, atol=1e-3 * gmax)


@pytest.mark.parametrize("form", sorted(FORMS), ids=[FORM_NAMES[f] for f in sorted(FORMS)])
def test_ex_with_the_first_pair_is_the_bare_call(form):
    """ucd_seg_losses_ex(ce_old_cl = K, UCD_KD_UNBIASED, alpha = 1) is ucd_seg_losses: the same launch.  The loss values (a fixed
    summation order in every form) and the fixed-point forms' gradients are compared bit for bit.  The register form and the
    many-class form on an unaligned d_sem add with fp32 atomics, whose last bits depend on the execution order even between two
    calls of ONE entry (include/ucd_hip.h, "Gradient arithmetic"): their gradients are held to 1e-6 of the largest element,
    a few ulps of an fp32 sum taken in another order, far below any change of arithmetic."""
    Ctot, K, unaligned = FORMS[form]
    for geo in ("bench", "nonsquare", "small"):
        sem, sem_t, labels = _inputs(f"bare-{geo}-{form}", Ctot, K, GEOMETRIES[geo])
        a = launch("bare", sem, sem_t, labels, K, "unbiased", "unbiased", 1.0, CE_W, KD_W, unaligned, want_form=form)
        b = launch("ex", sem, sem_t, labels, K, "unbiased", "unbiased", 1.0, CE_W, KD_W, unaligned, want_form=form)
        assert a[0] == b[0] and a[1] == b[1], (geo, a[:2], b[:2])
        if form in FIXED_POINT:
            assert torch.equal(a[2], b[2]), geo
        else:
            assert ((a[2] - b[2]).abs().max() / a[2].abs().max()).item() < 1e-6, geo


def test_plain_mode_at_the_benchmark_shape():
    """24 x 21 classes, 33 -> 513, kd_weight 100 (--method LWF): (1) the fused call equals the un-fused torch composition on the
    GPU; (2) with ce_weight = 0 the gradient is exactly zero in the new-class columns; (3) the fixed-point form returns the same
    bits on repeated calls; (4) the fused loss + backward allocates at least one [24, 21, 513, 513] fp32 tensor less than the
    composition at its peak (no up-sampled logit tensor exists)."""
    import torch.nn as nn
    from ucd_amd import hip
    from ucd_amd.loss import KnowledgeDistillationLoss, fused_seg_losses
    dev = torch.device("cuda:0")
    B, Ctot, K, h, H = 24, 21, 16, 33, 513
    sem0 = synth.t_normal(191, (B, Ctot, h, h), stream=2).to(dev).mul_(2.0)
    sem_t = synth.t_normal(192, (B, K, h, h), stream=2).to(dev).mul_(2.0)
    labels = synth.seg_labels(193, B, H, H, range(16, 21)).to(dev)
    f = C.c_int()
    assert hip.load().ucd_seg_losses_plan_ex(H, H, h, h, Ctot, K, 1, hip.KD_PLAIN, 1, 1, -1, C.byref(f), None, None, None) == 0
    assert f.value == PK16
    up = lambda t: F.interpolate(t, size=(H, H), mode="bilinear", align_corners=False)

    def fused(ce_w):
        s = sem0.clone().requires_grad_(True)
        total, ce, kd = fused_seg_losses(s, sem_t, labels, 1, ce_w, 100.0, kd="plain", alpha=1.0)
        total.backward()
        return total, ce, kd, s.grad

    def composed(ce_w):
        s = sem0.clone().requires_grad_(True)
        u = up(s)
        ce = nn.CrossEntropyLoss(ignore_index=255, reduction="none")(u, labels).mean()
        kd = KnowledgeDistillationLoss(alpha=1.0)(u, up(sem_t))
        total = ce_w * ce + 100.0 * kd
        total.backward()
        return total, ce, kd, s.grad

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        r = fn(1.0)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated(dev) - base, r

    fused(1.0)                                       # workspaces exist before anything is measured
    p_fused, (total, ce, kd, g) = peak(fused)
    p_comp, (total_r, ce_r, kd_r, g_r) = peak(composed)
    print(f"peak bytes above the inputs: fused {p_fused}, composition {p_comp}")
    check("bench plain", (ce.item(), kd.item(), g), (ce_r.item(), kd_r.item(), g_r))
    assert total.item() == pytest.approx(total_r.item(), rel=1e-4)
    assert p_comp - p_fused >= B * Ctot * H * H * 4, (p_fused, p_comp)
    g0 = fused(0.0)[3]
    assert bool((g0[:, K:] == 0).all()) and bool((g0[:, :K] != 0).any())
    for _ in range(5):
        total1, _, _, g1 = fused(1.0)
        assert total1.item() == total.item() and torch.equal(g1, g)


# ---- ILT's encoder term as one operation (ucd_attn_mse, csrc/featdist.hip) ------------------------------------------------------
ATTN_SHAPES = [(2, 81, 256, 256), (2, 81, 2048, 2048), (24, 1089, 2048, 2048), (2, 81, 203, 208)]     # B, HW, C, leading dimension


def _attn_ref(xs, xt, weight):
    """float64 from the same (already rounded) inputs: (loss, d_x) by the formulas of include/ucd_hip.h."""
    xs, xt = xs.double(), xt.double()

    def att(x):
        a = (x ** 2).sum(dim=2)                               # [B, HW]
        return a / a.norm(dim=1, keepdim=True)

    a_s, a_t = att(xs), att(xt)
    diff = a_s.unsqueeze(2) * xs - a_t.unsqueeze(2) * xt
    return (diff ** 2).mean().item(), weight * 2.0 * a_s.unsqueeze(2) * diff / diff.numel()


def _attn_call(xs, xt, ld, weight):
    """ucd_attn_mse through the C ABI on rows of pitch ``ld`` >= C whose padding columns are NaN; (loss, d_x [B, HW, C])."""
    from ucd_amd import hip
    lib = hip.load()
    B, HW, Cc = xs.shape
    dev = xs.device
    pad = lambda t: torch.cat((t, torch.full((B, HW, ld - Cc), float("nan"), dtype=t.dtype, device=dev)), dim=2).contiguous()
    s_buf, t_buf = pad(xs), pad(xt)
    d = torch.full((B, HW, ld), 777.0, dtype=xs.dtype, device=dev)
    out = torch.full((1,), float("nan"), device=dev)
    nbytes = lib.ucd_attn_mse_workspace_bytes(B, HW)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    hip._check(lib.ucd_attn_mse(hip.ptr(s_buf), ld, hip.ptr(t_buf), ld, hip.dtype_code(xs), B, HW, Cc, weight, hip.ptr(out), hip.ptr(d), ld,
                                hip.ptr(ws), nbytes, hip.stream()), "ucd_attn_mse")
    torch.cuda.synchronize()
    assert bool((d[:, :, Cc:] == 777.0).all())              # nothing written past the channels
    return out.item(), d[:, :, :Cc].clone()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", ATTN_SHAPES, ids=["x".join(map(str, s[:3])) for s in ATTN_SHAPES])
def test_attn_mse_vs_float64(shape, dtype):
    """fp32: loss rel 1e-4, gradient L2-relative 1e-4.  bf16: the loss as for fp32 (it is accumulated in fp32 from the rounded
    inputs); the gradient's only extra error is its one rounding to bf16 (2^-9 relative, doubled) over a floor for the fp32
    rounding of a nearly cancelling difference: |d - ref| <= 2^-8 |ref| + 2^-20 max |ref|.  Student and teacher are drawn
    independently.  Two calls give identical bits."""
    B, HW, Cc, ld = shape
    dev = torch.device("cuda:0")
    g = torch.Generator(dev).manual_seed(1000 + Cc + HW)
    xs = (torch.randn(B, HW, Cc, device=dev, generator=g) * 0.7).to(dtype)
    xt = (torch.randn(B, HW, Cc, device=dev, generator=g) * 0.7 + 0.1).to(dtype)
    weight = 100.0
    loss, d = _attn_call(xs, xt, ld, weight)
    loss_r, d_r = _attn_ref(xs, xt, weight)
    err = (d.double() - d_r).abs()
    l2 = (err.norm() / d_r.norm()).item()
    print(f"attn_mse {shape} {dtype}: loss {loss:.6e} ref {loss_r:.6e} | grad L2-rel {l2:.2e} max |ref| {d_r.abs().max().item():.3e}")
    assert loss == pytest.approx(loss_r, rel=1e-4)
    if dtype == torch.float32:
        assert l2 < 1e-4
    else:
        assert bool((err <= 2.0 ** -8 * d_r.abs() + 2.0 ** -20 * d_r.abs().max()).all()), (err - 2.0 ** -8 * d_r.abs()).max().item()
    loss2, d2 = _attn_call(xs, xt, ld, weight)
    assert loss2 == loss and torch.equal(d2, d)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_fused_attn_mse_gradient_equals_autograd_through_the_composition(dtype):
    """fused_attn_mse on [B, C, h, w] channels-last maps against autograd through the torch composition (att_map's
    differentiable branch, fp32 copies, MSELoss) in float64 on the same inputs, at the bounds of the test above."""
    import torch.nn as nn
    from ucd_amd.loss import fused_attn_mse
    dev = torch.device("cuda:0")
    B, Cc, h = 2, 256, 9
    g = torch.Generator(dev).manual_seed(77)
    xs = (torch.randn(B, Cc, h, h, device=dev, generator=g)).to(dtype).contiguous(memory_format=torch.channels_last)
    xt = (torch.randn(B, Cc, h, h, device=dev, generator=g) + 0.2).to(dtype).contiguous(memory_format=torch.channels_last)

    def att(x):
        a = (x ** 2).sum(dim=1)
        a = a / a.flatten(1).norm(dim=1)[:, None, None]
        return a.unsqueeze(1).detach() * x

    s = xs.clone().requires_grad_(True)
    loss = fused_attn_mse(s, xt, 100.0)
    (0.5 * loss).backward()
    r = xs.double().requires_grad_(True)
    loss_r = 100.0 * nn.MSELoss()(att(r), att(xt.double()))
    (0.5 * loss_r).backward()
    assert s.grad.dtype == dtype and s.grad.shape == xs.shape
    assert loss.item() == pytest.approx(loss_r.item(), rel=1e-4)
    err = (s.grad.double() - r.grad).abs()
    if dtype == torch.float32:
        assert (err.norm() / r.grad.norm()).item() < 1e-4
    else:
        # two roundings to bf16 here: d_x, then its product with the upstream gradient 0.5 (exact: a power of two)
        assert bool((err <= 2.0 ** -8 * r.grad.abs() + 2.0 ** -20 * r.grad.abs().max()).all())
