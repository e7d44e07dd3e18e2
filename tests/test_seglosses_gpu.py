"""GPU: fused bilinear up-sampling + UnbiasedCE + UnbiasedKD (ucd_seg_losses, through the C ABI) against
the CPU oracle, which up-samples with F.interpolate and applies the reference's loss restatements."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import losses as OL
from ucd_amd import synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,Ctot,K,h,H,with_kd", [
    (2, 21, 16, 9, 129, True),       # VOC 15-5
    (3, 21, 16, 33, 513, True),      # full-size crop
    (2, 20, 14, 12, 190, True),      # Cityscapes 13-6, non-integer scale
    (2, 151, 101, 8, 128, True),     # ADE 100-50
    (2, 21, 16, 9, 129, False),      # cross entropy only
    (2, 21, 1, 9, 129, False),       # step 0: plain cross entropy (old_cl = 1)
    (3, 151, 101, 32, 512, True),    # ADE 100-50 at the per-rank shape of configs[3] (the many-class kernel at full size)
    (2, 41, 27, 11, 173, True),      # many-class kernel: class counts off the 4-grid, non-integer scale, ragged tiles
    (2, 151, 1, 8, 128, False),      # many-class kernel without a teacher (ADE step 0)
])
def test_fused_seg_losses_vs_oracle(B, Ctot, K, h, H, with_kd):
    from ucd_amd.loss import fused_seg_losses
    seed = 7000 + Ctot + h
    sem = synth.t_normal(seed, (B, Ctot, h, h), stream=1, scale=2.0)
    sem_t = synth.t_normal(seed, (B, K, h, h), stream=2, scale=2.0)
    labels = synth.seg_labels(seed, B, H, H, range(K, Ctot) if K < Ctot else [1], rects=4)
    if K == 1:
        labels = torch.from_numpy(np.where(synth.randint(seed, (B, H, H), 0, Ctot + 2, stream=5) >= Ctot, 255,
                                           synth.randint(seed, (B, H, H), 0, Ctot, stream=6)))
    kd_w = 10.0 if with_kd else 0.0
    # oracle
    s_ref = sem.clone().requires_grad_(True)
    up = F.interpolate(s_ref, size=(H, H), mode="bilinear", align_corners=False)
    ce_ref = OL.unbiased_cross_entropy(up, labels, K).mean()
    kd_ref = OL.unbiased_kd(up, F.interpolate(sem_t, size=(H, H), mode="bilinear", align_corners=False)) if with_kd \
        else torch.zeros(())
    (ce_ref + kd_w * kd_ref).backward()
    # HIP
    dev = torch.device("cuda:0")
    s_dev = sem.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    total, ce, kd = fused_seg_losses(s_dev, sem_t.to(dev) if with_kd else None, labels.to(dev), K, 1.0, kd_w)
    total.backward()
    assert ce.item() == pytest.approx(ce_ref.item(), rel=1e-4)
    if with_kd:
        assert kd.item() == pytest.approx(kd_ref.item(), rel=1e-4)
    assert total.item() == pytest.approx((ce_ref + kd_w * kd_ref).item(), rel=1e-4)
    g, gr = s_dev.grad.cpu(), s_ref.grad
    assert (g - gr).abs().max().item() / gr.abs().max().item() < 1e-3
    assert (g - gr).norm().item() / gr.norm().item() < 1e-4


def test_full_size_invariants_b24_513():
    """The benchmark shape (24 x 21 classes, 33x33 logits up-sampled to 513x513) against properties that hold at any size:
    (1) the fused kernel equals the un-fused torch composition ON THE GPU (bilinear up-sampling, then the unbiased CE / KD
    modules of this package, which tests above pin to the oracle); (2) every loss term is a difference of log-sum-exps of
    the same logits, so its gradient sums to zero over the classes at every low-resolution cell."""
    from ucd_amd.loss import UnbiasedCrossEntropy, UnbiasedKnowledgeDistillationLoss, fused_seg_losses
    dev = torch.device("cuda:0")
    B, Ctot, K, h, H = 24, 21, 16, 33, 513
    sem = synth.t_normal(91, (B, Ctot, h, h), stream=2).to(dev).mul_(2.0).requires_grad_(True)
    sem_t = synth.t_normal(92, (B, K, h, h), stream=2).to(dev).mul_(2.0)
    labels = synth.seg_labels(93, B, H, H, range(16, 21)).to(dev)
    total, ce, kd = fused_seg_losses(sem, sem_t, labels, K, 1.0, 10.0)
    total.backward()
    g = sem.grad.clone()
    ref_in = sem.detach().clone().requires_grad_(True)
    up = lambda t: F.interpolate(t, size=(H, H), mode="bilinear", align_corners=False)
    ce_ref = UnbiasedCrossEntropy(old_cl=K, ignore_index=255, reduction="none")(up(ref_in), labels.clone()).mean()
    kd_ref = UnbiasedKnowledgeDistillationLoss(alpha=1.0)(up(ref_in), up(sem_t))
    (ce_ref + 10.0 * kd_ref).backward()
    assert ce.item() == pytest.approx(ce_ref.item(), rel=1e-4)
    assert kd.item() == pytest.approx(kd_ref.item(), rel=1e-4)
    assert ((g - ref_in.grad).norm() / ref_in.grad.norm()).item() < 1e-4
    assert (g.sum(dim=1).abs().max() / g.abs().max()).item() < 1e-4


def test_packed_form_gradient_is_bit_reproducible():
    """Round 5: up to four 64 x 64 pixel tiles add into one low-resolution cell of the logit gradient.  With fp32 atomics the order of
    those additions - and with it the last bit of a few gradient values - changed from run to run (one bf16 rounding of the logit
    gradient flipped in about one training run in eight: two discrete trajectories).  The packed form adds 32-bit
    fixed-point words (csrc/seglogit_loss.hip): the same inputs give the same bits, whatever else the chip is doing."""
    from ucd_amd import synth
    from ucd_amd.loss import fused_seg_losses
    dev = torch.device("cuda:0")
    B, H, h, Ctot, K = 24, 513, 33, 21, 16
    g = torch.Generator(dev).manual_seed(5)
    sem0 = torch.randn(B, Ctot, h, h, device=dev, generator=g).contiguous(memory_format=torch.channels_last)
    sem_old = torch.randn(B, K, h, h, device=dev, generator=g).contiguous(memory_format=torch.channels_last)
    labels = synth.seg_labels(7, B, H, H, range(K, Ctot)).to(dev)
    junk = torch.empty(1 << 26, device=dev)

    def once():
        sem = sem0.clone().requires_grad_(True)
        total, ce, kd = fused_seg_losses(sem, sem_old, labels, K, 1.0, 10.0)
        total.backward()
        return total.item(), sem.grad.clone()

    l0, g0 = once()
    for i in range(40):
        if i % 2:
            junk.normal_()
            (junk[: 1 << (14 + i % 12)] * 2).sum()          # other kernels of varying length in front
        l1, g1 = once()
        assert l1 == l0 and torch.equal(g0, g1), i



# ---- every form of the kernel against a float64 reference --------------------------------------------------------------------
# The cases below name the kernel form they are written for; before anything is launched the host-side plan
# (ucd_seg_losses_plan, checked on the CPU by test_seglosses_cpu.py) is asked which form the call will get, so a later change
# of the dispatch cannot silently move a case onto another kernel.
import dataclasses
import os
import subprocess
import sys
import zlib

PK16, PK20, PK12, REG16, REG24, WIDE_FX, WIDE_F32 = 1, 2, 3, 4, 5, 6, 7
FORM_NAMES = {PK16: "pk<16,8>", PK20: "pk<20,4>", PK12: "pk<12,12>", REG16: "reg<24,16>", REG24: "reg<24,24>",
              WIDE_FX: "wide/fixed", WIDE_F32: "wide/f32"}
# class split -> (Ctot, K, form of an aligned default launch)
SPLITS = {"pk16": (21, 16, PK16), "pk20": (21, 20, PK20), "pk12": (21, 11, PK12), "reg24": (24, 18, REG24),
          "wide": (41, 27, WIDE_FX), "ade": (151, 101, WIDE_FX)}
FEW = ("pk16", "pk20", "pk12", "reg24")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    split: str
    geo: tuple                   # B, H, W, h, w
    labels: str = "mixed"        # mixed | all_ignored | one_new | no_ignored
    regime: str = "n2"           # n2 | n12 | trained | pm80 | headroom
    ce_w: float = 1.0
    kd_w: float = 10.0
    teacher: bool = True
    ignore: int = 255
    pad: tuple = (0, 0, 0)       # columns added to ld_s, ld_t, ld_d (C ABI)
    unaligned: bool = False      # d_sem 4 bytes off the 16-byte grid (C ABI)
    fallback: bool = False       # a geometry whose packed form passes the LDS budget: the register form serves it

    @property
    def id(self):
        return f"{self.name}-{self.split}"


def _expected_form(case, pk0=False):
    Ctot, K, form = SPLITS[case.split]
    if form in (PK16, PK20, PK12) and (pk0 or case.unaligned or case.fallback):
        return REG16 if K <= 16 else REG24
    if form == WIDE_FX and case.unaligned:
        return WIDE_F32
    return form


GEOMETRIES = {
    "nonsquare": (1, 190, 321, 12, 21),      # 15.83 x 15.29, ragged tiles
    "f64x8": (2, 128, 72, 2, 9),             # factor exactly 64 and exactly 8
    "f16": (2, 96, 160, 6, 10),              # exactly 16, H not a multiple of the tile
    "subtile": (2, 24, 40, 3, 5),            # smaller than one tile in both axes (H < 32, W < 64)
    "h1": (1, 64, 100, 1, 20),               # one source row at factor 64, factor 5 across
    "w1": (2, 48, 64, 3, 1),                 # one source column at factor 64
    "r513": (1, 513, 129, 33, 9),            # 513 / 33 and 129 / 9
}
SMALL = (2, 129, 129, 9, 9)


def _cases():
    out = []
    for split in SPLITS:
        if split == "ade":
            out.append(Case("bench", "ade", (2, 512, 512, 32, 32)))
            out.append(Case("bench_unaligned", "ade", (1, 512, 512, 32, 32), unaligned=True))
            continue
        out.append(Case("bench", split, (3, 513, 513, 33, 33)))
        for g, geo in GEOMETRIES.items():
            out.append(Case("geo_" + g, split, geo))
        out.append(Case("all_ignored", split, SMALL, labels="all_ignored"))
        out.append(Case("one_new", split, SMALL, labels="one_new"))
        out.append(Case("ignore250", split, SMALL, ignore=250))
        out.append(Case("no_ignored", split, SMALL, labels="no_ignored"))
        out.append(Case("no_teacher", split, SMALL, teacher=False, kd_w=0.0))
        for regime in ("n12", "trained", "pm80"):
            out.append(Case(regime, split, SMALL, regime=regime))
        out.append(Case("ce0", split, SMALL, ce_w=0.0))
        out.append(Case("kd0", split, SMALL, kd_w=0.0))
        out.append(Case("both0", split, SMALL, ce_w=0.0, kd_w=0.0))
        out.append(Case("ld_padded", split, (2, 190, 129, 12, 9), pad=(3, 5, 7)))
        out.append(Case("unaligned", split, (2, 190, 129, 12, 9), unaligned=True, pad=(0, 0, 3)))
        out.append(Case("unaligned_bench", split, (1, 513, 513, 33, 33), unaligned=True))
        out.append(Case("headroom", split, (1, 128, 128, 2, 2), labels="one_new", regime="headroom", teacher=False, kd_w=0.0))
        if SPLITS[split][2] in (PK16, PK20, PK12):
            # --output_stride 8: 10 x 10 cells under a tile, the packed forms do not fit and the register form takes over
            out.append(Case("stride8", split, (1, 192, 192, 24, 24), fallback=True))
    return out


CASES = _cases()


def _blocks(seed, B, H, W, lo, hi, stream, block=8):
    g = synth.randint(seed, (B, -(-H // block), -(-W // block)), lo, hi, stream=stream)
    return np.repeat(np.repeat(g, block, axis=1), block, axis=2)[:, :H, :W]


def _inputs(case):
    """(sem [B, Ctot, h, w] fp32, teacher [B, K, h, w] fp32 or None, labels [B, H, W] int64), deterministic in the case."""
    Ctot, K, _ = SPLITS[case.split]
    B, H, W, h, w = case.geo
    seed = zlib.crc32(case.id.encode()) % 100000
    # label maps in 8 x 8 pixel blocks: background, OLD-class ids 1 .. K-1 (the reference scores them as background), new classes, ignored
    kind = _blocks(seed, B, H, W, 0, 10, 3)
    old = _blocks(seed, B, H, W, 1, max(K, 2), 4) if K > 1 else np.zeros((B, H, W), dtype=np.int64)
    new = _blocks(seed, B, H, W, K, Ctot, 5)
    cell_cls = None
    if case.regime == "trained":                     # labels follow the low-resolution cells, whose class the logits favour
        yy = np.minimum((np.arange(H) * h) // H, h - 1)
        xx = np.minimum((np.arange(W) * w) // W, w - 1)
        pick = lambda a: a[:, yy][:, :, xx]
        ck, co, cn = (synth.randint(seed, (B, h, w), lo, hi, stream=s) for lo, hi, s in ((0, 10, 3), (1, max(K, 2), 4), (K, Ctot, 5)))
        if K == 1:
            co = np.zeros_like(co)
        cell_cls = np.where(ck < 3, 0, np.where(ck < 5, co, cn))
        kind, old, new = pick(ck), pick(co), pick(cn)
    lab = np.where(kind < 3, 0, np.where(kind < 5, old, new))
    if case.labels in ("mixed",):
        lab = np.where(kind == 9, case.ignore, lab)
    elif case.labels == "all_ignored":
        lab = np.full((B, H, W), case.ignore, dtype=np.int64)
    elif case.labels == "one_new":
        lab = np.full((B, H, W), K, dtype=np.int64)
    labels = torch.from_numpy(lab.astype(np.int64))
    scale = 12.0 if case.regime == "n12" else 2.0
    sem = synth.t_normal(seed, (B, Ctot, h, w), stream=1, scale=scale)
    sem_t = synth.t_normal(seed, (B, K, h, w), stream=2, scale=scale)
    if case.regime == "trained":                     # the labelled class leads by about 15 (N(0, 1) around it)
        sem, sem_t = sem / 2.0, sem_t / 2.0
        cc = torch.from_numpy(cell_cls)
        sem.scatter_add_(1, cc.unsqueeze(1), torch.full((B, 1, h, w), 15.0))
        sem_t.scatter_add_(1, torch.where(cc < K, cc, torch.zeros_like(cc)).unsqueeze(1), torch.full((B, 1, h, w), 15.0))
    elif case.regime == "pm80":                      # one class at +80, all others at -80, student and teacher
        top = torch.from_numpy(synth.randint(seed, (B, 1, h, w), 0, Ctot, stream=6))
        sem = torch.full((B, Ctot, h, w), -80.0).scatter_(1, top, 80.0)
        sem_t = torch.full((B, K, h, w), -80.0).scatter_(1, top % K, 80.0)
    elif case.regime == "headroom":                  # ~ all mass on a class that is not the label: every pixel adds ~ +gmax / -gmax
        sem = sem * 0.0
        sem[:, K + 1 if K + 1 < Ctot else 0] = 40.0
    return sem, (sem_t if case.teacher else None), labels


def _plan(case, lib):
    import ctypes as C
    Ctot, K, _ = SPLITS[case.split]
    B, H, W, h, w = case.geo
    f = C.c_int()
    rc = lib.ucd_seg_losses_plan(H, W, h, w, Ctot, K, int(case.teacher), int(not case.unaligned), -1, C.byref(f), None, None, None)
    assert rc == 0, lib.ucd_last_error().decode()
    return f.value


def _launch(case, inputs, pk0=False):
    """(ce, kd, gradient [B, Ctot, h, w]) as float64 numpy, from the kernel form the case is named for."""
    from ucd_amd import hip
    from ucd_amd.loss import fused_seg_losses
    lib = hip.load()
    dev = torch.device("cuda:0")
    Ctot, K, _ = SPLITS[case.split]
    B, H, W, h, w = case.geo
    sem, sem_t, labels = inputs
    want = _expected_form(case, pk0)
    got = _plan(case, lib)
    assert got == want, f"{case.id}: planned {FORM_NAMES[got]}, the case is written for {FORM_NAMES[want]}"
    if case.pad == (0, 0, 0) and not case.unaligned:
        s = sem.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        total, ce, kd = fused_seg_losses(s, None if sem_t is None else sem_t.to(dev), labels.to(dev), K, case.ce_w, case.kd_w,
                                         ignore_index=case.ignore)
        total.backward()
        return ce.item(), kd.item(), s.grad.double().cpu().numpy()
    rows = B * h * w
    ld_s, ld_t, ld_d = Ctot + case.pad[0], K + case.pad[1], Ctot + case.pad[2]
    nan = float("nan")
    s_buf = torch.full((rows, ld_s), nan, device=dev)
    s_buf[:, :Ctot] = sem.permute(0, 2, 3, 1).reshape(rows, Ctot).to(dev)
    t_buf = None
    if sem_t is not None:
        t_buf = torch.full((rows, ld_t), nan, device=dev)
        t_buf[:, :K] = sem_t.permute(0, 2, 3, 1).reshape(rows, K).to(dev)
    off = 1 if case.unaligned else 0
    store = torch.full((rows * ld_d + 8,), nan, device=dev)
    d = store[off:off + rows * ld_d].view(rows, ld_d)
    assert d.data_ptr() % 16 == 4 * off
    out = torch.full((2,), nan, device=dev)
    nbytes = lib.ucd_seg_losses_workspace_bytes(B, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lab = labels.to(dev)
    hip._check(lib.ucd_seg_losses(hip.ptr(s_buf), ld_s, hip.ptr(t_buf), ld_t, hip.ptr(lab), B, H, W, h, w, Ctot, K, case.ignore,
                                  case.ce_w, case.kd_w, hip.ptr(out), hip.ptr(d), ld_d, hip.ptr(ws), nbytes, hip.stream()),
               "ucd_seg_losses")
    torch.cuda.synchronize()
    # the columns past the classes are the zeros of the entry point's memset; nothing outside the block was written
    assert bool((d[:, Ctot:] == 0).all())
    assert bool(torch.isnan(store[:off]).all()) and bool(torch.isnan(store[off + rows * ld_d:]).all())
    g = d[:, :Ctot].reshape(B, h, w, Ctot).permute(0, 3, 1, 2)
    return out[0].item(), out[1].item(), g.double().cpu().numpy()


_REF = {}


def _references(case, inputs):
    """float64 on the CPU (the reference of the comparison) and the un-fused fp32 torch composition on the GPU (the yardstick of
    what an fp32 evaluation of the same sums can reach): (ce, kd, gradient) each."""
    if case.id in _REF:
        return _REF[case.id]
    from ucd_amd.loss import UnbiasedCrossEntropy, UnbiasedKnowledgeDistillationLoss
    Ctot, K, _ = SPLITS[case.split]
    B, H, W, h, w = case.geo
    sem, sem_t, labels = inputs
    up = lambda t: F.interpolate(t, size=(H, W), mode="bilinear", align_corners=False)
    s64 = sem.double().requires_grad_(True)
    u = up(s64)
    ce64 = OL.unbiased_cross_entropy(u, labels, K, ignore_index=case.ignore).mean()
    kd64 = OL.unbiased_kd(u, up(sem_t.double())) if sem_t is not None else torch.zeros((), dtype=torch.float64)
    (case.ce_w * ce64 + case.kd_w * kd64).backward()
    dev = torch.device("cuda:0")
    s32 = sem.to(dev).requires_grad_(True)
    u = up(s32)
    ce32 = UnbiasedCrossEntropy(old_cl=K, ignore_index=case.ignore, reduction="none")(u, labels.to(dev)).mean()
    kd32 = UnbiasedKnowledgeDistillationLoss(alpha=1.0)(u, up(sem_t.to(dev))) if sem_t is not None else torch.zeros((), device=dev)
    (case.ce_w * ce32 + case.kd_w * kd32).backward()
    _REF[case.id] = ((ce64.item(), kd64.item(), s64.grad.numpy()), (ce32.item(), kd32.item(), s32.grad.double().cpu().numpy()))
    return _REF[case.id]


def _fixed_point_allowance(case, form):
    """A of the gradient bound.  The packed and the many-class form add a tile's contribution to a low-resolution cell as a
    32-bit fixed-point word of quantum q = gmax / 2^17, gmax = (|ce_weight| + 2 |kd_weight| / K) / (B H W) (the launcher's
    fx_gmax: the largest gradient of one pixel).  A tile sums in fp64 and rounds once to the nearest word: at most q / 2 per
    add, one add per tile and cell.  A cell's bilinear support spans 2 f pixels per axis, which at most ceil(2 f / tile) + 1
    tiles cover: A = (q / 2) (ceil(2 f_y / tile_y) + 1) (ceil(2 f_x / 64) + 1).  The fp32-atomic forms have no quantum: A = 0."""
    if form in (REG16, REG24, WIDE_F32):
        return 0.0
    Ctot, K, _ = SPLITS[case.split]
    B, H, W, h, w = case.geo
    gmax = (abs(case.ce_w) + 2.0 * abs(case.kd_w) / K) / (B * H * W)
    tile_y = 32 if form == WIDE_FX else 64
    n_tiles = (int(np.ceil(2.0 * H / h / tile_y)) + 1) * (int(np.ceil(2.0 * W / w / 64)) + 1)
    return gmax / 2.0 ** 17 / 2.0 * n_tiles


REPORT = os.environ.get("UCD_SEGLOSS_REPORT")      # a file that collects one line of measured errors per case


def _check(case, form, got, ref64, ref32):
    """Losses: |L - L64| <= max(4 |L32 - L64|, 1e-6 |L64|).  Gradient, element-wise: |g - g64| <= A + R with A derived
    (_fixed_point_allowance) and R = 4 max |g32 - g64| over the case.  4: the kernel and the torch composition are both fp32
    evaluations of the same sums in different orders; a wrong term shows up at 1e-2 of the values or more."""
    (ce, kd, g), (ce64, kd64, g64), (ce32, kd32, g32) = got, ref64, ref32
    A = _fixed_point_allowance(case, form)
    R = 4.0 * float(np.abs(g32 - g64).max())
    err = float(np.abs(g - g64).max())
    gmax = (abs(case.ce_w) + 2.0 * abs(case.kd_w) / SPLITS[case.split][1]) / np.prod(case.geo[:3])
    line = (f"{case.id} | {FORM_NAMES[form]} | ce {ce64:.6e} comp32 {abs(ce32 - ce64):.2e} kernel {abs(ce - ce64):.2e} | "
            f"kd {kd64:.6e} comp32 {abs(kd32 - kd64):.2e} kernel {abs(kd - kd64):.2e} | "
            f"grad max {np.abs(g64).max():.3e} gmax {gmax:.3e} comp32 {R / 4:.2e} kernel {err:.2e} A {A:.2e} "
            f"median|g64| {np.median(np.abs(g64)):.2e}")
    print(line)
    if REPORT:
        with open(REPORT, "a") as fh:
            fh.write(line + "\n")
    assert np.isfinite(ce) and np.isfinite(kd) and np.isfinite(g).all()
    assert abs(ce - ce64) <= max(4.0 * abs(ce32 - ce64), 1e-6 * abs(ce64)), ("ce", ce, ce64, ce32)
    if case.teacher:
        assert abs(kd - kd64) <= max(4.0 * abs(kd32 - kd64), 1e-6 * abs(kd64)), ("kd", kd, kd64, kd32)
    if case.ce_w == 0.0 and case.kd_w == 0.0:
        assert not g.any()                         # fx_scale = 1 branch: exactly zero
    assert err <= A + R, (err, A, R)
    if case.labels == "all_ignored":
        assert ce == 0.0


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_every_form_vs_float64(case):
    """One case of the geometry / label / logit-range / weight / leading-dimension lists of this file on the kernel form it
    names, against float64 (F.interpolate of float64 logits + the oracle's losses + autograd).  Bounds: _check.

    Regime "pm80" (one class at +80, the others at -80) is the case that found a bug: every form took the log-sum-exps of
    the class SUBSETS (old classes; background + new classes) from exponentials relative to the maximum over ALL classes, so
    a subset more than ~87 below that maximum summed to 0 in fp32 - CE = inf, KD and gradient NaN in all seven paths (float64
    CE 44.18, torch fp32 off by 2.9e-6).  The kernels now take such a pixel's subset sums around the subset's own maximum
    (kSubsetTiny in csrc/seg_loss_common.h)."""
    inputs = _inputs(case)
    form = _expected_form(case)
    got = _launch(case, inputs)
    _check(case, form, got, *_references(case, inputs))


def test_every_form_is_reached():
    """Each of the seven paths behind ucd_seg_losses is the planned form of at least one parity case."""
    assert {_expected_form(c) for c in CASES} == set(FORM_NAMES)


def test_unaligned_d_sem_agrees_with_aligned():
    """The same inputs through the fixed-point form and - d_sem moved by 4 bytes - the fp32-atomic form: both inside their
    bound of float64 (the parity cases), and within the sum of the two bounds of each other."""
    for split in ("pk16", "wide"):
        a = Case("pair", split, (2, 190, 129, 12, 9))
        u = dataclasses.replace(a, unaligned=True)
        inputs = _inputs(a)
        ga, gu = _launch(a, inputs)[2], _launch(u, inputs)[2]
        ref64, ref32 = _references(a, inputs)
        R = 4.0 * float(np.abs(ref32[2] - ref64[2]).max())
        assert np.abs(ga - gu).max() <= _fixed_point_allowance(a, _expected_form(a)) + 2 * R


FEW_CASES = [c for c in CASES if c.split in FEW]


def _child_main(path):
    """UCD_SEG_PK=0 process: every few-class case on the register form; results to an .npz."""
    assert os.environ.get("UCD_SEG_PK") == "0"
    res = {}
    for case in FEW_CASES:
        ce, kd, g = _launch(case, _inputs(case), pk0=True)
        res[case.id + "::loss"] = np.array([ce, kd])
        res[case.id + "::grad"] = g
    np.savez(path, **res)


def test_switch_pk0_register_form_vs_float64(tmp_path):
    """UCD_SEG_PK=0 (read once per process: a fresh child, one for all cases) puts every few-class case on the register
    form; the same float64 reference and bounds, A = 0."""
    path = str(tmp_path / "pk0.npz")
    env = dict(os.environ, UCD_SEG_PK="0", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", f"import test_seglosses_gpu as t; t._child_main({path!r})"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = np.load(path)
    failed = []
    for case in FEW_CASES:
        form = _expected_form(case, pk0=True)
        assert form in (REG16, REG24)
        ce, kd = res[case.id + "::loss"]
        inputs = _inputs(case)
        try:
            _check(dataclasses.replace(case, name="pk0_" + case.name), form, (float(ce), float(kd), res[case.id + "::grad"]),
                   *_references(case, inputs))
        except AssertionError as e:
            failed.append((case.id, str(e).splitlines()[0] if str(e) else "not finite"))
    assert not failed, failed


def test_argument_rejection_launches_nothing():
    """Every documented argument error of ucd_seg_losses: its code, a message that names the cause, and loss_out / d_sem -
    pre-filled with a sentinel - untouched (no memset, no kernel)."""
    from ucd_amd import hip
    lib = hip.load()
    dev = torch.device("cuda:0")
    B, H, W, h, w, Ctot, K = 1, 64, 64, 4, 4, 21, 16
    s = torch.zeros(B * h * w, Ctot, device=dev)
    t = torch.zeros(B * h * w, K, device=dev)
    lab = torch.zeros(B, H, W, dtype=torch.int64, device=dev)
    out = torch.full((2,), 777.0, device=dev)
    d = torch.full((B * h * w, Ctot), 777.0, device=dev)
    need = lib.ucd_seg_losses_workspace_bytes(B, 65 * h, W)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -3, -4

    def call(**kw):
        a = dict(sem_s=hip.ptr(s), ld_s=Ctot, sem_t=hip.ptr(t), ld_t=K, labels=hip.ptr(lab), B=B, H=H, W=W, h=h, w=w, Ctot=Ctot, K=K,
                 ignore=255, ce=1.0, kd=10.0, out=hip.ptr(out), d=hip.ptr(d), ld_d=Ctot, ws=hip.ptr(ws),
                 nbytes=lib.ucd_seg_losses_workspace_bytes(B, H, W))
        a.update(kw)
        rc = lib.ucd_seg_losses(a["sem_s"], a["ld_s"], a["sem_t"], a["ld_t"], a["labels"], a["B"], a["H"], a["W"], a["h"], a["w"],
                                a["Ctot"], a["K"], a["ignore"], a["ce"], a["kd"], a["out"], a["d"], a["ld_d"], a["ws"], a["nbytes"],
                                hip.stream())
        return rc, lib.ucd_last_error().decode()

    bad = [
        (dict(sem_s=None), EINVAL, "NULL"), (dict(labels=None), EINVAL, "NULL"), (dict(out=None), EINVAL, "NULL"),
        (dict(d=None), EINVAL, "NULL"), (dict(ws=None), EINVAL, "NULL"),
        (dict(K=0), EINVAL, "bad sizes"), (dict(K=Ctot + 1), EINVAL, "bad sizes"), (dict(B=0), EINVAL, "bad sizes"),
        (dict(ld_s=Ctot - 1), EINVAL, "leading dimension"), (dict(ld_d=Ctot - 1), EINVAL, "leading dimension"),
        (dict(ld_t=K - 1), EINVAL, "leading dimension"),
        (dict(nbytes=lib.ucd_seg_losses_workspace_bytes(B, H, W) - 1), EWORKSPACE, "workspace too small"),
        (dict(H=65 * h, nbytes=need), EUNSUPPORTED, "above 64"),
        (dict(H=3 * h), EUNSUPPORTED, "below 4"),
        (dict(H=2), EINVAL, "bad scale"),
        (dict(H=128, W=128, h=32, w=32, nbytes=need), EUNSUPPORTED, "factors 4 x 4"),       # 19 x 19 cells of 21 classes: no form fits
        (dict(Ctot=2000, ld_s=2000, ld_d=2000), EUNSUPPORTED, "bytes of LDS for 2000 classes"),
    ]
    for kw, code, text in bad:
        rc, msg = call(**kw)
        assert rc == code and text in msg and "ucd_seg_losses" in msg, (kw, rc, msg)
    rc, msg = call(H=128, W=128, h=32, w=32, nbytes=need)
    assert "bytes of LDS" in msg and "21 classes" in msg
    torch.cuda.synchronize()
    assert bool((out == 777.0).all()) and bool((d == 777.0).all())
    rc, _ = call()                                  # and the same arguments unharmed are served
    torch.cuda.synchronize()
    assert rc == 0 and bool((out != 777.0).all()) and bool((d != 777.0).all())


ARGMAX_SEEDS = {g: 40 + i for i, g in enumerate(GEOMETRIES)}


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_confusion_kernel_over_the_geometry_list(geo):
    """ucd_seg_confusion on the geometries of the loss cases: the histogram is exact for the predictions the kernel made; a
    prediction may differ from the float64 arg-max only where the float64 top-two margin is below 1e-5, at no more than 1e-4 of
    the pixels.  The cap is a condition on the inputs, not a measurement: the fp32 CPU arg-max of the same seed is checked
    against the float64 one first."""
    from oracle.metrics import StreamSegMetrics as OracleMetrics
    from ucd_amd import hip
    B, H, W, h, w = GEOMETRIES[geo]
    B, Ctot = max(B, 2), 21
    sem = synth.t_normal(ARGMAX_SEEDS[geo], (B, Ctot, h, w), stream=1, scale=2.0)
    labels = torch.from_numpy(synth.randint(ARGMAX_SEEDS[geo], (B, H, W), 0, Ctot + 3, stream=2))
    labels[labels >= Ctot] = 255
    up64 = F.interpolate(sem.double(), size=(H, W), mode="bilinear", align_corners=False)
    pred64 = up64.max(dim=1)[1]
    top2 = up64.topk(2, dim=1)[0]
    margin = top2[:, 0] - top2[:, 1]
    cap = 1e-4 * B * H * W
    pred32 = F.interpolate(sem, size=(H, W), mode="bilinear", align_corners=False).max(dim=1)[1]
    d32 = pred32 != pred64
    assert int(d32.sum()) <= cap and (not d32.any() or float(margin[d32].max()) < 1e-5), "pick another seed"
    dev = torch.device("cuda:0")
    s = sem.to(dev).permute(0, 2, 3, 1).reshape(B * h * w, Ctot).contiguous()
    hist = torch.zeros(Ctot, Ctot, dtype=torch.int64, device=dev)
    pred = torch.full((B, H, W), -1, dtype=torch.int64, device=dev)
    hip._check(hip.load().ucd_seg_confusion(hip.ptr(s), Ctot, hip.ptr(labels.to(dev)), B, H, W, h, w, Ctot, Ctot, hip.ptr(hist),
                                            hip.ptr(pred), hip.stream()), "ucd_seg_confusion")
    pred = pred.cpu()
    diff = pred != pred64
    print(geo, "pixels off the float64 arg-max:", int(diff.sum()), "of", B * H * W)
    assert int(diff.sum()) <= cap
    assert not diff.any() or float(margin[diff].max()) < 1e-5
    om = OracleMetrics(Ctot)
    om.update(labels.numpy(), pred.numpy())
    assert np.array_equal(hist.cpu().numpy(), om.confusion_matrix)
