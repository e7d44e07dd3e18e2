"""Helpers of the BCE-loss tests (test_seg_bce_cpu.py, test_seg_bce_gpu.py, test_lwfmc_step_gpu.py): a float64 torch restatement
of the three formulas of include/ucd_hip.h (ucd_seg_bce), written here - not imported from oracle/ or the reference - and the
inputs of tests/golden/bce_losses.npz rebuilt from ucd_amd.synth."""
import numpy as np
import torch
import torch.nn.functional as F

from ucd_amd import synth

GOLDEN_SHAPES = [(2, 21, 16, 9, 129), (2, 20, 14, 12, 190), (2, 41, 27, 11, 173)]       # B, Ctot, K, h, H
HARD_W, SOFT_W = 1.0, 10.0


def bce(z, t):
    """max(z, 0) - t z + log1p(exp(-|z|))"""
    return z.clamp(min=0) - t * z + torch.log1p(torch.exp(-z.abs()))


def restatement(sem, sem_t, labels, hard_w=1.0, soft_w=0.0, ignore=255):
    """(L_bce, soft, gradient of hard_w * L_bce + soft_w * soft w.r.t. the low-resolution logits) in float64, each from its formula:
        L_bce = 1/(BHW) sum_p [y_p valid] sum_c bce(z_pc, [c == y_p])
        soft  = 1/(BHW) sum_p sum_{c<K} bce(z_pc, s(zt_pc))
        grad  = 1/(BHW) sum_p w_p(i, j) (hard_w [y_p valid] (s(z_pc) - [c == y_p]) + soft_w [c < K] (s(z_pc) - s(zt_pc)))
    with z = up(sem), zt = up(sem_t); the bilinear weights w_p(i, j) are applied by the transpose of F.interpolate (its autograd)."""
    s = sem.detach().double().clone().requires_grad_(True)
    B, Ctot = s.shape[:2]
    H, W = labels.shape[-2:]
    z = F.interpolate(s, size=(H, W), mode="bilinear", align_corners=False)
    labels = labels.to(s.device)
    valid = (labels != ignore) & (labels >= 0) & (labels < Ctot)
    hot = F.one_hot(torch.where(valid, labels, torch.zeros_like(labels)), Ctot).permute(0, 3, 1, 2).double()
    vm = valid.unsqueeze(1).double()
    n = float(B * H * W)
    zd = z.detach()
    l_bce = (bce(zd, hot) * vm).sum() / n
    g = hard_w * vm * (torch.sigmoid(zd) - hot)
    l_soft = torch.zeros((), dtype=torch.float64, device=s.device)
    if sem_t is not None:
        K = sem_t.shape[1]
        tgt = torch.sigmoid(F.interpolate(sem_t.detach().double(), size=(H, W), mode="bilinear", align_corners=False))
        l_soft = bce(zd[:, :K], tgt).sum() / n
        g[:, :K] += soft_w * (torch.sigmoid(zd[:, :K]) - tgt)
    (grad,) = torch.autograd.grad(z, s, g / n)
    return l_bce.item(), l_soft.item(), grad


def golden_inputs(shape):
    """(student logits, teacher logits, labels) of one golden shape, as tests/golden/make_bce_golden.py builds them: the inputs of
    kd_losses.npz (make_kd_golden.unit_inputs) with 255 in 8 x 8 blocks over about a tenth of the label map."""
    B, Ctot, K, h, H = shape
    seed = 8100 + Ctot + h
    sem = synth.t_normal(seed, (B, Ctot, h, h), stream=1, scale=2.0)
    sem_t = synth.t_normal(seed, (B, K, h, h), stream=2, scale=2.0)
    labels = synth.seg_labels(seed, B, H, H, range(K, Ctot), rects=4)
    old = torch.from_numpy(synth.randint(seed, (B, H, H), 1, K, stream=7))
    pick = torch.from_numpy(synth.randint(seed, (B, H // 8 + 1, H // 8 + 1), 0, 4, stream=8))
    pick = pick.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :H]
    labels = torch.where((pick == 0) & (labels == 0), old, labels)
    ign = torch.from_numpy(synth.randint(seed, (B, H // 8 + 1, H // 8 + 1), 0, 10, stream=9))
    ign = ign.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :H]
    return sem, sem_t, torch.where(ign == 0, torch.full_like(labels, 255), labels)


def golden_grad_errors(gold, prefix, arr):
    """(largest element-wise error, its bound's scale) of ``arr`` against a gradient stored by make_goldens.compact(): whole arrays
    element by element; compact ones on their samples, and - what an element-wise error e implies - row sums within n_row * e."""
    from conftest import sample_idx
    arr = np.asarray(arr, dtype=np.float64)
    if prefix in gold:
        ref = gold[prefix].astype(np.float64)
        return np.abs(arr - ref).max(), np.abs(ref).max()
    assert tuple(gold[prefix + "::shape"]) == arr.shape
    flat = arr.reshape(-1)
    ref = gold[prefix + "::samples"].astype(np.float64)
    err = np.abs(flat[sample_idx(flat.size, 512)] - ref).max()
    rs = gold[prefix + "::rowsum"]
    if rs.size:
        err = max(err, np.abs(arr.reshape(-1, arr.shape[-1]).sum(axis=1) - rs).max() / arr.shape[-1])
    return err, np.abs(ref).max()


def golden_key(shape):
    return "x".join(str(v) for v in shape)


def random_case(seed, B, Ctot, K, h, w, H, W, scale=2.0, ignore_tenths=1):
    """Logits and a label map of every class in 4 x 4 blocks, ``ignore_tenths`` tenths of them 255; deterministic in the seed."""
    sem = synth.t_normal(seed, (B, Ctot, h, w), stream=1, scale=scale)
    sem_t = synth.t_normal(seed, (B, K, h, w), stream=2, scale=scale)
    blocks = lambda lo, hi, s: np.repeat(np.repeat(synth.randint(seed, (B, -(-H // 4), -(-W // 4)), lo, hi, stream=s), 4, 1), 4, 2)[:, :H, :W]
    lab = np.where(blocks(0, 10, 3) < ignore_tenths, 255, blocks(0, Ctot, 4))
    return sem, sem_t, torch.from_numpy(lab.astype(np.int64))
