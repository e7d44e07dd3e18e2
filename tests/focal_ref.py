"""The float64 definition of the focal cross entropy the fused logit-loss kernels compute (include/ucd_hip.h), written out on the
up-sampled logits: nothing here is imported from the package's loss code.

    ce_p  = the pixel's cross entropy: log-sum-exp over all classes minus the label's logit, or - for a label below old_cl, which
            counts as background - minus the log-sum-exp over the classes [0, old_cl); 0 for an ignored pixel
    u     = clamp(1 - exp(-ce_p), 0, 1)
    F_p   = alpha u^gamma ce_p          (0 where u is 0 and gamma > 0; alpha ce_p for gamma == 0)
    loss  = 1 / (B H W) sum_b w_b sum_p F_p
"""
import torch
import torch.nn.functional as F


def ce_map(up, labels, old_cl=1, ignore_index=255):
    """[B, H, W] float64 cross entropy of up-sampled logits ``up`` [B, C, H, W]; labels >= C match no class (their logit counts 0)."""
    C = up.shape[1]
    den = torch.logsumexp(up, dim=1)
    ignore = labels == ignore_index
    lab = torch.where(ignore | (labels < old_cl), torch.zeros_like(labels), labels)
    picked = up.gather(1, lab.clamp(max=C - 1).unsqueeze(1)).squeeze(1)
    picked = torch.where(lab >= C, torch.zeros_like(picked), picked)
    if old_cl > 1:
        picked = torch.where(lab == 0, torch.logsumexp(up[:, :old_cl], dim=1), picked)
    return torch.where(ignore, torch.zeros_like(den), den - picked)


def modulate(ce, gamma, alpha):
    """F_p of the definition, with its zero rule; differentiable."""
    if gamma == 0:
        return alpha * ce
    u = (1.0 - torch.exp(-ce)).clamp(0.0, 1.0)
    zero = u <= 0
    safe = torch.where(zero, torch.ones_like(u), u)
    return torch.where(zero, torch.zeros_like(ce), alpha * torch.exp(gamma * torch.log(safe)) * ce)


def focal_loss(sem, labels, gamma, alpha, old_cl=1, weight=None, ignore_index=255):
    """(loss, up-sampled ce map) from LOW-resolution logits ``sem`` [B, C, h, w] (float64, may require a gradient): bilinear
    up-sampling to the label size, the definition above, ``weight`` [B] the optional per-image weight."""
    up = F.interpolate(sem, size=labels.shape[-2:], mode="bilinear", align_corners=False)
    ce = ce_map(up, labels, old_cl, ignore_index)
    f = modulate(ce, float(gamma), float(alpha))
    if weight is not None:
        f = f * torch.as_tensor(weight, dtype=f.dtype).view(-1, 1, 1)
    return f.mean(), ce
