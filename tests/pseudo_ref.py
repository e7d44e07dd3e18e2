"""Float64 reference of the pseudo-labelling on the CPU: ``F.interpolate`` in double, then the
definitions - pseudo-class, normalised entropy, candidates, histogram, interpolated median, label rule, adaptive factor - and the
LOOSE mask: the pixels at which an fp32 evaluation may legitimately decide differently."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

MARGIN = 1e-5        # four times the largest fp32-against-float64 difference of u measured for the torch evaluation (2.4e-6)
IGNORE = 255


def teacher_logits(seed, B, K, h, w, rounded, ld_pad=3):
    """Teacher rows [B*h*w, K + ld_pad] fp32 with NaN in the padding columns, and the same logits as [B, K, h, w] float64.
    ``rounded``: multiples of 1/8 (exact in fp32, sums of four bilinear products nearly so)."""
    g = torch.Generator().manual_seed(seed)
    z = 3.0 * torch.randn(B, K, h, w, generator=g, dtype=torch.float64)
    if rounded:
        z = torch.round(8.0 * z) / 8.0
    z = z.float().double()
    rows = torch.full((B * h * w, K + ld_pad), float("nan"), dtype=torch.float32)
    rows[:, :K] = z.permute(0, 2, 3, 1).reshape(B * h * w, K).float()
    return rows, z


def mixed_labels(seed, B, H, W, K, n_new=3):
    """0, old classes, new classes and 255, in blobs of a few pixels plus single-pixel noise."""
    g = torch.Generator().manual_seed(seed + 1000)
    values = torch.tensor([0] * 4 + list(range(1, K)) + list(range(K, K + n_new)) + [IGNORE] * 2)
    coarse = values[torch.randint(0, len(values), (B, (H + 3) // 4, (W + 3) // 4), generator=g)]
    lab = coarse.repeat_interleave(4, dim=1).repeat_interleave(4, dim=2)[:, :H, :W].clone()
    noise = torch.rand(B, H, W, generator=g) < 0.1
    lab[noise] = values[torch.randint(0, len(values), (int(noise.sum()),), generator=g)]
    return lab.contiguous()


def view(z, labels):
    """(candidates, c*, u, top-two gap) [B, H, W] in float64."""
    K = z.shape[1]
    up = F.interpolate(z, size=labels.shape[-2:], mode="bilinear", align_corners=False)
    m, arg = up.max(dim=1)
    d = up - m.unsqueeze(1)
    e = d.exp()
    S = e.sum(dim=1)
    u = (S.log() - (d * e).sum(dim=1) / S) / np.log(K) if K > 1 else torch.zeros_like(m)
    gap = (m - up.topk(2, dim=1).values[:, 1]) if K > 1 else torch.full_like(m, float("inf"))
    cand = (labels >= 0) & (labels < K) & (labels != IGNORE)
    return cand, arg, u, gap


def histogram(cand, arg, u, K, bins):
    b = (u * bins).floor().long().clamp_max(bins - 1)
    return torch.bincount((arg * bins + b)[cand], minlength=K * bins).view(K, bins)


def median(hist, floor):
    """Brute force: expand every bin into its counts spread evenly over the bin, take the interpolated median by walking."""
    hist = np.asarray(hist, dtype=np.float64)
    K, bins = hist.shape
    out = np.full(K, floor)
    for c in range(K):
        n = hist[c].sum()
        if n == 0:
            continue
        half, run = n / 2.0, 0.0
        for j in range(bins):
            if run + hist[c, j] >= half:
                out[c] = max((j + (half - run) / hist[c, j]) / bins, floor)
                break
            run += hist[c, j]
    return out


class Case:
    """Everything the tests compare against for one (K, geometry): computed once, shared, left unchanged."""

    def __init__(self, K, h, w, H, W, bins=100, floor=0.001, f_min=0.0, seed=0, B=2):
        self.K, self.h, self.w, self.H, self.W, self.B, self.bins, self.f_min = K, h, w, H, W, B, bins, f_min
        self.rows, self.z = teacher_logits(seed + 7 * K, B, K, h, w, rounded=(H, W) != (h, w))
        self.labels = mixed_labels(seed + K, B, H, W, K)
        self.cand, self.arg, self.u, gap = view(self.z, self.labels)
        self.hist = histogram(self.cand, self.arg, self.u, K, bins)
        self.thresholds = median(self.hist.numpy(), floor)
        tau = torch.from_numpy(self.thresholds)[self.arg]
        self.passed = self.cand & (self.u < tau)
        self.labels_out = torch.where(self.passed, self.arg, torch.where(self.cand, torch.full_like(self.labels, IGNORE), self.labels))
        self.num, self.den = self.passed.flatten(1).sum(1), self.cand.flatten(1).sum(1)
        # loose pixels: a decision within the margin of flipping
        self.tie = self.cand & (gap < MARGIN)
        self.loose = self.tie | (self.cand & ((self.u - tau).abs() < MARGIN))
        ub = self.u * bins
        self.bin_loose = self.cand & ((ub - ub.round()).abs() < MARGIN * bins)
        self.unc = torch.where(self.cand, self.u, torch.zeros_like(self.u))


@functools.lru_cache(maxsize=None)
def case(K, h, w, H, W, seed=0):
    return Case(K, h, w, H, W, seed=seed)


def hist_allowance(c, bins):
    """Where a histogram from an fp32 evaluation may differ from ``histogram(...)`` of the reference, cell by cell: ``(cells [K, bins],
    rows [K])``.  A candidate can leave its cell only when it is loose, and only to the cells its decision can flip to: the rows of the
    classes within MARGIN of its maximum (a tie moves a pixel between the rows of the tied classes, in the bin it falls in), and,
    when ``u * bins`` is within ``MARGIN * bins`` of an integer, the two bins at that edge.  ``cells[k, j]`` counts the loose
    pixels that can sit in cell (k, j); ``rows[k]`` the tie pixels that can sit in row k.  A pixel that is not loose adds nothing."""
    K = c.K
    up = F.interpolate(c.z, size=c.labels.shape[-2:], mode="bilinear", align_corners=False)
    near = (up.max(dim=1, keepdim=True).values - up) < MARGIN            # [B, K, H, W]: the classes that can win the arg-max
    ub = c.u * bins
    own = ub.floor().long().clamp_max(bins - 1)
    edge = ub.round().long()
    cells = torch.zeros(K, bins, dtype=torch.int64)
    rows = torch.zeros(K, dtype=torch.int64)
    sel = c.cand & (c.tie | c.bin_loose)
    for b, y, x in sel.nonzero().tolist():
        ks = near[b, :, y, x].nonzero().flatten().tolist() if c.tie[b, y, x] else [int(c.arg[b, y, x])]
        js = {int(own[b, y, x])}
        if c.bin_loose[b, y, x]:
            e = int(edge[b, y, x])
            js |= {min(max(e - 1, 0), bins - 1), min(e, bins - 1)}
        for k in ks:
            for j in js:
                cells[k, j] += 1
            if c.tie[b, y, x]:
                rows[k] += 1
    return cells, rows
