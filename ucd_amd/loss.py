"""Losses of the ``--method UCD`` step, reference interface (utils/loss.py).

``UnbiasedCrossEntropy`` (utils/loss.py:89-109), ``KnowledgeDistillationLoss`` (:112-136) and
``UnbiasedKnowledgeDistillationLoss`` (:139-184) keep the reference's module interface on full-resolution logits
(the unfused path: the CPU, ``UCD_SEG_KD_EX=0``, tests).  The training step itself calls ``fused_seg_losses``: bilinear
x16 up-sampling + (unbiased or plain) CE + (unbiased or plain) KD at any ``--alpha`` + the gradient w.r.t. the
LOW-resolution logits in one HIP kernel (``ucd_seg_losses_ex``, csrc/seglogit_loss.hip) - the
``[B, Ctot, H, W]`` tensors never exist.  A geometry whose tiles do not fit the LDS of those kernels (ADE at ``--output_stride 8``)
goes to the gather form (``ucd_seg_losses_gather``, csrc/seg_gather.hip; ``seg_losses_route`` says which).
The contrastive loss lives in :mod:`ucd_amd.contrastive`.
"""
from __future__ import annotations

import functools
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import hip
from . import switches as _switches
from .contrastive import PixelConLossV2, pre_contractive_pixel, ucd_contrastive_loss  # noqa: F401


class _LowResLogitLoss(torch.autograd.Function):
    """What the fused logit-loss Functions share.  A library call takes the LOW-resolution logits as ``[B*h*w, C]`` fp32 rows and
    writes two loss means and, where asked, ``d_sem``: the gradient of ``w0 * loss0 + w1 * loss1`` w.r.t. the student rows.  The
    up-sampled [B, Ctot, H, W] tensors never exist.  A subclass keeps its library call and its weights; ``sem``, the first input,
    is the only one with a gradient."""

    @staticmethod
    def operands(ctx, sem, sem_old, labels, K, want_d):
        """(student rows, teacher rows or None, K - with a teacher: its class count -, labels, out[2], d_sem or None,
        (B, H, W, h, w, Ctot)).  ``want_d``: the call writes the gradient rows, kept for ``backward``."""
        B, Ctot, h, w = sem.shape
        H, W = labels.shape[-2:]
        s = sem.detach().permute(0, 2, 3, 1).reshape(B * h * w, Ctot).float().contiguous()
        t = None
        if sem_old is not None:
            K = sem_old.shape[1]
            t = sem_old.detach().permute(0, 2, 3, 1).reshape(B * h * w, K).float().contiguous()
        out = torch.empty(2, dtype=torch.float32, device=sem.device)
        d = torch.empty(B * h * w, Ctot, dtype=torch.float32, device=sem.device) if want_d else None
        if want_d:
            ctx.save_for_backward(d)
        ctx.meta = (B, Ctot, h, w, sem.dtype)
        return s, t, K, labels.contiguous(), out, d, (B, H, W, h, w, Ctot)

    @staticmethod
    def weighted(ctx, out, w0, w1):
        loss0, loss1 = out[0], out[1]
        ctx.mark_non_differentiable(loss0, loss1)
        return w0 * loss0 + w1 * loss1, loss0, loss1

    @staticmethod
    def backward(ctx, g, _g0, _g1):
        (d,) = ctx.saved_tensors
        B, Ctot, h, w, dtype = ctx.meta
        grad = (d * g).view(B, h, w, Ctot).permute(0, 3, 1, 2).to(dtype)
        return (grad,) + (None,) * (len(ctx.needs_input_grad) - 1)


class _FusedSegLosses(_LowResLogitLoss):
    """total = ce_weight * mean(CE) + kd_weight * mean(KD) (ucd_seg_losses_ex, or ucd_seg_losses_gather for ``form="gather"``;
    SURVEY.md section 8-f1).  Every call names its loss pair: the cross entropy pools ``max(old_cl, 1)`` classes.  The pair the
    kernels were first built for (one class count for both losses, unbiased KD, alpha 1) is the launch, and the bits, of
    ucd_seg_losses: the library picks its kernels by these values, not by the entry.  ``sample_weight`` ([B] fp32 on the device, each
    in [0, 1]; None: the calls without one, launch for launch) weighs image b's cross entropy, in the loss and the gradient
    (ucd_seg_losses_ex_w / ucd_seg_losses_gather_w).  ``focal`` ((gamma, alpha); None: the calls without it, launch for launch)
    modulates each pixel's cross entropy (ucd_seg_losses_focal / ucd_seg_losses_gather_focal, which take the weight or NULL)."""

    @staticmethod
    def forward(ctx, sem, sem_old, labels, old_cl, ce_weight, kd_weight, ignore_index, kd_mode, alpha, form, sample_weight=None,
                focal=None):
        lib = hip.load()
        gather = form == "gather"
        # the gather form writes d_sem only where asked (the same loss bits without); the tiled forms always accumulate into it
        s, t, K, labels, out, d, (B, H, W, h, w, Ctot) = _LowResLogitLoss.operands(ctx, sem, sem_old, labels, int(old_cl),
                                                                                   ctx.needs_input_grad[0] or not gather)
        name = "ucd_seg_losses_gather" if gather else "ucd_seg_losses_ex"
        sw = ()
        if focal is not None:
            name = "ucd_seg_losses_gather_focal" if gather else "ucd_seg_losses_focal"
            sw = (hip.ptr(sample_weight), float(focal[0]), float(focal[1]))
        elif sample_weight is not None:
            name += "_w"
            sw = (hip.ptr(sample_weight),)
        nbytes = lib.ucd_seg_losses_gather_workspace_bytes(B, h, w) if gather else lib.ucd_seg_losses_workspace_bytes(B, H, W)
        ws = hip.workspace(nbytes, sem.device, "seglosses_gather" if gather else "seglosses")
        # one wave per cell reads its rows once; a tiled form also adds into them
        with hip._timed("ucd_seg_losses_gather" if gather else "ucd_seg_losses",
                        B * H * W * 8 + (1 if gather else 2) * B * h * w * (2 * Ctot + K) * 4):
            hip._check(getattr(lib, name)(hip.ptr(s), Ctot, hip.ptr(t), K, hip.ptr(labels), B, H, W, h, w, Ctot, max(K, 1),
                                          max(int(old_cl), 1), int(kd_mode), float(alpha), int(ignore_index), float(ce_weight),
                                          float(kd_weight), *sw, hip.ptr(out), hip.ptr(d), Ctot, hip.ptr(ws), nbytes, hip.stream()), name)
        return _LowResLogitLoss.weighted(ctx, out, ce_weight, kd_weight)


class _FusedSegBCE(_LowResLogitLoss):
    """total = hard_weight * BCE + soft_weight * soft (ucd_seg_bce, csrc/seg_gather.hip): BCE is the reference's
    ``BCEWithLogitsLossWithIgnoreIndex(reduction='none')(up(sem), labels).mean()``, soft its combined iCaRL term
    ``K * BCEWithLogitsLoss()(up(sem)[:, :K], sigmoid(up(sem_old)))``.  Without a gradient to form, the kernel gets no ``d_sem``."""

    @staticmethod
    def forward(ctx, sem, sem_old, labels, hard_weight, soft_weight, ignore_index):
        lib = hip.load()
        s, t, K, labels, out, d, (B, H, W, h, w, Ctot) = _LowResLogitLoss.operands(ctx, sem, sem_old, labels, 1, ctx.needs_input_grad[0])
        nbytes = lib.ucd_seg_bce_workspace_bytes(B, h, w)
        ws = hip.workspace(nbytes, sem.device, "seg_bce")
        with hip._timed("ucd_seg_bce", B * H * W * 8 + B * h * w * (2 * Ctot + K) * 4):
            hip._check(lib.ucd_seg_bce(hip.ptr(s), Ctot, hip.ptr(t), K, hip.ptr(labels), B, H, W, h, w, Ctot, K, int(ignore_index),
                                       float(hard_weight), float(soft_weight), hip.ptr(out), hip.ptr(d), Ctot, hip.ptr(ws), nbytes,
                                       hip.stream()), "ucd_seg_bce")
        return _LowResLogitLoss.weighted(ctx, out, hard_weight, soft_weight)


def fused_seg_bce(sem, sem_old, labels, hard_weight=1.0, soft_weight=0.0, ignore_index=255):
    """Returns (hard_weight*BCE + soft_weight*soft [differentiable w.r.t. ``sem``], BCE, soft) from the LOW-resolution logits:
    BCE is the reference's ``BCEWithLogitsLossWithIgnoreIndex(reduction='none')(up(sem), labels).mean()`` (utils/loss.py:31-54,
    train.py:112/116) and soft, with a teacher of K classes, ``K * nn.BCEWithLogitsLoss()(up(sem)[:, :K], sigmoid(up(sem_old)))``
    (the combined iCaRL term of train.py:119-124 before ``icarl_importance``; 0 without ``sem_old``); ``up`` = bilinear to the label
    size.  A label outside ``[0, Ctot)`` counts as ignored.  Under ``torch.no_grad()`` or with a ``sem`` that requires no gradient
    only the losses are computed."""
    if not sem.is_cuda:
        raise RuntimeError("ucd_amd.loss.fused_seg_bce runs on the GPU only (there is no CPU fallback)")
    if sem_old is not None and (sem_old.shape[0] != sem.shape[0] or sem_old.shape[2:] != sem.shape[2:] or sem_old.shape[1] > sem.shape[1]):
        raise ValueError(f"student and teacher logits do not match: {tuple(sem.shape)} vs {tuple(sem_old.shape)}")
    return _FusedSegBCE.apply(sem, sem_old, labels, hard_weight, soft_weight, ignore_index)


class _FusedAttnMSE(torch.autograd.Function):
    """weight * MSE(att(x_s), att(x_t)) from the raw maps (ucd_attn_mse, csrc/featdist.hip); the attention factor of the
    student is detached, as in the reference (segmentation_module.py:93)."""

    @staticmethod
    def forward(ctx, x_s, x_t, weight):
        lib = hip.load()
        xt = x_t.detach()
        if xt.dtype != x_s.dtype:
            xt = xt.to(x_s.dtype)
        xs, M, C, HW, ld_s = hip.rows_view(x_s.detach())
        xt, _, _, _, ld_t = hip.rows_view(xt)
        B = x_s.shape[0]
        d = hip.empty_like_rows(xs)
        out = torch.empty(1, dtype=torch.float32, device=x_s.device)
        nbytes = lib.ucd_attn_mse_workspace_bytes(B, HW)
        ws = hip.workspace(nbytes, x_s.device, "attn_mse")
        with hip._timed("ucd_attn_mse", 5 * M * C * xs.element_size()):
            hip._check(lib.ucd_attn_mse(hip.ptr(xs), ld_s, hip.ptr(xt), ld_t, hip.dtype_code(xs), B, HW, C, float(weight), hip.ptr(out),
                                        hip.ptr(d), C, hip.ptr(ws), nbytes, hip.stream()), "ucd_attn_mse")
        ctx.save_for_backward(d)
        return weight * out[0]

    @staticmethod
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        return (d * g).to(d.dtype), None, None


def fused_attn_mse(x_s_raw, x_t_raw, weight=1.0):
    """``weight * nn.MSELoss()(att_map(x_s_raw), att_map(x_t_raw))`` (the reference's ``loss_de`` term for one pair of maps,
    train.py:129) from the RAW [B, C, h, w] maps in one HIP operation; differentiable w.r.t. ``x_s_raw``."""
    if not x_s_raw.is_cuda:
        raise RuntimeError("ucd_amd.loss.fused_attn_mse runs on the GPU only (there is no CPU fallback)")
    if x_s_raw.shape != x_t_raw.shape:
        raise ValueError(f"student and teacher maps differ in shape: {tuple(x_s_raw.shape)} vs {tuple(x_t_raw.shape)}")
    return _FusedAttnMSE.apply(x_s_raw, x_t_raw, weight)


POD_SCALES = (1, 2, 4)


def _pod_check(x_s, x_t, slope, scales):
    """The argument rules of a Local POD level (the library's, restated for the paths that never reach it)."""
    if x_s.dim() != 4 or x_s.shape != x_t.shape:
        raise ValueError(f"student and teacher maps must be [B, C, h, w] of one shape: {tuple(x_s.shape)} vs {tuple(x_t.shape)}")
    if not 0.0 < float(slope) <= 1.0:
        raise ValueError(f"the slope {slope} is outside (0, 1]")
    scales = tuple(int(s) for s in scales)
    if not 1 <= len(scales) <= 4 or any(not 1 <= s <= 8 for s in scales) or any(b <= a for a, b in zip(scales, scales[1:])):
        raise ValueError(f"scales must be 1 to 4 strictly increasing values in 1 .. 8, got {scales}")
    if min(x_s.shape[2:]) < scales[-1]:
        raise ValueError(f"a {x_s.shape[2]} x {x_s.shape[3]} map is smaller than the largest scale {scales[-1]}")
    return scales


def _pod_embed(x, slope, scales):
    """[B, n_E]: every row pool and column pool of every region of every scale of ``Q = P^2``, ``P`` the map in front of the
    leaky-ReLU of slope ``slope``."""
    x = _wide(x)
    p = torch.where(x >= 0, x, x / slope)
    q = p * p
    B, C, h, w = q.shape
    parts = []
    for s in scales:
        kh, kw = h // s, w // s
        v = q[:, :, :s * kh, :s * kw].reshape(B, C, s, kh, s, kw)
        parts.append(v.mean(dim=5).reshape(B, -1))         # per (channel, region row): the mean over the region's columns
        parts.append(v.mean(dim=3).reshape(B, -1))         # per (channel, region column): the mean over the region's rows
    return torch.cat(parts, dim=1)


def local_pod_torch(x_s, x_t, slope=1.0, scales=POD_SCALES, weight=1.0):
    """``weight`` times the Local POD distance of one level as a differentiable torch composition (PLOP's ``_local_pod`` on
    ``[B, C, h, w]`` maps of any aspect): multi-scale strip pooling of the squared pre-activation maps, L2-normalised per sample,
    ``mean_b |E^_s - E^_t|``.  The teacher is detached.  fp64 maps stay fp64 (the tests), half-precision maps compute in fp32.
    Serves CPU devices, geometries the kernels refuse and ``UCD_FUSED_POD=0``."""
    scales = _pod_check(x_s, x_t, slope, scales)
    e_s = _pod_embed(x_s, slope, scales)
    e_t = _pod_embed(x_t.detach().to(x_s.dtype), slope, scales)
    e_s = e_s / e_s.norm(dim=1, keepdim=True).clamp_min(1e-12)
    e_t = e_t / e_t.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return weight * (e_s - e_t).norm(dim=1).mean()


@functools.lru_cache(maxsize=None)
def _pod_plan(h, w, C, scales, B, dtype):
    return hip.pod_plan(h, w, C, scales, B, dtype)


class _FusedLocalPOD(torch.autograd.Function):
    """weight * Local POD of one level on the HIP kernels (ucd_pod_forward / ucd_pod_backward, csrc/pod.hip).  The forward keeps
    the coefficient strips ``g_E`` ([B, n_E] fp32: 22 % of the bytes of a bf16 map at 129 x 129, 83 % at 33 x 33 - about half of
    the tapped maps' bytes over the five levels of a step); the backward reads the student map once more and writes ``dX`` - no
    second resident copy of the map."""

    @staticmethod
    def forward(ctx, x_s, x_t, slope, scales, weight):
        lib = hip.load()
        xt = x_t.detach()
        if xt.dtype != x_s.dtype:
            xt = xt.to(x_s.dtype)
        xs, M, C, HW, ld_s = hip.rows_view(x_s.detach())
        xt, _, _, _, ld_t = hip.rows_view(xt)
        B, _, h, w = xs.shape
        code = hip.dtype_code(xs)
        plan = _pod_plan(h, w, C, scales, B, code)
        arr, n = hip.pod_scales(scales)
        g = torch.empty(B, plan["n_E"], dtype=torch.float32, device=xs.device)
        out = torch.empty(1, dtype=torch.float32, device=xs.device)
        nbytes = plan["workspace_bytes"]
        ws = hip.workspace(nbytes, xs.device, "pod")
        # one read of each map; the tile partials and the strips are written and read once more
        with hip._timed("ucd_pod_forward", 2 * M * C * xs.element_size()):
            hip._check(lib.ucd_pod_forward(hip.ptr(xs), ld_s, hip.ptr(xt), ld_t, code, B, C, h, w, float(slope),
                                           hip.C.cast(arr, hip.C.c_void_p), n, float(weight), hip.ptr(out), hip.ptr(g), hip.ptr(ws),
                                           nbytes, hip.stream()), "ucd_pod_forward")
        ctx.save_for_backward(xs, g)
        ctx.meta = (ld_s, float(slope), scales)
        return weight * out[0]

    @staticmethod
    def backward(ctx, grad):
        xs, g = ctx.saved_tensors
        ld_s, slope, scales = ctx.meta
        B, C, h, w = xs.shape
        arr, n = hip.pod_scales(scales)
        go = grad.detach().reshape(1).to(torch.float32).contiguous()
        d = hip.empty_like_rows(xs)
        with hip._timed("ucd_pod_backward", 2 * B * h * w * C * xs.element_size()):
            hip._check(hip.load().ucd_pod_backward(hip.ptr(xs), ld_s, hip.dtype_code(xs), B, C, h, w, slope,
                                                   hip.C.cast(arr, hip.C.c_void_p), n, hip.ptr(g), hip.ptr(go), hip.ptr(d), C,
                                                   hip.stream()), "ucd_pod_backward")
        return d, None, None, None, None


def pod_kernels_take(x):
    """Do the Local POD kernels serve this map?  bf16 or fp32 on a GPU, C a multiple of 8 up to 8192, at most 1024 rows and
    columns (ucd_pod_plan states the same bounds)."""
    return (x.is_cuda and x.dtype in (torch.bfloat16, torch.float32) and x.shape[1] % 8 == 0 and x.shape[1] <= 8192
            and max(x.shape[2:]) <= 1024)


def fused_local_pod(x_s, x_t, slope=1.0, scales=POD_SCALES, weight=1.0):
    """``weight * mean_b |E^(x_s)_b - E^(x_t)_b|``: the Local POD distance of one level (PLOP) between a student and a teacher
    map ``[B, C, h, w]`` taken BEHIND a leaky-ReLU of slope ``slope`` (1: take the maps as they are); differentiable w.r.t.
    ``x_s``.  On the GPU it is four HIP launches forward and one backward (csrc/pod.hip); CPU tensors, maps the kernels refuse
    (``pod_kernels_take``) and ``UCD_FUSED_POD=0`` run ``local_pod_torch``."""
    scales = _pod_check(x_s, x_t, slope, scales)
    if not pod_kernels_take(x_s) or _switches.get("UCD_FUSED_POD", "1") == "0":
        return local_pod_torch(x_s, x_t, slope, scales, weight)
    return _FusedLocalPOD.apply(x_s, x_t, float(slope), scales, float(weight))


def _pod_logits_check(sem_s, sem_t, scales, normalize):
    """The argument rules of the Local POD level on the logits; returns (scales, normalize as 0 / 1)."""
    if sem_s.dim() != 4 or sem_t.dim() != 4 or sem_s.shape[0] != sem_t.shape[0] or sem_s.shape[2:] != sem_t.shape[2:] \
            or not 1 <= sem_t.shape[1] <= sem_s.shape[1]:
        raise ValueError(f"student and teacher logits must be [B, Ctot, h, w] and [B, K, h, w] with 1 <= K <= Ctot: "
                         f"{tuple(sem_s.shape)} vs {tuple(sem_t.shape)}")
    if normalize not in (0, 1, False, True):
        raise ValueError(f"normalize must be 0 or 1, got {normalize!r}")
    # the scale rules are those of every level
    return _pod_check(sem_s, sem_s, 1.0, scales), int(normalize)


def local_pod_logits_torch(sem_s, sem_t, scales=POD_SCALES, weight=1.0, normalize=1):
    """``weight`` times the Local POD distance on the logits (PLOP's last level, ``extra_channels: "sum"``) as a differentiable
    torch composition: the student's channels from ``K`` on are summed into its background channel, then the level is
    ``local_pod_torch`` at slope 1 on ``K`` channels; ``normalize=0`` leaves the embeddings un-normalised.  The teacher is
    detached.  fp64 logits stay fp64.  Serves CPU devices, shapes the kernels refuse and ``UCD_FUSED_POD=0``."""
    scales, normalize = _pod_logits_check(sem_s, sem_t, scales, normalize)
    K = sem_t.shape[1]
    m = _wide(sem_s)
    if K < m.shape[1]:
        m = torch.cat([m[:, :1] + m[:, K:].sum(dim=1, keepdim=True), m[:, 1:K]], dim=1)
    e_s = _pod_embed(m, 1.0, scales)
    e_t = _pod_embed(sem_t.detach().to(m.dtype), 1.0, scales)
    if normalize:
        e_s = e_s / e_s.norm(dim=1, keepdim=True).clamp_min(1e-12)
        e_t = e_t / e_t.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return weight * (e_s - e_t).norm(dim=1).mean()


@functools.lru_cache(maxsize=None)
def _pod_logits_plan(h, w, Ctot, K, scales, B, normalize):
    return hip.pod_logits_plan(h, w, Ctot, K, scales, B, normalize)


def _logit_rows(x):
    """[B, C, h, w] logits -> (tensor, pitch): fp32 channels-last rows with a constant pitch.  A tensor whose strides already say
    so (a channels_last tensor or a channel slice of one - the kernels ask for 4-byte alignment only) is taken as it is."""
    B, Cc, h, w = x.shape
    if x.dtype == torch.float32 and Cc > 1 and w > 1 and h > 1:
        sb, sc, sh, sw = x.stride()
        if sc == 1 and sw >= Cc and sh == w * sw and sb == h * w * sw:
            return x, sw
    return x.float().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), Cc


class _FusedLocalPODLogits(torch.autograd.Function):
    """weight * Local POD on the logits on the HIP kernels (ucd_pod_logits_forward / ucd_pod_logits_backward, csrc/pod.hip): four
    launches forward, which keep the coefficient strips ``g_E`` ([B, n_E] fp32 on K channels), one backward, which reads the
    student rows once more and writes ``d sem`` (fp32 rows, cast to the logits' dtype where that differs)."""

    @staticmethod
    def forward(ctx, sem_s, sem_t, scales, weight, normalize):
        lib = hip.load()
        xs, ld_s = _logit_rows(sem_s.detach())
        xt, ld_t = _logit_rows(sem_t.detach())
        B, Ctot, h, w = xs.shape
        K = xt.shape[1]
        plan = _pod_logits_plan(h, w, Ctot, K, scales, B, normalize)
        arr, n = hip.pod_scales(scales)
        g = torch.empty(B, plan["n_E"], dtype=torch.float32, device=xs.device)
        out = torch.empty(1, dtype=torch.float32, device=xs.device)
        nbytes = plan["workspace_bytes"]
        ws = hip.workspace(nbytes, xs.device, "pod")
        with hip._timed("ucd_pod_logits_forward", B * h * w * (Ctot + K) * 4):
            hip._check(lib.ucd_pod_logits_forward(hip.ptr(xs), ld_s, hip.ptr(xt), ld_t, hip.F32, B, Ctot, K, h, w,
                                                  hip.C.cast(arr, hip.C.c_void_p), n, normalize, float(weight), hip.ptr(out),
                                                  hip.ptr(g), hip.ptr(ws), nbytes, hip.stream()), "ucd_pod_logits_forward")
        ctx.save_for_backward(xs, g)
        ctx.meta = (ld_s, K, scales, sem_s.dtype)
        return weight * out[0]

    @staticmethod
    def backward(ctx, grad):
        xs, g = ctx.saved_tensors
        ld_s, K, scales, dtype = ctx.meta
        B, Ctot, h, w = xs.shape
        arr, n = hip.pod_scales(scales)
        go = grad.detach().reshape(1).to(torch.float32).contiguous()
        d = torch.empty((B, h, w, Ctot), dtype=torch.float32, device=xs.device).permute(0, 3, 1, 2)
        with hip._timed("ucd_pod_logits_backward", 2 * B * h * w * Ctot * 4):
            hip._check(hip.load().ucd_pod_logits_backward(hip.ptr(xs), ld_s, hip.F32, B, Ctot, K, h, w,
                                                          hip.C.cast(arr, hip.C.c_void_p), n, hip.ptr(g), hip.ptr(go), hip.ptr(d), Ctot,
                                                          hip.stream()), "ucd_pod_logits_backward")
        return (d if dtype == torch.float32 else d.to(dtype)), None, None, None, None


def pod_logits_kernels_take(sem_s):
    """Do the kernels of the level on the logits serve these student logits?  bf16 or fp32 on a GPU, at most 256 channels, at most
    1024 rows and columns (ucd_pod_logits_plan states the same bounds)."""
    return (sem_s.is_cuda and sem_s.dtype in (torch.bfloat16, torch.float32) and sem_s.shape[1] <= 256
            and max(sem_s.shape[2:]) <= 1024)


def fused_local_pod_logits(sem_s, sem_t, scales=POD_SCALES, weight=1.0, normalize=1):
    """``weight * mean_b |E(M)_b - E(sem_t)_b|``: PLOP's Local POD on the logits between the student's ``[B, Ctot, h, w]`` and the
    teacher's ``[B, K, h, w]``, ``M`` the student's logits with the channels from ``K`` on summed into the background channel;
    the embeddings L2-normalised per sample unless ``normalize=0``; differentiable w.r.t. ``sem_s``.  On the GPU it is four HIP
    launches forward and one backward (csrc/pod.hip); CPU tensors, logits the kernels refuse (``pod_logits_kernels_take``) and
    ``UCD_FUSED_POD=0`` run ``local_pod_logits_torch``."""
    scales, normalize = _pod_logits_check(sem_s, sem_t, scales, normalize)
    if not pod_logits_kernels_take(sem_s) or _switches.get("UCD_FUSED_POD", "1") == "0":
        return local_pod_logits_torch(sem_s, sem_t, scales, weight, normalize)
    return _FusedLocalPODLogits.apply(sem_s, sem_t, scales, float(weight), normalize)


KD_MODES = {"unbiased": hip.KD_UNBIASED, "plain": hip.KD_PLAIN}


SEG_LOSS_FORMS = ("auto", "tiled", "gather")


@functools.lru_cache(maxsize=None)
def seg_losses_route(H, W, h, w, Ctot, K, has_teacher, ce_old_cl=None):
    """``"tiled"`` or ``"gather"``: which kernel ``fused_seg_losses(form="auto")`` launches for a geometry and a class split.  A pure
    host function: it asks ``ucd_seg_losses_plan_ex`` (a 16-byte aligned ``d_sem``, the packed forms as ``UCD_SEG_PK`` says) and
    answers ``"gather"`` exactly when no tiled form serves the geometry (``UCD_EUNSUPPORTED``).  Arguments the plan calls illegal
    stay ``"tiled"``: the call itself then reports them, under its own name, as it always did.  ``K`` is the teacher's class count
    (without a teacher: the cross entropy's ``old_cl``), ``ce_old_cl`` the cross entropy's when it differs.  Cached per argument
    tuple: the plan walks every tile of the label map."""
    K = max(int(K), 1)
    rc = hip.load().ucd_seg_losses_plan_ex(int(H), int(W), int(h), int(w), int(Ctot), K, K if ce_old_cl is None else int(ce_old_cl),
                                           hip.KD_UNBIASED, int(bool(has_teacher)), 1, -1, None, None, None, None)
    return "gather" if rc == hip.EUNSUPPORTED else "tiled"


def fused_seg_losses(sem, sem_old, labels, old_cl, ce_weight=1.0, kd_weight=0.0, ignore_index=255, *, kd="unbiased", alpha=1.0,
                     form="auto", sample_weight=None, focal=None):
    """Returns (ce_weight*CE + kd_weight*KD [differentiable w.r.t. ``sem``], CE, KD) where CE / KD are the
    reference's ``UnbiasedCrossEntropy(old_cl)(up(sem), labels).mean()`` (``old_cl`` 1: ``nn.CrossEntropyLoss``) and
    ``UnbiasedKnowledgeDistillationLoss(alpha=alpha)(up(sem), up(sem_old))`` or, with ``kd="plain"``,
    ``KnowledgeDistillationLoss(alpha=alpha)(...)`` (``up`` = bilinear to the label size).

    With a teacher of K classes ``old_cl`` is 1 or K (the reference produces no other pair; the kernel refuses one).

    ``form``: ``"tiled"`` is the scatter kernels (``ucd_seg_losses_ex``), which refuse a geometry whose tiles do
    not fit their LDS; ``"gather"`` is ``ucd_seg_losses_gather`` - any up-sampling factor >= 1, a gradient with the same bits on every
    run, and, under ``torch.no_grad()`` or with a ``sem`` that needs no gradient, the losses alone; ``"auto"`` is ``"tiled"`` wherever
    that serves (the call, and the bits, it always was) and ``"gather"`` elsewhere (``seg_losses_route``).

    ``sample_weight`` ([B], each in [0, 1] - the adaptive factor of ``fused_pseudo_labels``): CE becomes
    ``1 / (BHW) sum_b sample_weight[b] sum_p CE_p``; KD is untouched.  None (the default) is the call without a weight.

    ``focal`` (``(gamma, alpha)``, ``gamma >= 0``, ``alpha > 0``): CE becomes the reference's ``FocalLoss`` on the same cross
    entropy, ``mean(alpha (1 - exp(-CE_p))^gamma CE_p)`` over all pixels (times the image's ``sample_weight``), inside the same
    kernels (``focal_modulate`` states the rule where ``1 - exp(-CE_p)`` rounds to 0); KD is untouched.  None (the default) is the
    call without it; ``(0, 1)`` gives its bits."""
    if not sem.is_cuda:
        raise RuntimeError("ucd_amd.loss.fused_seg_losses runs on the GPU only (there is no CPU fallback)")
    if kd not in KD_MODES:
        raise ValueError(f"kd must be 'unbiased' or 'plain', not {kd!r}")
    if form not in SEG_LOSS_FORMS:
        raise ValueError(f"form must be 'auto', 'tiled' or 'gather', not {form!r}")
    if sample_weight is not None:
        if sample_weight.shape != (sem.shape[0],) or sample_weight.device != sem.device:
            raise ValueError(f"sample_weight must be [{sem.shape[0]}] on {sem.device}, got {tuple(sample_weight.shape)} on "
                             f"{sample_weight.device}")
        sample_weight = sample_weight.detach().float().contiguous()
    if focal is not None:
        focal = _focal_check(*focal)
    if form == "auto":
        K = int(old_cl) if sem_old is None else sem_old.shape[1]
        form = seg_losses_route(labels.shape[-2], labels.shape[-1], sem.shape[2], sem.shape[3], sem.shape[1], K, sem_old is not None,
                                max(int(old_cl), 1))
    return _FusedSegLosses.apply(sem, sem_old, labels, old_cl, ce_weight, kd_weight, ignore_index, KD_MODES[kd], float(alpha), form,
                                 sample_weight, focal)


# ---- SDR's class-prototype feature losses (csrc/proto.hip) ------------------------------------------------
def proto_classes_torch(labels, sem_t, T, K, hw, ignore_index=255):
    """The class of every low-resolution pixel, int32 ``[B, h, w]``: the label at ``sy = min(floor(i * (float)H / h), H - 1)`` (and
    ``sx`` likewise: ``F.interpolate(mode='nearest')``), -1 where it is ``ignore_index`` or outside ``[0, T)``; with teacher logits
    ``sem_t`` [B, >= K, h, w] a background pixel takes the first arg-max of the teacher's first ``K`` channels.  The torch
    composition of ``proto_classes``."""
    h, w = int(hw[0]), int(hw[1])
    B, H, W = labels.shape
    dev = labels.device
    fy, fx = torch.tensor(H, dtype=torch.float32) / h, torch.tensor(W, dtype=torch.float32) / w       # (float)H / h, in fp32
    sy = (torch.arange(h, dtype=torch.float32) * fy).floor().long().clamp_max(H - 1).to(dev)
    sx = (torch.arange(w, dtype=torch.float32) * fx).floor().long().clamp_max(W - 1).to(dev)
    y = labels[:, sy][:, :, sx]
    cls = torch.where((y == ignore_index) | (y < 0) | (y >= T), torch.full_like(y, -1), y)
    if sem_t is not None:
        if K < 1 or sem_t.shape[1] < K or tuple(sem_t.shape[2:]) != (h, w):
            raise ValueError(f"teacher logits [B, >= {K}, {h}, {w}] are expected, got {tuple(sem_t.shape)}")
        cls = torch.where(cls == 0, sem_t[:, :K].detach().float().argmax(dim=1), cls)
    return cls.to(torch.int32)


def proto_classes(labels, sem_t, T, K, hw, ignore_index=255):
    """``proto_classes_torch`` as one HIP launch (ucd_proto_classify); CPU tensors, more than 256 classes and ``UCD_FUSED_PROTO=0``
    run the composition."""
    if labels.dim() != 3 or labels.dtype != torch.int64:
        raise ValueError(f"int64 labels [B, H, W] are expected, got {tuple(labels.shape)} {labels.dtype}")
    if not 0 <= K <= T:
        raise ValueError(f"K = {K} teacher classes must be in 0 .. T = {T}")
    h, w = int(hw[0]), int(hw[1])
    if not labels.is_cuda or T > hip.PROTO_MAX_T or _switches.get("UCD_FUSED_PROTO", "1") == "0":
        return proto_classes_torch(labels, sem_t, T, K, hw, ignore_index)
    rows = None
    if sem_t is not None:
        if K < 1 or sem_t.shape[1] < K or tuple(sem_t.shape[2:]) != (h, w):
            raise ValueError(f"teacher logits [B, >= {K}, {h}, {w}] are expected, got {tuple(sem_t.shape)}")
        rows = _pseudo_rows(sem_t)
    cls = hip.proto_classify(labels.contiguous(), rows, rows.shape[1] if rows is not None else 0, h, w, T, K, ignore_index)
    return cls.view(labels.shape[0], h, w)


def _safe_norm(d):
    """L2 norm over the last dimension whose gradient at a zero distance is 0."""
    s = (d * d).sum(dim=-1)
    pos = s > 0
    return torch.where(pos, torch.where(pos, s, torch.ones_like(s)).sqrt(), torch.zeros_like(s))


def _proto_check(x, cls, state, old, weights):
    """The argument rules of the class-prototype losses; returns (state_sum, state_n, O or None, valid or None, weights, T, K)."""
    if x.dim() != 4:
        raise ValueError(f"a feature map [B, C, h, w] is expected, got {tuple(x.shape)}")
    B, Cc, h, w = x.shape
    if tuple(cls.shape) != (B, h, w) or cls.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"cls must be an integer [{B}, {h}, {w}] map, got {tuple(cls.shape)} {cls.dtype}")
    state_sum, state_n = state
    if state_sum.dim() != 2 or state_sum.shape[1] != Cc or state_sum.dtype != torch.float64 or tuple(state_n.shape) != (state_sum.shape[0],) \
            or state_n.dtype != torch.int64:
        raise ValueError(f"the state is (float64 [T, {Cc}], int64 [T]), got {tuple(state_sum.shape)} {state_sum.dtype} and "
                         f"{tuple(state_n.shape)} {state_n.dtype}")
    T = state_sum.shape[0]
    O = valid = None
    K = 0
    if old is not None and old[0] is not None and old[0].shape[0] > 0:
        O, valid = old
        K = O.shape[0]
        if O.dim() != 2 or O.shape[1] != Cc or K > T or tuple(valid.shape) != (K,) or valid.dtype != torch.bool:
            raise ValueError(f"the old prototypes are ([K <= {T}, {Cc}], bool [K]), got {tuple(O.shape)} and {tuple(valid.shape)} {valid.dtype}")
    weights = tuple(float(v) for v in weights)
    if len(weights) != 3 or not all(math.isfinite(v) and v >= 0.0 for v in weights):
        raise ValueError(f"the weights (match, attract, repel) must be three finite values >= 0, got {weights}")
    return state_sum, state_n, O, valid, weights, T, K


def proto_losses_torch(x, cls, state, old, weights):
    """``fused_proto_losses`` as a differentiable torch composition (``index_add_`` over the rows and ``[T, T, C]`` broadcasts):
    serves CPU tensors, shapes the kernels refuse and ``UCD_FUSED_PROTO=0``.  fp64 maps stay fp64 (the tests); half-precision maps
    compute in fp32, with the running prototypes rounded to fp32 as the kernels' tables hold them.  On the GPU ``index_add_`` adds
    with float atomics, so two runs agree to the rounding of re-ordered sums, not bit for bit."""
    state_sum, state_n, O, valid, (w_m, w_a, w_r), T, K = _proto_check(x, cls, state, old, weights)
    B, Cc, h, w = x.shape
    X = _wide(x).permute(0, 2, 3, 1).reshape(B * h * w, Cc)
    c = cls.reshape(-1).long()
    has = (c >= 0) & (c < T)
    idx = torch.where(has, c, torch.zeros_like(c))
    hasf = has.to(X.dtype)
    n = torch.zeros(T, dtype=X.dtype, device=X.device).index_add_(0, idx, hasf)
    S = torch.zeros(T, Cc, dtype=X.dtype, device=X.device).index_add_(0, idx, X * hasf.unsqueeze(1))
    present = n > 0
    nn_ = n.clamp_min(1.0)
    mu = S / nn_.unsqueeze(1)
    zero = X.new_zeros(())
    l_match = zero
    if K > 0:
        A = present[:K] & valid.to(X.device)
        d = _safe_norm(mu[:K] - O.to(device=X.device, dtype=X.dtype))
        l_match = torch.where(A, d, torch.zeros_like(d)).sum() / A.sum().clamp_min(1).to(X.dtype)
    seen = state_n.to(X.device) > 0
    Bs = present & seen
    R = (state_sum.to(X.device) / state_n.to(X.device).clamp_min(1).unsqueeze(1).double())
    R = R.to(X.dtype) if X.dtype == torch.float64 else R.float().to(X.dtype)
    R = torch.where(seen.unsqueeze(1), R, torch.zeros_like(R))
    diff = X - R[idx]
    sq = (diff * diff).sum(dim=1) * (has & Bs[idx]).to(X.dtype)
    per_class = torch.zeros(T, dtype=X.dtype, device=X.device).index_add_(0, idx, sq) / nn_
    l_attr = per_class.sum() / Bs.sum().clamp_min(1).to(X.dtype)
    D = _safe_norm(mu.unsqueeze(1) - mu.unsqueeze(0))
    pair = present.unsqueeze(1) & present.unsqueeze(0) & ~torch.eye(T, dtype=torch.bool, device=X.device)
    l_rep = torch.where(pair, 1.0 / (D + 1e-6), torch.zeros_like(D)).sum() / present.sum().clamp_min(1).to(X.dtype)
    total = w_m * l_match + w_a * l_attr + w_r * l_rep
    parts = {"match": l_match.detach(), "attract": l_attr.detach(), "repel": l_rep.detach(),
             "sums": S.detach().double(), "n": n.detach().round().long()}
    return total, parts


class _FusedProto(torch.autograd.Function):
    """The weighted class-prototype losses on the HIP kernels (ucd_proto_forward / ucd_proto_backward, csrc/proto.hip): three
    launches forward, one backward.  The forward keeps the tables ``a | R | G`` ((2 C + 1) T floats) and no copy of the map."""

    @staticmethod
    def forward(ctx, x, cls, state_sum, state_n, O, valid, weights):
        xs, M, Cc, HW, ld = hip.rows_view(x.detach())
        T = state_sum.shape[0]
        K = 0 if O is None else O.shape[0]
        out, tables, sums, n = hip.proto_forward(xs, ld, M, Cc, cls, T, K, state_sum, state_n, O, valid, weights)
        ctx.save_for_backward(xs, cls, tables)
        ctx.meta = (ld, T)
        vals = out[1:]
        ctx.mark_non_differentiable(vals, sums, n)
        return out[0], vals, sums, n

    @staticmethod
    def backward(ctx, grad, *unused):
        xs, cls, tables = ctx.saved_tensors
        ld, T = ctx.meta
        B, Cc, h, w = xs.shape
        go = grad.detach().reshape(1).to(torch.float32).contiguous()
        d = hip.empty_like_rows(xs)
        hip.proto_backward(xs, ld, B * h * w, Cc, cls, T, tables, go, d, Cc)
        return d, None, None, None, None, None, None


def proto_kernels_take(x, T):
    """Do the class-prototype kernels serve this map?  bf16 or fp32 on a GPU, C a multiple of 8 up to 512, at most 256 classes
    (ucd_proto_plan states the same bounds)."""
    return (x.is_cuda and x.dtype in (torch.bfloat16, torch.float32) and x.shape[1] % 8 == 0 and x.shape[1] <= hip.PROTO_MAX_C
            and T <= hip.PROTO_MAX_T and x.shape[0] * x.shape[2] * x.shape[3] < 2 ** 31)


def fused_proto_losses(x, cls, state, old, weights):
    """SDR's class-prototype feature losses on the raw pre-logits ``x`` [B, C, h, w]: ``(total, parts)`` with ``total = w_m L_match +
    w_a L_attr + w_r L_rep`` (differentiable w.r.t. ``x``) and ``parts = {"match", "attract", "repel"`` (the three unweighted values),
    ``"sums"`` [T, C] fp64, ``"n"`` [T] int64 (this batch's per-class sums and counts: what ``proto_update`` adds to the state)``}``.

    ``cls`` [B, h, w] is the class map of ``proto_classes`` (-1: none); ``state = (sum [T, C] fp64, N [T] int64)`` the running
    prototypes as they stood before this batch; ``old = (O [K, C] fp32, valid [K] bool)`` the previous step's prototypes, or None;
    ``weights = (w_m, w_a, w_r)``.  ``L_match`` is the mean distance of the batch means to the valid old prototypes, ``L_attr`` the
    mean over classes of the mean squared distance of a class's pixels to its running prototype, ``L_rep`` the mean over present
    classes of ``sum_k 1 / (|mu_c - mu_k| + 1e-6)``; an empty index set and a zero distance give 0 and no gradient.  On the GPU
    it is three HIP launches forward and one backward (csrc/proto.hip), fixed summation order; CPU tensors, shapes the kernels
    refuse (``proto_kernels_take``) and ``UCD_FUSED_PROTO=0`` run ``proto_losses_torch``."""
    state_sum, state_n, O, valid, weights, T, K = _proto_check(x, cls, state, old, weights)
    if not proto_kernels_take(x, T) or _switches.get("UCD_FUSED_PROTO", "1") == "0":
        return proto_losses_torch(x, cls, state, old, weights)
    dev = x.device
    if O is not None:
        O = O.detach().to(device=dev, dtype=torch.float32).contiguous()
        valid = valid.to(dev).contiguous()
    cls32 = cls.to(torch.int32).contiguous().view(-1)
    total, vals, sums, n = _FusedProto.apply(x, cls32, state_sum.contiguous(), state_n.contiguous(), O, valid, weights)
    return total, {"match": vals[0], "attract": vals[1], "repel": vals[2], "sums": sums, "n": n}


def proto_update(state, parts):
    """``sum += parts["sums"]``, ``N += parts["n"]`` in place (ucd_proto_update on the GPU: one launch, fp64 and int64)."""
    state_sum, state_n = state
    if state_sum.is_cuda and state_sum.shape[0] <= hip.PROTO_MAX_T and state_sum.shape[1] <= hip.PROTO_MAX_C \
            and _switches.get("UCD_FUSED_PROTO", "1") != "0":
        hip.proto_update(state_sum, state_n, parts["sums"].contiguous(), parts["n"].contiguous())
    else:
        state_sum += parts["sums"].to(state_sum.dtype)
        state_n += parts["n"].to(state_n.dtype)


# ---- PLOP's pseudo-labelling (csrc/pseudo_label.hip) ------------------------------------------------------
def _pseudo_check(sem_old, labels):
    if sem_old.dim() != 4 or labels.dim() != 3 or labels.shape[0] != sem_old.shape[0] or labels.dtype != torch.int64:
        raise ValueError(f"teacher logits [B, K, h, w] and int64 labels [B, H, W] are expected, got {tuple(sem_old.shape)} and "
                         f"{tuple(labels.shape)} {labels.dtype}")
    if labels.shape[1] < sem_old.shape[2] or labels.shape[2] < sem_old.shape[3]:
        raise ValueError(f"the label map {tuple(labels.shape[1:])} is smaller than the logits {tuple(sem_old.shape[2:])}")


def pseudo_view_torch(sem_old, labels, ignore_index=255):
    """(candidate mask, pseudo-class c*, uncertainty u) [B, H, W] of the definitions: ``z`` the teacher logits up-sampled to the label
    size, ``c*`` its first arg-max, ``u = H(softmax z) / log K`` (``H = log S - T / S`` around the maximum, no epsilon; 0 for
    K = 1), candidates the pixels with ``0 <= label < K`` that are not ``ignore_index``.  fp64 logits stay fp64."""
    _pseudo_check(sem_old, labels)
    K = sem_old.shape[1]
    z = F.interpolate(_wide(sem_old.detach()), size=labels.shape[-2:], mode="bilinear", align_corners=False)
    m, arg = z.max(dim=1)
    d = z - m.unsqueeze(1)
    e = d.exp()
    S = e.sum(dim=1)
    u = (S.log() - (d * e).sum(dim=1) / S) / math.log(K) if K > 1 else torch.zeros_like(m)
    cand = (labels >= 0) & (labels < K) & (labels != ignore_index)
    return cand, arg, u.clamp(0., 1.)


def pseudo_labels_torch(sem_old, labels, thresholds, f_min=0.0, ignore_index=255):
    """``fused_pseudo_labels`` as a torch composition on the up-sampled ``[B, K, H, W]`` logits: serves CPU tensors and
    ``UCD_FUSED_PSEUDO=0``."""
    cand, arg, u = pseudo_view_torch(sem_old, labels, ignore_index)
    passed = cand & (u < thresholds.to(u.dtype)[arg])
    out = torch.where(passed, arg, torch.where(cand, torch.full_like(labels, ignore_index), labels))
    counts = torch.stack((passed.flatten(1).sum(dim=1), cand.flatten(1).sum(dim=1)), dim=1).to(torch.int32)
    num, den = counts[:, 0].double(), counts[:, 1].double()
    factor = torch.where(den > 0, num / (den + 1e-6), torch.zeros_like(den)).clamp_min(float(f_min)).float()
    return out, factor, counts


def pseudo_hist_torch(sem_old, labels, hist, ignore_index=255):
    """``pseudo_hist`` as a torch composition: adds ``bincount(c* bins + bin(u))`` of the candidates into ``hist`` [K, bins] int64."""
    cand, arg, u = pseudo_view_torch(sem_old, labels, ignore_index)
    K, bins = hist.shape
    b = (u * bins).floor().long().clamp_max(bins - 1)
    hist += torch.bincount((arg * bins + b)[cand], minlength=K * bins).view(K, bins)
    return hist


def _pseudo_rows(sem_old):
    B, K, h, w = sem_old.shape
    return sem_old.detach().permute(0, 2, 3, 1).reshape(B * h * w, K).float().contiguous()      # as _LowResLogitLoss.operands


def _pseudo_fused(sem_old):
    return sem_old.is_cuda and _switches.get("UCD_FUSED_PSEUDO", "1") != "0"


def fused_pseudo_labels(sem_old, labels, thresholds, f_min=0.0, ignore_index=255, uncertainty=False):
    """PLOP's pseudo-labels from the LOW-resolution teacher logits ``sem_old`` [B, K, h, w]: ``(labels_out, factor, counts)``.
    A candidate pixel (``0 <= label < K``, not ``ignore_index``) becomes the teacher's arg-max ``c*`` where the normalised entropy
    ``u`` of its up-sampled soft-max is below ``thresholds[c*]`` and ``ignore_index`` where not; any other pixel keeps its label.
    ``counts`` [B, 2] int32 = (passed, candidates) per image, ``factor`` [B] = ``max(passed / (candidates + 1e-6), f_min)``: the
    weight ``fused_seg_losses(sample_weight=...)`` takes.  ``uncertainty=True`` appends the ``u`` map (0 off the candidates).
    On the GPU one HIP launch plus the factor launch (ucd_pseudo_label; no [B, K, H, W] tensor); CPU tensors and
    ``UCD_FUSED_PSEUDO=0`` run ``pseudo_labels_torch``."""
    _pseudo_check(sem_old, labels)
    B, K, h, w = sem_old.shape
    if thresholds.shape != (K,):
        raise ValueError(f"thresholds must be [{K}], got {tuple(thresholds.shape)}")
    if not 0.0 <= float(f_min) <= 1.0:          # the library's rule, for the composition too: the factor is a weight in [0, 1]
        raise ValueError(f"f_min = {f_min} is outside [0, 1]")
    if not _pseudo_fused(sem_old):
        res = pseudo_labels_torch(sem_old, labels, thresholds, f_min, ignore_index)
        if uncertainty:
            cand, _, u = pseudo_view_torch(sem_old, labels, ignore_index)
            res += (torch.where(cand, u, torch.zeros_like(u)).float(),)
        return res
    H, W = labels.shape[-2:]
    t, labels = _pseudo_rows(sem_old), labels.contiguous()
    thr = thresholds.detach().to(device=t.device, dtype=torch.float32).contiguous()
    out = torch.empty_like(labels)
    counts = torch.empty(B, 2, dtype=torch.int32, device=t.device)
    factor = torch.empty(B, dtype=torch.float32, device=t.device)
    unc = torch.empty(B, H, W, dtype=torch.float32, device=t.device) if uncertainty else None
    # labels read once and written once, plus the teacher rows
    with hip._timed("ucd_pseudo_label", B * H * W * 16 + t.numel() * 4):
        hip._check(hip.load().ucd_pseudo_label(hip.ptr(t), K, hip.ptr(labels), B, H, W, h, w, K, int(ignore_index), hip.ptr(thr),
                                               float(f_min), hip.ptr(out), hip.ptr(counts), hip.ptr(factor), hip.ptr(unc),
                                               hip.stream()), "ucd_pseudo_label")
    return (out, factor, counts, unc) if uncertainty else (out, factor, counts)


def pseudo_hist(sem_old, labels, hist, ignore_index=255):
    """Adds the uncertainty histogram of one batch into ``hist`` [K, bins] int64 (on the device of ``sem_old``): ``hist[c*,
    min(floor(u bins), bins - 1)] += 1`` over the candidate pixels - what ``pseudo_median`` turns into the per-class thresholds.
    Integer adds: exact, independent of order.  ucd_pseudo_hist on the GPU, ``pseudo_hist_torch`` on the CPU or under
    ``UCD_FUSED_PSEUDO=0``."""
    _pseudo_check(sem_old, labels)
    B, K, h, w = sem_old.shape
    if hist.dim() != 2 or hist.shape[0] != K or hist.dtype != torch.int64 or not hist.is_contiguous() or hist.device != sem_old.device:
        raise ValueError(f"hist must be a contiguous int64 [{K}, bins] on {sem_old.device}, got {tuple(hist.shape)} {hist.dtype}")
    if not 2 <= hist.shape[1] <= 1024:
        raise ValueError(f"{hist.shape[1]} bins are outside [2, 1024]")
    if not _pseudo_fused(sem_old):
        return pseudo_hist_torch(sem_old, labels, hist, ignore_index)
    H, W = labels.shape[-2:]
    t, labels = _pseudo_rows(sem_old), labels.contiguous()
    with hip._timed("ucd_pseudo_hist", B * H * W * 8 + t.numel() * 4):
        hip._check(hip.load().ucd_pseudo_hist(hip.ptr(t), K, hip.ptr(labels), B, H, W, h, w, K, int(ignore_index), hist.shape[1],
                                              hip.ptr(hist), hip.stream()), "ucd_pseudo_hist")
    return hist


def pseudo_median(hist, floor=0.0):
    """The per-class thresholds [K] (numpy float64) of a histogram [K, bins]: the interpolated median of each row,
    ``(j + (n / 2 - cum_<j) / hist[j]) / bins`` with ``j`` the first bin whose cumulative count reaches half of the row's ``n``,
    floored at ``floor``; an empty row gets the floor.  (PLOP's published loop advances its running sum by the bin index; this is
    the median its paper describes.)"""
    import numpy as np
    hist = np.asarray(hist.cpu() if torch.is_tensor(hist) else hist, dtype=np.float64)
    K, bins = hist.shape
    out = np.full(K, float(floor), dtype=np.float64)
    cum = np.cumsum(hist, axis=1)
    for c in range(K):
        n = cum[c, -1]
        if n <= 0:
            continue
        half = n / 2.0
        j = int(np.argmax(cum[c] >= half))
        out[c] = max((j + (half - (cum[c, j] - hist[c, j])) / hist[c, j]) / bins, float(floor))
    return out


def _wide(x):
    """fp32 arithmetic for half-precision logits; fp32 and fp64 inputs keep their type (the float64 references of the tests)."""
    return x if x.dtype in (torch.float32, torch.float64) else x.float()


# ---- focal cross entropy (the reference's FocalLoss, utils/loss.py:6-28) -----------------------------------
def _focal_check(gamma, alpha):
    """The domain of the focal arguments (the library's rule, for the composition too); returns them as floats."""
    gamma, alpha = float(gamma), float(alpha)
    if not (math.isfinite(gamma) and gamma >= 0.0):
        raise ValueError(f"focal gamma = {gamma} must be finite and >= 0")
    if not (math.isfinite(alpha) and alpha > 0.0):
        raise ValueError(f"focal alpha = {alpha} must be finite and > 0")
    return gamma, alpha


def focal_modulate(ce_map, gamma=2.0, alpha=1.0):
    """``alpha * u^gamma * ce`` with ``u = clamp(1 - exp(-ce), 0, 1)``, element by element, on a ``reduction='none'`` cross-entropy
    map (an ignored pixel holds 0); differentiable.  Where ``u`` rounds to 0 the value and the gradient are 0 for ``gamma > 0``
    (``0^(gamma-1) * ce`` is never formed: for ``gamma < 1`` it would be ``inf * 0``); ``gamma == 0`` is ``alpha * ce``.  The torch
    composition of what ``fused_seg_losses(focal=...)`` does inside its kernels: serves CPU tensors and ``UCD_FUSED_FOCAL=0``."""
    gamma, alpha = _focal_check(gamma, alpha)
    if gamma == 0.0:
        return alpha * ce_map
    u = (1.0 - torch.exp(-ce_map)).clamp(0.0, 1.0)
    zero = u <= 0
    base = torch.where(zero, torch.ones_like(u), u)          # the power and its derivative never see a 0
    return torch.where(zero, torch.zeros_like(ce_map), alpha * base.pow(gamma) * ce_map)


class FocalLoss(nn.Module):
    """The reference's ``FocalLoss`` (utils/loss.py:13-28) on full-resolution logits: ``alpha * (1 - p_t)^gamma * CE`` of the plain
    cross entropy, averaged over ALL pixels (ignored ones count as 0) or summed."""

    def __init__(self, alpha=1, gamma=2, size_average=True, ignore_index=255):
        super().__init__()
        self.gamma, self.alpha = _focal_check(gamma, alpha)
        self.size_average, self.ignore_index = size_average, ignore_index

    def forward(self, inputs, targets):
        ce = F.cross_entropy(_wide(inputs), targets, reduction="none", ignore_index=self.ignore_index)
        focal = focal_modulate(ce, self.gamma, self.alpha)
        return focal.mean() if self.size_average else focal.sum()


class UnbiasedCrossEntropy(nn.Module):
    """Cross entropy in which the background competes as the pooled old classes:
    ``log p(bkg) = LSE(x[:, :old_cl]) - LSE(x)``; labels below ``old_cl`` count as background."""

    def __init__(self, old_cl=None, reduction="mean", ignore_index=255):
        super().__init__()
        self.reduction, self.ignore_index, self.old_cl = reduction, ignore_index, old_cl

    def forward(self, inputs, targets):
        old_cl = self.old_cl
        inputs = _wide(inputs)
        den = torch.logsumexp(inputs, dim=1)
        log_bkg = torch.logsumexp(inputs[:, :old_cl], dim=1) - den
        # gather instead of materialising the [B, Ctot, H, W] log-probability tensor (loss.py:99-102)
        labels = torch.where(targets < old_cl, torch.zeros_like(targets), targets)   # loss.py:104-105
        ignore = labels == self.ignore_index
        idx = torch.where(ignore, torch.zeros_like(labels), labels)
        picked = inputs.gather(1, idx.unsqueeze(1)).squeeze(1) - den
        logp = torch.where(idx == 0, log_bkg, picked)
        loss = torch.where(ignore, torch.zeros_like(logp), -logp)
        if self.reduction == "none":
            return loss
        if self.reduction == "sum":
            return loss.sum()
        return loss.sum() / (~ignore).sum()      # nll_loss 'mean': over the non-ignored pixels


class KnowledgeDistillationLoss(nn.Module):
    """Plain soft-target distillation on the old classes (utils/loss.py:112-136)."""

    def __init__(self, reduction="mean", alpha=1.):
        super().__init__()
        self.reduction, self.alpha = reduction, alpha

    def forward(self, inputs, targets, mask=None):
        inputs = _wide(inputs.narrow(1, 0, targets.shape[1]))
        loss = (torch.log_softmax(inputs, dim=1) * torch.softmax(_wide(targets) * self.alpha, dim=1)).mean(dim=1)
        if mask is not None:
            loss = loss * mask.float()
        if self.reduction == "mean":
            return -loss.mean()
        if self.reduction == "sum":
            return -loss.sum()
        return -loss


class UnbiasedKnowledgeDistillationLoss(nn.Module):
    """The student's background is compared with the teacher's as ``p(bkg or any new class)``
    (utils/loss.py:162-174).  The reference also evaluates an unused ``gamma`` from a global average pool
    (:155-156); it never reaches the output and is dropped."""

    def __init__(self, reduction="mean", alpha=1.):
        super().__init__()
        self.reduction, self.alpha = reduction, alpha

    def forward(self, inputs, targets, mask=None):
        K = targets.shape[1]
        inputs, targets = _wide(inputs), _wide(targets) * self.alpha
        den = torch.logsumexp(inputs, dim=1)
        out_old = inputs[:, 1:K] - den.unsqueeze(1)
        # LSE over {background} U {new classes}: index_select-free
        bkg_new = torch.cat((inputs[:, :1], inputs[:, K:]), dim=1)
        out_bkg = torch.logsumexp(bkg_new, dim=1) - den
        q = torch.softmax(targets, dim=1)
        loss = (q[:, 0] * out_bkg + (q[:, 1:] * out_old).sum(dim=1)) / K
        if mask is not None:
            loss = loss * mask.float()
        if self.reduction == "mean":
            return -loss.mean()
        if self.reduction == "sum":
            return -loss.sum()
        return -loss
