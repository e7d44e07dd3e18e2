"""What an evaluation run shows: prediction maps, colour-coded maps and de-normalised images (the reference's ``test.py:216-238``
with ``utils.color_map`` / ``Label2Color`` / ``Denormalize``).

The reference copies fp32 images, int64 labels and int64 predictions of the whole test set to the host and colours them there.
Here ``render`` makes one fused pass per batch on the device (``ucd_seg_render``, csrc/seg_render.hip; the attention map from
``ucd_attn_energy``) and only ``uint8`` maps leave it; ``save_samples`` writes them with PIL.

Differences from the reference, all deliberate:

* ``color_map`` returns the PASCAL VOC palette for every dataset.  The reference's Cityscapes and ADE palettes are hand-typed
  tables; they are not reproduced.  Pass ``palette=`` for another one.
* The de-normalised image is clamped to [0, 255] before the cast; the reference's ``astype(uint8)`` wraps.
* Files are true RGB.  The reference writes RGB arrays through ``cv2.imwrite``, which takes BGR: its colour-coded files have red
  and blue swapped.  Ground-truth files are PNG (``NNNNgt.png``, ``NNNNgt_clo.png``), not JPEG: label ids must survive the file.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import hip

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)          # the normalisation the loaders apply (dataset.py)


def color_map(dataset=None, palette=None):
    """``uint8 [256, 3]`` palette.  For every ``dataset`` this is the PASCAL VOC palette, by the published devkit algorithm: the
    bits of class id ``i`` are dealt out three at a time - bit ``3k`` to red, ``3k + 1`` to green, ``3k + 2`` to blue - and the
    ``k``-th group lands on bit ``7 - k`` of its channel (most significant first).  0 -> (0, 0, 0), 1 -> (128, 0, 0),
    15 -> (192, 128, 128), 255 -> (224, 224, 192).  The reference's hand-typed Cityscapes and ADE tables are not reproduced;
    ``palette`` takes any ``[256, 3]`` array of values in 0 .. 255 instead (returned as a ``uint8`` copy)."""
    if palette is not None:
        pal = np.asarray(palette)
        if pal.shape != (256, 3) or pal.min() < 0 or pal.max() > 255:
            raise ValueError(f"palette must be a [256, 3] array of values in 0 .. 255, got shape {pal.shape}")
        return pal.astype(np.uint8).copy()
    ids = np.arange(256, dtype=np.uint32)
    cmap = np.zeros((256, 3), dtype=np.uint32)
    for k in range(3):                                     # 8 bits of the id: groups 0, 1 and the two bits of group 2
        for ch in range(3):
            cmap[:, ch] |= ((ids >> (3 * k + ch)) & 1) << (7 - k)
    return cmap.astype(np.uint8)


_cmaps = {}


def _device_cmap(cmap, device):
    if cmap is None:
        key = (device.type, device.index)
        if key not in _cmaps:
            _cmaps[key] = torch.from_numpy(color_map()).to(device)
        return _cmaps[key]
    t = torch.as_tensor(cmap)
    if t.shape != (256, 3) or t.dtype != torch.uint8:
        raise ValueError(f"cmap must be uint8 [256, 3], got {t.dtype} {tuple(t.shape)}")
    return t.to(device).contiguous()


def attn_energy(body):
    """``a = sum_c body^2`` per cell over the Frobenius norm of its image's map (train.py:339-342 of the reference) from a RAW
    ``[B, C, h, w]`` map, fp32 or bf16: fp32 ``[B, h, w]`` (``ucd_attn_energy``)."""
    if not body.is_cuda:
        raise RuntimeError("ucd_amd.visual.attn_energy runs on the GPU only (there is no CPU fallback)")
    x, M, C, HW, ld = hip.rows_view(body.detach())
    B, _, h, w = body.shape
    a = torch.empty(B, h, w, dtype=torch.float32, device=body.device)
    hip._check(hip.load().ucd_attn_energy(hip.ptr(x), ld, hip.dtype_code(x), B, HW, C, hip.ptr(a), hip.stream()), "ucd_attn_energy")
    return a


def render(sem, labels=None, images=None, body=None, cmap=None, mean=MEAN, std=STD, want=None, pred=None):
    """One fused pass over a batch (``ucd_seg_render``): from the LOW-resolution logits ``sem`` [B, Ctot, h, w] (and, each
    optional, ``labels`` int64 [B, H, W], the normalised ``images`` [B, 3, H, W] in any memory format, the raw ``body`` map
    [B, C, ha, wa]) to a dict of device tensors:

    ``pred_u8`` [B, H, W], ``pred_rgb`` [B, H, W, 3]; with labels ``label_u8`` (the labels as ``uint8``) and ``label_rgb``; with
    images ``image_u8`` [B, H, W, 3]; with body ``att`` fp32 [B, H, W] and ``att_low`` [B, ha, wa].

    The output size is that of the labels, else of the images (one of the two is required).  ``want`` restricts the kernel's outputs
    to a subset of ``("pred_u8", "pred_rgb", "label_rgb", "image_u8", "att")``.  With ``pred`` (an integer map [B, H, W] on the
    device, e.g. the fused prediction of ``StreamSegMetrics.update_from_views``) ``pred_u8`` and ``pred_rgb`` show that map - a cast
    and one colour-table index - and the kernel is asked for the other outputs only.  GPU only: a CPU tensor raises
    ``RuntimeError``."""
    if not sem.is_cuda:
        raise RuntimeError("ucd_amd.visual.render runs on the GPU only (there is no CPU fallback)")
    if labels is None and images is None:
        raise ValueError("render needs labels or images: they give the output size")
    B, Ctot, h, w = sem.shape
    H, W = (labels if labels is not None else images).shape[-2:]
    dev = sem.device
    names = {"pred_u8", "pred_rgb"} | ({"label_rgb"} if labels is not None else set()) | \
        ({"image_u8"} if images is not None else set()) | ({"att"} if body is not None else set())
    if want is not None:
        if not set(want) <= names:
            raise ValueError(f"want {sorted(set(want) - names)}: not available from the given inputs ({sorted(names)})")
        names = set(want)
    s = sem.detach().permute(0, 2, 3, 1).reshape(B * h * w, Ctot).float().contiguous()
    lab = None
    if labels is not None:
        lab = labels.contiguous()
        if lab.dtype != torch.int64:
            lab = lab.long()
    img, strides = None, (0, 0, 0, 0)
    if images is not None and "image_u8" in names:
        img = images.detach() if images.dtype == torch.float32 else images.detach().float()
        strides = img.stride()
    att_low, ha, wa = None, 1, 1
    if body is not None and "att" in names:
        att_low = attn_energy(body)
        ha, wa = att_low.shape[-2:]
    cm = _device_cmap(cmap, dev)
    out = {}
    if pred is not None:
        if tuple(pred.shape) != (B, H, W) or pred.device != dev or pred.dtype.is_floating_point:
            raise ValueError(f"pred must be an integer [{B}, {H}, {W}] tensor on {dev}")
        given = {"pred_u8": lambda: pred.to(torch.uint8), "pred_rgb": lambda: cm[pred.long()]}
        out = {name: make() for name, make in given.items() if name in names}
        names = names - set(given)
    kout = {}                                   # what the kernel writes: never the maps made from a given pred
    for name in sorted(names):
        shape = (B, H, W) if name in ("pred_u8", "att") else (B, H, W, 3)
        kout[name] = torch.empty(shape, dtype=torch.float32 if name == "att" else torch.uint8, device=dev)
    if kout:
        with hip._timed("ucd_seg_render", B * H * W * (8 + 12 + 14) + B * h * w * Ctot * 4):
            hip._check(hip.load().ucd_seg_render(hip.ptr(s), Ctot, hip.ptr(lab), hip.ptr(img), *strides, *[float(v) for v in mean],
                                                 *[float(v) for v in std], hip.ptr(cm), hip.ptr(att_low), ha, wa, B, H, W, h, w, Ctot,
                                                 hip.ptr(kout.get("pred_u8")), hip.ptr(kout.get("pred_rgb")),
                                                 hip.ptr(kout.get("label_rgb")), hip.ptr(kout.get("image_u8")), hip.ptr(kout.get("att")),
                                                 hip.stream()), "ucd_seg_render")
    out.update(kout)
    if lab is not None:
        out["label_u8"] = lab.to(torch.uint8)
    if att_low is not None:
        out["att_low"] = att_low
    return out


def save_samples(directory, start_index, rendered):
    """Write one set of files per image of a rendered batch, numbered from ``start_index`` (``NNNN`` = four digits):
    ``NNNNpre.png`` (the raw ``pred_u8``), ``NNNNgt.png`` (the raw labels as ``uint8``), ``NNNNpre_clo.png``, ``NNNNgt_clo.png`` (colour
    coded) and ``NNNNrgb.jpg`` (the de-normalised image) - each only where ``rendered`` holds its tensor.  True RGB; see the module
    docstring for the differences from the reference's files.  Returns the index after the last image."""
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    files = (("pred_u8", "pre.png"), ("label_u8", "gt.png"), ("pred_rgb", "pre_clo.png"), ("label_rgb", "gt_clo.png"),
             ("image_u8", "rgb.jpg"))
    host = {k: rendered[k].cpu().numpy() for k, _ in files if k in rendered}
    n = next(iter(host.values())).shape[0] if host else 0
    for j in range(n):
        stem = os.path.join(directory, f"{start_index + j:04d}")
        for key, suffix in files:
            if key in host:
                Image.fromarray(host[key][j]).save(stem + suffix)
    return start_index + n


class SampleWriter:
    """A ``sink`` for ``Trainer.test``: ``save_samples`` into one directory, numbering the images across batches."""

    def __init__(self, directory):
        self.directory, self.count = directory, 0

    def __call__(self, batch_index, rendered):
        self.count = save_samples(self.directory, self.count, rendered)
