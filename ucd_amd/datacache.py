"""Decoded samples kept in HBM (``--cache_gb``): every epoch of a step decodes the same JPEG / PNG files again on the host, while
an MI355X has room for the decoded uint8 bytes of every dataset the launcher supports.  ``DeviceSampleCache`` keeps the raw
``(image [H, W, 3], label [H, W])`` pair of a sample as views into large uint8 slabs; ``dataset.DeviceLoader`` fills it during the
first epoch and afterwards decodes only what did not fit.  No eviction, nothing persists across processes, and the cache is not
part of a checkpoint.  The bookkeeping works on any device (the CPU tests use ``"cpu"``); only the batch kernel needs the GPU.
"""
from __future__ import annotations

import torch

ALIGN = 16                                   # every stored image and label starts at a multiple of 16 bytes


def _aligned(nbytes):
    return (int(nbytes) + ALIGN - 1) // ALIGN * ALIGN


def sample_bytes(height, width):
    """Slab bytes of one decoded sample: the RGB image and the label map, each padded to the alignment."""
    return _aligned(height * width * 3) + _aligned(height * width)


class DeviceSampleCache:
    """``put(index, image_u8, label_u8) -> bool`` / ``get(index) -> (image, label) | None`` over slabs of ``slab_bytes`` that are
    allocated one at a time as they fill, never more than ``budget_bytes`` in all (``siblings``: other caches whose slabs count
    against the same budget).  A sample that does not fit into what is left of the current slab opens the next one; one larger
    than a slab gets a slab of its own size.  ``put`` returns False and stores nothing when the budget does not allow it - a
    later, smaller sample may still fit.  ``hits`` / ``misses`` count ``get`` calls until ``reset_counters()``."""

    def __init__(self, device, budget_bytes, slab_bytes=256 << 20, siblings=()):
        self.device = torch.device(device)
        self.budget_bytes, self.slab_bytes = int(budget_bytes), int(slab_bytes)
        self.siblings = siblings             # may be a list the owner keeps appending to, this cache included
        self.slabs = []                      # uint8 tensors
        self._fill = 0                       # bytes taken in the last slab
        self._views = {}                     # index -> (image view [H, W, 3], label view [H, W])
        self.bytes_used = 0                  # bytes taken in all slabs, alignment padding included
        self.hits = self.misses = 0

    @property
    def bytes_reserved(self):
        """Bytes of the slabs allocated so far: what the cache holds of the device's memory."""
        return sum(s.numel() for s in self.slabs)

    def _room(self):
        return self.budget_bytes - self.bytes_reserved - sum(c.bytes_reserved for c in self.siblings if c is not self)

    def put(self, index, image_u8, label_u8):
        if index in self._views:
            return True
        if image_u8.dtype != torch.uint8 or image_u8.dim() != 3 or image_u8.shape[2] != 3:
            raise ValueError("images must be [H, W, 3] uint8 RGB")
        if label_u8.dtype != torch.uint8 or tuple(label_u8.shape) != tuple(image_u8.shape[:2]):
            raise ValueError(f"the label map of a {tuple(image_u8.shape)} image must be {tuple(image_u8.shape[:2])} uint8")
        H, W = int(image_u8.shape[0]), int(image_u8.shape[1])
        image_bytes, need = _aligned(H * W * 3), sample_bytes(H, W)
        if not self.slabs or self._fill + need > self.slabs[-1].numel():
            size = min(max(self.slab_bytes, need), self._room())
            if size < need:
                return False
            self.slabs.append(torch.empty(size, dtype=torch.uint8, device=self.device))
            self._fill = 0
        slab, at = self.slabs[-1], self._fill
        image = slab[at:at + H * W * 3].view(H, W, 3)
        label = slab[at + image_bytes:at + image_bytes + H * W].view(H, W)
        image.copy_(image_u8, non_blocking=True)
        label.copy_(label_u8, non_blocking=True)
        self._fill += need
        self.bytes_used += need
        self._views[index] = (image, label)
        return True

    def get(self, index):
        views = self._views.get(index)
        if views is None:
            self.misses += 1
        else:
            self.hits += 1
        return views

    def peek(self, index):
        """``get`` without counting: the views of a sample the caller has just stored."""
        return self._views.get(index)

    def shape(self, index):
        """(H, W) of a stored sample."""
        return tuple(self._views[index][1].shape)

    def reset_counters(self):
        self.hits = self.misses = 0

    def __contains__(self, index):
        return index in self._views

    def __len__(self):
        return len(self._views)
