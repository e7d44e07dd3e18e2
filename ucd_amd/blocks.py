"""Bottleneck residual block and DeepLab-V3 ASPP head of the UCD student / teacher.

Host-side mirror of the reference's ``modules/residual.py:7-98`` (``ResidualBlock``) and
``modules/deeplab.py:8-89`` (``DeeplabV3``): same constructor arguments, same sub-module
names (so ``state_dict`` keys are interchangeable with reference checkpoints), same
arithmetic.  What differs is where the HBM-bound glue runs.  When the ``norm_act`` modules
are this package's HIP ABN (``ucd_amd.abn``), the block epilogue
``bn3 -> + residual -> leaky_relu`` (``residual.py:84-97``) and the head's
``cat -> map_bn`` / ``out += pool -> red_bn`` (``deeplab.py:56-69``) are single fused
kernels:

* ``bn3`` normalises, adds the shortcut and applies the block activation in one pass;
* ``map_bn`` runs per 256-channel branch and writes straight into its channel slice of the
  1024-wide ``red_conv`` input, so the concatenation is never materialised;
* the image-level pooling branch enters ``red_bn`` as a per-(image, channel) bias, so the
  ``repeat`` + ``+=`` over the full map never happens.

With any other ``norm_act`` (e.g. a stock BatchNorm shim in the CPU tests) the same modules
fall back to the literal op sequence of the reference.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import NamedTuple

import torch
import torch.nn as nn
import torch.nn.functional as F


def _wgrad_split(M: int) -> int:
    """Number of K-chunks for the weight-gradient GEMM dW = dY^T X of a 1x1 convolution over M = B*H*W rows.
    hipBLASLt's pick for the plain product is a 64x256 macro tile without split-K: 16 workgroups on 256 CUs,
    145 us for 1024x256 at M = 26136.  Splitting M in 8 batched chunks + a sum is 41 us (tools/wgrad_probe.py);
    below ~8k rows the plain product is as fast."""
    if M >= 8192:
        for S in (8, 4, 12, 6, 3, 2):
            if M % S == 0:
                return S
    return 1


from . import switches as _switches


def _env(name, default):
    """An A/B switch (ucd_amd.switches): resolved once per process, a dict lookup afterwards (the layer code asks ~600 times per
    step)."""
    return _switches.get(name, default)


def _own_wgrad() -> bool:
    """Weight gradients on the own kernel (csrc/wgrad.hip: ucd_conv_wgrad_ex) instead of MIOpen's weight-gradient solvers / the
    batched split-M library products; ``UCD_OWN_WGRAD=0`` restores those (the A/B reference of the tests and probes)."""
    return _env("UCD_OWN_WGRAD", "1") != "0"


def _lib_gemm():
    """``ucd_amd.hip`` when its hipBLASLt entry point (tuned once per shape, ~12 us of host time per call instead of
    ~19 through the framework) can be used, else None (then the same products go through torch)."""
    from . import hip
    return hip if hip.gemm_available() else None


_node_cache = [False]


def _gemm_node():
    """ucd_amd._abn_node (C++ autograd nodes) when built and the tuned-GEMM entry point is usable, else None."""
    if _node_cache[0] is False:
        from . import abn
        mod = abn._abn_node()
        _node_cache[0] = mod if (mod is not None and hasattr(mod, "gemm1x1") and _lib_gemm() is not None) else None
    return _node_cache[0]


def _hip_stream():
    from . import hip
    return hip.stream()


def _mm_nt(rows, w):
    """rows[M, K] @ w[N, K]^T (bf16)."""
    lib = _lib_gemm() if rows.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 else None
    if lib is None:
        return rows @ w.t()
    return lib.gemm_bf16(0, rows, w, torch.empty(rows.shape[0], w.shape[0], dtype=rows.dtype, device=rows.device))


class _Gemm1x1(torch.autograd.Function):
    """rows[M, Ci] x w[Co, Ci, 1, 1]^T with the weight gradient computed as a split-K batched GEMM and returned in
    the weight's own 4-D layout (so autograd adopts it without a re-striding copy)."""

    @staticmethod
    def forward(ctx, rows, w4):
        ctx.save_for_backward(rows, w4)
        return _mm_nt(rows, w4.reshape(w4.shape[0], w4.shape[1]))

    @staticmethod
    def backward(ctx, dy):
        rows, w4 = ctx.saved_tensors
        w = w4.reshape(w4.shape[0], w4.shape[1])
        dy = dy.contiguous()
        lib = _lib_gemm() if dy.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 else None
        dx = None
        if ctx.needs_input_grad[0]:
            dx = dy @ w if lib is None else lib.gemm_bf16(1, dy, w, torch.empty_like(rows))
        dw = _conv_wgrad(dy, rows, w4, 1, WGRAD_OWN, WGRAD_SPLIT, lib) if ctx.needs_input_grad[1] else None
        return dx, dw


class Conv2d(nn.Conv2d):
    """``nn.Conv2d`` that computes with a bf16 working copy of its weight when one is attached and autocast is on
    (``ucd_amd/master.py``): no per-call cast of the fp32 master weight, no cast node in the backward.  Parameters,
    ``state_dict`` keys and the fp32 behaviour are those of ``nn.Conv2d``."""

    _w16 = None
    _w16_flip = None        # w16.flip(2, 3).transpose(0, 1) kept by ucd_amd.master.Bf16Weights (refreshed with the working copy)

    def working_weight(self):
        w = self._w16
        if w is not None and torch.is_autocast_enabled():
            return w
        return None

    def forward(self, x):
        w = self.working_weight()
        if w is None:
            return super().forward(x)
        return self._conv_forward(x, w, self.bias)


def _rows(t):
    """[B, C, H, W] map -> its [B*H*W, C] row matrix.  A view only of a dense channels-last map: every caller has checked that
    layout, or made it (``.contiguous(memory_format=torch.channels_last)``), before it hands the rows to a kernel that writes them."""
    return t.permute(0, 2, 3, 1).reshape(t.shape[0] * t.shape[2] * t.shape[3], t.shape[1])


def _w16(conv, x):
    """The layer's weight in the dtype of its input ``x``: the bf16 working copy where one is attached and autocast is on
    (``Conv2d.working_weight``), else a per-call cast of the master weight."""
    w = conv.working_weight()
    return w if w is not None else conv.weight.to(x.dtype)


def _cached_flip(conv):
    """The flipped / transposed twin ucd_amd.master.Bf16Weights keeps next to the working copy, when that copy is the weight in use."""
    return conv._w16_flip if conv.working_weight() is not None else None


def _w_matrix(w):
    """[N, K, k, k] weight in channels-last memory order -> its [N, k k K] matrix (tap-major; [N, 9 K] of a 3x3 layer), a view."""
    return _rows(w).reshape(w.shape[0], -1)


def try_index(scalar_or_list, i):
    """``x[i]`` when indexable, else ``x`` (reference ``models/util.py:1-5``)."""
    try:
        return scalar_or_list[i]
    except TypeError:
        return scalar_or_list


class _StrideOneConvFn(torch.autograd.Function):
    """Stride-1 convolution (3x3 with dilation d and padding d, or 1x1) whose INPUT gradient runs on the forward solver:
    dx = conv2d(dy, w.flip(2, 3).transpose(0, 1), padding=d, dilation=d).  Measured on MI355X with MIOpen's solver
    search (tools/dgrad_probe.py, tools/dgrad1x1_probe.py; bf16 channels-last, B = 24): the backward-data solvers take
    75 / 217 / 367 us where the forward ones take 58 / 138 / 275 us on the same problem (3x3: 256x256 at 33^2 / 512x512
    dilated / the ASPP branches), and 89 / 62 / 110 us against 43 / 32 / 73 us on the narrow 1x1 layers
    (256->64 at 129^2 / 512->128 at 65^2 / 256->128 at 129^2)."""

    @staticmethod
    def forward(ctx, x, w, d, wt=None, own_fwd=False, own_dgrad=False):
        ctx.d = d
        ctx.wt = wt          # w.flip(2, 3).transpose(0, 1), channels-last, when the caller keeps it cached (ucd_amd/master.py)
        ctx.own_dgrad = own_dgrad
        ctx.save_for_backward(x, w)
        if own_fwd:
            return _own3x3(x, w, d)
        return F.conv2d(x, w, None, 1, d * (w.shape[2] // 2), d)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        d = ctx.d
        pad = d * (w.shape[2] // 2)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            wt = ctx.wt
            if wt is None:
                wt = (w.transpose(0, 1) if w.shape[2] == 1 else w.flip(2, 3).transpose(0, 1)).contiguous(
                    memory_format=torch.channels_last)
            if ctx.own_dgrad and dy.dtype == torch.bfloat16:
                dx = _own3x3(dy.contiguous(memory_format=torch.channels_last), wt, d)
            else:
                dx = F.conv2d(dy, wt, None, 1, pad, d)
        dw = _conv_wgrad(dy, x, w, d, WGRAD_OWN, WGRAD_LIBRARY) if ctx.needs_input_grad[1] else None
        return dx, dw, None, None, None, None


# Route of a layer's weight gradient (the same values as csrc/abn_node.cpp WgradRoute): the batched split-M library products (1x1
# layers only: a 3x3 layer takes the library instead), MIOpen's weight-gradient solver, or the own kernel (csrc/wgrad.hip)
WGRAD_SPLIT, WGRAD_LIBRARY, WGRAD_OWN = 0, 1, 2


def _conv_wgrad(dz, x, w4, d, route, fallback, lib=None):
    """Weight gradient of a stride-1 convolution of dilation ``d`` (Python twin of csrc/abn_node.cpp::conv_wgrad): ``dz`` / ``x``
    the gradient of the output and the input, maps or (a 1x1 layer) [M, C] row matrices, ``w4`` the weight.  ``WGRAD_OWN`` takes the
    own kernel where the layer is one it takes and UCD_OWN_WGRAD is on, else the ``fallback`` route; the split products of an M too
    short to split run on ``lib``'s hipBLASLt entry point, or through torch when it is None.  The gradient has the weight's sizes,
    in the weight's own memory order on the own and split routes."""
    N, K, k = w4.shape[0], w4.shape[1], w4.shape[2]
    if route == WGRAD_OWN:
        if x.dim() == 2:
            ok = x.is_contiguous()
        else:
            ok = (dz.is_cuda and x.shape[2] > 1 and x.shape[3] > 1 and x.is_contiguous(memory_format=torch.channels_last)
                  and x.shape[0] * x.shape[2] * x.shape[3] < (1 << 22)
                  and (k == 1 or (tuple(w4.shape[2:]) == (3, 3) and w4.is_contiguous(memory_format=torch.channels_last))))
        if ok and _own_wgrad() and dz.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and N % 64 == 0 and K % 64 == 0:
            from . import hip
            dw = torch.empty((N, k * k * K), dtype=x.dtype, device=x.device)
            if x.dim() == 2:
                hip.conv_wgrad(dz, x, dw)
                return dw.as_strided(w4.shape, w4.stride())
            if not dz.is_contiguous(memory_format=torch.channels_last):
                dz = dz.contiguous(memory_format=torch.channels_last)
            H, W = x.shape[2], x.shape[3]
            hip.conv_wgrad(_rows(dz), _rows(x), dw, conv3=(H, W, d) if k == 3 else None)
            return dw.view(N, k, k, K).permute(0, 3, 1, 2)
        route = fallback
    if route == WGRAD_SPLIT and k == 1:
        dzr, xr = (dz, x) if x.dim() == 2 else (_rows(dz), _rows(x))
        M = dzr.shape[0]
        S = _wgrad_split(M)
        if S > 1:      # K = B*H*W is long: 8 batched chunks + a sum beat every single-kernel candidate (41 vs 96 us)
            dw = torch.bmm(dzr.view(S, M // S, N).transpose(1, 2), xr.view(S, M // S, K)).sum(0)
        elif lib is None:
            dw = dzr.t() @ xr
        else:
            dw = lib.gemm_bf16(2, dzr, xr, torch.empty(N, K, dtype=dz.dtype, device=dz.device))
        return dw.as_strided(w4.shape, w4.stride())     # [N, K, 1, 1] is one memory order in either format
    return torch.ops.aten.convolution_backward(dz, x, w4, None, [1, 1], [d * (k // 2)] * 2, [d, d], False, [0, 0], 1,
                                               [False, True, False])[1]


def _own3x3(x, w, d):
    """3x3 convolution (stride 1, padding = dilation d) of a dense channels-last bf16 map on the implicit-GEMM kernel; ``w``
    [N, K, 3, 3] in channels-last memory order."""
    from . import hip
    B, K, H, W = x.shape
    N = w.shape[0]
    y = torch.empty((B, N, H, W), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    hip.conv1x1(_rows(x), _w_matrix(w), _rows(y), conv3=(H, W, d))
    return y


def _own3x3_ok(conv, x):
    """Can this stand-alone 3x3 layer (the ASPP branches) run on the own kernel at all (layout / alignment)?"""
    return (x.is_cuda and x.dim() == 4 and x.dtype == torch.bfloat16 and conv.bias is None and conv.stride == (1, 1)
            and conv.padding == conv.dilation and conv.dilation[0] == conv.dilation[1] and conv.groups == 1
            and conv.in_channels % 64 == 0 and conv.out_channels % 64 == 0 and x.shape[2] > 1 and x.shape[3] > 1
            and x.is_contiguous(memory_format=torch.channels_last) and _env("UCD_FUSED_CONV1X1", "1") != "0")


def _stride_one_conv(x, w, d, wt=None, own_fwd=False, own_dgrad=False):
    """The C++ autograd node when built (no Python in the backward), else the Python Function: same library calls."""
    from . import abn
    node = abn._abn_node()
    if node is not None and hasattr(node, "conv_stride1"):
        return node.conv_stride1(x, w, d, wt, bool(own_fwd), bool(own_dgrad), _hip_stream(), _own_wgrad())
    return _StrideOneConvFn.apply(x, w, d, wt, bool(own_fwd), bool(own_dgrad))


def _own_f32_conv(M, K, N, taps):
    """Shape gate of the fp32 split-bf16 kernels (csrc/conv_f32.hip) against MIOpen fp32, a pure function of the product's shape:
    M = B*H*W rows, K -> N channels, taps 1 (1x1) or 9 (3x3).  Channels on the kernels' grid (multiples of 32, at least 64) and
    maps that give the chip some tiles (M >= 1024: the image-pooling branch's [B, C, 1, 1] products stay on the library).  Measured
    per shape at B = 24 (tools/conv_f32_probe.py, profiles/r07_conv_f32_probe.txt, forward / input gradient us, own vs MIOpen
    fp32): 1.1 - 2.5x faster on every stride-1 layer (ASPP branches 774 - 860 vs 1753 - 1772, 2048 -> 512 239 vs 472, 3x3
    128 -> 128 at 65^2 128 vs 283) except the 64 -> 64 1x1 layer at 129^2 (51.5 vs 43.7 forward, 54.3 vs 54.7 input gradient),
    which stays on the library.  Measured at B = 24 only; the gate applies the same verdict at any M >= 1024.  The weight gradient
    has a gate of its own (``_own_f32_wgrad``)."""
    if not (taps in (1, 9) and K % 32 == 0 and N % 32 == 0 and K >= 64 and N >= 64 and M >= 1024):
        return False
    return not (taps == 1 and K == 64 and N == 64)


def _own_f32_wgrad(M, K, N, taps):
    """Weight gradient of a layer that passed ``_own_f32_conv``: on ucd_conv_f32_wgrad when both channel counts fill the 128-wide
    tile; the 64-channel layers (129^2: 64 -> 256 173 vs 141 us, 256 -> 64 180 vs 143, 3x3 64 -> 64 666 vs 303;
    profiles/r07_conv_f32_probe.txt) keep MIOpen's weight-gradient solvers.  Every other shape of that table is 1.25 - 1.95x
    faster on the own kernel (2048 -> 512 224 vs 436, ASPP branches 1319 - 1409 vs 1807 - 1811).  Measured at B = 24 only; the
    gate applies the same verdict at any M >= 1024."""
    return _own_f32_conv(M, K, N, taps) and min(K, N) >= 128


def _f32_conv_ok(conv, x):
    """Does this stride-1 layer call run on the fp32 split-bf16 kernels?  ``UCD_F32_OWN_CONV=1`` and a channels-last fp32 GPU map
    with a 16-byte aligned base and autocast off, no bias, stride 1, 1x1 with padding 0 or 3x3 with padding = dilation, and the
    shape gate ``_own_f32_conv``."""
    if _env("UCD_F32_OWN_CONV", "0") != "1":
        return False
    if not (x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and not torch.is_autocast_enabled() and conv.bias is None
            and conv.weight.dtype == torch.float32 and conv.groups == 1 and conv.stride == (1, 1)
            and x.is_contiguous(memory_format=torch.channels_last) and not (x.data_ptr() & 15)):
        return False
    if conv.kernel_size == (1, 1):
        if conv.padding != (0, 0):
            return False
        taps = 1
    elif conv.kernel_size == (3, 3) and conv.padding == conv.dilation and conv.dilation[0] == conv.dilation[1]:
        taps = 9
    else:
        return False
    return _own_f32_conv(x.shape[0] * x.shape[2] * x.shape[3], conv.in_channels, conv.out_channels, taps)


def _f32_rows(t):
    """[B, C, H, W] fp32 map -> its channels-last [B*H*W, C] row matrix (a view of a channels-last tensor, else a copy)."""
    return _rows(t.contiguous(memory_format=torch.channels_last))


def _f32_conv_fwd(x, w, d):
    """y = conv2d(x, w, stride 1, padding d, dilation d) (d = 0: 1x1) on ucd_conv_f32; y channels-last fp32."""
    from . import hip
    B, K, H, W = x.shape
    N = w.shape[0]
    y = torch.empty((B, N, H, W), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    wm = _w_matrix(w)                                    # [N, taps K] in the weight's channels-last order
    if wm.stride(1) != 1 or (wm.data_ptr() & 15):
        wm = wm.contiguous()
    hip.conv_f32(_f32_rows(x), wm, _f32_rows(y), conv3=(H, W, d) if d > 0 else None)
    return y


class _F32ConvFn(torch.autograd.Function):
    """fp32 stride-1 convolution (1x1, or 3x3 with padding = dilation d) with forward, input gradient and weight gradient on the
    split-bf16 kernels (csrc/conv_f32.hip; ~1e-5 relative per product; the weight gradient of the 64-channel layers on MIOpen,
    ``_own_f32_wgrad``).  Like ``_StrideOneConvFn`` the input gradient is the
    forward product on the rearranged weight: w^T (1x1) or w.flip(2, 3).transpose(0, 1) (3x3)."""

    @staticmethod
    def forward(ctx, x, w, d):
        ctx.d = d
        ctx.save_for_backward(x, w)
        return _f32_conv_fwd(x, w, d)

    @staticmethod
    def backward(ctx, dy):
        from . import hip
        x, w = ctx.saved_tensors
        d = ctx.d
        dy = dy.contiguous(memory_format=torch.channels_last)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            wt = (w.transpose(0, 1) if d == 0 else w.flip(2, 3).transpose(0, 1)).contiguous(memory_format=torch.channels_last)
            dx = _f32_conv_fwd(dy, wt, d)
        if ctx.needs_input_grad[1]:
            B, K, H, W = x.shape
            N = w.shape[0]
            k = 3 if d > 0 else 1
            if _own_f32_wgrad(B * H * W, K, N, k * k):
                dwm = torch.empty((N, k * k * K), dtype=torch.float32, device=x.device)
                hip.conv_f32_wgrad(_f32_rows(dy), _f32_rows(x), dwm, conv3=(H, W, d) if d > 0 else None)
                dw = dwm.view(N, k, k, K).permute(0, 3, 1, 2)
                if not w.is_contiguous(memory_format=torch.channels_last):
                    dw = dw.contiguous()
            else:
                dl = max(d, 1)
                dw = torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [d, d], [dl, dl], False, [0, 0], 1,
                                                         [False, True, False])[1]
        return dx, dw, None


def _f32_conv(conv, x):
    """The layer on the fp32 split-bf16 kernels (after ``_f32_conv_ok``): autograd node when anything needs a gradient, else the
    plain forward (the frozen teacher)."""
    d = conv.dilation[0] if conv.kernel_size == (3, 3) else 0
    if torch.is_grad_enabled() and (x.requires_grad or conv.weight.requires_grad):
        return _F32ConvFn.apply(x, conv.weight, d)
    return _f32_conv_fwd(x, conv.weight, d)


class Conv3x3(Conv2d):
    """3x3, stride 1, padding = dilation: the bottleneck conv2 layers and the ASPP branches (modules/residual.py:69,
    modules/deeplab.py:27-29).  Same parameters and state_dict keys as nn.Conv2d."""

    def forward(self, x):
        if _f32_conv_ok(self, x):
            return _f32_conv(self, x)
        # forward and input gradient on the own kernel wherever the layout allows it
        own = _own3x3_ok(self, x) and self.weight.is_contiguous(memory_format=torch.channels_last)
        if (x.is_cuda and torch.is_grad_enabled() and self.weight.requires_grad and self.bias is None
                and x.dtype == torch.bfloat16 and _env("UCD_DGRAD_VIA_FWD", "1") != "0"):
            w = _w16(self, x)               # the working copy has the master weight's layout; so has a cast
            return _stride_one_conv(x, w, self.dilation[0], _cached_flip(self),
                                    own and w.is_contiguous(memory_format=torch.channels_last), own)
        if own and not torch.is_grad_enabled():
            w = _w16(self, x)                              # the frozen teacher's ASPP branches
            if w.is_contiguous(memory_format=torch.channels_last):
                return _own3x3(x, w, self.dilation[0])
        return super().forward(x)


class Conv1x1(Conv2d):
    """1x1 stride-1 convolution with the reference's parameter shape ([Cout, Cin, 1, 1]).  On the GPU every layer with
    64-aligned channel counts runs as a product on the channels-last row matrix [B*H*W, Cin] x [Cin, Cout] instead of an
    MIOpen implicit-GEMM convolution: inside ``_conv_abn_train`` / the teacher's fused blocks on the own kernel
    (csrc/conv1x1.hip) with the ABN work in its epilogue, called on its own through the tuned library GEMM (measured on
    MI355X, tools/gemm_vs_conv_probe.py / conv1x1_probe.py, bf16, B = 24: the library 1.2x faster than MIOpen at 1024<->256,
    1.5-1.7x at 2048<->512, 2.4x at 1024->2048; the own kernel 1.4-2.1x faster than MIOpen on the narrow layers).  Layers
    off the 64 grid (the classifier heads) stay with MIOpen."""

    def __init__(self, in_channels, out_channels, bias=False):
        super().__init__(in_channels, out_channels, 1, stride=1, padding=0, bias=bias)
        # wide: the tuned library GEMM beats MIOpen's convolution (docstring); as_gemm: the layer runs on the row matrix at all -
        # the narrow 64-aligned layers too since the own kernel exists (tools/conv1x1_probe.py: 256->64 at 129^2 39 us against
        # 55 us hipBLASLt and 61 us MIOpen; 64->256 41 / 54 / 86; 512->128 at 65^2 25 / 29 / 44; 128->512 28 / 36 / 50)
        self.wide = min(in_channels, out_channels) >= 256 and max(in_channels, out_channels) >= 1024
        self.as_gemm = self.wide or (in_channels % 64 == 0 and out_channels % 64 == 0)
        # input gradient d x = d z . w (a GEMM with K = Co, N = Ci) through the own kernel on the cached transposed weight where
        # it beats the library: short K (tools/conv1x1_probe.py: 256 -> 1024 22.8 vs 31.3 us, the narrow layers 25-41 vs 29-54)
        self.own_dgrad = (in_channels % 64 == 0 and out_channels % 64 == 0 and out_channels <= 512
                          and in_channels * out_channels <= (1 << 18))
        # set by ResidualBlock for a layer whose input comes from a conv+ABN node that feeds nothing else: its input-gradient
        # product then also does that ABN's backward reduction (out_mode 3, ``_conv_abn_train``) - worth the own kernel on the
        # transposed weight even where the plain library product is a little faster
        self.link_dgrad = False

    def forward(self, x):
        if _f32_conv_ok(self, x):          # UCD_F32_OWN_CONV=1: the fp32 mode's layers on csrc/conv_f32.hip
            return _f32_conv(self, x)
        # bf16 activations only: in the fp32 parity mode (--opt_level O0) every convolution stays on one code
        # path (MIOpen), which is what the 1e-3 logit comparison with the reference was validated on
        if not (self.as_gemm and x.is_cuda and x.dim() == 4 and (x.dtype != torch.float32 or torch.is_autocast_enabled())):
            if (x.is_cuda and x.dim() == 4 and x.dtype == torch.bfloat16 and torch.is_grad_enabled() and self.bias is None
                    and self.weight.requires_grad and x.shape[0] * x.shape[2] * x.shape[3] >= 8192
                    and _env("UCD_DGRAD_VIA_FWD", "1") != "0"):
                return _stride_one_conv(x, _w16(self, x), 1, _cached_flip(self))                  # narrow layer: MIOpen
            return super().forward(x)
        B, C, H, W = x.shape
        rows = _rows(x.contiguous(memory_format=torch.channels_last))      # a view of a channels-last tensor
        if self.bias is None and rows.dtype != torch.float32 and torch.is_grad_enabled() and self.weight.requires_grad:
            w4 = _w16(self, rows)
            node = _gemm_node() if rows.dtype == torch.bfloat16 else None
            if node is not None:          # same library calls, autograd node in C++ (host time per layer 71 -> ~25 us)
                y = node.gemm1x1(rows, w4, _hip_stream(), _own_wgrad())
            else:
                y = _Gemm1x1.apply(rows, w4)
        else:
            w16 = self.working_weight()
            w = w16 if (w16 is not None and rows.dtype == w16.dtype) else self.weight
            w = w.reshape(self.out_channels, C)
            if self.bias is None and not torch.is_grad_enabled() and rows.dtype == torch.bfloat16:
                y = _mm_nt(rows, w if w.dtype == rows.dtype else w.to(rows.dtype))      # the frozen teacher
            else:
                y = F.linear(rows, w, self.bias)
        return y.view(B, H, W, self.out_channels).permute(0, 3, 1, 2)


def _conv1_with_skip(conv, x):
    """(conv(x), x') for the first 1x1 convolution of an identity-shortcut block, x' an alias of x to use as the residual:
    the C++ node folds the shortcut's gradient into the input-gradient GEMM (dx = dskip + dy w, beta = 1) instead of
    leaving a separate 3-pass add to autograd.  None when that path does not apply (then the caller does the usual)."""
    if not (isinstance(conv, Conv1x1) and conv.as_gemm and conv.bias is None and x.is_cuda and x.dim() == 4
            and x.dtype == torch.bfloat16 and torch.is_grad_enabled() and conv.weight.requires_grad and x.requires_grad):
        return None
    node = _gemm_node()
    if node is None or not hasattr(node, "gemm1x1_skip"):
        return None
    B, C, H, W = x.shape
    if not x.is_contiguous(memory_format=torch.channels_last):
        return None
    y, skip = node.gemm1x1_skip(_rows(x), _w16(conv, x), _hip_stream(), _own_wgrad())
    return (y.view(B, H, W, conv.out_channels).permute(0, 3, 1, 2), skip.view(B, H, W, C).permute(0, 3, 1, 2))


def _is_fused_abn(m) -> bool:
    return getattr(m, "ucd_fused_abn", False)


def _own_stride(conv):
    """The stride s > 1 of a layer the own strided kernels take (csrc/conv1x1.hip ``stride``, csrc/wgrad.hip STR): the first
    block of a stage - conv2 3x3 with padding = dilation and proj_conv 1x1 with padding 0 (modules/residual.py:57-82), 128-aligned
    channels - else 0.  MIOpen needs 209-263 us for each of the four forward products at B = 24 (tools/aten_ops.py), 5-15x their
    traffic / MFMA time.  ``UCD_OWN_STRIDED=0`` keeps the library (A/B)."""
    if not (isinstance(conv, Conv2d) and conv.stride[0] == conv.stride[1] and conv.stride[0] > 1 and conv.groups == 1
            and conv.in_channels % 128 == 0 and conv.out_channels % 128 == 0 and _env("UCD_OWN_STRIDED", "1") != "0"):
        return 0
    if conv.kernel_size == (1, 1) and conv.padding == (0, 0):
        return conv.stride[0]
    if conv.kernel_size == (3, 3) and conv.padding == conv.dilation and conv.dilation[0] == conv.dilation[1]:
        return conv.stride[0]
    return 0


LINK_CHAIN, LINK_BLOCK = 1, 3     # csrc/abn_node.cpp Link::Kind


class Link(NamedTuple):
    """The backward link a conv + ABN node offers on its output (csrc/abn_node.cpp: offer / serve / claim): the producer's ``z``,
    statistics buffer, bias, ``partial`` and flag, its activation code and slope.  ``LINK_CHAIN`` hangs on the output as
    ``_ucd_link`` (the one consumer is the next conv + ABN node), ``LINK_BLOCK`` as ``_ucd_blink`` (the producer is the last node of a
    residual block, the consumer the first convolution + shortcut of the next; ``bias`` None, ``act`` 0: the block activation)."""
    z: torch.Tensor
    buf: torch.Tensor
    bias: object
    partial: torch.Tensor
    flag: object
    act: int
    slope: float
    kind: int


def _offer_link(y, z, buf, bias, partial, flag, act, slope, block):
    if block:
        y._ucd_blink = Link(z, buf, None, partial, flag, 0, float(slope), LINK_BLOCK)
    else:
        y._ucd_link = Link(z, buf, bias, partial, flag, int(act), float(slope), LINK_CHAIN)


class _ConvABNFunction(torch.autograd.Function):
    """Python twin of csrc/abn_node.cpp::ConvABNTrainNode (single process; the node adds the SyncBN exchange and the
    shortcut fold): z = x . w^T with the statistics in the GEMM epilogue -> finalize -> y = act(norm(z) [+ residual]).
    The complete implementation and the fallback; bench.py's instrumented pass runs it (every library call visible)."""

    @staticmethod
    def forward(ctx, x, w4, weight, bias, residual, running_mean, running_var, momentum, eps, act, slope, dilation=0, wflip=None,
                own_dgrad=False, wgrad_conv=False, make_link=False, link=None, with_skip=False):
        from . import hip
        B, K, H, W = x.shape
        N = w4.shape[0]
        M, HW = B * H * W, H * W
        z = torch.empty((B, N, H, W), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        y = torch.empty_like(z)
        buf = torch.empty(6 * N, dtype=torch.float32, device=x.device)
        conv3 = dilation > 0
        w2 = _w_matrix(w4) if conv3 else w4.reshape(N, K)
        ctx.conv3 = (dilation, wflip, own_dgrad, wgrad_conv)
        ctx.link = link                                 # the Link consumed (see ConvABNTrainNode), or None
        ctx.my_link = None
        part = hip.conv1x1_stats_partial(M, N, x.device)
        hip.conv1x1(_rows(x), w2, _rows(z), out_mode=2, partial=part, conv3=(H, W, dilation) if conv3 else None)
        hip.conv1x1_stats_finalize(part, M, N, weight, running_mean, running_var, momentum, eps, buf, None, act)
        hip.abn_apply(z, N, y, N, residual, N if residual is not None else 0, M, N, None, HW, buf[3 * N:4 * N], buf[5 * N:],
                      bias, act, slope)
        needs_y = residual is not None and (act & hip.ACT_MASK) != hip.ACT_IDENTITY
        ctx.save_for_backward(x, w4, z, y if needs_y else None, weight, bias, buf)
        ctx.cfg = (act, slope, residual is not None)
        if make_link and bias is not None and (act & hip.ACT_MASK) != hip.ACT_ELU and (residual is None or needs_y):
            partial = torch.empty(hip.conv1x1_row_tiles(M), 2, N, dtype=torch.float32, device=x.device)
            ctx.my_link = (partial, [0, 0, 0])   # {served, address of the consumer's dx, its version} (see LinkFlag in csrc/abn_node.cpp)
            _offer_link(y, z, buf, bias, partial, ctx.my_link[1], act, slope, block=residual is not None)
        if with_skip:
            return y, x.view_as(x)
        return y

    @staticmethod
    def backward(ctx, dy, dskip=None):
        from . import hip
        x, w4, z, y, weight, bias, buf = ctx.saved_tensors
        act, slope, has_res = ctx.cfg
        B, K, H, W = x.shape
        N = w4.shape[0]
        M, HW = B * H * W, H * W
        if ctx.my_link is not None and ctx.my_link[1][0] == 1 and (dy.data_ptr() != ctx.my_link[1][1]
                                                                   or dy._version != ctx.my_link[1][2]):
            ctx.my_link[1][0] = 0
            raise RuntimeError("ucd conv+abn node: the backward link was served but the gradient that arrived is not the consumer's "
                               "input gradient - the linked map has a second consumer (hook, ret_intermediate tap, retain_graph "
                               "replay).  Run with UCD_BWD_LINK=0.")
        dy_in = dy
        dy, _, _, _, _ = hip.rows_view(dy if dy.dtype == x.dtype else dy.to(x.dtype))
        dz = torch.empty_like(z)
        linked = ctx.my_link is not None and ctx.my_link[1][0] == 1
        dres = torch.empty_like(z) if (has_res and not linked) else None
        sums = torch.empty(2 * N, dtype=torch.float32, device=x.device)
        if linked:
            # the consumer's input-gradient product applied the activation derivative and left the sums as per-tile partials
            ctx.my_link[1][0] = 0
            part = ctx.my_link[0]
            hip._check(hip.load().ucd_abn_reduce_partials(hip.ptr(part), part.shape[0], N, hip.ptr(sums), None, hip.ptr(weight),
                                                          act & hip.NORM_ABS_GAMMA, hip.stream()), "ucd_abn_reduce_partials")
            hip.abn_bwd_apply(z, N, dy, N, None, 0, dz, N, None, 0, M, N, None, HW, buf[3 * N:4 * N], buf[4 * N:5 * N], buf[5 * N:],
                              bias, weight, sums, float(M), 0, hip.ACT_IDENTITY | (act & hip.NORM_ABS_GAMMA), 0.0)
            if has_res:
                dres = dy_in            # block link: dy IS d pre, and so is the shortcut's gradient
        else:
            hip.abn_backward(z, N, dy, N, y, N if y is not None else 0, dz, N, dres, N if has_res else 0, M, N, None, HW,
                             buf[3 * N:4 * N], buf[4 * N:5 * N], buf[5 * N:], bias, weight, sums, float(M), True, True, act, slope)
        dilation, wflip, own_dgrad, wgrad_conv = ctx.conv3
        link = ctx.link

        def serve(dx):     # the producer's backward reduction as the epilogue of the product that writes dx; marks the link served
            C = link.z.shape[1]
            link.flag[:3] = 1, dx.data_ptr(), dx._version
            mean, invstd = link.buf[3 * C:4 * C], link.buf[4 * C:5 * C]
            if link.kind == LINK_BLOCK:        # out_mode 4 against the block in front
                return dict(out_mode=4, out_norm=(mean, None, None, invstd, hip.ACT_LEAKY_RELU, link.slope), residual=_rows(x),
                            side2=_rows(link.z), partial=link.partial)
            return dict(out_mode=3, out_norm=(mean, link.buf[5 * C:], link.bias, invstd, link.act & hip.ACT_MASK, link.slope),
                        residual=_rows(link.z), partial=link.partial)
        dx = None
        if dilation > 0:
            if ctx.needs_input_grad[0]:
                if wflip is None:
                    wflip = w4.flip(2, 3).transpose(0, 1).contiguous(memory_format=torch.channels_last)
                if own_dgrad:
                    dx = torch.empty_like(x)
                    hip.conv1x1(_rows(dz), _w_matrix(wflip), _rows(dx), conv3=(H, W, dilation),
                                **(serve(dx) if link is not None else {}))
                else:
                    dx = F.conv2d(dz, wflip, None, 1, dilation, dilation)
        elif ctx.needs_input_grad[0]:
            fold = (dskip is not None and dskip.dtype == x.dtype
                    and dskip.is_contiguous(memory_format=torch.channels_last) and own_dgrad and wflip is not None)
            dx = dskip if fold else torch.empty_like(x)
            if own_dgrad and wflip is not None:
                # a chain link needs dx to be the whole gradient; a block link also takes the shortcut's folded in
                served = link is not None and (dskip is None or (fold and link.kind == LINK_BLOCK))
                hip.conv1x1(_rows(dz), wflip.reshape(K, N), _rows(dx), accumulate=fold, **(serve(dx) if served else {}))
            else:
                hip.gemm_bf16(1, _rows(dz), w4.reshape(N, K), _rows(dx))
            if dskip is not None and not fold:
                dx = dx + dskip
        # the own kernel's fallback is MIOpen here, where the C++ node falls back to the split products on a 1x1 layer
        dw = _conv_wgrad(dz, x, w4, dilation or 1, wgrad_conv, WGRAD_LIBRARY) if ctx.needs_input_grad[1] else None
        return (dx, dw, sums[N:], sums[:N], dres) + (None,) * 13


class _Route(NamedTuple):
    """What ``_conv_abn_route`` decided for one conv + ABN pair (the arguments of the node of the same names)."""
    is3: bool
    stride: int          # 0: not one of the own strided layers
    dilation: int
    own_dgrad: bool
    wflip: object        # the cached flipped / transposed bf16 weight, where there is one
    wgrad_conv: int
    link: object         # the Link this node may serve, or None
    make_link: bool


def _conv_abn_route(conv, bn, x, residual, with_skip, make_link):
    """Is the pair eligible for the one-node path, and on which kernels does it run?  None: the module path."""
    if _env("UCD_FUSED_CONV1X1", "1") == "0":
        return None
    links = _env("UCD_BWD_LINK", "1") != "0"
    block_links = links and _env("UCD_BLOCK_LINK", "1") != "0"      # UCD_BLOCK_LINK=0 switches only this kind off
    # x is the output of a conv + ABN node (chain link) or, for the first convolution of an identity-shortcut block, of the residual
    # block in front (block link), which offers its backward reduction to this node's input-gradient product (csrc/abn_node.cpp)
    link = getattr(x, "_ucd_blink", None) if (with_skip and block_links) else None
    if link is None and links:
        link = getattr(x, "_ucd_link", None)
    make_link = bool(make_link and (links if residual is None else block_links))
    is3 = isinstance(conv, Conv3x3)
    stride = _own_stride(conv) if not (with_skip or residual is not None) else 0
    if stride:
        is3 = conv.kernel_size == (3, 3)
    if not ((is3 or stride or (isinstance(conv, Conv1x1) and conv.as_gemm)) and conv.bias is None and conv.weight.requires_grad
            and _is_fused_abn(bn) and bn.training and bn.weight is not None and torch.is_grad_enabled() and x.is_cuda
            and x.dim() == 4 and x.dtype == torch.bfloat16 and conv.in_channels % 64 == 0 and conv.out_channels % 64 == 0):
        return None
    dilation, wflip, own_dgrad, wgrad_conv = 0, None, False, WGRAD_LIBRARY
    if stride:
        # the strided layers of a stage's first block: forward (+ statistics) and weight gradient on the own kernels, the input
        # gradient stays with the library's backward-data solver; no link consumed (the producer falls back to its own reduction)
        if is3 and not conv.weight.is_contiguous(memory_format=torch.channels_last):
            return None
        dilation, link = (conv.dilation[0] if is3 else 0), None
    elif is3:
        if not (conv.stride == (1, 1) and conv.padding == conv.dilation and conv.dilation[0] == conv.dilation[1]
                and conv.groups == 1 and not with_skip and conv.weight.is_contiguous(memory_format=torch.channels_last)):
            return None
        dilation, own_dgrad, wflip = conv.dilation[0], True, _cached_flip(conv)
    else:
        own_dgrad = conv.own_dgrad or (link is not None and conv.link_dgrad and (link.kind == LINK_BLOCK or not with_skip))
        # the transposed weight: cached with the bf16 working copies, else made per call (same kernels either way)
        wflip = _cached_flip(conv) if own_dgrad else None
        # narrow layers (<= 512 channels at 65^2 / 129^2): MIOpen's weight-gradient solver beats the split-M products
        wgrad_conv = WGRAD_SPLIT if conv.wide else WGRAD_LIBRARY
    if _own_wgrad():
        wgrad_conv = WGRAD_OWN
    # the consumer's input gradient must run on the own kernel; a chain link wants no shortcut next to it, a block link a 1x1 layer
    if link is not None and (not own_dgrad or (is3 if link.kind == LINK_BLOCK else with_skip)):
        link = None
    return _Route(is3, stride, dilation, bool(own_dgrad), wflip, int(wgrad_conv), link, make_link)


def _conv_abn_train(conv, bn, x, residual=None, activation=None, activation_param=None, with_skip=False, make_link=False):
    """``bn(conv(x) [, residual])`` of a wide 1x1 convolution and a training-mode HIP ABN as ONE autograd node
    (csrc/abn_node.cpp::ConvABNTrainNode): the ABN's batch statistics come out of the GEMM's epilogue.  Returns None when the
    pair is not eligible (the caller then runs the modules one after the other), else ``y`` or ``(y, shortcut alias of x)``.
    ``make_link``: the caller promises that ``y`` feeds exactly one further ``_conv_abn_train`` call and nothing else; ``y`` then
    carries the link (``y._ucd_link``) through which that consumer's input-gradient product does this ABN's backward reduction
    in its epilogue (csrc/abn_node.cpp; under SyncBN the producer all-reduces the combined sums; ``UCD_BWD_LINK=0`` switches it
    off)."""
    r = _conv_abn_route(conv, bn, x, residual, with_skip, make_link)
    if r is None:
        return None
    from . import abn as _abn
    from . import hip
    node = _gemm_node()
    if node is None or not hasattr(node, "conv_abn_train"):
        # no C++ node (not built, or switched off by bench.py's instrumented pass): the Python twin, single process only and
        # without a strided form (the module path)
        node = None
        dense = lambda t: t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last) and t.shape[2] > 1 and t.shape[3] > 1
        if (r.stride or _lib_gemm() is None or _abn._group_size(bn._group()) > 1 or not dense(x)
                or (residual is not None and not (dense(residual) and residual.dtype == x.dtype))):
            return None
    else:
        if not node.dense_channels_last(x):
            return None
        if residual is not None and not (residual.dtype == x.dtype and node.dense_channels_last(residual)):
            return None
        group = bn._group()
        world = _abn._group_size(group)
        sync = group is not False and (world > 1 or (_abn._FORCE_SYNC and torch.distributed.is_initialized()))
        comm = _abn.direct_comm(group) if sync else None
        if sync and comm is None:
            return None
    w16 = _w16(conv, x)
    wflip = r.wflip
    if r.own_dgrad and not r.is3 and wflip is None:
        wflip = w16.reshape(conv.out_channels, conv.in_channels).t().contiguous().view(conv.in_channels, conv.out_channels, 1, 1)
    act = _abn._act_code(bn.activation if activation is None else activation) | (hip.NORM_ABS_GAMMA if bn._abs_gamma else 0)
    slope = bn.activation_param if activation_param is None else activation_param
    bn.__dict__.pop("_eval_cache", None)
    if node is None:
        return _ConvABNFunction.apply(x, w16, bn.weight, bn.bias, residual, bn.running_mean, bn.running_var, bn.momentum, bn.eps,
                                      act, slope, r.dilation, wflip, r.own_dgrad, r.wgrad_conv, r.make_link, r.link,
                                      bool(with_skip))
    out = node.conv_abn_train(x, w16, bn.weight, bn.bias, residual, bn.running_mean, bn.running_var, bn.momentum, bn.eps, act,
                              slope, comm.handle if comm is not None else 0, world, _hip_stream(), bn._direct_grad_ptr(),
                              bool(with_skip), r.dilation, wflip, r.own_dgrad, r.wgrad_conv, r.make_link, r.link,
                              r.stride or 1, _env("UCD_STAT_ATOMIC", "1") != "0")
    k = 2 if with_skip else 1
    if len(out) > k:                             # the node made a link: (z, buf, partial, flag) follow the regular outputs
        _offer_link(out[0], out[k], out[k + 1], bn.bias, out[k + 2], out[k + 3], act, slope, block=residual is not None)
    return (out[0], out[1]) if with_skip else out[0]


def _apply_act(x, activation, param):
    if activation == "leaky_relu":
        return F.leaky_relu(x, negative_slope=param, inplace=True)
    if activation == "elu":
        return F.elu(x, alpha=param, inplace=True)
    if activation == "identity":
        return x
    raise RuntimeError(f"unknown activation {activation!r}")


class ResidualBlock(nn.Module):
    """``channels`` of length 3 -> bottleneck 1x1 / 3x3(stride, dilation) / 1x1, length 2 -> basic
    3x3 / 3x3.  The last norm of the block is created like the others and then switched to
    ``activation = "identity"`` (reference ``residual.py:52,65``); the projection shortcut exists
    when the stride or the channel count changes (``residual.py:48,79-82``).
    """

    def __init__(self, in_channels, channels, stride=1, dilation=1, groups=1,
                 norm_act=nn.BatchNorm2d, dropout=None):
        super().__init__()
        if len(channels) not in (2, 3):
            raise ValueError("channels must contain either two or three values")
        if len(channels) == 2 and groups != 1:
            raise ValueError("groups > 1 are only valid if len(channels) == 3")

        def conv(cin, cout, k, s=1, g=1):
            if k == 1 and s == 1 and g == 1:
                return Conv1x1(cin, cout)
            pad = dilation if k == 3 else 0
            if k == 3 and s == 1 and g == 1:
                return Conv3x3(cin, cout, 3, stride=1, padding=dilation, dilation=dilation, bias=False)
            return Conv2d(cin, cout, k, stride=s, padding=pad, dilation=dilation if k == 3 else 1,
                             groups=g, bias=False)

        if len(channels) == 3:
            spec = [(1, 1, 1), (3, stride, groups), (1, 1, 1)]
        else:
            spec = [(3, stride, 1), (3, 1, 1)]
        layers, cin = [], in_channels
        for i, ((k, s, g), cout) in enumerate(zip(spec, channels), 1):
            layers.append((f"conv{i}", conv(cin, cout, k, s, g)))
            layers.append((f"bn{i}", norm_act(cout)))
            if dropout is not None and i == len(spec) - 1:
                layers.append(("dropout", dropout()))
            cin = cout
        layers[-1][1].activation = "identity"
        self.convs = nn.Sequential(OrderedDict(layers))
        self._last_bn = f"bn{len(spec)}"
        c3 = getattr(self.convs, "conv3", None)
        if (isinstance(c3, Conv1x1) and isinstance(getattr(self.convs, "conv2", None), Conv3x3) and c3.in_channels % 64 == 0
                and c3.out_channels % 64 == 0 and c3.out_channels <= 1024):
            c3.link_dgrad = True          # conv2 + bn2 -> conv3: bn2's backward reduction rides on conv3's input gradient

        c1 = getattr(self.convs, "conv1", None)
        if (stride == 1 and in_channels == channels[-1] and isinstance(c1, Conv1x1) and len(channels) == 3
                and c1.in_channels % 64 == 0 and c1.out_channels % 64 == 0):
            # identity shortcut: conv1's input-gradient product (with the shortcut's gradient folded in) forms the gradient
            # w.r.t. the previous block's output - the block link has it do that block's bn3 backward reduction too, which
            # needs the own kernel on the cached transposed weight
            c1.link_dgrad = True

        if stride != 1 or in_channels != channels[-1]:
            self.proj_conv = (Conv1x1(in_channels, channels[-1]) if stride == 1 else
                              Conv2d(in_channels, channels[-1], 1, stride=stride, padding=0, bias=False))
            self.proj_bn = norm_act(channels[-1])
            self.proj_bn.activation = "identity"

    # -- frozen-statistics forward (the teacher): each 1x1 convolution and the ABN that follows it are ONE kernel ----------
    def _eval_fusable(self, x):
        c = self.convs
        if not (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4 and len(c) >= 6 and hasattr(c, "conv3")):
            return False
        if not (isinstance(c.conv1, Conv1x1) and isinstance(c.conv3, Conv1x1) and c.conv1.bias is None and c.conv3.bias is None):
            return False
        norms = [c.bn1, c.bn2, c.bn3] + ([self.proj_bn] if hasattr(self, "proj_conv") else [])
        if not all(_is_fused_abn(m) and m.activation in ("leaky_relu", "identity") and m.weight is not None for m in norms):
            return False
        chans = (c.conv1.in_channels, c.conv1.out_channels, c.conv3.in_channels, c.conv3.out_channels)
        st = x.stride()
        return (all(v % 64 == 0 for v in chans) and "dropout" not in c._modules
                and st[1] == 1 and st[3] == x.shape[1] and _env("UCD_FUSED_CONV1X1", "1") != "0")

    @staticmethod
    def _eval_norm(m, act=None, slope=None):
        """(mean, scale, shift, invstd, act code, slope) of an ABN layer under its running statistics."""
        from . import hip
        consts = m._eval_constants()
        a = m.activation if act is None else act
        return (m.running_mean, consts[1], m.bias, None, hip.ACT_CODES[a], m.activation_param if slope is None else slope)

    def _forward_eval_fused(self, x):
        """Every convolution with the ABN behind it as ONE product with the affine + activation epilogue (csrc/conv1x1.hip): conv1 +
        bn1, conv2 + bn2 (3x3 implicit GEMM; stride 1, or the stride of a stage's first block), the projection + proj_bn likewise,
        conv3 + bn3 + shortcut + block activation.  A conv2 / projection the kernels do not take runs its modules.  Same arithmetic as
        the layer-by-layer path with the conv outputs kept in fp32 up to the activation."""
        from . import hip
        c = self.convs
        B, C, H, W = x.shape
        cl = torch.channels_last

        def new_map(channels, stride=1):
            return torch.empty((B, channels, (H - 1) // stride + 1, (W - 1) // stride + 1), dtype=x.dtype, device=x.device,
                               memory_format=cl)

        def w2d(conv):
            return _w16(conv, x).reshape(conv.out_channels, conv.in_channels)

        xr = _rows(x)
        h1 = new_map(c.conv1.out_channels)
        hip.conv1x1(xr, w2d(c.conv1), _rows(h1), out_mode=1, out_norm=self._eval_norm(c.bn1))
        cv = c.conv2
        if (isinstance(cv, Conv3x3) and cv.stride == (1, 1) and cv.padding == cv.dilation and cv.bias is None
                and cv.in_channels % 64 == 0 and cv.out_channels % 64 == 0):
            st = 1
        else:
            st = _own_stride(cv) if cv.kernel_size == (3, 3) else 0          # the stage's first block: conv2 with a stride
        if st:                                                               # conv2 + bn2: one kernel
            w3 = _w16(cv, x).contiguous(memory_format=cl)
            h2 = new_map(cv.out_channels, st)
            hip.conv1x1(_rows(h1), _w_matrix(w3), _rows(h2), out_mode=1, out_norm=self._eval_norm(c.bn2),
                        conv3=(H, W, cv.dilation[0]) if st == 1 else (H, W, cv.dilation[0], st))
        else:
            h2 = c.bn2(c.conv2(h1))                                # in place under no_grad (InPlaceABN contract)
        if hasattr(self, "proj_conv"):
            pc = self.proj_conv
            if isinstance(pc, Conv1x1) and pc.in_channels % 64 == 0:
                st = 1
            else:
                st = _own_stride(pc) if pc.kernel_size == (1, 1) else 0      # strided shortcut projection: a row-gather product
            if st:                                                           # projection + proj_bn: one kernel
                res = new_map(pc.out_channels, st)
                hip.conv1x1(xr, w2d(pc), _rows(res), out_mode=1, out_norm=self._eval_norm(self.proj_bn),
                            strided=None if st == 1 else (H, W, st))
            else:
                res = self.proj_bn(pc(x))
        else:
            res = x
        h2 = h2.contiguous(memory_format=cl)
        res = res.contiguous(memory_format=cl)
        out = torch.empty((h2.shape[0], c.conv3.out_channels, h2.shape[2], h2.shape[3]), dtype=x.dtype, device=x.device,
                          memory_format=cl)
        hip.conv1x1(_rows(h2), w2d(c.conv3), _rows(out), out_mode=1,
                    out_norm=self._eval_norm(c.bn3, c.bn1.activation, c.bn1.activation_param), residual=_rows(res))
        return out

    def forward(self, x):
        if not self.training and not torch.is_grad_enabled() and self._eval_fusable(x):
            return self._forward_eval_fused(x)
        act, slope = self.convs.bn1.activation, self.convs.bn1.activation_param
        last = getattr(self.convs, self._last_bn)
        fused_train = (self.training and _is_fused_abn(last) and last.activation == "identity" and self._last_bn == "bn3"
                       and "dropout" not in self.convs._modules and x.is_cuda and x.dtype == torch.bfloat16)

        def project(t):
            r = _conv_abn_train(self.proj_conv, self.proj_bn, t) if self.training else None
            return r if r is not None else self.proj_bn(self.proj_conv(t))

        has_proj = hasattr(self, "proj_conv")
        # projection blocks in training: the block input feeds conv1 AND the projection; like the identity blocks, conv1's node
        # returns an alias of x for the second consumer, so x has ONE consumer and the projection's input gradient arrives as
        # the accumulate operand of conv1's input-gradient product instead of a separate 3-pass add (UCD_PROJ_ALIAS=0: A/B)
        defer = has_proj and fused_train and x.requires_grad and _env("UCD_PROJ_ALIAS", "1") != "0"
        residual = x if not has_proj else (None if defer else project(x))
        if fused_train:
            # wide bottleneck in training: every 1x1 convolution and its ABN are one node (statistics in the GEMM epilogue)
            c = self.convs
            skip = (residual is x or defer) and x.requires_grad
            first = _conv_abn_train(c.conv1, c.bn1, x, with_skip=skip, make_link=True)      # h1 feeds conv2 only
            if first is None and defer:
                residual = project(x)
            if first is not None:
                h1, res = first if skip else (first, residual)
                if defer:
                    res = project(res)                       # the alias of x: the shortcut's only path to the block input
                h2 = _conv_abn_train(c.conv2, c.bn2, h1, make_link=True)      # 3x3 as implicit GEMM + statistics; h2 feeds conv3 only
                if h2 is None:
                    h2 = c.bn2(c.conv2(h1))
                out = _conv_abn_train(c.conv3, c.bn3, h2, residual=res, activation=act, activation_param=slope, make_link=True)
                if out is None:
                    out = c.bn3(c.conv3(h2), residual=res, activation=act, activation_param=slope)
                return out
        if _is_fused_abn(last) and last.activation == "identity" and act in ("leaky_relu", "identity"):
            # fused epilogue: act(bn(conv_out) + residual) in one HBM pass
            h, first = x, None
            if residual is x and self.training:
                first = _conv1_with_skip(self.convs.conv1, x)
                if first is not None:
                    h, residual = first
            bn2_done = False
            for name, mod in self.convs.named_children():
                if mod is last:
                    h = mod(h, residual=residual, activation=act, activation_param=slope)
                elif first is not None and name == "conv1":
                    continue                                   # already applied together with the shortcut
                elif name == "conv2" and self.training and hasattr(self.convs, "bn2") and self.convs.bn2 is not last:
                    y = _conv_abn_train(mod, self.convs.bn2, h)   # narrow blocks: the 3x3 + its ABN as one node
                    bn2_done = y is not None
                    h = y if bn2_done else mod(h)
                elif name == "bn2" and bn2_done:
                    continue
                else:
                    h = mod(h)
            return h
        return _apply_act(self.convs(x) + residual, act, slope)


class DeeplabV3(nn.Module):
    """ASPP head: four parallel 2048->256 convs (1x1 and 3x3 with dilation 6/12/18 at output
    stride 16, 12/24/32 at 8), ABN over the 1024 concatenated channels, 1x1 reduction, plus the
    image-level pooling branch added before the last ABN (reference ``deeplab.py:54-70``).
    """

    def __init__(self, in_channels, out_channels, hidden_channels=256, out_stride=16,
                 norm_act=nn.BatchNorm2d, pooling_size=None):
        super().__init__()
        self.pooling_size = pooling_size
        if out_stride == 16:
            dilations = (6, 12, 18)
        elif out_stride == 8:
            dilations = (12, 24, 32)
        else:
            raise ValueError("out_stride must be 8 or 16")
        self.hidden_channels = hidden_channels

        branches = [Conv1x1(in_channels, hidden_channels)]
        branches += [Conv3x3(in_channels, hidden_channels, 3, bias=False, dilation=d, padding=d)
                     for d in dilations]
        self.map_convs = nn.ModuleList(branches)
        self.map_bn = norm_act(hidden_channels * len(branches))

        self.global_pooling_conv = Conv2d(in_channels, hidden_channels, 1, bias=False)
        self.global_pooling_bn = norm_act(hidden_channels)

        self.red_conv = Conv1x1(hidden_channels * len(branches), out_channels)
        self.pool_red_conv = Conv2d(hidden_channels, out_channels, 1, bias=False)
        self.red_bn = norm_act(out_channels)

        self.reset_parameters(self.map_bn.activation, self.map_bn.activation_param)

    def reset_parameters(self, activation, slope):
        """Xavier-normal conv weights with the activation's gain, unit/zero affine norms
        (reference ``deeplab.py:41-52``)."""
        gain = nn.init.calculate_gain(activation, slope)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_normal_(m.weight.data, gain)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.BatchNorm2d) or _is_fused_abn(m):
                if getattr(m, "weight", None) is not None:
                    nn.init.constant_(m.weight, 1)
                if getattr(m, "bias", None) is not None:
                    nn.init.constant_(m.bias, 0)

    # -- image-level pooling -----------------------------------------------------------------
    def _global_pooling(self, x):
        """(pooled map, replicate-padding still to apply or None).  Training: the plain global average [B, C, 1, 1].
        Evaluation: sliding average of (at most) pooling_size, stride 1, replicate-padded back to the input size
        (reference deeplab.py:77-88).  The reference pads first and runs the branch's two 1x1 convolutions and its
        norm on the full-size map; they are pointwise, so they commute with the replication and run here on the
        small pooled map (2x2 at 513^2 with the default --pooling 32) - same values, 270x fewer pixels."""
        if self.training or self.pooling_size is None:
            if _is_fused_abn(self.red_bn):
                from . import abn as _abn
                return _abn.global_avg_pool(x), None
            return x.flatten(2).mean(dim=-1)[:, :, None, None], None
        ph = min(try_index(self.pooling_size, 0), x.shape[2])
        pw = min(try_index(self.pooling_size, 1), x.shape[3])
        pad = ((pw - 1) // 2, (pw - 1) // 2 + (1 - pw % 2),
               (ph - 1) // 2, (ph - 1) // 2 + (1 - ph % 2))
        if (x.is_cuda and _is_fused_abn(self.red_bn) and not torch.is_grad_enabled()
                and x.shape[1] % (8 if x.dtype == torch.bfloat16 else 4) == 0 and x.dtype in (torch.bfloat16, torch.float32)):
            from . import hip
            return hip.window_mean(x, ph, pw), pad                # separable running sums: one read of the map
        return F.avg_pool2d(x, (ph, pw), stride=1), pad

    def forward(self, x):
        fused = _is_fused_abn(self.map_bn) and _is_fused_abn(self.red_bn)
        if fused:
            # each branch is normalised on its own channel slice and lands in the shared
            # 1024-channel buffer that red_conv reads: no cat
            out = self.map_bn.forward_branches([m(x) for m in self.map_convs])
        else:
            out = self.map_bn(torch.cat([m(x) for m in self.map_convs], dim=1))
        out = self.red_conv(out)

        pool, pad = self._global_pooling(x)
        pool = self.pool_red_conv(self.global_pooling_bn(self.global_pooling_conv(pool)))
        if pad is not None and pool.shape[-2:] != (1, 1):
            pool = F.pad(pool, pad=pad, mode="replicate")
        if fused and pool.shape[-2:] == (1, 1):
            # per-(image, channel) bias folded into red_bn's statistics and apply passes
            return self.red_bn(out, plane_bias=pool)
        if pool.shape[-2:] == (1, 1):
            pool = pool.expand(-1, -1, x.size(2), x.size(3))
        out = out + pool
        return self.red_bn(out)
