"""GPU probe: the fp32 split-bf16 convolutions of csrc/conv_f32.hip against MIOpen fp32 (F.conv2d / convolution_backward, solver
search on) on every distinct stride-1 layer shape of the bench (B = 24, 513^2, --opt_level O0): forward, input gradient (the
forward call on the rearranged weight) and weight gradient.  Device events after warm-up; achieved TF/s against the f32 MFMA peak
(157 TF) and against 3/16 of the bf16 dense peak (2.5 PF: the ceiling of three bf16 MFMAs per product).
usage: python tools/conv_f32_probe.py [B]"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ucd_amd import hip  # noqa: E402

dev = torch.device("cuda:0")
torch.backends.cudnn.benchmark = True
torch.backends.cudnn.allow_tf32 = False
CL = torch.channels_last
F32_PEAK, SPLIT_PEAK = 157.3e12, 2.5e15 * 3 / 16

# (map side, K, N, dilation; 0 = 1x1) of the stride-1 layers of the ResNet-101 body (output stride 16) and the DeepLab-V3 head
SHAPES = [(129, 64, 64, 0), (129, 64, 64, 1), (129, 64, 256, 0), (129, 256, 64, 0), (129, 256, 128, 0),
          (65, 128, 128, 1), (65, 128, 512, 0), (65, 512, 128, 0), (65, 512, 256, 0),
          (33, 256, 256, 1), (33, 256, 1024, 0), (33, 1024, 256, 0), (33, 1024, 512, 0), (33, 1024, 2048, 0),
          (33, 512, 512, 2), (33, 512, 2048, 0), (33, 2048, 512, 0),
          (33, 2048, 256, 0), (33, 2048, 256, 6), (33, 2048, 256, 12), (33, 2048, 256, 18), (33, 1024, 256, 0)]


def bench(fn, iters=20, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def rows(t):
    b, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(b * h * w, c)


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    print(f"B = {B}; us per call, own / MIOpen fp32; TF/s of the own kernel and its fraction of 157 TF (f32 MFMA) and of 469 TF "
          f"(3/16 of the bf16 dense peak)")
    print(f"{'layer':>24} {'pass':>6} {'own us':>9} {'miopen us':>10} {'speedup':>8} {'TF/s':>7} {'/f32pk':>7} {'/split':>7}")
    tot = {"own": 0.0, "lib": 0.0}
    for S, K, N, d in SHAPES:
        k = 3 if d else 1
        pad = d if d else 0
        x = torch.randn((B, K, S, S), device=dev).contiguous(memory_format=CL)
        w = (torch.randn((N, K, k, k), device=dev) / (K * k * k) ** 0.5).contiguous(memory_format=CL)
        dy = torch.randn((B, N, S, S), device=dev).contiguous(memory_format=CL)
        wt = (w.transpose(0, 1) if not d else w.flip(2, 3).transpose(0, 1)).contiguous(memory_format=CL)
        y = torch.empty((B, N, S, S), device=dev).contiguous(memory_format=CL)
        dx = torch.empty((B, K, S, S), device=dev).contiguous(memory_format=CL)
        dw = torch.empty((N, k * k * K), device=dev)
        c3 = (S, S, d) if d else None
        wm, wtm = w.permute(0, 2, 3, 1).reshape(N, -1), wt.permute(0, 2, 3, 1).reshape(K, -1)
        flop = 2.0 * B * S * S * K * N * k * k
        passes = {
            "fwd": (lambda: hip.conv_f32(rows(x), wm, rows(y), conv3=c3),
                    lambda: F.conv2d(x, w, None, 1, pad, max(d, 1))),
            "dgrad": (lambda: hip.conv_f32(rows(dy), wtm, rows(dx), conv3=c3),
                      lambda: torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [pad, pad], [max(d, 1)] * 2, False, [0, 0],
                                                                  1, [True, False, False])),
            "wgrad": (lambda: hip.conv_f32_wgrad(rows(dy), rows(x), dw, conv3=c3),
                      lambda: torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [pad, pad], [max(d, 1)] * 2, False, [0, 0],
                                                                  1, [False, True, False])),
        }
        name = f"{S}^2 {K}->{N} " + (f"3x3 d{d}" if d else "1x1")
        for p, (own, lib) in passes.items():
            t_own, t_lib = bench(own), bench(lib)
            tot["own"] += t_own
            tot["lib"] += t_lib
            tf = flop / (t_own * 1e-6)
            print(f"{name:>24} {p:>6} {t_own:9.1f} {t_lib:10.1f} {t_lib / t_own:8.2f} {tf / 1e12:7.1f} {tf / F32_PEAK:7.2f} "
                  f"{tf / SPLIT_PEAK:7.2f}", flush=True)
        del x, w, dy, wt, y, dx, dw
    print(f"sum over the distinct shapes (one call each): own {tot['own'] / 1e3:.2f} ms, MIOpen {tot['lib'] / 1e3:.2f} ms")


if __name__ == "__main__":
    main()
