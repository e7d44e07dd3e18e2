"""GPU probe: the implicit-GEMM 3x3 mode of csrc/conv1x1.hip against F.conv2d (MIOpen, solver search on) - result and time,
forward and the input gradient (same kernel on the flipped / transposed weight), on the 3x3 layer shapes of the workload.
usage: python tools/conv3x3_probe.py            the table of every 3x3 layer shape
       python tools/conv3x3_probe.py --taps     the ASPP branches with UCD_CONV3_TAP_CLASSES off / on: interleaved rounds in one
                                                process, median us per launch beside the walked-step fractions of the plan"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ucd_amd import hip  # noqa: E402

dev = torch.device("cuda:0")
torch.backends.cudnn.benchmark = True


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


def own(x, w, y, d, **kw):
    B, K, H, W = x.shape
    N = w.shape[0]
    return hip.conv1x1(rows(x), w.permute(0, 2, 3, 1).reshape(N, 9 * K), rows(y), conv3=(H, W, d), **kw)


def run(B, K, N, H, W, d):
    cl = torch.channels_last
    x = torch.randn(B, K, H, W, device=dev).bfloat16().contiguous(memory_format=cl)
    w = (torch.randn(N, K, 3, 3, device=dev) * (2.0 / (9 * K)) ** 0.5).bfloat16().contiguous(memory_format=cl)
    y = torch.empty(B, N, H, W, device=dev, dtype=torch.bfloat16).contiguous(memory_format=cl)
    own(x, w, y, d)
    ref = F.conv2d(x.float(), w.float(), None, 1, d, d)
    err = ((y.float() - ref).norm() / ref.norm()).item()
    part = hip.conv1x1_stats_partial(B * H * W, N, dev)
    t_lib = bench(lambda: F.conv2d(x, w, None, 1, d, d))
    t_own = bench(lambda: own(x, w, y, d))
    t_stats = bench(lambda: own(x, w, y, d, out_mode=2, partial=part))
    v = torch.rand(N, device=dev) + 0.5
    t_aff = bench(lambda: own(x, w, y, d, out_mode=1, out_norm=(v, v, v, None, 1, 0.01)))
    # input gradient: conv of dy [B, N, H, W] with w.flip(2, 3).transpose(0, 1) [K, N, 3, 3]
    dy = torch.randn(B, N, H, W, device=dev).bfloat16().contiguous(memory_format=cl)
    wt = w.flip(2, 3).transpose(0, 1).contiguous(memory_format=cl)
    dx = torch.empty_like(x)
    own(dy, wt, dx, d)
    refdx = torch.nn.grad.conv2d_input(x.shape, w.float(), dy.float(), 1, d, d)
    errdx = ((dx.float() - refdx).norm() / refdx.norm()).item()
    t_dlib = bench(lambda: F.conv2d(dy, wt, None, 1, d, d))
    t_down = bench(lambda: own(dy, wt, dx, d))
    gf = 2 * B * H * W * K * N * 9 / 1e9
    form = lambda n, k, mode: hip.conv1x1_plan(B * H * W, n, k, taps=9, out_mode=mode)["form"]
    print(f"B={B} {K:4d}->{N:4d} {H}x{W} d={d:2d}  err {err:.1e} dx {errdx:.1e} | fwd MIOpen {t_lib:7.1f} us own {t_own:7.1f} [{form(N, K, 0)}] ({gf / t_own * 1e3:6.0f} TF/s) "
          f"+stats {t_stats:7.1f} [{form(N, K, 2)}] affine {t_aff:7.1f} [{form(N, K, 1)}] | dgrad MIOpen(fwd solver) {t_dlib:7.1f} own {t_down:7.1f} [{form(K, N, 0)}]", flush=True)


def walked(B, H, W, d, rows, on):
    """Fraction of tile x tap steps a launch walks: the plan's masks, or (off) the kernel-row rule of live_taps on raster tiles."""
    if on:
        _, masks, _ = hip.conv3_tap_plan(B, H, W, d, rows)
        return sum(bin(int(m)).count("1") for m in masks) / (9.0 * len(masks))
    M, hw, tot, n = B * H * W, H * W, 0, 0
    for m0 in range(0, M, rows):
        m1, nt = min(m0 + rows, M), 9
        if m1 - m0 < hw:
            first, last = m0 % hw, (m1 - 1) % hw
            ymin, ymax = (0, H - 1) if first > last else (first // W, last // W)
            nt -= 3 * (ymax < d) + 3 * (ymin >= H - d)
        tot, n = tot + nt, n + 1
    return tot / (9.0 * n)


def run_taps(B, K, N, H, W, d, rounds=7, iters=20):
    cl = torch.channels_last
    x = torch.randn(B, K, H, W, device=dev).bfloat16().contiguous(memory_format=cl)
    w = (torch.randn(N, K, 3, 3, device=dev) * (2.0 / (9 * K)) ** 0.5).bfloat16().contiguous(memory_format=cl)
    dy = torch.randn(B, N, H, W, device=dev).bfloat16().contiguous(memory_format=cl)
    wt = w.flip(2, 3).transpose(0, 1).contiguous(memory_format=cl)
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    was = hip.conv3_tap_classes()
    for name, a, ww, out, n_out in (("fwd", x, w, y, N), ("dgrad", dy, wt, dx, K)):
        res, path = {}, {}
        for on in (False, True):
            hip.conv3_tap_classes(int(on))
            own(a, ww, out, d)
            res[on] = out.clone()
            _, rows_, path[on] = hip.conv3_tap_stats()      # the tile height the library picked, and whether it took the class order
        t = {False: [], True: []}
        for _ in range(rounds):
            for on in (False, True):
                hip.conv3_tap_classes(int(on))
                t[on].append(bench(lambda: own(a, ww, out, d), iters=iters, warm=3))
        hip.conv3_tap_classes(was)
        med = {on: sorted(v)[len(v) // 2] for on, v in t.items()}
        f = {on: walked(B, H, W, d, rows_, path[on]) for on in (False, True)}
        form = hip.conv1x1_plan(B * H * W, n_out, a.shape[1], taps=9)["form"]
        print(f"B={B:2d} {a.shape[1]:4d}->{n_out:4d} {H}x{W} d={d:2d} {name:5s} {form} rows {rows_:3d} | off {med[False]:7.1f} us (min {min(t[False]):7.1f}) "
              f"on {med[True]:7.1f} us (min {min(t[True]):7.1f}) time x{med[True] / med[False]:.3f} | steps {f[False]:.3f} -> {f[True]:.3f} "
              f"x{f[True] / f[False]:.3f} | {'class order' if path[True] else 'raster (gate)'} | equal {torch.equal(res[False], res[True])}", flush=True)


if __name__ == "__main__":
    if "--taps" in sys.argv:
        for B in (24, 3):
            for d in (6, 12, 18):
                run_taps(B, 2048, 256, 33, 33, d)
        sys.exit(0)
    for cfg in [(24, 256, 256, 33, 33, 1), (24, 512, 512, 33, 33, 2), (24, 128, 128, 65, 65, 1), (24, 64, 64, 129, 129, 1),
                (24, 2048, 256, 33, 33, 6), (24, 2048, 256, 33, 33, 18), (3, 256, 256, 33, 33, 1)]:
        run(*cfg)
