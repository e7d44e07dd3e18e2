"""GPU micro-benchmark of the ABN kernels over the layer shapes of ResNet-101/DeepLab-V3 at B=24, 513^2.
usage: python tools/abn_bench.py [images] [--dtype bf16|f32] [--act leaky_relu|identity|elu] [--plane-bias] [--shapes CxHW,...]
ABN_ONLY=STATS|APPLY|BRED|BAPP in the environment: one kernel, one `CxHW=us` per shape on a single line."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ucd_amd import hip
ap = argparse.ArgumentParser()
ap.add_argument("images", nargs="?", type=int, default=24)
ap.add_argument("--dtype", choices=("bf16", "f32"), default="bf16")
ap.add_argument("--act", choices=("leaky_relu", "identity", "elu"), default="leaky_relu")
ap.add_argument("--plane-bias", action="store_true", help="with a per-(image, channel) bias (the pooled ASPP branch)")
ap.add_argument("--shapes", default="", help="comma-separated CxHW (e.g. 256x33) instead of every layer shape")
args = ap.parse_args()
dev = torch.device("cuda:0")
B = args.images
td = torch.bfloat16 if args.dtype == "bf16" else torch.float32
act = {"identity": 0, "leaky_relu": 1, "elu": 2}[args.act]
slope = {"identity": 1.0, "leaky_relu": 0.01, "elu": 1.0}[args.act]
shapes = [(64, 257), (64, 129), (256, 129), (128, 65), (512, 65), (256, 33), (1024, 33), (2048, 33), (512, 33)]
if args.shapes:
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
def timeit(f, n=20):
    for _ in range(3): f()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for s, e in evs:
        s.record(); f(); e.record()
    torch.cuda.synchronize()
    t = sorted(s.elapsed_time(e) for s, e in evs)
    return t[n // 2] * 1e3   # us
if not os.environ.get("ABN_ONLY"): print("%-14s %8s | %18s | %18s | %18s | %18s" % ("C x HW", "MB", "stats us (GB/s)", "apply us (GB/s)", "bwd_reduce", "bwd_apply"))
for C, hw in shapes:
    x = torch.randn(B, C, hw, hw, device=dev).to(td).contiguous(memory_format=torch.channels_last)
    dy = torch.randn_like(x); y = torch.empty_like(x); dx = torch.empty_like(x)
    M, HW = B * hw * hw, hw * hw
    buf = torch.zeros(6 * C, device=dev); w = torch.ones(C, device=dev); b = torch.zeros(C, device=dev)
    pb = torch.randn(B, C, device=dev) if args.plane_bias else None
    sums, ks, mean, invstd, scale = buf[:2*C], buf[2*C:3*C], buf[3*C:4*C], buf[4*C:5*C], buf[5*C:]
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    mb = x.numel() * x.element_size() / 1e6
    def f_stats(): hip.abn_stats_finalize(x, C, M, C, pb, HW, sums, ks, w, rm, rv, 0.1, 1e-5, mean, invstd, scale)
    def f_apply(): hip.abn_apply(x, C, y, C, None, 0, M, C, pb, HW, mean, scale, b, act, slope)
    def f_red(): hip.abn_bwd_reduce(x, C, dy, C, None, 0, M, C, pb, HW, mean, invstd, scale, b, act, slope, sums)
    def f_bapp(): hip.abn_bwd_apply(x, C, dy, C, None, 0, dx, C, None, 0, M, C, pb, HW, mean, invstd, scale, b, w, sums, M, 0, act, slope)
    f_stats()
    res = []
    only = os.environ.get("ABN_ONLY")
    if only:
        f = {"STATS": f_stats, "APPLY": f_apply, "BRED": f_red, "BAPP": f_bapp}[only]
        print("%s=%.1f" % (f"{C}x{hw}", timeit(f)), end=" ", flush=True)
        continue
    for f, nb in ((f_stats, 1), (f_apply, 2), (f_red, 2), (f_bapp, 3)):
        us = timeit(f)
        res.append("%8.1f (%6.0f)" % (us, nb * mb / us * 1e3))
    print("%-14s %8.1f | %18s | %18s | %18s | %18s" % (f"{C}x{hw}^2", mb, *res))

print()
