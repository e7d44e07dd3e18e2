"""GPU timing of the contrastive loss call at the ADE per-rank shape (B, N, h, K, H) = (3, 256, 32, K, 512) for several teacher
class counts K, in the precisions the trainer uses.
usage: python tools/pixcon_manyclass_bench.py [--k 101,141] [--prec f32,f16] [--repeats 5] [--calls 20]
Each repeat is `calls` timed calls (HIP events around ucd_pixcon_loss alone, the batch prepared once, label-sorted rows as the
trainer runs it) after 5 warm-up calls; one line per (K, precision) with the median of every repeat and their spread.  A class
count the build refuses is reported as such (the commit before the many-class kernels refuses K > 110 / 112)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from ucd_amd import synth
from ucd_amd.contrastive import pixcon_loss_raw, pixcon_prepare

ap = argparse.ArgumentParser()
ap.add_argument("--k", default="101,141")
ap.add_argument("--prec", default="f32,f16")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--calls", type=int, default=20)
args = ap.parse_args()
dev = torch.device("cuda:0")
B, N, h, H = 3, 256, 32, 512
for K in [int(v) for v in args.k.split(",")]:
    new_ids = list(range(K, 151)) if K < 151 else [K]
    f_n, f_o, l_po, labels = synth.contrastive_case(4000 + K, B, N, h, h, K, H, H, new_ids)
    f_n = f_n.to(dev).contiguous(memory_format=torch.channels_last)
    f_o, l_po, labels = f_o.to(dev), l_po.to(dev), labels.to(dev)
    for prec in args.prec.split(","):
        pb = pixcon_prepare(f_n, labels, l_po, f_o, max_label=max(150, K), sort_by_label=True, fp16=prec != "f32")
        m = pb.meta_host()
        run = lambda: pixcon_loss_raw(pb, 0.07, True, True, need_grad=True, precision=prec)
        try:
            for _ in range(5):
                out = run()
            torch.cuda.synchronize()
        except RuntimeError as e:
            print(f"K {K} {prec}: refused: {str(e)[:140]}")
            continue
        meds = []
        for _ in range(args.repeats):
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.calls)]
            for s, e in evs:
                s.record(); out = run(); e.record()
            torch.cuda.synchronize()
            ts = sorted(s.elapsed_time(e) for s, e in evs)
            meds.append(ts[len(ts) // 2])
        flop = float(m.A) * (m.A + m.Co) * (4 * N + 2 * K)
        mid = sorted(meds)[len(meds) // 2]
        print(f"K {K} {prec}: A {m.A} Co {m.Co} | medians of {args.repeats} x {args.calls} calls (ms): "
              + " ".join(f"{v:.4f}" for v in meds)
              + f" | median {mid:.4f} spread {max(meds) - min(meds):.4f} | {flop / mid / 1e9:.1f} TFLOP/s algorithmic"
              + f" | loss {out[0][0].item():.6f}")
