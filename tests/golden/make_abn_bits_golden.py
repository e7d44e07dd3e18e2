"""GPU: records the bits of the element-wise ABN passes (ucd_amd/csrc/abn.hip) in tests/golden/abn_bits.json.

The per-element kernels (one value at a time through Vec<T>::get/set) were the reference of the packed-pair kernels: same
operations, same order, bit-identical outputs.  This script pinned their outputs before they were deleted: it ran every case
twice in child processes - the library's default dispatch and UCD_ABN_GENERIC=1 (the per-element kernels everywhere, a switch
that existed only in the library this was recorded against) - refused to write unless the two agreed on every digest, and
stored the SHA-256 of each output's bytes together with the SHA-256 of the abn.hip it ran against.  The JSON is a record of
that library; it is never regenerated from a later one.  tests/test_abn_gpu.py replays ``run_case`` below in-process and compares
digests (test_elementwise_passes_reproduce_the_recorded_per_element_bits).

    python tests/golden/make_abn_bits_golden.py [OUT.json]          # on a tree whose abn.hip still has both kernel families

Inputs come from integer arithmetic on the CPU (an index hash scaled into about +-4, no random generator), so they are the
same bytes everywhere.
"""
import hashlib
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
JSON_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "abn_bits.json")
ABN_HIP = os.path.join(ROOT, "ucd_amd", "csrc", "abn.hip")

IDENTITY, LEAKY, ELU, ABS_GAMMA = 0, 1, 2, 0x100

# name: (dtype, B, C, H, W, slope, act, plane_bias, unaligned) - and the property each case is there for
CASES = {
    # the six shapes of the former two-process test, bf16
    "bf16_3x64x33x32": ("bf16", 3, 64, 33, 32, 0.01, LEAKY, False, False),      # 13 row bands of 256 rows, the last one 96 rows = 3 row steps: shorter than a four-row batch
    "bf16_2x64x65x67": ("bf16", 2, 64, 65, 67, 0.01, LEAKY, False, False),      # odd M: the last band ends in the middle of a row step
    "bf16_2x256x33x33": ("bf16", 2, 256, 33, 33, 0.01, LEAKY, False, False),    # TX = 32, TY = 8
    "bf16_3x1024x17x19_identity": ("bf16", 3, 1024, 17, 19, 1.0, IDENTITY, False, False),   # two channel-group columns (gx = 2), identity
    "bf16_1x8x5x7": ("bf16", 1, 8, 5, 7, 0.2, LEAKY, False, False),             # TX = 1, TY = 256: tail rows only
    "bf16_2x128x9x11_absgamma": ("bf16", 2, 128, 9, 11, 0.01, LEAKY | ABS_GAMMA, False, False),   # |gamma| + eps, the sign of d weight
    # fp32: two pairs per lane
    "f32_3x64x33x32": ("f32", 3, 64, 33, 32, 0.01, LEAKY, False, False),        # 25 bands, the last one a four-row batch plus two tail rows
    "f32_2x256x33x33": ("f32", 2, 256, 33, 33, 0.01, LEAKY, False, False),      # TX = 64, TY = 4
    "f32_2x24x9x11": ("f32", 2, 24, 9, 11, 0.01, LEAKY, False, False),          # six channel groups: TX = 6 does not divide 256, the block carries idle threads
    # ELU (alpha = slope = 1): a per-half select of expm1 / exp
    "bf16_2x64x9x11_elu": ("bf16", 2, 64, 9, 11, 1.0, ELU, False, False),
    "f32_2x64x9x11_elu": ("f32", 2, 64, 9, 11, 1.0, ELU, False, False),
    # plane bias (the pooled ASPP branch): one more pair add, the image index r / HW changes inside a band
    "bf16_3x64x9x11_pb": ("bf16", 3, 64, 9, 11, 0.01, LEAKY, True, False),
    "bf16_3x64x9x11_pb_elu": ("bf16", 3, 64, 9, 11, 1.0, ELU, True, False),
    "f32_3x64x9x11_pb": ("f32", 3, 64, 9, 11, 0.01, LEAKY, True, False),
    "f32_3x64x9x11_pb_elu": ("f32", 3, 64, 9, 11, 1.0, ELU, True, False),
    "bf16_2x256x5x5_pb": ("bf16", 2, 256, 5, 5, 0.01, LEAKY, True, False),
    "bf16_2x256x5x5_pb_elu": ("bf16", 2, 256, 5, 5, 1.0, ELU, True, False),
    "f32_2x256x5x5_pb": ("f32", 2, 256, 5, 5, 0.01, LEAKY, True, False),
    "f32_2x256x5x5_pb_elu": ("f32", 2, 256, 5, 5, 1.0, ELU, True, False),
    # M = 1: one row, one band, 255 of 256 row threads without work
    "bf16_1x64x1x1": ("bf16", 1, 64, 1, 1, 0.01, LEAKY, False, False),
    "f32_1x64x1x1": ("f32", 1, 64, 1, 1, 0.01, LEAKY, False, False),
    # mean / invstd / scale / shift / sums are views offset by one float: the per-channel vectors are not 16-byte aligned
    "bf16_2x64x9x11_unaligned": ("bf16", 2, 64, 9, 11, 0.01, LEAKY, False, True),
    "f32_2x64x9x11_unaligned": ("f32", 2, 64, 9, 11, 0.01, LEAKY, False, True),
}


def _hash(n, seed):
    """n values in [-4, 4) from an integer hash of the index (int64 arithmetic below 2^63, no random generator)."""
    h = (torch.arange(n, dtype=torch.int64) * 2654435761 + seed * 40503 + 12345) & 0xFFFFFFFF
    h = h ^ (h >> 15)
    h = (h * 73244475) & 0xFFFFFFFF
    h = h ^ (h >> 13)
    h = (h * 73244475) & 0xFFFFFFFF
    h = h ^ (h >> 16)
    return ((h & 0xFFFF) - 32768).to(torch.float32) / 8192.0


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _vec(n, dev, unaligned):
    """A zeroed float vector; ``unaligned``: a view one float into its allocation."""
    return torch.zeros(n + 1, device=dev)[1:] if unaligned else torch.zeros(n, device=dev)


def run_case(name, dev="cuda:0"):
    """Runs every call of one case; returns {output name: SHA-256 of its bytes}."""
    from ucd_amd import hip
    dtype, B, C, H, W, slope, act, with_pb, unaligned = CASES[name]
    td = torch.bfloat16 if dtype == "bf16" else torch.float32
    M, HW = B * H * W, H * W
    seed = sum(name.encode())
    chan = ((torch.arange(C) % 7) - 3).to(torch.float32) * 0.25           # non-zero channel means
    x = (_hash(M * C, seed).view(M, C) + chan).to(td).to(dev)
    dy = _hash(M * C, seed + 1).view(M, C).to(td).to(dev)
    r = _hash(M * C, seed + 2).view(M, C).to(td).to(dev)
    w = 0.4 + (_hash(C, seed + 3) + 4.0) * 0.15                           # signed weights: one negative
    w[1] = -0.7
    w = w.to(dev)
    b = _vec(C, dev, unaligned)
    b.copy_(_hash(C, seed + 4) * 0.05)
    pb = (_hash(B * C, seed + 5) * 0.25).view(B, C).to(dev) if with_pb else None
    buf = _vec(6 * C, dev, unaligned)
    sums, ks, mean, invstd, scale = buf[:2 * C], buf[2 * C:3 * C], buf[3 * C:4 * C], buf[4 * C:5 * C], buf[5 * C:]
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    out = {}
    hip.abn_stats_finalize(x, C, M, C, pb, HW, sums, ks, w, rm, rv, 0.1, 1e-5, mean, invstd, scale, act & ABS_GAMMA)
    out.update(mean=digest(mean), invstd=digest(invstd), scale=digest(scale))

    def e():
        return torch.empty_like(x)
    y, y2, y3 = e(), e(), e()
    hip.abn_apply(x, C, y, C, None, 0, M, C, pb, HW, mean, scale, b, act, slope)
    hip.abn_apply(x, C, y2, C, r, C, M, C, pb, HW, mean, scale, b, act, slope)
    hip.abn_apply(x, C, y3, C, None, 0, M, C, pb, HW, mean, scale, None, act, slope)
    out.update(y=digest(y), y_res=digest(y2), y_noshift=digest(y3))
    s2, s3 = _vec(2 * C, dev, unaligned), _vec(2 * C, dev, unaligned)
    dx, dx2, dz, dx3 = e(), e(), e(), e()
    hip.abn_bwd_reduce(x, C, dy, C, None, 0, M, C, pb, HW, mean, invstd, scale, b, act, slope, s2)                # sign from x
    hip.abn_bwd_apply(x, C, dy, C, None, 0, dx, C, None, 0, M, C, pb, HW, mean, invstd, scale, b, w, s2, M, 0, act, slope)
    hip.abn_bwd_reduce(x, C, dy, C, y, C, M, C, pb, HW, mean, invstd, scale, b, act, slope, s3)                   # sign from y, with dz
    hip.abn_bwd_apply(x, C, dy, C, y, C, dx2, C, dz, C, M, C, pb, HW, mean, invstd, scale, b, w, s3, M, 0, act, slope)
    hip.abn_bwd_apply(x, C, dy, C, y, C, dx3, C, None, 0, M, C, pb, HW, mean, invstd, scale, b, w, s3, M, 1, act, slope)   # frozen
    out.update(sums=digest(s2), dx=digest(dx), sums_y=digest(s3), dx_y=digest(dx2), dz=digest(dz), dx_frozen=digest(dx3))

    if dtype == "bf16" and (act & 0xFF) != ELU and not with_pb and not unaligned:
        # the forms that finalise in the kernel: statistics from raw sums about a shift, split over `reps` replicas
        raw, kshift = torch.zeros(2 * C, device=dev), torch.zeros(C, device=dev)
        hip.abn_stats(x, C, M, C, None, HW, raw, kshift)
        for reps in (1, 3):
            acc = raw[None] * torch.tensor([1.0] if reps == 1 else [0.5, 0.25, 0.25], device=dev)[:, None]
            for res in (None, r):
                fb = torch.zeros(6 * C, device=dev)
                frm, frv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
                yy = e()
                hip.abn_apply_stats(x, yy, res, M, C, acc.contiguous(), kshift, M, w, b, frm, frv, 0.1, 1e-5, fb, act, slope, reps)
                tag = f"fin_r{reps}_{'res' if res is not None else 'plain'}"
                out[tag + "_y"] = digest(yy)
                out[tag + "_consts"] = digest(fb[3 * C:])
                out[tag + "_running"] = digest(torch.cat([frm, frv]))
        # backward apply from raw (unsigned) link sums, the parameter gradients written by the same launch
        for reps in (1, 3):
            split = torch.tensor([1.0] if reps == 1 else [0.5, 0.25, 0.25], device=dev)[:, None]
            rs, rg = (s2[None] * split).contiguous(), (s3[None] * split).contiguous()
            for gs_name, gs in (("same", None), ("sep", rg)):
                forms = ((None, False), (y, True)) + (((y, False), (None, True)) if reps == 1 and gs is None else ())
                for yo, want_dz in forms:
                    d1, d2, go = e(), (e() if want_dz else None), torch.zeros(2 * C, device=dev)
                    hip.abn_bwd_apply_raw(x, dy, yo, d1, d2, M, C, mean, invstd, scale, b, w, rs, gs, go, M, act, slope, reps)
                    tag = f"raw_r{reps}_{gs_name}_{'y' if yo is not None else 'x'}{'_dz' if want_dz else ''}"
                    out[tag + "_dx"] = digest(d1)
                    out[tag + "_grad"] = digest(go)
                    if want_dz:
                        out[tag + "_dzout"] = digest(d2)
    torch.cuda.synchronize()
    return out


def run_all():
    return {name: run_case(name) for name in CASES}


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        with open(sys.argv[2], "w") as f:
            json.dump(run_all(), f)
        return
    out_path = sys.argv[1] if len(sys.argv) > 1 else JSON_PATH
    with open(ABN_HIP, "rb") as f:
        src_text = f.read()
    if b"UCD_ABN_GENERIC" not in src_text or b"fast_path" not in src_text:
        sys.exit(f"{ABN_HIP} no longer has the per-element kernels behind UCD_ABN_GENERIC: both runs would be the same kernels "
                 "and the record would come from the code it is meant to check.  Nothing written.")
    import tempfile
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for mode in ("packed", "per_element"):
            env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
            env.pop("UCD_ABN_GENERIC", None)
            if mode == "per_element":
                env["UCD_ABN_GENERIC"] = "1"
            path = os.path.join(tmp, mode + ".json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env, check=True, timeout=900)
            with open(path) as f:
                res[mode] = json.load(f)
    bad = [(c, t) for c, d in res["packed"].items() for t in d if res["per_element"][c].get(t) != d[t]]
    if bad or res["packed"].keys() != res["per_element"].keys():
        sys.exit(f"packed and per-element kernels disagree, nothing written: {bad}")
    src = hashlib.sha256(src_text).hexdigest()
    with open(out_path, "w") as f:
        json.dump({"abn_hip_sha256": src, "cases": res["packed"]}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{out_path}: {sum(len(d) for d in res['packed'].values())} digests over {len(CASES)} cases, both kernel families agree")


if __name__ == "__main__":
    main()
