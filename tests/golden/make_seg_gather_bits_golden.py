"""GPU: records the bits of the two gather-form loss kernels (ucd_seg_losses_gather, ucd_seg_bce) in
tests/golden/seg_gather_bits.json.

Both kernels give the same bits on every run (one wave per low-resolution cell, no atomics, fixed reduction orders), so their
output can be pinned.  This script ran once, against the library in which each kernel still carried its own copy of the cell walk
(ucd_amd/csrc/seg_bce.hip and the end of ucd_amd/csrc/seglogit_loss.hip), and stored the SHA-256 of the bytes of ``loss_out``, of
``d_sem`` (the NaN-filled padding columns of a padded ``ld_d`` excluded) and of the per-cell ``part`` pairs of every case, together
with the SHA-256 of those two source files.  The JSON is a record of that library; it is never regenerated from a later one.
tests/test_seg_gather_gpu.py and tests/test_seg_bce_gpu.py replay ``run_case`` below in-process and compare digests.

    python tests/golden/make_seg_gather_bits_golden.py [OUT.json]      # on a tree that still has csrc/seg_bce.hip

Every case goes through the C ABI.  Inputs come from integer arithmetic on the CPU (an index hash, no random generator), so they
are the same bytes everywhere.
"""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
JSON_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "seg_gather_bits.json")
SOURCES = [os.path.join(ROOT, "ucd_amd", "csrc", n) for n in ("seg_bce.hip", "seglogit_loss.hip")]

KD_UNBIASED, KD_PLAIN = 0, 1
IGNORE = 255

# B, H, W, h, w - and what each geometry is there for
GEOS = {
    "f1": (2, 8, 8, 8, 8),            # factor 1: every pixel has one cell
    "ragged": (1, 9, 7, 3, 2),        # non-integer, non-square factors, clamped last row and column
    "h1": (2, 19, 23, 1, 5),          # h = 1: y0 == y1 everywhere
    "f64x8": (1, 64, 16, 1, 2),       # factor 64 x 8: several 64-pixel chunks per cell
}
VARIANT_GEO = "ragged"

# the soft-max form, (Ctot, K): one split per instantiation of seg_losses_gather_kernel<NR>
SM_SPLITS = [(21, 16), (100, 65), (151, 101)]             # NR 1, 2, 3: on every geometry
SM_LARGE = [(300, 200), (700, 450)]                       # NR 8, 29: on VARIANT_GEO only
SM_VARIANT_SPLITS = [(21, 16), (151, 101)]
# name: (teacher, kd_mode, alpha, ce_old_cl [None: K], d_sem, padding of ld_s / ld_t / ld_d, labels, logits)
SM_VARIANTS = {
    "base": (True, KD_UNBIASED, 1.0, None, True, 0, "plain", "hash"),
    "no_teacher": (False, KD_UNBIASED, 1.0, None, True, 0, "plain", "hash"),
    "kd_plain": (True, KD_PLAIN, 1.0, None, True, 0, "plain", "hash"),
    "alpha05": (True, KD_UNBIASED, 0.5, None, True, 0, "plain", "hash"),
    "ce1": (True, KD_UNBIASED, 1.0, 1, True, 0, "plain", "hash"),
    "no_d_sem": (True, KD_UNBIASED, 1.0, None, False, 0, "plain", "hash"),
    "padded": (True, KD_UNBIASED, 1.0, None, True, 3, "plain", "hash"),
    "labels": (True, KD_UNBIASED, 1.0, None, True, 0, "odd", "hash"),          # ignore_index, a negative value, values >= Ctot
    "pm80": (True, KD_UNBIASED, 1.0, None, True, 0, "plain", "pm80"),          # one class at +80, the rest at -80: the rescue branch
}

# the BCE form: Ctot 24 (one full register chunk), 25 (a second chunk with one class), 49 (three chunks); K 7 and K = Ctot
BCE_CTOT = [24, 25, 49]
# name: (teacher, d_sem, padding, labels, logits)
BCE_VARIANTS = {
    "base": (True, True, 0, "plain", "hash"),
    "no_teacher": (False, True, 0, "plain", "hash"),
    "no_d_sem": (True, False, 0, "plain", "hash"),
    "padded": (True, True, 3, "plain", "hash"),
    "labels": (True, True, 0, "odd", "hash"),
    "pm90": (True, True, 0, "plain", "pm90"),                                   # logits of +-90: nothing overflows
}


def _cases():
    sm, bce = {}, {}
    for g in GEOS:
        for Ctot, K in SM_SPLITS:
            sm[f"sm_{g}_{Ctot}_{K}_base"] = (g, Ctot, K, "base")
        for Ctot in BCE_CTOT:
            for K in (7, Ctot):
                bce[f"bce_{g}_{Ctot}_{K}_base"] = (g, Ctot, K, "base")
    for Ctot, K in SM_LARGE:
        sm[f"sm_{VARIANT_GEO}_{Ctot}_{K}_base"] = (VARIANT_GEO, Ctot, K, "base")
    for Ctot, K in SM_VARIANT_SPLITS:
        for v in SM_VARIANTS:
            sm[f"sm_{VARIANT_GEO}_{Ctot}_{K}_{v}"] = (VARIANT_GEO, Ctot, K, v)
    for Ctot in BCE_CTOT:
        for K in (7, Ctot):
            for v in BCE_VARIANTS:
                bce[f"bce_{VARIANT_GEO}_{Ctot}_{K}_{v}"] = (VARIANT_GEO, Ctot, K, v)
    return sm, bce


SM_CASES, BCE_CASES = _cases()
CASES = {**SM_CASES, **BCE_CASES}


def _hash_u32(n, seed):
    """n 32-bit hashes of the index (int64 arithmetic below 2^63, no random generator)."""
    h = (torch.arange(n, dtype=torch.int64) * 2654435761 + seed * 40503 + 12345) & 0xFFFFFFFF
    h = h ^ (h >> 15)
    h = (h * 73244475) & 0xFFFFFFFF
    h = h ^ (h >> 13)
    h = (h * 73244475) & 0xFFFFFFFF
    return h ^ (h >> 16)


def _hash(n, seed):
    """n values in [-4, 4)."""
    return ((_hash_u32(n, seed) & 0xFFFF) - 32768).to(torch.float32) / 8192.0


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _rows(cells, C, pad, kind, seed, dev):
    """[cells, C + pad] logits rows, the padding columns NaN (a kernel that reads one poisons its output)."""
    if kind == "hash":
        v = _hash(cells * C, seed).view(cells, C)
    elif kind == "pm80":
        lead = (_hash_u32(cells, seed) % C).view(cells, 1)
        v = torch.where(torch.arange(C).view(1, C) == lead, 80.0, -80.0).to(torch.float32)
    else:
        v = torch.where((_hash_u32(cells * C, seed) & 1) == 1, 90.0, -90.0).to(torch.float32).view(cells, C)
    out = torch.full((cells, C + pad), float("nan"), dtype=torch.float32)
    out[:, :C] = v
    return out.to(dev)


def _labels(B, H, W, Ctot, kind, seed, dev):
    n = B * H * W
    lab = (_hash_u32(n, seed) % Ctot).to(torch.int64)
    idx = torch.arange(n)
    lab[idx % 11 == 3] = IGNORE
    if kind == "odd":
        lab[idx % 7 == 1] = -3
        lab[idx % 7 == 4] = Ctot
        lab[idx % 13 == 5] = Ctot + 5
    return lab.view(B, H, W).to(dev)


def run_case(name, dev="cuda:0"):
    """Runs one case through the C ABI; returns {output name: SHA-256 of its bytes}."""
    from ucd_amd import hip
    lib = hip.load()
    bce = name in BCE_CASES
    geo, Ctot, K, variant = CASES[name]
    B, H, W, h, w = GEOS[geo]
    if bce:
        teacher, want_d, pad, lab_kind, logits = BCE_VARIANTS[variant]
    else:
        teacher, kd_mode, alpha, ce_old_cl, want_d, pad, lab_kind, logits = SM_VARIANTS[variant]
        ce_old_cl = K if ce_old_cl is None else ce_old_cl
    cells, seed = B * h * w, sum(name.encode())
    s = _rows(cells, Ctot, pad, logits, seed, dev)
    t = _rows(cells, K, pad, logits, seed + 1, dev) if teacher else None
    labels = _labels(B, H, W, Ctot, lab_kind, seed + 2, dev)
    d = torch.full((cells, Ctot + pad), float("nan"), dtype=torch.float32, device=dev) if want_d else None
    out = torch.full((2,), float("nan"), dtype=torch.float32, device=dev)
    part = torch.full((cells, 2), float("nan"), dtype=torch.float32, device=dev)
    if bce:
        assert lib.ucd_seg_bce_workspace_bytes(B, h, w) == part.numel() * 4
        hip._check(lib.ucd_seg_bce(hip.ptr(s), Ctot + pad, hip.ptr(t), K + pad, hip.ptr(labels), B, H, W, h, w, Ctot, K, IGNORE, 1.0, 3.0,
                                   hip.ptr(out), hip.ptr(d), Ctot + pad, hip.ptr(part), part.numel() * 4, hip.stream()), "ucd_seg_bce")
    else:
        assert lib.ucd_seg_losses_gather_workspace_bytes(B, h, w) == part.numel() * 4
        hip._check(lib.ucd_seg_losses_gather(hip.ptr(s), Ctot + pad, hip.ptr(t), K + pad, hip.ptr(labels), B, H, W, h, w, Ctot, K,
                                             ce_old_cl, kd_mode, alpha, IGNORE, 1.0, 10.0, hip.ptr(out), hip.ptr(d), Ctot + pad,
                                             hip.ptr(part), part.numel() * 4, hip.stream()), "ucd_seg_losses_gather")
    torch.cuda.synchronize()
    res = {"loss_out": digest(out), "part": digest(part)}
    if want_d:
        assert torch.isnan(d[:, Ctot:]).all(), f"{name}: the padding columns of d_sem were written"
        res["d_sem"] = digest(d[:, :Ctot])
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else JSON_PATH
    if not all(os.path.exists(p) for p in SOURCES):
        sys.exit(f"{SOURCES[0]} is gone: this tree no longer has the kernels the record is of, and it would come from the code it is "
                 "meant to check.  Nothing written.")
    sys.path.insert(0, ROOT)
    first = {name: run_case(name) for name in CASES}
    again = {name: run_case(name) for name in CASES}
    if first != again:
        sys.exit(f"two runs disagree, nothing written: {[n for n in CASES if first[n] != again[n]]}")
    src = {}
    for p in SOURCES:
        with open(p, "rb") as f:
            src[os.path.basename(p) + "_sha256"] = hashlib.sha256(f.read()).hexdigest()
    with open(out_path, "w") as f:
        json.dump({**src, "cases": first}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{out_path}: {sum(len(d) for d in first.values())} digests over {len(CASES)} cases ({len(SM_CASES)} soft-max, "
          f"{len(BCE_CASES)} BCE), two runs agree")


if __name__ == "__main__":
    main()
