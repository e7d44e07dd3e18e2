"""CPU: the host half of the fused logit-loss launch (ucd_seg_losses_plan, csrc/seglogit_loss.hip).  The plan decides
which of the kernel forms a call gets, how many low-resolution cells are staged per tile and how many bytes of LDS the
launch asks for; the kernels index that LDS with their own source-index arithmetic (up_src).  Nothing here needs a
device: the plan is a host function of libucd_hip.so."""
import ctypes as C

import numpy as np
import pytest

from ucd_amd import hip

PK16, PK20, PK12, REG16, REG24, WIDE_FX, WIDE_F32 = 1, 2, 3, 4, 5, 6, 7
EINVAL, EUNSUPPORTED = -1, -4
LDS_BUDGET = 150 * 1024


def plan(H, W, h, w, Ctot, K, teacher=1, aligned=1, pk=1):
    """(form, ny, nx, lds_bytes) or (error code, message)."""
    lib = hip.load()
    f, ny, nx, lds = C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
    rc = lib.ucd_seg_losses_plan(H, W, h, w, Ctot, K, teacher, aligned, pk, C.byref(f), C.byref(ny), C.byref(nx), C.byref(lds))
    if rc:
        return rc, lib.ucd_last_error().decode()
    return f.value, ny.value, nx.value, lds.value


def up_src_np(out, in_size):
    """The kernels' up_src for every destination index 0 .. out-1 in numpy float32: the same operations in the same order
    (scale = float(in) / float(out); src = scale * (dst + 0.5) - 0.5; clamp at 0; truncate; clamp at in - 1).  The library is
    compiled with -ffp-contract=off, so the device evaluates exactly these separately rounded float32 operations and no
    fused multiply-add: that is what makes a numpy restatement a statement about the kernel."""
    scale = np.float32(in_size) / np.float32(out)
    src = scale * (np.arange(out, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5)
    src = np.where(src < np.float32(0), np.float32(0), src)
    i0 = np.minimum(src.astype(np.int32), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    return i0, i1


def footprint(out, in_size, tile):
    """Largest number of source cells any tile touches, from EVERY pixel of every tile."""
    i0, i1 = up_src_np(out, in_size)
    starts = np.arange(0, out, tile)
    return int((np.maximum.reduceat(i1, starts) - np.minimum.reduceat(i0, starts) + 1).max())


def test_plan_footprint_covers_every_pixel_of_every_tile():
    """For every (out, in) with in = 1 .. 100, 4 <= out / in <= 64 and out <= 1100: the cells the plan sizes the LDS for equal the
    largest per-tile footprint of the kernels' source-index arithmetic over all pixels (not only a tile's first and last),
    for the 64-row tiles of the few-class forms, the 32-row tiles of the many-class form and the 64-pixel tile width.  A plan
    below the footprint would be an LDS overrun (the packed form traps, the other forms do not check); one above it wastes LDS
    that decides the occupancy."""
    checked = 0
    for in_size in range(1, 101):
        for out in range(4 * in_size, min(64 * in_size, 1100) + 1):
            f64, f32 = footprint(out, in_size, 64), footprint(out, in_size, 32)
            # the other axis is 4 <- 1 (one cell), so the LDS budget never interferes; 2 classes: 64-row tiles, 25: 32-row tiles
            p = plan(out, 4, in_size, 1, 2, 1, teacher=0)
            assert p[1:3] == (f64, 1), (out, in_size, p, f64)
            p = plan(out, 4, in_size, 1, 25, 1, teacher=0)
            assert p[0] == WIDE_FX and p[1:3] == (f32, 1), (out, in_size, p, f32)
            p = plan(4, out, 1, in_size, 2, 1, teacher=0)
            assert p[1:3] == (1, f64), (out, in_size, p, f64)
            checked += 1
    assert checked > 80000


def test_plan_pins_the_benchmark_geometry():
    """VOC 15-5 at 513 <- 33: the packed <16,8> form on 6 x 6 cells with the LDS bytes of the round-5 launch (two workgroups per
    CU); the many-class form at ADE's 512 <- 32."""
    assert plan(513, 513, 33, 33, 21, 16) == (PK16, 6, 6, 65544)
    assert plan(512, 512, 32, 32, 21, 16) == (PK16, 6, 6, 65544)
    assert plan(512, 512, 32, 32, 151, 101) == (WIDE_FX, 4, 6, 83040)


@pytest.mark.parametrize("Ctot,K,aligned,pk,form", [
    (21, 16, 1, 1, PK16),       # VOC 15-5
    (20, 14, 1, 1, PK16),       # Cityscapes 13-6
    (21, 20, 1, 1, PK20),       # VOC 19-1 step 1, 15-5s step 5
    (17, 16, 1, 1, PK16),       # 15-5s step 1 fits the first packed form already
    (21, 11, 1, 1, PK12),       # VOC 10-10
    (24, 12, 1, 1, PK12),
    (21, 1, 1, 1, REG16),       # step 0: one old class, no packed form holds 20 new ones
    (21, 16, 1, 0, REG16),      # UCD_SEG_PK=0
    (21, 16, 0, 1, REG16),      # d_sem off the 16-byte grid
    (21, 11, 1, 0, REG16),
    (21, 20, 1, 0, REG24),
    (21, 20, 0, 1, REG24),
    (24, 18, 1, 1, REG24),      # K > 16, 6 new classes: no packed form
    (24, 18, 1, 0, REG24),
    (25, 16, 1, 1, WIDE_FX),    # first class count of the many-class form
    (151, 101, 1, 1, WIDE_FX),  # ADE 100-50
    (151, 101, 1, 0, WIDE_FX),  # the switch does not touch it
    (151, 101, 0, 1, WIDE_F32),
    (151, 1, 0, 1, WIDE_F32),
])
def test_plan_form_table(Ctot, K, aligned, pk, form):
    got = plan(513, 513, 33, 33, Ctot, K, teacher=int(K > 1), aligned=aligned, pk=pk)
    assert got[0] == form and got[1:3] == ((6, 6) if Ctot <= 24 else (4, 6)), got
    assert got[3] <= LDS_BUDGET


def test_plan_reads_the_switch_once_per_process(tmp_path):
    """pk = -1 asks the process's UCD_SEG_PK (cached in a function static): a child per value."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import ctypes as C\nfrom ucd_amd import hip\nlib = hip.load()\nf = C.c_int()\n"
            "assert lib.ucd_seg_losses_plan(513, 513, 33, 33, 21, 16, 1, 1, -1, C.byref(f), None, None, None) == 0\nprint(f.value)\n")
    for value, form in ((None, PK16), ("1", PK16), ("0", REG16)):
        env = {k: v for k, v in os.environ.items() if k != "UCD_SEG_PK"}
        env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
        if value is not None:
            env["UCD_SEG_PK"] = value
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=root)
        assert out.returncode == 0, out.stderr
        assert int(out.stdout.split()[-1]) == form, (value, out.stdout)


SPLITS = {"voc 15-5": (21, 16), "voc 15-5s step 2": (17, 16), "voc 15-5s step 5": (21, 20), "voc 19-1": (21, 20),
          "voc 10-10": (21, 11), "cityscapes 13-6": (20, 14), "voc 19-1 step 0": (20, 1), "ade 100-50": (151, 101)}
# form at --output_stride 16 / 8 (DESIGN.md section 3.5 carries this table); None: not served
SERVED = {"voc 15-5": (PK16, REG16), "voc 15-5s step 2": (PK16, REG16), "voc 15-5s step 5": (PK20, REG24), "voc 19-1": (PK20, REG24),
          "voc 10-10": (PK12, REG16), "cityscapes 13-6": (PK16, REG16), "voc 19-1 step 0": (REG16, REG16),
          "ade 100-50": (WIDE_FX, None)}


@pytest.mark.parametrize("crop", [512, 513, 768])
@pytest.mark.parametrize("split", sorted(SPLITS))
def test_plan_supported_range_of_the_launcher(split, crop):
    """The launcher's crops x --output_stride 16 and 8 x the class splits of the benchmark configurations plus 19-1 and 10-10.
    Stride 16 keeps the round-5 forms; at stride 8 a 64 x 64 tile covers 10 x 10 cells: the packed forms' eight accumulator
    copies pass the LDS budget and the register form takes over (fp32-atomic gradient); ADE's many-class form fits nowhere at
    stride 8 and the call must say so - with the factor and the bytes, not the class count."""
    Ctot, K = SPLITS[split]
    teacher = int(K > 1)
    for stride, want in zip((16, 8), SERVED[split]):
        hw = (crop - 1) // stride + 1
        got = plan(crop, crop, hw, hw, Ctot, K, teacher=teacher)
        if want is None:
            assert got[0] == EUNSUPPORTED, got
            assert "factors" in got[1] and "207456 bytes" in got[1] and ("%.4g" % (crop / hw)) in got[1], got
        else:
            cells = (4 if Ctot > 24 else 6, 6) if stride == 16 else (10, 10)
            assert got[0] == want and got[1:3] == cells and got[3] <= LDS_BUDGET, (stride, got)


def test_plan_stride_8_falls_back_to_the_register_form():
    """512 <- 64 with 21 classes: the packed form asks for 8 x (2400 + 1) x 8 bytes of accumulators alone, over the budget; the
    register form needs (100 x (17 x 21 + 16) + 8) x 4 = 149 232 bytes and is taken."""
    assert plan(512, 512, 64, 64, 21, 16) == (REG16, 10, 10, 149232)
    assert plan(512, 512, 64, 64, 21, 16, pk=0) == (REG16, 10, 10, 149232)
    # one axis at 8 only: 6 x 10 cells, the packed form still fits
    got = plan(512, 512, 32, 64, 21, 16)
    assert got[0] == PK16 and got[1:3] == (6, 10)


def test_plan_rejections():
    for args in ((0, 64, 1, 4, 21, 16), (64, 64, 0, 4, 21, 16), (64, 64, 4, 4, 0, 1), (64, 64, 4, 4, 21, 0), (64, 64, 4, 4, 21, 22)):
        got = plan(*args)
        assert got[0] == EINVAL and "bad sizes" in got[1], got
    got = plan(16, 64, 32, 4, 21, 16)
    assert got[0] == EINVAL and "bad scale" in got[1], got
    got = plan(65 * 4, 64, 4, 4, 21, 16)
    assert got[0] == EUNSUPPORTED and "above 64" in got[1], got
    got = plan(64, 15, 4, 4, 21, 16)
    assert got[0] == EUNSUPPORTED and "below 4" in got[1], got
    got = plan(400, 400, 100, 100, 21, 16)             # factor 4 with 21 classes: 19 x 19 cells
    assert got[0] == EUNSUPPORTED and "factors 4 x 4" in got[1] and "bytes of LDS" in got[1], got
    got = plan(512, 512, 32, 32, 2000, 16)              # class count beyond the LDS at the model's own factor
    assert got[0] == EUNSUPPORTED and "bytes of LDS for 2000 classes" in got[1], got
    assert plan(64 * 2, 64 * 2, 2, 2, 21, 16)[0] == PK16   # exactly 64 is served
    assert plan(16, 16, 4, 4, 21, 16)[0] == PK16           # exactly 4 (smaller than one tile)
