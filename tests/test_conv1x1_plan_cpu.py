"""CPU: the host half of the conv GEMM launch (ucd_conv1x1_plan, csrc/conv1x1.hip).  The plan names the kernel form (single stage,
double buffer, loader waves on 128- / 256- / 64-row tiles), the tile, the grid, the threads and the dynamic LDS of a product from
its shape and mode alone; ucd_conv1x1 launches with exactly these numbers.  Nothing here needs a device.

``parent`` below restates the launch code of the commit BEFORE the plan existed (the body of ucd_conv1x1, pick_pipe, launch_db and
the single-stage launch macros of csrc/conv1x1.hip), independently of the library, so that every product provably keeps the launch
it had.  The three tuning variables are read once per process: each override is compared in one child process."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import pytest

from ucd_amd import hip

SINGLE, DB, LW128, LW256, LW64 = range(5)
EINVAL, EUNSUPPORTED = -1, -4
ROWS = {SINGLE: 128, DB: 128, LW128: 128, LW256: 256, LW64: 64}
THREADS = {SINGLE: 256, DB: 256, LW128: 512, LW256: 1024, LW64: 384}
PIPES = {"2x64": DB, "lw64": LW128, "lw256": LW256}          # UCD_CONV_PIPE: lw64 is the loader-wave form on 128-row tiles
FIELDS = ("form", "tile_rows", "tile_cols", "tiles_m", "tiles_n", "grid", "threads", "lds_bytes", "param_off")
NS = (64, 128, 192, 256, 512, 1024, 2048)
KS = (64, 192, 256, 2048)                                    # 192 / 256: nk64 = 3 / 4 for a 1x1 product


def cdiv(a, b):
    return -(-a // b)


def parent(M, N, K, taps, out_mode, stat_acc, pro, forced=None, bn64_below=128, lw64_below=128):
    t128 = cdiv(M, 128)
    BN = 128 if N % 128 == 0 and t128 * (N // 128) > bn64_below else 64
    tiles_n = N // BN
    db = ((taps == 9 or not pro) and t128 * tiles_n <= 640) or (out_mode == 4 and BN == 128)
    if not db or pro:
        form = SINGLE
    else:
        nk64 = (9 if taps == 9 else 1) * K // 64
        if forced is not None:
            form = forced
        elif t128 * tiles_n <= 256 and nk64 >= 4:
            form = LW128
        elif BN == 128 and out_mode <= 2 and cdiv(M, 256) * tiles_n <= 256 and nk64 >= 4:
            form = LW256
        else:
            form = DB
        if form == LW128 and BN == 64 and t128 * tiles_n <= lw64_below and (out_mode < 2 or stat_acc):
            form = LW64
        if form == LW256 and (BN == 64 or out_mode > 2):
            form = DB
    k_out, k_red = 64 * (BN + 4) * 4, 16384
    lds = {SINGLE: max((128 + BN) * 128, k_out, k_red), DB: max((128 + BN) * 256, k_out, k_red),
           LW128: max((128 + BN) * 384, k_out, k_red), LW256: max((256 + BN) * 384, k_out), LW64: (64 + BN) * 384}[form]
    param_off = 0
    if pro:
        param_off = cdiv(lds, 16) * 16
        lds = param_off + 3 * K * 4
    tiles_m = cdiv(M, ROWS[form])
    return dict(form=form, tile_rows=ROWS[form], tile_cols=BN, tiles_m=tiles_m, tiles_n=tiles_n, grid=cdiv(tiles_m, 8) * 8 * tiles_n,
                threads=THREADS[form], lds_bytes=lds, param_off=param_off)


def plan(M, N, K, taps=1, out_mode=0, stat_acc=False, pro=False):
    """dict of the plan's answers, or (error code, message)."""
    lib = hip.load()
    d, p = hip.Conv1x1Desc(), hip.Conv1x1Plan()
    d.M, d.N, d.K, d.taps, d.out_mode = M, N, K, taps, out_mode
    d.in_scale, d.stat_acc = (16 if pro else None), (16 if stat_acc else None)       # never dereferenced
    rc = lib.ucd_conv1x1_plan(C.byref(d), C.byref(p))
    if rc:
        return rc, lib.ucd_last_error().decode()
    return {f: getattr(p, f) for f in FIELDS}


def row_counts(N, bn64_below=128):
    """3 / 6 / 24 images of the three map sizes, and per column width the M on either side of every bound of the rules:
    t128 * tiles_n at 128 | 129, 256 | 257, 640 | 641 and ceil(M / 256) * tiles_n at 256 | 257 (the largest M at or below the bound
    and the next row, which starts one more row tile)."""
    ms = {b * hw * hw for b in (3, 6, 24) for hw in (33, 65, 129)}
    for BN in (64, 128):
        if N % BN:
            continue
        tiles_n = N // BN
        for bound in (128, 256, 640, bn64_below):
            if bound // tiles_n:
                ms |= {bound // tiles_n * 128, bound // tiles_n * 128 + 1}
        ms |= {256 // tiles_n * 256, 256 // tiles_n * 256 + 1} if 256 // tiles_n else set()
    return sorted(ms)


def modes():
    """(taps, out_mode, stat_acc, pro) that validation lets through: out_mode 4 and the input transform on 1x1 products only, never
    together."""
    for taps, out_mode, stat_acc, pro in itertools.product((1, 9), range(5), (False, True), (False, True)):
        if (taps == 9 and (out_mode == 4 or pro)) or (out_mode == 4 and pro):
            continue
        yield taps, out_mode, stat_acc, pro


def compare_grid(forced=None, bn64_below=128, lw64_below=128):
    """Every field of every case against ``parent``; returns the number of cases and the forms seen."""
    n, seen = 0, set()
    for N in NS:
        for M in row_counts(N, bn64_below):
            for K in KS:
                for taps, out_mode, stat_acc, pro in modes():
                    want = parent(M, N, K, taps, out_mode, stat_acc, pro, forced, bn64_below, lw64_below)
                    got = plan(M, N, K, taps, out_mode, stat_acc, pro)
                    assert got == want, ((M, N, K, taps, out_mode, stat_acc, pro), got, want)
                    assert got["lds_bytes"] <= 160 * 1024 and (got["form"] != SINGLE or got["lds_bytes"] <= 64 * 1024), got
                    assert got["tiles_m"] * got["tile_rows"] >= M > (got["tiles_m"] - 1) * got["tile_rows"]
                    n, seen = n + 1, seen | {got["form"]}
    return n, seen


def test_every_product_keeps_the_launch_it_had():
    n, seen = compare_grid()
    assert seen == {SINGLE, DB, LW128, LW256, LW64}, seen
    assert n == sum(len(row_counts(N)) for N in NS) * len(KS) * len(list(modes()))      # nothing skipped
    # the bounds the grid is built around are hit from both sides
    for M, N, BN in ((128 * 128, 128, 64), (128 * 128 + 1, 128, 128), (64 * 128, 256, 64), (64 * 128 + 1, 256, 128)):
        assert plan(M, N, 256)["tile_cols"] == BN, (M, N)
    assert plan(128 * 128, 256, 256)["form"] == LW128 and plan(128 * 128 + 1, 256, 256)["form"] == LW256       # 256 | 258 tiles
    assert plan(128 * 256, 256, 256)["form"] == LW256 and plan(128 * 256 + 1, 256, 256)["form"] == DB          # 256 | 258 as 256 rows
    assert plan(320 * 128, 256, 256)["form"] == DB and plan(320 * 128 + 1, 256, 256)["form"] == SINGLE         # 640 | 642 tiles
    assert plan(128 * 128, 64, 192)["form"] == DB and plan(128 * 128, 64, 256)["form"] == LW64                 # nk64 3 | 4
    assert plan(128 * 128 + 1, 64, 256)["form"] == LW128                                                       # 129 tiles of 128 x 64


_CHILD = """
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_conv1x1_plan_cpu as T
n, seen = T.compare_grid(%(args)s)
print("compared", n, "forms", sorted(seen))
"""

_UNKNOWN_CHILD = """
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_conv1x1_plan_cpu as T
print(T.plan(26136, 256, 256))
"""


def _child(script, env_over, **fmt):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **env_over)
    for k in ("UCD_CONV_PIPE", "UCD_CONV_BN64_TILES", "UCD_CONV_LW64_TILES"):
        if k not in env_over:
            env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", script % dict(root=root, tests=os.path.join(root, "tests"), **fmt)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.strip()


@pytest.mark.parametrize("env,args", [({"UCD_CONV_PIPE": "2x64"}, "forced=T.DB"), ({"UCD_CONV_PIPE": "lw64"}, "forced=T.LW128"),
                                      ({"UCD_CONV_PIPE": "lw256"}, "forced=T.LW256"), ({"UCD_CONV_BN64_TILES": "0"}, "bn64_below=0"),
                                      ({"UCD_CONV_LW64_TILES": "0"}, "lw64_below=0")],
                         ids=["2x64", "lw64", "lw256", "bn64_tiles=0", "lw64_tiles=0"])
def test_overrides_are_the_parents(env, args):
    out = _child(_CHILD, env, args=args)
    assert out.startswith("compared") and "compared 0 " not in out, out
    if env.get("UCD_CONV_PIPE") == "lw256":
        assert str(DB) in out.split("forms")[1], out        # the fall-back of 64-column tiles and out_mode 3 / 4 was compared
    if "UCD_CONV_LW64_TILES" in env:
        assert str(LW64) not in out.split("forms")[1], out


def test_an_unknown_pipeline_form_is_refused_by_the_plan():
    out = _child(_UNKNOWN_CHILD, {"UCD_CONV_PIPE": "lw128"})
    assert out.startswith(f"({EINVAL},") and "UCD_CONV_PIPE=lw128" in out, out
    assert all(name in out for name in ("auto", "2x64", "lw64", "lw256")), out


def test_shapes_no_call_could_launch_are_refused():
    assert plan(0, 64, 64)[0] == EINVAL and plan(128, 64, 64, taps=3)[0] == EINVAL and plan(128, 64, 64, out_mode=5)[0] == EINVAL
    assert plan(128, 64, 96)[0] == EUNSUPPORTED and plan(128, 96, 64)[0] == EUNSUPPORTED
    assert plan(128, 64, 64, taps=9, out_mode=4)[0] == EINVAL and plan(128, 64, 64, taps=9, pro=True)[0] == EINVAL
    assert plan(128, 64, 64, out_mode=4, pro=True)[0] == EINVAL
    # the input-transform constants next to the single stage: 3 K floats behind 24 576 bytes (64 columns) or 33 792 (128 columns)
    got = plan(26136, 256, 2752, pro=True)
    assert got[0] == EUNSUPPORTED and "K = 2752 is too wide" in got[1], got
    assert plan(26136, 64, 2752, pro=True)["lds_bytes"] == 24576 + 3 * 2752 * 4
    assert hip.load().ucd_conv1x1_plan(None, None) == EINVAL


def test_python_binding():
    assert hip.CONV_FORMS == ("single", "2x64", "lw/128", "lw/256", "lw/64")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ucd_hip.h")).read()
    assert "#define UCD_CONV_FORM_NAMES {" + ", ".join(f'"{n}"' for n in hip.CONV_FORMS) + "}" in header
    # the ASPP branch shapes of tests/test_conv3_tap_classes_gpu.py's default-choice test
    p = hip.conv1x1_plan(33 * 33, 64, 64, taps=9)
    assert (p["form"], p["tile_rows"], p["tile_cols"], p["grid"], p["threads"]) == ("lw/64", 64, 64, 24, 384), p
    p = hip.conv1x1_plan(24 * 33 * 33, 256, 64, taps=9)
    assert (p["form"], p["tile_rows"], p["tiles_m"] * p["tiles_n"], p["lds_bytes"]) == ("lw/256", 256, 206, 147456), p
    p = hip.conv1x1_plan(24 * 33 * 33, 512, 64, taps=9)
    assert (p["form"], p["tile_rows"], p["tiles_m"] * p["tiles_n"], p["lds_bytes"]) == ("single", 128, 820, 33792), p      # the fp32 output tile: 64 x (128 + 4) floats
    assert hip.conv1x1_plan(3267, 256, 1024, out_mode=2)["form"] == "lw/128"
    assert hip.conv1x1_plan(3267, 256, 1024, out_mode=2, stat_acc=True)["form"] == "lw/64"
    assert hip.conv1x1_plan(26136, 256, 256, in_transform=True)["param_off"] == 33792
    with pytest.raises(RuntimeError, match="multiples of 64"):
        hip.conv1x1_plan(128, 64, 96)
