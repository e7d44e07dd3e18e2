"""CPU: the host half of the weight-gradient launch (ucd_conv_wgrad_plan, csrc/wgrad.hip).  The plan names the kernel form (tile,
strided, row3), the tile, the row chunks and their split over the XCDs, the grid, the threads, the dynamic LDS, the slab sum and
the workspace bytes of a call from its shape and the environment alone; ucd_conv_wgrad_ex launches with exactly these numbers.
Nothing here needs a device.

``parent`` below restates the launch code of the commit BEFORE the plan existed (make_plan, make_plan3 - one body, written twice
there -, wgrad_target, wgrad_three, make_sum and the grid / threads / LDS expressions of wgrad_launch_on in csrc/wgrad.hip),
independently of the library, so that every call provably keeps the launch it had.  The three tuning variables are read at every
call of the plan; ``parent`` takes them as a dict."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from ucd_amd import hip

TILE, STRIDED, ROW3 = range(3)
EINVAL, EUNSUPPORTED = -1, -4
FIELDS = tuple(n for n, _ in hip.Conv_WgradPlan._fields_)
VARS = ("UCD_WGRAD3", "UCD_WGRAD_TARGET", "UCD_WGRAD3_TARGET")
CHANNELS = (64, 128, 192, 256, 512, 1024, 2048)


def cdiv(a, b):
    return -(-a // b)


def _atoi(env, name):
    try:
        return int(env.get(name, "0"))
    except ValueError:
        return 0


def _cut(M, per_chunk, tiles_k, target):
    """chunks, rows, ksplit: the 20 lines make_plan and make_plan3 shared."""
    chunks, ksplit = min(target // per_chunk, (M + 255) // 256), 1
    if chunks >= 8:
        chunks = chunks // 8 * 8
    else:
        chunks = max(chunks, 1)
        while chunks & (chunks - 1):
            chunks -= 1
        ksplit = 8 // chunks
        while ksplit > 1 and tiles_k % ksplit:
            ksplit >>= 1
    rows = cdiv(cdiv(M, chunks), 64) * 64
    return cdiv(M, rows), rows, ksplit


def make_plan(M, N, K, taps, env):
    bno, bko = (128 if N % 128 == 0 else 64), (128 if K % 128 == 0 else 64)
    tiles_n, tiles_k = N // bno, K // bko
    per_chunk = tiles_n * tiles_k * taps
    target = _atoi(env, "UCD_WGRAD_TARGET")
    if target <= 0:                                            # wgrad_target
        target = (512 if per_chunk >= 64 else 256) if taps == 1 else (512 if per_chunk <= 9 and taps == 9 else 1024)
    return (bno, bko, tiles_n, tiles_k) + _cut(M, per_chunk, tiles_k, target)


def make_plan3(M, N, K, env):
    tiles_n, tiles_k = N // 128, K // 128
    target = _atoi(env, "UCD_WGRAD3_TARGET")
    return (128, 128, tiles_n, tiles_k) + _cut(M, tiles_n * tiles_k * 3, tiles_k, target if target > 0 else 256)


def parent_bound(M, N, K, taps, env):
    chunks = make_plan(M, N, K, taps, env)[4]
    if taps == 9 and N % 128 == 0 and K % 128 == 0:
        chunks = max(chunks, make_plan3(M, N, K, env)[4])
    return chunks * N * taps * K * 4


def parent(M, N, K, taps=1, H=0, W=0, d=1, stride=1, env={}):
    three = (taps == 9 and stride <= 1 and N % 128 == 0 and K % 128 == 0 and d <= 18 and d < W and 64 // W + 1 <= H and M >= 8192
             and not env.get("UCD_WGRAD3", "1").startswith("0"))                                       # wgrad_three
    bno, bko, tiles_n, tiles_k, chunks, rows, ksplit = make_plan3(M, N, K, env) if three else make_plan(M, N, K, taps, env)
    grid = cdiv(chunks * ksplit, 8) * 8 * tiles_n * (tiles_k // ksplit) * (3 if three else taps)
    nx = 0 if not three else 3 if 64 + 2 * d <= 96 else 4
    lds = 3 * (17408 + nx * 8 * 1024) if three else 2 * 64 * (bno + bko) * 2
    total = N * taps * K                                                                                 # make_sum
    if chunks >= 64 and total // 8 <= 16 * 1024:
        lanes, blocks = 16, (total // 8 + 15) // 16
    elif chunks >= 16 and total // 8 <= 64 * 1024:
        lanes, blocks = 4, (total // 8 + 63) // 64
    else:
        lanes, blocks = 1, (total // 8 + 255) // 256
    return dict(form=ROW3 if three else STRIDED if stride > 1 else TILE, tile_n=bno, tile_k=bko, tiles_n=tiles_n, tiles_k=tiles_k,
                chunks=chunks, rows_per_chunk=rows, ksplit=ksplit, x_tile_rows=32 * nx, grid=grid, threads=512 if three else 256,
                lds_bytes=lds, sum_lanes=lanes, sum_blocks=blocks, workspace_bytes=chunks * total * 4)


def plan(M, N, K, taps=1, H=0, W=0, d=1, stride=1):
    """dict of the plan's answers, or (error code, message)."""
    lib = hip.load()
    p = hip.Conv_WgradPlan()
    rc = lib.ucd_conv_wgrad_plan(M, N, K, taps, H, W, d, stride, C.byref(p))
    if rc:
        return rc, lib.ucd_last_error().decode()
    return {f: getattr(p, f) for f in FIELDS}


# (call, form, tile_n x tile_k (None: not stated), tiles, chunks, rows, ksplit, grid, threads, LDS, workspace, x_tile_rows, environment)
ANCHORS = [
    (dict(M=300, N=64, K=64), TILE, (64, 64), (1, 1), 2, 192, 1, 8, 256, 32768, 32768, 0, {}),
    (dict(M=1000, N=128, K=256), TILE, (128, 128), (1, 2), 4, 256, 2, 8, 256, 65536, 524288, 0, {}),
    (dict(M=26136, N=256, K=1024), TILE, None, (2, 8), 16, 1664, 1, 256, 256, 65536, 16777216, 0, {}),
    (dict(M=399384, N=64, K=256), TILE, (64, 128), (1, 2), 128, 3136, 1, 256, 256, 49152, 8388608, 0, {}),
    (dict(M=198, N=64, K=128, taps=9, H=9, W=11, d=1), TILE, (64, 128), (1, 1), 1, 256, 1, 72, 256, 49152, 294912, 0, {}),
    (dict(M=8712, N=256, K=256, taps=9, H=33, W=33, d=1), ROW3, None, (2, 2), 16, 576, 1, 192, 512, 125952, 37748736, 96, {}),
    (dict(M=8712, N=256, K=256, taps=9, H=33, W=33, d=17), ROW3, None, (2, 2), 16, 576, 1, 192, 512, 150528, 37748736, 128, {}),
    (dict(M=8712, N=256, K=256, taps=9, H=33, W=33, d=19), TILE, None, (2, 2), 23, 384, 1, 864, 256, 65536, 54263808, 0, {}),
    (dict(M=8712, N=256, K=256, taps=9, H=33, W=33, d=1), TILE, None, (2, 2), 23, 384, 1, 864, 256, 65536, 54263808, 0,
     {"UCD_WGRAD3": "0"}),
    (dict(M=8712, N=256, K=256, taps=9, H=33, W=33, d=1), ROW3, None, (2, 2), 28, 320, 1, 384, 512, 125952, 66060288, 96,
     {"UCD_WGRAD3_TARGET": "512"}),
    (dict(M=26136, N=256, K=2048, taps=9, H=33, W=33, d=12), ROW3, None, (2, 16), 2, 13120, 4, 192, 512, 125952, 37748736, 96, {}),
    (dict(M=7168, N=128, K=128, taps=9, H=32, W=32, d=1), TILE, None, (1, 1), 23, 320, 1, 216, 256, 65536, 13565952, 0, {}),
    (dict(M=60, N=128, K=128, taps=9, H=9, W=11, d=1, stride=2), STRIDED, None, (1, 1), 1, 64, 1, 72, 256, 65536, 589824, 0, {}),
]


def test_the_restatement_reproduces_the_anchors():
    """The table of the rules' answers, worked out by hand from the parent's code: ``parent`` is trusted only behind it."""
    for call, form, tile, tiles, chunks, rows, ksplit, grid, threads, lds, ws, xrows, env in ANCHORS:
        p = parent(env=env, **call)
        got = (p["form"], (p["tiles_n"], p["tiles_k"]), p["chunks"], p["rows_per_chunk"], p["ksplit"], p["grid"], p["threads"],
               p["lds_bytes"], p["workspace_bytes"], p["x_tile_rows"])
        assert got == (form, tiles, chunks, rows, ksplit, grid, threads, lds, ws, xrows), (call, env, p)
        assert tile is None or (p["tile_n"], p["tile_k"]) == tile, (call, p)


def cases():
    """Every call of the comparison grid as keyword arguments of ``plan`` / ``parent``."""
    out = []
    maps = [(b, hw) for b in (3, 6, 24) for hw in (33, 65, 129)]
    # the clamp ceil(M / 256) from both sides: 7 | 8 chunks (a power of two with ksplit | a multiple of 8), 15 | 16 and 63 | 64
    # (the lanes of the slab sum)
    clamp = [256 * c + e for c in (1, 2, 4, 7, 8, 15, 16, 17, 63, 64, 65) for e in (0, 1)]
    pairs = [(N, K) for N in CHANNELS for K in CHANNELS] + [(896, 1152), (1024, 1024)]       # 63 | 64 tiles of a 1x1 chunk: target 256 | 512
    for N, K in pairs:
        for M in [b * hw * hw for b, hw in maps] + clamp + [8192, 7168]:
            out.append(dict(M=M, N=N, K=K))
        for b, hw in maps:
            for d in (1, 2, 12, 16, 17, 18, 19, 36):                     # x_tile_rows 96 | 128 at 16 | 17, row3 | tile at 18 | 19
                out.append(dict(M=b * hw * hw, N=N, K=K, taps=9, H=hw, W=hw, d=d))
        for M in clamp:                                                  # a map of one image row: any M is B * H * W
            out.append(dict(M=M, N=N, K=K, taps=9, H=1, W=M, d=1))
        for b in (8, 7):                                                 # the three-tap form needs 8192 rows
            out.append(dict(M=b * 32 * 32, N=N, K=K, taps=9, H=32, W=32, d=1))
        for d in (15, 16):                                               # dilation < W
            out.append(dict(M=32 * 16 * 16, N=N, K=K, taps=9, H=16, W=16, d=d))
        out.append(dict(M=128 * 8 * 8, N=N, K=K, taps=9, H=8, W=8, d=1))  # 64 / W + 1 <= H: 9 > 8 | 9 <= 9
        out.append(dict(M=114 * 9 * 8, N=N, K=K, taps=9, H=9, W=8, d=1))
        if N % 128 == 0 and K % 128 == 0:                                # the strided layers
            for b, H, W in ((2, 9, 11), (3, 65, 65), (24, 65, 65), (24, 129, 129)):
                M = b * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1)
                out.append(dict(M=M, N=N, K=K, H=H, W=W, stride=2))
                out.append(dict(M=M, N=N, K=K, taps=9, H=H, W=W, d=1, stride=2))
    return out


def compare_grid(env={}):
    """Every field of every case against ``parent`` under ``env`` (the caller has put it into os.environ); returns the number of
    cases and what was seen."""
    lib = hip.load()
    n, seen = 0, dict(form=set(), x_tile_rows=set(), sum_lanes=set(), ksplit=set())
    for call in cases():
        want, got = parent(env=env, **call), plan(**call)
        assert got == want, (call, got, want)
        M, taps = call["M"], call.get("taps", 1)
        assert got["lds_bytes"] <= 160 * 1024, (call, got)
        assert got["chunks"] * got["rows_per_chunk"] >= M > (got["chunks"] - 1) * got["rows_per_chunk"], (call, got)
        assert got["rows_per_chunk"] % 64 == 0 and got["grid"] % 8 == 0, (call, got)
        bound = lib.ucd_conv_wgrad_workspace_bytes(M, call["N"], call["K"], taps)
        assert bound >= got["workspace_bytes"] and bound == parent_bound(M, call["N"], call["K"], taps, env), (call, got, bound)
        n += 1
        for k in seen:
            seen[k].add(got[k])
    return n, seen


@pytest.fixture
def no_overrides(monkeypatch):
    for v in VARS:
        monkeypatch.delenv(v, raising=False)


def test_every_call_keeps_the_launch_it_had(no_overrides):
    n, seen = compare_grid()
    assert n == len(cases()) == 51 * 133 + 27 * 8 == 6999                # nothing skipped: 51 channel pairs, 27 of them 128-aligned
    assert seen["form"] == {TILE, STRIDED, ROW3} and seen["x_tile_rows"] == {0, 96, 128}, seen
    assert seen["sum_lanes"] == {1, 4, 16} and seen["ksplit"] == {1, 2, 4, 8}, seen
    # the bounds the grid is built around are hit from both sides
    c3 = dict(N=256, K=256, taps=9)
    assert plan(M=8192, H=32, W=32, d=1, **c3)["form"] == ROW3 and plan(M=7168, H=32, W=32, d=1, **c3)["form"] == TILE
    assert [plan(M=8712, H=33, W=33, d=d, **c3)["x_tile_rows"] for d in (16, 17, 18, 19)] == [96, 128, 128, 0]
    assert plan(M=8192, H=16, W=16, d=15, **c3)["form"] == ROW3 and plan(M=8192, H=16, W=16, d=16, **c3)["form"] == TILE
    assert plan(M=8192, H=8, W=8, d=1, **c3)["form"] == TILE and plan(M=8208, H=9, W=8, d=1, **c3)["form"] == ROW3
    p7, p8 = plan(256 * 7, 128, 256), plan(256 * 7 + 1, 128, 256)        # clamped to 7 chunks: 4, the k tiles over two XCDs | to 8
    assert (p7["chunks"], p7["ksplit"], p8["chunks"], p8["ksplit"]) == (4, 2, 8, 1), (p7, p8)
    assert plan(1000, 128, 192)["ksplit"] == 1 and plan(1000, 128, 256)["ksplit"] == 2        # tiles_k 3: no split of the k tiles
    assert plan(399384, 896, 1152)["chunks"] == 4 and plan(399384, 1024, 1024)["chunks"] == 8   # 256 // 63 | 512 // 64
    assert plan(M=7168, N=128, K=128, taps=9, H=32, W=32)["chunks"] == 23                      # 512 // 9 = 56, clamped to 28 -> 24 -> 23
    assert plan(M=7168, N=256, K=128, taps=9, H=32, W=32)["chunks"] == 23                      # 1024 // 18 = 56
    assert [plan(256 * c, 256, 256)["sum_lanes"] for c in (15, 16, 63, 64)] == [1, 4, 4, 16]   # 8, 16, 56, 64 chunks
    assert plan(399384, 256, 256)["sum_lanes"] == 16 and plan(399384, 256, 512)["sum_lanes"] == 4    # 64 chunks | 32 chunks
    assert plan(M=26136, N=256, K=256, taps=9, H=33, W=33, d=19)["sum_lanes"] == 1               # 24 chunks, 73 728 groups > 65 536
    assert plan(M=26136, N=128, K=128, taps=9, H=33, W=33, d=19)["sum_lanes"] == 4


_CHILD = """
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_wgrad_plan_cpu as T
n, seen = T.compare_grid({k: os.environ[k] for k in T.VARS if k in os.environ})
print("compared", n, "forms", sorted(seen["form"]))
"""


@pytest.mark.parametrize("env", [{"UCD_WGRAD3": "0"}, {"UCD_WGRAD_TARGET": "384"}, {"UCD_WGRAD3_TARGET": "512"}],
                         ids=["wgrad3=0", "target=384", "target3=512"])
def test_overrides_are_the_parents(env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    full = {k: v for k, v in os.environ.items() if k not in VARS}
    full.update(env)
    r = subprocess.run([sys.executable, "-c", _CHILD % dict(root=root, tests=os.path.join(root, "tests"))], env=full,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.strip()
    assert out.startswith(f"compared {len(cases())} "), out
    assert (str(ROW3) in out.split("forms")[1]) == ("UCD_WGRAD3" not in env), out


def test_the_variables_are_read_at_every_call(no_overrides):
    """tests/test_conv1x1_fused_gpu.py (the three-tap / nine-tap comparison) and tools/wgrad_probe2.py change them inside one
    process."""
    call = dict(M=8712, N=256, K=256, taps=9, H=33, W=33, d=1)
    forms = [plan(**call)["form"]]
    os.environ["UCD_WGRAD3"] = "0"
    try:
        forms.append(plan(**call)["form"])
        bound0 = hip.load().ucd_conv_wgrad_workspace_bytes(8712, 256, 256, 9)
    finally:
        del os.environ["UCD_WGRAD3"]
    forms.append(plan(**call)["form"])
    assert forms == [ROW3, TILE, ROW3]
    assert bound0 == 54263808 == hip.load().ucd_conv_wgrad_workspace_bytes(8712, 256, 256, 9)     # the bound covers both forms
    # the five shapes of the GPU comparison take the form it names
    for M, N, K, sp in [(26136, 256, 256, (33, 33, 1)), (26136, 512, 512, (33, 33, 2)), (26136, 256, 2048, (33, 33, 12)),
                        (23 * 33 * 33, 128, 128, (33, 33, 18)), (24 * 65 * 65, 128, 128, (65, 65, 1))]:
        call = dict(M=M, N=N, K=K, taps=9, H=sp[0], W=sp[1], d=sp[2])
        assert parent(**call)["form"] == ROW3 and parent(env={"UCD_WGRAD3": "0"}, **call)["form"] == TILE, call


def test_shapes_no_call_could_launch_are_refused(no_overrides):
    """The plan's code and message are the call's: the same arguments go to ucd_conv_wgrad_ex with operand addresses that are
    never dereferenced (every one of these is refused before the first use of the device)."""
    lib = hip.load()
    geometry = "ucd_conv_wgrad: the 3x3 / strided forms need H, W, dilation and M = B*OH*OW"
    refused = [
        (dict(M=128, N=96, K=64), EUNSUPPORTED, "ucd_conv_wgrad: N (96) and K (64) must be multiples of 64"),
        (dict(M=128, N=64, K=64, taps=3), EINVAL, "ucd_conv_wgrad: taps must be 1 or 9"),
        (dict(M=128, N=64, K=64, taps=9), EINVAL, geometry),
        (dict(M=1000, N=64, K=64, taps=9, H=33, W=33, d=1), EINVAL, geometry),
        (dict(M=60, N=64, K=128, H=9, W=11, stride=2), EUNSUPPORTED, "ucd_conv_wgrad: the strided form takes N and K multiples of 128"),
        (dict(M=1 << 22, N=64, K=64), EUNSUPPORTED, "ucd_conv_wgrad: M = 4194304 rows exceed the index arithmetic of the 3x3 form (2^22)"),
    ]
    for call, code, message in refused:
        assert plan(**call) == (code, message), call
        M, N, K, taps = call["M"], call["N"], call["K"], call.get("taps", 1)
        rc = lib.ucd_conv_wgrad_ex(16, N, 16, K, M, N, K, taps, call.get("H", 0), call.get("W", 0), call.get("d", 1),
                                   call.get("stride", 1), 16, None, 0, 16, 1 << 40, 0, None)
        assert (rc, lib.ucd_last_error().decode()) == (code, message), call
    # wrong in several ways: the first check in the call's order answers
    assert plan(M=128, N=96, K=64, taps=3)[0] == EUNSUPPORTED and plan(M=1 << 22, N=64, K=64, taps=9)[0] == EINVAL
    assert lib.ucd_conv_wgrad_plan(300, 64, 64, 1, 0, 0, 1, 1, None) == EINVAL


def test_python_binding(no_overrides):
    assert hip.WGRAD_FORMS == ("tile", "strided", "row3")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ucd_hip.h")).read()
    assert "#define UCD_WGRAD_FORM_NAMES {" + ", ".join(f'"{n}"' for n in hip.WGRAD_FORMS) + "}" in header
    p = hip.conv_wgrad_plan(1000, 128, 256)
    assert (p["form"], p["chunks"], p["rows_per_chunk"], p["ksplit"], p["grid"], p["workspace_bytes"]) == ("tile", 4, 256, 2, 8, 524288), p
    p = hip.conv_wgrad_plan(8712, 256, 256, conv3=(33, 33, 17))
    assert (p["form"], p["x_tile_rows"], p["chunks"], p["grid"], p["threads"], p["lds_bytes"]) == ("row3", 128, 16, 192, 512, 150528), p
    p = hip.conv_wgrad_plan(60, 128, 128, conv3=(9, 11, 1, 2))
    assert (p["form"], p["grid"], p["workspace_bytes"]) == ("strided", 72, 589824), p
    assert hip.conv_wgrad_plan(60, 128, 128, strided=(9, 11, 2))["form"] == "strided"
    with pytest.raises(RuntimeError, match="multiples of 64"):
        hip.conv_wgrad_plan(128, 96, 64)
