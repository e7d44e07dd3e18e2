"""GPU: the stand-alone dilated 3x3 products (the ASPP branches, modules/deeplab.py:27-29) on class-ordered rows
(csrc/conv1x1.hip RT kernels, csrc/conv3_taps.h; ``UCD_CONV3_TAP_CLASSES``).  The rows of the implicit GEMM are taken in the order
of the plan and every row tile walks only the taps of its mask; the skipped steps would have added exact zeros and the live steps
keep their order, so the claim is BIT equality with the raster order - for every tile form, forward and input gradient - next to
the float64 convolution of the same bf16 operands (the bound of tests/test_conv1x1_gpu.py's dilated case: 0.03 of the largest
reference value, one bf16 rounding of the output).  Shapes: several tiles, several classes per axis, tiles that mix classes and
images, an M tail.  ``UCD_CONV_PIPE`` and the tile bounds are read once per process: one child process per forced form."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (B, H = W, d, K, N)
SMALL = [(3, 17, 6, 128, 128), (3, 17, 12, 128, 128), (2, 33, 18, 64, 128)]
TOL = 0.03      # tests/test_conv1x1_gpu.py::test_dilated_3x3_skips_only_kernel_rows_that_read_padding


def _operands(B, hw, d, K, N, dev):
    g = torch.Generator(dev).manual_seed(K + N + d + B)
    cl = torch.channels_last
    x = torch.randn(B, K, hw, hw, device=dev, generator=g).bfloat16().contiguous(memory_format=cl)
    w = (torch.randn(N, K, 3, 3, device=dev, generator=g) * (2.0 / (9 * K)) ** 0.5).bfloat16().contiguous(memory_format=cl)
    dy = torch.randn(B, N, hw, hw, device=dev, generator=g).bfloat16().contiguous(memory_format=cl)
    return x, w, dy


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _product(a, w, hw, d, on, accumulate_into=None):
    """The 3x3 product of map ``a`` with weight ``w`` through ucd_conv1x1, with the switch ``on`` (0 off, 1 on, 2 on for every
    launch: also those mode 1 leaves in raster order) - and the proof of the path: the library's count of launches that took the
    class-ordered kernels grows by exactly one, or not at all."""
    from ucd_amd import hip
    N, K = w.shape[0], w.shape[1]
    if accumulate_into is None:
        y = torch.full((a.shape[0], N, hw, hw), float("nan"), device=a.device, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    else:
        y = accumulate_into.clone(memory_format=torch.channels_last)
    hip.conv3_tap_classes(int(on))
    before = hip.conv3_tap_stats()[0]
    hip.conv1x1(_rows(a), w.permute(0, 2, 3, 1).reshape(N, 9 * K), _rows(y), conv3=(hw, hw, d), accumulate=accumulate_into is not None)
    took, tile_rows, last = hip.conv3_tap_stats()
    assert tile_rows == hip.conv1x1_plan(a.shape[0] * hw * hw, N, K, taps=9)["tile_rows"], tile_rows     # the launch is the plan's
    if int(on) != 1:
        assert took - before == (1 if on else 0) and last == bool(on), (on, took - before, last)
    return y


def check_case(B, hw, d, K, N, dev):
    """Forward and input gradient (the same kernel on the flipped, transposed weight) of one shape: on == off bit for bit, and both
    within TOL of float64.  Returns the figures."""
    from ucd_amd import hip
    x, w, dy = _operands(B, hw, d, K, N, dev)
    wt = w.flip(2, 3).transpose(0, 1).contiguous(memory_format=torch.channels_last)
    out = {}
    was = hip.conv3_tap_classes()
    try:
        for name, a, ww in (("fwd", x, w), ("dgrad", dy, wt)):
            off = _product(a, ww, hw, d, 0)
            on = _product(a, ww, hw, d, 2)
            again = _product(a, ww, hw, d, 2)              # the plan is resident now
            ref = F.conv2d(a.double(), ww.double(), None, 1, d, d)
            err = (on.double() - ref).abs().max().item()
            bound = TOL * ref.abs().max().item()
            print(f"{name} B={B} {hw}x{hw} d={d} K={K} N={N}: max err {err:.3e} bound {bound:.3e}")
            assert torch.equal(on, off), (name, (on.float() - off.float()).abs().max().item())
            assert torch.equal(again, on), name
            assert err < bound, (name, err, bound)
            out[name] = (err, bound)
    finally:
        hip.conv3_tap_classes(was)
    return out


def test_class_ordered_rows_equal_raster_order_in_the_form_the_grid_picks():
    """No forced form: these grids take the 64-row loader-wave form (<= 128 tiles of 128 x 64)."""
    dev = torch.device("cuda:0")
    for case in SMALL:
        check_case(*case, dev)


_FORMS = {
    "2x64": {"UCD_CONV_PIPE": "2x64"},                                           # double-buffered, 128 x 64 tiles
    "2x64-bn128": {"UCD_CONV_PIPE": "2x64", "UCD_CONV_BN64_TILES": "0"},          # double-buffered, 128 x 128 tiles
    "lw64": {"UCD_CONV_PIPE": "lw64"},                                           # loader waves, 64-row tiles
    "lw64-128rows": {"UCD_CONV_PIPE": "lw64", "UCD_CONV_LW64_TILES": "0"},        # loader waves, 128-row tiles
    "lw256": {"UCD_CONV_PIPE": "lw256", "UCD_CONV_BN64_TILES": "0"},              # loader waves, 256-row tiles (128 columns)
}

_CHILD = """
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import torch
import test_conv3_tap_classes_gpu as T
dev = torch.device("cuda:0")
for case in T.SMALL:
    T.check_case(*case, dev)
print("all equal")
"""


@pytest.mark.parametrize("form", sorted(_FORMS))
def test_class_ordered_rows_equal_raster_order_in_every_forced_form(form):
    env = dict(os.environ, **_FORMS[form])
    for k in ("UCD_CONV_PIPE", "UCD_CONV_BN64_TILES", "UCD_CONV_LW64_TILES", "UCD_CONV3_TAP_CLASSES"):
        if k not in _FORMS[form]:
            env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], env=env,
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "all equal" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_single_stage_form_of_the_full_grids():
    """More than 640 tiles of 128 x 128 (the benchmark's input gradients, 256 -> 2048 at 24 images: 3280): the single-stage form at
    four workgroups per CU.  Here 205 row tiles x 4 column tiles; all nine classes, tiles that mix classes and images."""
    check_case(24, 33, 18, 64, 512, torch.device("cuda:0"))


def test_accumulating_product_reads_and_writes_the_same_permuted_rows():
    """out_mode 0 with accumulate: the old y of a GEMM row is read from the row it is written to."""
    dev = torch.device("cuda:0")
    B, hw, d, K, N = SMALL[0]
    x, w, dy = _operands(B, hw, d, K, N, dev)
    from ucd_amd import hip
    was = hip.conv3_tap_classes()
    try:
        off = _product(x, w, hw, d, 0, accumulate_into=dy)
        on = _product(x, w, hw, d, 2, accumulate_into=dy)
    finally:
        hip.conv3_tap_classes(was)
    assert torch.equal(on, off)
    ref = F.conv2d(x.double(), w.double(), None, 1, d, d) + dy.double()
    assert (on.double() - ref).abs().max().item() < TOL * ref.abs().max().item()


def test_dilation_beyond_the_map_is_the_1x1_product_of_the_centre_weights():
    """B = 2, 9 x 9, d = 12: no pixel has a neighbour at distance d inside the map - centre tap only, one class."""
    from ucd_amd import hip
    dev = torch.device("cuda:0")
    B, hw, d, K, N = 2, 9, 12, 128, 128
    x, w, _ = _operands(B, hw, d, K, N, dev)
    was = hip.conv3_tap_classes()
    try:
        off = _product(x, w, hw, d, 0)
        on = _product(x, w, hw, d, 2)
    finally:
        hip.conv3_tap_classes(was)
    centre = w[:, :, 1, 1].contiguous()
    one = torch.empty(B * hw * hw, N, device=dev, dtype=torch.bfloat16)
    hip.conv1x1(_rows(x).contiguous(), centre, one)
    assert torch.equal(on, off)
    assert torch.equal(_rows(on), one)
    ref = F.conv2d(x.double(), centre.double()[:, :, None, None])
    assert (on.double() - ref).abs().max().item() < TOL * ref.abs().max().item()


def test_default_mode_leaves_single_wave_64_row_launches_whose_heaviest_tile_keeps_its_taps():
    """Mode 1 (the default): 3 images of 17 x 17 run on 64-row tiles, one workgroup per CU at the most.  At d = 6 the pixels of
    rows and columns 6 .. 10 have all four neighbours: the heaviest tile walks nine taps in either order, and the launch stays in
    raster order.  At d = 12 no pixel has both neighbours of an axis: heaviest tile 6 -> 4 taps, class order."""
    from ucd_amd import hip
    dev = torch.device("cuda:0")
    was = hip.conv3_tap_classes()
    try:
        for (B, hw, d, K, N), want in ((SMALL[0], False), (SMALL[1], True)):
            x, w, _ = _operands(B, hw, d, K, N, dev)
            off = _product(x, w, hw, d, 0)
            before = hip.conv3_tap_stats()[0]
            on = _product(x, w, hw, d, 1)
            took, rows, last = hip.conv3_tap_stats()
            assert rows == 64 and last == want and took - before == int(want), (d, rows, last, took - before)
            assert torch.equal(on, off)
    finally:
        hip.conv3_tap_classes(was)


def test_default_choice_of_form_is_the_launch():
    """No forced form, the ASPP map (33 x 33, d = 12): one shape per tile height the grid rule picks, each confirmed on the plan
    first.  The launch reports the plan's tile height, and the class-ordered output equals the raster-order one bit for bit."""
    from ucd_amd import hip
    dev = torch.device("cuda:0")
    was = hip.conv3_tap_classes()
    try:
        for B, K, N, form, rows, tiles in ((1, 64, 64, "lw/64", 64, 18), (24, 64, 256, "lw/256", 256, 206), (24, 64, 512, "single", 128, 820)):
            plan = hip.conv1x1_plan(B * 33 * 33, N, K, taps=9)
            assert (plan["form"], plan["tile_rows"], plan["tiles_m"] * plan["tiles_n"]) == (form, rows, tiles), plan
            x, w, _ = _operands(B, 33, 12, K, N, dev)
            off = _product(x, w, 33, 12, 0)
            on = _product(x, w, 33, 12, 1)
            assert hip.conv3_tap_stats()[1] == plan["tile_rows"], (form, hip.conv3_tap_stats())
            assert torch.equal(on, off), (form, (on.float() - off.float()).abs().max().item())
    finally:
        hip.conv3_tap_classes(was)


@pytest.mark.usefixtures("deterministic_stats")
def test_whole_step_is_bit_equal_with_and_without_the_class_order():
    """The small scheduled step of tests/test_step_gpu.py (3 images, 257 x 257: 17 x 17 ASPP maps, dilations 6 / 12 / 18) with the
    switch on and off: losses and updated parameters bit-equal, eager and replayed from the step graph.  The eager run comes first,
    so the plans are resident before the graph run captures; its own eager warm-up iterations would build them too.  That the
    ASPP products took the class-ordered kernels - also while the graph was captured - shows in the library's launch count."""
    from test_step_gpu import _scheduled_steps
    from ucd_amd import hip
    was = hip.conv3_tap_classes()
    runs = {}
    try:
        for on in (True, False):
            hip.conv3_tap_classes(int(on))
            for sg in ("0", "1"):
                before = hip.conv3_tap_stats()[0]
                runs[(on, sg)] = _scheduled_steps(sg, steps=5 if sg == "1" else 3)
                took = hip.conv3_tap_stats()[0] - before
                # every iteration that launches (the eager ones, the capture) takes the class order at least for the student's forward
                # at d = 12 and d = 18 (d = 6 on 17 x 17 stays in raster order: the test above)
                assert (took >= 2 * 3) if on else took == 0, (on, sg, took)
    finally:
        hip.conv3_tap_classes(was)
    for sg in ("0", "1"):
        (la, pa, ga, _, ea), (lb, pb, gb, _, eb) = runs[(False, sg)], runs[(True, sg)]
        assert ea is None and eb is None, (ea, eb)
        assert ga == gb and (sg == "0" or ga >= 1), (ga, gb)
        assert np.array_equal(la, lb), (sg, la, lb)
        for n in pa:
            assert torch.equal(pa[n], pb[n]), (sg, n)
