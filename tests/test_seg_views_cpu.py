"""CPU: the host side of the evaluation with scaled and mirrored views - ucd_seg_views_plan (csrc/seg_views.hip: which pixel tile and
how many bytes of LDS a set of views gets, without a device call), its refusals, and the command line (--eval_scales, --eval_flip,
argparser.eval_views, --fusion-mode)."""
import ctypes as C

import pytest

from ucd_amd import argparser, hip

EINVAL, EUNSUPPORTED = -1, hip.EUNSUPPORTED
BUDGET = 150 * 1024
TILES = [(32, 64), (32, 32), (16, 32), (16, 16), (8, 16), (8, 8)]
SCALES = (1.0, 0.5, 0.75, 1.25, 1.5, 1.75)


def _raw_plan(H, W, views, Ctot, n):
    arr = lambda vals: (C.c_int * max(len(vals), 1))(*vals)
    ty, tx, lds = C.c_int(-1), C.c_int(-1), C.c_size_t(0)
    lib = hip.load()
    rc = lib.ucd_seg_views_plan(H, W, len(views), arr([v[0] for v in views]), arr([v[1] for v in views]),
                                arr([int(v[2]) for v in views]), Ctot, n, C.byref(ty), C.byref(tx), C.byref(lds))
    return rc, ty.value, tx.value, lds.value, lib.ucd_last_error().decode()


def _ade_default_views():
    """ADE, --output_stride 16, 512^2: the image at six scales, each plain and mirrored; a view's map is ceil(size / 16) cells wide"""
    return [((int(512 * s + 0.5) + 15) // 16,) * 2 + (f,) for s in SCALES for f in (False, True)]


def test_symbols_are_declared():
    assert "ucd_seg_views" in hip.SIGNATURES and "ucd_seg_views_plan" in hip.SIGNATURES
    assert hip.SEG_VIEW_MODES == {"mean": 0, "max": 1, "voting": 2}


def test_plan_serves_the_ade_default_views():
    views = _ade_default_views()
    assert len(views) == 12
    p = hip.seg_views_plan(512, 512, views, 151, 151)
    print("ADE default, 12 views, 151 classes:", p)
    assert (p["tile_y"], p["tile_x"]) in TILES
    assert 0 < p["lds_bytes"] <= BUDGET
    # the same views with 21 classes and the LDS histogram fit the largest tile
    q = hip.seg_views_plan(513, 513, [((int(513 * s + 0.5) + 15) // 16,) * 2 + (f,) for s in SCALES for f in (False, True)], 21, 21)
    assert (q["tile_y"], q["tile_x"]) == TILES[0] and q["lds_bytes"] <= BUDGET


def test_plan_counts_the_cells_of_a_single_view():
    """One plain view at an integer factor of 16 under a 32 x 64 tile: (32 / 16 + 2) x (64 / 16 + 2) cells at an inner tile, times the
    classes, plus the 272-byte table and the n^2 words of the LDS histogram."""
    p = hip.seg_views_plan(512, 512, [(32, 32, False)], 21, 21)
    assert (p["tile_y"], p["tile_x"]) == (32, 64)
    assert p["lds_bytes"] == 4 * 6 * 21 * 4 + 272 + 21 * 21 * 4
    p = hip.seg_views_plan(512, 512, [(32, 32, False)], 151, 151)          # above 64 classes: no LDS histogram
    assert p["lds_bytes"] == 4 * 6 * 151 * 4 + 272


def test_plan_takes_a_smaller_tile_before_it_refuses():
    """151 classes at an up-sampling factor of 2: the 32 x 64 tile would need 17 x 33 cells; the plan walks down its list."""
    p = hip.seg_views_plan(64, 96, [(16, 24, False), (32, 48, True)], 151, 151)
    assert (p["tile_y"], p["tile_x"]) in TILES[1:] and p["lds_bytes"] <= BUDGET
    bigger = TILES[TILES.index((p["tile_y"], p["tile_x"])) - 1]
    cells = lambda t, f: (min(t[0] // f, 64 // f) + 1) * (min(t[1] // f, 96 // f) + 1)      # lower bound of a tile's footprint
    assert (cells(bigger, 2) + cells(bigger, 4)) * 151 * 4 > BUDGET


def test_plan_refuses_what_cannot_fit_and_names_the_bytes():
    rc, _, _, _, msg = _raw_plan(64, 64, [(64, 64, False)] * 16, 151, 151)
    assert rc == EUNSUPPORTED
    # 16 views x 9 x 9 cells under the 8 x 8 tile at factor 1, 151 classes, and the table
    assert str(16 * 81 * 151 * 4 + 272) in msg and str(BUDGET) in msg and "bytes" in msg
    with pytest.raises(RuntimeError, match="bytes of LDS"):
        hip.seg_views_plan(64, 64, [(64, 64, False)] * 16, 151, 151)


def test_plan_refuses_bad_sizes():
    ok = [(8, 8, False)]
    assert _raw_plan(64, 64, [], 21, 21)[0] == EINVAL                                      # V = 0
    assert _raw_plan(64, 64, ok * 17, 21, 21)[0] == EINVAL                                 # V = 17
    assert _raw_plan(64, 64, ok * 16, 21, 21)[0] == 0
    assert _raw_plan(64, 64, [(65, 8, False)], 21, 21)[0] == EINVAL                        # h > H
    assert _raw_plan(64, 64, [(8, 65, False)], 21, 21)[0] == EINVAL                        # w > W
    assert _raw_plan(64, 64, [(0, 8, False)], 21, 21)[0] == EINVAL
    assert _raw_plan(0, 64, ok, 21, 21)[0] == EINVAL
    assert _raw_plan(64, 64, ok, 256, 21)[0] == EINVAL                                     # Ctot > 255
    assert _raw_plan(64, 64, ok, 21, 0)[0] == EINVAL
    rc, _, _, _, msg = _raw_plan(64, 64, [(8, 8, False), (65, 8, True)], 21, 21)
    assert rc == EINVAL and "view 1" in msg
    lib = hip.load()
    assert lib.ucd_seg_views_plan(64, 64, 1, None, None, None, 21, 21, None, None, None) == EINVAL
    # the launch asks the plan first: the same refusals before any device call (the pointers are never followed)
    one = (C.c_int * 1)
    sem = (C.c_void_p * 1)(16)
    assert lib.ucd_seg_views(sem, one(21), one(65), one(8), one(0), 1, 16, 1, 64, 64, 21, 21, 0, 16, None, None) == EINVAL
    assert lib.ucd_seg_views(sem, one(20), one(8), one(8), one(0), 1, 16, 1, 64, 64, 21, 21, 0, 16, None, None) == EINVAL       # ld < Ctot
    assert lib.ucd_seg_views(sem, one(21), one(8), one(8), one(0), 1, 16, 1, 64, 64, 21, 21, 3, 16, None, None) == EINVAL       # mode
    assert lib.ucd_seg_views(sem, one(21), one(8), one(8), one(0), 0, 16, 1, 64, 64, 21, 21, 0, 16, None, None) == EINVAL       # V = 0


@pytest.mark.parametrize("H,W,h,w", [(512, 512, 32, 32), (512, 512, 56, 56), (512, 640, 24, 40), (128, 192, 9, 13)])
def test_mirrored_view_gets_the_cells_of_the_plain_one_on_a_symmetric_grid(H, W, h, w):
    """W a multiple of every tile width: the mirrored pixel ranges of the tiles are the tiles again, so a mirrored view needs exactly
    the cells of the plain one."""
    for Ctot in (21, 151):
        plain = hip.seg_views_plan(H, W, [(h, w, False)], Ctot, Ctot)
        mirrored = hip.seg_views_plan(H, W, [(h, w, True)], Ctot, Ctot)
        assert plain == mirrored
        both = hip.seg_views_plan(H, W, [(h, w, False), (h, w, True)], Ctot, Ctot)
        if (both["tile_y"], both["tile_x"]) == (plain["tile_y"], plain["tile_x"]):
            hist = Ctot * Ctot * 4 if Ctot <= 64 else 0
            assert both["lds_bytes"] - 272 - hist == 2 * (plain["lds_bytes"] - 272 - hist)


def _parse(*extra):
    return argparser.modify_command_options(argparser.get_argparser().parse_args(list(extra)))


def test_eval_views_order():
    assert argparser.eval_views(_parse()) == [(1.0, False)]
    assert argparser.eval_views(_parse("--eval_flip")) == [(1.0, False), (1.0, True)]
    assert argparser.eval_views(_parse("--eval_scales", "0.5", "1.0", "1.5")) == [(1.0, False), (0.5, False), (1.5, False)]
    o = _parse("--eval_scales", "0.5", "0.75", "1.0", "1.25", "1.5", "1.75", "--eval_flip")
    assert o.eval_scales == [0.5, 0.75, 1.0, 1.25, 1.5, 1.75] and o.eval_flip is True
    views = argparser.eval_views(o)
    assert views[0] == (1.0, False) and len(views) == 12
    assert views == [(s, f) for s in (1.0, 0.5, 0.75, 1.25, 1.5, 1.75) for f in (False, True)]
    for k in range(0, 12, 2):                                   # a mirror follows its view
        assert views[k + 1] == (views[k][0], True) and views[k][1] is False
    # defaults change nothing
    d = _parse()
    assert d.eval_scales == [1.0] and d.eval_flip is False


def test_eval_scales_without_the_plain_view_is_a_parser_error(capsys):
    with pytest.raises(SystemExit) as e:
        _parse("--eval_scales", "0.5", "1.5")
    assert e.value.code == 2
    assert "1.0" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        _parse("--eval_scales", "1.0", "-0.5")


def test_fusion_mode_parses_as_before():
    assert _parse().fusion_mode == "mean"
    assert _parse("--fusion-mode", "voting").fusion_mode == "voting"
    assert _parse("--fusion-mode", "max").fusion_mode == "max"
    with pytest.raises(SystemExit):
        _parse("--fusion-mode", "median")


def test_views_are_refused_without_a_gpu():
    import torch
    from ucd_amd.metrics import StreamSegMetrics
    m = StreamSegMetrics(21)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.update_from_views(torch.zeros(1, 16, 16, dtype=torch.long), [torch.zeros(1, 21, 4, 4)], [False])
    with pytest.raises(ValueError, match="fusion"):
        m.update_from_views(torch.zeros(1, 16, 16, dtype=torch.long), [torch.zeros(1, 21, 4, 4)], [False], fusion="median")
