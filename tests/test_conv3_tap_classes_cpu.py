"""CPU: the host plan of the class-ordered rows of the dilated 3x3 products (ucd_conv3_tap_plan, csrc/conv3_taps.h; the ASPP
branches of modules/deeplab.py:27-29).  A pixel is classed by which of its axis neighbours at distance d lie inside the map; the
GEMM rows are ordered class-major and every row tile walks only the taps of its mask.  Checked here against the definition,
per pixel and per tap: the order is a permutation, no mask misses a live tap, no mask holds a tap that is dead for the whole
tile, only the tiles on a class boundary mix classes, and the walked fraction stays within what those tiles can add to the
per-pixel ideal."""
import numpy as np
import pytest

from ucd_amd import hip

SHAPES = [(3, 17, 17, 6), (3, 17, 17, 12), (2, 33, 33, 18), (24, 33, 33, 6), (24, 33, 33, 12), (24, 33, 33, 18), (8, 48, 48, 18),
          (2, 9, 9, 12)]
_cache = {}


def _case(B, H, W, d, rows):
    """(perm, masks, n_classes, live[M, 9], cls[M]) of one plan; live / cls are indexed by PIXEL (raster order over the images)."""
    key = (B, H, W, d, rows)
    if key not in _cache:
        perm, masks, n = hip.conv3_tap_plan(B, H, W, d, rows)
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        live = np.zeros((H * W, 9), dtype=bool)
        for kh in range(3):
            for kw in range(3):
                yy, xx = y + (kh - 1) * d, x + (kw - 1) * d
                live[:, kh * 3 + kw] = ((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)).reshape(-1)
        cls = (((y - d >= 0) * 1 + (y + d < H) * 2) * 4 + (x - d >= 0) * 1 + (x + d < W) * 2).reshape(-1)
        _cache[key] = (perm, masks, n, np.tile(live, (B, 1)), np.tile(cls, B))
    return _cache[key]


def _tiles(a, rows):
    return [a[t:t + rows] for t in range(0, len(a), rows)]


@pytest.mark.parametrize("rows", [64, 128, 256])
@pytest.mark.parametrize("B,H,W,d", SHAPES)
def test_plan_against_the_definition(B, H, W, d, rows):
    perm, masks, n, live, cls = _case(B, H, W, d, rows)
    M = B * H * W
    tiles = (M + rows - 1) // rows
    assert perm.shape == (M,) and masks.shape == (tiles,)
    # 1. a permutation of the pixels
    assert np.array_equal(np.sort(perm), np.arange(M))
    assert n == len(np.unique(cls)) and n <= 16
    bits = (masks[:, None] >> np.arange(9)[None, :]) & 1                     # [tiles, 9]
    assert np.all(masks > 0) and np.all(masks < 512) and np.all(bits[:, 4] == 1)   # the centre tap is live everywhere
    mixed = 0
    for t, rows_t in enumerate(_tiles(perm, rows)):
        lt = live[rows_t]                                                    # [rows of the tile, 9]
        # 2. a tap outside the mask is dead for every row of the tile (a mask may be too large, never too small)
        assert not lt[:, bits[t] == 0].any(), t
        # 3. every tap of the mask is live for at least one row of the tile
        assert lt[:, bits[t] == 1].any(axis=0).all(), t
        mixed += len(np.unique(cls[rows_t])) > 1
    # 4. class-major: every class boundary falls into one tile
    assert mixed <= n - 1, (mixed, n)
    # class-major over the whole batch, raster order inside a class
    c = cls[perm]
    starts = np.flatnonzero(np.r_[True, c[1:] != c[:-1]])
    assert len(starts) == n
    for a, b in zip(starts, np.r_[starts[1:], M]):
        assert np.all(np.diff(perm[a:b]) > 0)
    # 5. the walked fraction against the per-pixel ideal plus what the mixed tiles can add (9 taps each at the most)
    walked = bits.sum() / (9.0 * tiles)
    ideal = live.sum() / (9.0 * M)
    assert walked <= ideal + 9.0 * (n - 1) / (9.0 * tiles) + 1e-12, (walked, ideal)


@pytest.mark.parametrize("rows", [64, 128, 256])
def test_dilation_beyond_half_the_map_leaves_the_centre_tap(rows):
    """d > H / 2 and d > W / 2: no pixel has a neighbour at distance d - one class, the raster order, centre tap only."""
    perm, masks, n, live, cls = _case(2, 9, 9, 12, rows)
    assert n == 1 and np.array_equal(perm, np.arange(2 * 81)) and np.all(masks == 1 << 4)


def test_benchmark_shape_walks_close_to_the_per_pixel_ideal():
    """24 images of 33 x 33 (the benchmark's ASPP input): 9 classes; the average pixel needs 0.772 / 0.574 / 0.405 of its taps at
    d = 6 / 12 / 18, and the 256-row forward tiles and 128-row input-gradient tiles walk at most 8 mixed tiles' worth more."""
    ideal_want = {6: 0.772, 12: 0.574, 18: 0.405}
    for d in (6, 12, 18):
        for rows in (256, 128):
            perm, masks, n, live, cls = _case(24, 33, 33, d, rows)
            assert n == 9
            ideal = live.sum() / (9.0 * len(perm))
            assert abs(ideal - ideal_want[d]) < 1e-3, (d, ideal)
            walked = sum(bin(int(m)).count("1") for m in masks) / (9.0 * len(masks))
            assert walked <= ideal + 8.0 / len(masks), (d, rows, walked, ideal)


def test_bad_arguments_are_refused():
    with pytest.raises(RuntimeError, match="tile_rows"):
        hip.conv3_tap_plan(2, 9, 9, 6, 100)
    with pytest.raises(RuntimeError, match="bad arguments"):
        hip.conv3_tap_plan(0, 9, 9, 6, 128)
