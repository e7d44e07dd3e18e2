// Host half of the class-ordered rows of the dilated 3x3 products (conv1x1.hip).
//
// A pixel of a [B, H, W] map is classed by which of its four axis neighbours at distance d lie inside the map: per axis
// {neither, low only, high only, both}, 16 classes at most.  All pixels of a class have the same set of live taps of the 3x3 grid
// (tap (kh, kw) is live when the row test of kh and the column test of kw both pass), so a row tile whose rows come from one
// class walks exactly the taps its pixels need.  The plan orders the GEMM rows class-major over the whole batch - the classes
// by falling number of live taps (the heaviest tiles are dispatched first, and the partly filled last tile is the lightest),
// raster order inside a class - and gives every tile of `tile_rows` rows the union of the live taps of its rows as a 9-bit mask
// (bit t = tap t = kh * 3 + kw).  Only tiles that hold a class boundary walk more than their rows need; the centre tap is live
// everywhere, so no mask is empty.  Nothing of this depends on data: a plan is a function of (B, H, W, d, tile_rows).
#pragma once
#include <cstdint>

namespace ucd {

inline int conv3_axis_class(int v, int n, int d) { return (v - d >= 0 ? 1 : 0) | (v + d < n ? 2 : 0); }   // bit 0: low, bit 1: high

// the 3-bit set of live kernel rows (or columns) of an axis class: bit 0 = shift -d, bit 1 = centre, bit 2 = shift +d
inline unsigned conv3_axis_taps(int cls) { return 2u | (cls & 1 ? 1u : 0u) | (cls & 2 ? 4u : 0u); }

inline unsigned conv3_class_mask(int cy, int cx) {
  const unsigned ty = conv3_axis_taps(cy), tx = conv3_axis_taps(cx);
  unsigned m = 0;
  for (int kh = 0; kh < 3; ++kh)
    for (int kw = 0; kw < 3; ++kw)
      if ((ty >> kh & 1) && (tx >> kw & 1)) m |= 1u << (kh * 3 + kw);
  return m;
}

// perm[M] (M = B * H * W): GEMM row r is pixel perm[r] (index into the raster order over the images); masks[ceil(M / tile_rows)].
// Returns the number of classes that occur.
inline int conv3_tap_plan_fill(int B, int H, int W, int d, int tile_rows, int32_t* perm, int32_t* masks) {
  const int HW = H * W, M = B * HW;
  int count[16] = {0}, order[16], start[16];
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) count[conv3_axis_class(y, H, d) * 4 + conv3_axis_class(x, W, d)] += B;
  int n = 0;
  for (int c = 0; c < 16; ++c)
    if (count[c]) order[n++] = c;
  auto taps = [](int c) { return __builtin_popcount(conv3_class_mask(c >> 2, c & 3)); };
  for (int i = 1; i < n; ++i)                       // insertion sort: falling tap count, ties by class id (stable)
    for (int j = i; j > 0 && taps(order[j]) > taps(order[j - 1]); --j) { const int t = order[j]; order[j] = order[j - 1]; order[j - 1] = t; }
  int at = 0;
  for (int i = 0; i < n; ++i) { start[order[i]] = at; at += count[order[i]]; }
  const int tiles = (M + tile_rows - 1) / tile_rows;
  for (int t = 0; t < tiles; ++t) masks[t] = 0;
  for (int b = 0; b < B; ++b)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const int cy = conv3_axis_class(y, H, d), cx = conv3_axis_class(x, W, d);
        const int r = start[cy * 4 + cx]++;
        perm[r] = b * HW + y * W + x;
        masks[r / tile_rows] |= (int32_t)conv3_class_mask(cy, cx);
      }
  return n;
}

}  // namespace ucd
