// The arithmetic of Pillow's resize that the data-pipeline kernels share (datapipe.hip, batch_path.hip): the BILINEAR
// coefficient entries of src/libImaging/Resample.c (precompute_coeffs + normalize_coeffs_8bpc, 22-bit fixed point) and the
// accumulating-double index rule of its NEAREST resize.  One definition of each expression: the kernels that keep whole tables
// in HBM and the one that computes its own entries per workgroup round identically (the library is built without fp
// contraction).
#pragma once
#include "common.h"

namespace ucd {

constexpr int kPrecisionBits = 22;

// where output index xx of the resize in_size -> out_size reads: taps [xmin, xmin + count) of the source axis, the
// triangle's centre and the reciprocal of its half width
struct CoeffWindow {
  int xmin, count;
  double center, ss;
};

__device__ __forceinline__ CoeffWindow image_coeff_window(int in_size, int out_size, int xx) {
  const double scale = (double)in_size / (double)out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  CoeffWindow c;
  c.center = ((double)xx + 0.5) * scale;
  c.ss = 1.0 / filterscale;
  int xmin = (int)(c.center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(c.center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  c.xmin = xmin;
  c.count = xmax - xmin;
  return c;
}

// the triangle filter at tap x of the window, before normalisation
__device__ __forceinline__ double image_coeff_weight(const CoeffWindow& c, int x) {
  double v = ((double)(x + c.xmin) - c.center + 0.5) * c.ss;
  if (v < 0.0) v = -v;
  return v < 1.0 ? 1.0 - v : 0.0;
}

// the normalising sum over the first `count` taps, added in tap order as Pillow does
__device__ __forceinline__ double image_coeff_sum(const CoeffWindow& c, int count) {
  double ww = 0.0;
  for (int x = 0; x < count; ++x) ww += image_coeff_weight(c, x);
  return ww;
}

// tap x as the 22-bit fixed-point integer of normalize_coeffs_8bpc
__device__ __forceinline__ int image_coeff_fixed(const CoeffWindow& c, double ww, int x) {
  double w = image_coeff_weight(c, x);
  if (ww != 0.0) w /= ww;
  return w < 0.0 ? (int)(-0.5 + w * (double)(1 << kPrecisionBits)) : (int)(0.5 + w * (double)(1 << kPrecisionBits));
}

// one entry {xmin, count, k[0..kmax)} of a coefficient table: output index xx of the resize in_size -> out_size
__device__ __forceinline__ void image_coeff_entry(int in_size, int out_size, int xx, int kmax, int* __restrict__ o) {
  CoeffWindow c = image_coeff_window(in_size, out_size, xx);
  if (c.count > kmax) c.count = kmax;                   // cannot happen when kmax = ceil(support) * 2 + 1
  const double ww = image_coeff_sum(c, c.count);
  o[0] = c.xmin;
  o[1] = c.count;
  for (int x = 0; x < kmax; ++x) o[2 + x] = x < c.count ? image_coeff_fixed(c, ww, x) : 0;
}

__device__ __forceinline__ int clip8(int v) {
  v >>= kPrecisionBits;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// Pillow's NEAREST resize picks source indices by ACCUMULATING in double: xo = a * 0.5; idx = (int)xo; xo += a with
// a = extent / out.  The sum rounds at every step, so entry x costs x dependent additions whoever computes it.
struct NearestWalk {
  double a, xo;
  int extent;
  __device__ __forceinline__ NearestWalk(int extent_, int out) : a((double)extent_ / (double)out), xo(a * 0.5), extent(extent_) {}
  __device__ __forceinline__ int next() {
    const int v = (int)xo;
    xo += a;
    return v < extent ? v : extent - 1;
  }
};

// entry x of that table alone: the x additions, then the index
__device__ __forceinline__ int nearest_index(int extent, int out, int x) {
  NearestWalk walk(extent, out);
  for (int k = 0; k < x; ++k) walk.xo += walk.a;
  return walk.next();
}

}  // namespace ucd
