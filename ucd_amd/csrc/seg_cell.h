// The walk of ONE low-resolution cell that the gather-form loss kernels share (seg_gather.hip: seg_bce_kernel,
// seg_losses_gather_kernel).  One wave owns cell (b, i, j): it stages the 3 x 3 cells around it (LDS, read
// only), walks the pixels whose bilinear footprint can contain the cell (a conservative rectangle: scan_range), takes each pixel's
// weight on the cell from the interpolation function itself and rebuilds the pixel's logits from the staged rows.  Device only.
// The kernels keep what differs: how lanes lie over pixels or classes, the label rule, the loss arithmetic.
// Every expression is written once, here, under -ffp-contract=off: both kernels round alike, and a change is made in one place.
#pragma once
#include "common.h"
#include "upsample_index.h"

namespace ucd {

// The four corners of a pixel among the nine staged rows and their bilinear weights.
struct CellCorners {
  int q00, q01, q10, q11;          // rows 0 .. 8 of the staged neighbourhood: (y0, x0), (y0, x1), (y1, x0), (y1, x1)
  float ly0, ly1, lx0, lx1;
  // torch's up-sampling arithmetic: h0*(w0*v00 + w1*v01) + h1*(w0*v10 + w1*v11), of class c in rows `stride` floats apart
  __device__ __forceinline__ float interp(const float* base, int stride, int c) const {
    return ly0 * (lx0 * base[q00 * stride + c] + lx1 * base[q01 * stride + c]) +
           ly1 * (lx0 * base[q10 * stride + c] + lx1 * base[q11 * stride + c]);
  }
};

// One pixel of the walk.  q00 .. q11 are valid ONLY when the pixel matters(): then y0, y1 lie in [i - 1, i + 1] and x0, x1 in
// [j - 1, j + 1]; for any other pixel of the rectangle they are numbers that index nothing.
struct CellPixel : CellCorners {
  int Y, X;
  float wgt;                       // the pixel's weight on this cell: the factor of dL/dz_pc in the cell's gradient
  bool owner;                      // (y0, x0) is this cell: it counts the pixel's loss
  __device__ __forceinline__ bool matters(bool want_grad) const { return owner || (want_grad && wgt != 0.f); }
};

struct CellWalk {
  int b, i, j, h, w;
  int ylo, xlo, ncol, npix;        // the scanned rectangle: pixel p is (ylo + p / ncol, xlo + p % ncol)
  float scale_h, scale_w;

  __device__ __forceinline__ CellWalk(int cell, int H, int W, int h_, int w_, float scale_h_, float scale_w_, float inv_scale_h,
                                      float inv_scale_w)
      : b(cell / (w_ * h_)), i((cell / w_) % h_), j(cell % w_), h(h_), w(w_), scale_h(scale_h_), scale_w(scale_w_) {
    int yhi, xhi;
    scan_range(i, H, inv_scale_h, ylo, yhi);
    scan_range(j, W, inv_scale_w, xlo, xhi);
    ncol = xhi - xlo + 1;
    npix = (yhi - ylo + 1) * ncol;
  }

  // dst[9][stride] <- mul * the C classes of the 3 x 3 cells around (i, j), by the 64 lanes of the wave.  Cells outside the map are
  // never indexed (up_src clamps to the map); they are staged as zeros.  mul == 1.f leaves every bit as it is.
  __device__ __forceinline__ void stage(float* dst, int stride, const float* __restrict__ src, int ld, int C, float mul, int lane) const {
    for (int n = lane; n < 9 * C; n += kWave) {
      const int q = n / C, c = n - q * C;
      const int cy = i - 1 + q / 3, cx = j - 1 + q % 3;
      const bool in = cy >= 0 && cy < h && cx >= 0 && cx < w;
      dst[q * stride + c] = in ? mul * src[((size_t)(b * h + cy) * w + cx) * ld + c] : 0.f;
    }
  }

  __device__ __forceinline__ CellPixel pixel(int p) const {
    CellPixel px;
    const int ry = p / ncol;
    px.Y = ylo + ry;
    px.X = xlo + (p - ry * ncol);
    int y0, y1, x0, x1;
    up_src(px.Y, h, scale_h, y0, y1, px.ly0, px.ly1);
    up_src(px.X, w, scale_w, x0, x1, px.lx0, px.lx1);
    // the pixel's weight on this cell, from the interpolation itself (at the clamped last row y0 == y1: the parts add to 1)
    const float wy = (y0 == i ? px.ly0 : 0.f) + (y1 == i ? px.ly1 : 0.f);
    const float wx = (x0 == j ? px.lx0 : 0.f) + (x1 == j ? px.lx1 : 0.f);
    px.wgt = wy * wx;
    px.owner = y0 == i && x0 == j;
    px.q00 = (y0 - i + 1) * 3 + (x0 - j + 1); px.q01 = (y0 - i + 1) * 3 + (x1 - j + 1);
    px.q10 = (y1 - i + 1) * 3 + (x0 - j + 1); px.q11 = (y1 - i + 1) * 3 + (x1 - j + 1);
    return px;
  }
};

}  // namespace ucd
