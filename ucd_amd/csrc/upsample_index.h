// The source-index arithmetic of the bilinear up-sampling (F.interpolate, align_corners=False), shared by the kernels that
// rebuild full-resolution logits from the low-resolution ones (seglogit_loss.hip, seg_cell.h).  One copy: host and device,
// under -ffp-contract=off on both sides, so a plan computed on the host rounds exactly as the kernel it sizes.
#pragma once
#include <hip/hip_runtime.h>

namespace ucd {

// torch's align_corners=False source index.  Host and device: ucd_seg_losses_plan sizes the LDS with the very function the
// kernels index it with (-ffp-contract=off on both sides: the same roundings)
__host__ __device__ __forceinline__ void up_src(int dst, int in_size, float scale, int& i0, int& i1, float& l0, float& l1) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = (int)src < in_size - 1 ? (int)src : in_size - 1;
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.f - l1;
}

// the low-resolution cells under the pixels [t0, min(t0 + tile, out)) of one dimension: the first cell and their count (the source
// index is monotone in the pixel).  The one copy of the footprint arithmetic: the kernels index their LDS with it, the plan sizes it
__host__ __device__ __forceinline__ void tile_span(int t0, int tile, int out, int in_size, float scale, int& first, int& count) {
  int last, dummy;
  float f0, f1;
  up_src(t0, in_size, scale, first, dummy, f0, f1);
  up_src((t0 + tile < out ? t0 + tile : out) - 1, in_size, scale, dummy, last, f0, f1);
  count = last - first + 1;
}

// The gather forms (seg_cell.h: the walk of seg_gather.hip's kernels): the pixels of one dimension that can touch cell i, src = scale * (p + 0.5)
// - 0.5 in (i - 1, i + 1).  The bounds are strict, so floor / ceil of the real-valued ends already take one pixel more on either
// side than the footprint has: rounding (of these ends, of up_src) moves nothing by a pixel.  Outside the footprint the weight is
// zero; no exact inverse is needed.
__device__ __forceinline__ void scan_range(int i, int out, float inv_scale, int& lo, int& hi) {
  lo = (int)floorf(((float)i - 0.5f) * inv_scale - 0.5f);
  hi = (int)ceilf(((float)i + 1.5f) * inv_scale - 0.5f);
  lo = lo < 0 ? 0 : lo;
  hi = hi > out - 1 ? out - 1 : hi;
}

}  // namespace ucd
