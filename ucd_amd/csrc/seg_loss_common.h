// What the tiled forms (seglogit_loss.hip) and the gather forms (seg_gather.hip) of the fused logit losses both need, defined once:
// the rescue threshold of the class-subset sums, the argument rules of the _ex entries and the launch that turns per-tile or
// per-cell loss pairs into the two means.  The kernel sits in an anonymous namespace: one source copy, compiled into each unit.
#pragma once
#include "common.h"

#include <cmath>

namespace ucd {
namespace {

// The sums over the class subsets (old classes; background + new classes) are taken from the exponentials relative to the maximum
// over ALL classes.  A subset that trails that maximum by more than ~87 underflows to a zero sum (log -> -inf, 1 / sum -> inf):
// below this threshold a pixel takes its subset sums again around each subset's own maximum (what torch.logsumexp does).  Rare in
// training (a class set 70 below the leader), so a branch: the common path keeps its arithmetic.
constexpr float kSubsetTiny = 1e-30f;

// the argument rules of ucd_seg_losses_ex / ucd_seg_losses_plan_ex / ucd_seg_losses_gather that ucd_seg_losses cannot break (host
// only, before anything else)
inline int seg_ex_check(const char* fn, int Ctot, int K, int ce_old_cl, int kd_mode, float alpha, int has_teacher) {
  UCD_REQUIRE(Ctot > 0 && K >= 1 && K <= Ctot, UCD_EINVAL, "%s: bad sizes", fn);
  UCD_REQUIRE(ce_old_cl >= 1 && ce_old_cl <= Ctot, UCD_EINVAL, "%s: ce_old_cl = %d is outside [1, Ctot = %d]", fn, ce_old_cl, Ctot);
  UCD_REQUIRE(kd_mode == UCD_KD_UNBIASED || kd_mode == UCD_KD_PLAIN, UCD_EINVAL,
              "%s: kd_mode = %d is neither UCD_KD_UNBIASED (0) nor UCD_KD_PLAIN (1)", fn, kd_mode);
  UCD_REQUIRE(std::isfinite(alpha) && alpha != 0.f, UCD_EINVAL, "%s: alpha = %g must be finite and non-zero", fn, (double)alpha);
  UCD_REQUIRE(!has_teacher || ce_old_cl == 1 || ce_old_cl == K, UCD_EINVAL,
              "%s: with a teacher ce_old_cl = %d must be 1 (plain cross entropy) or K = %d", fn, ce_old_cl, K);
  return 0;
}

// the argument rules of the focal entries (host only, the first thing an entry does)
inline int seg_focal_check(const char* fn, float focal_gamma, float focal_alpha) {
  UCD_REQUIRE(std::isfinite(focal_gamma) && focal_gamma >= 0.f, UCD_EINVAL, "%s: focal_gamma = %g must be finite and >= 0", fn,
              (double)focal_gamma);
  UCD_REQUIRE(std::isfinite(focal_alpha) && focal_alpha > 0.f, UCD_EINVAL, "%s: focal_alpha = %g must be finite and > 0", fn,
              (double)focal_alpha);
  return 0;
}

// Focal modulation of one pixel's cross entropy ce (include/ucd_hip.h): returns F = alpha u^gamma ce, u = clamp(1 - exp(-ce), 0, 1),
// and sets g = alpha (u^gamma + gamma u^(gamma-1) exp(-ce) ce), the factor on the pixel's cross-entropy gradient coefficient.
// Where u rounds to 0 (ce below ~6e-8, or a negative ce of a label that is no class) both are 0; gamma == 0 is alpha ce and alpha.
// u^(gamma-1) is taken of max(u, 2^-24), the smallest u that is not 0: no infinity is ever formed.  gamma is uniform: gamma == 2
// runs without exp2 / log.  Scalars in, scalars out: nothing here lives across a class loop.
__device__ __forceinline__ float focal_pixel(float ce, float gamma, float alpha, float& g) {
  if (gamma == 0.f) { g = alpha; return alpha * ce; }
  const float p = __builtin_amdgcn_exp2f(-ce * 1.4426950408889634f);
  const float u = fminf(fmaxf(1.f - p, 0.f), 1.f);
  float ug, ug1;                               // u^gamma, u^(gamma-1)
  if (gamma == 2.f) { ug = u * u; ug1 = u; }
  else {
    const float l = __builtin_amdgcn_logf(fmaxf(u, 5.9604644775390625e-8f));
    ug = __builtin_amdgcn_exp2f(gamma * l);
    ug1 = __builtin_amdgcn_exp2f((gamma - 1.f) * l);
  }
  const bool zero = !(u > 0.f);
  g = zero ? 0.f : alpha * (ug + gamma * ug1 * (p * ce));
  return zero ? 0.f : alpha * (ug * ce);
}

// part: [n][2] loss sums of tiles or cells -> out[0], out[1] = their sums in index order (fp64), times inv_pix: the means over ALL
// pixels, ignored ones counting as 0 (train.py:116 .mean(); loss.py:178).  A fixed order: the same bits on every run
__global__ __launch_bounds__(1024) void seg_pair_reduce_kernel(const float* __restrict__ part, int n, float inv_pix,
                                                              float* __restrict__ out) {
  __shared__ double red[2][16];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) { a += part[2 * i]; b += part[2 * i + 1]; }
  for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off, 64); b += __shfl_xor(b, off, 64); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sa = 0.0, sb = 0.0;
    for (int i = 0; i < 16; ++i) { sa += red[0][i]; sb += red[1][i]; }
    out[0] = (float)(sa * inv_pix);
    out[1] = (float)(sb * inv_pix);
  }
}

inline int seg_pair_reduce(const char* fn, const float* part, int n, float inv_pix, float* out, hipStream_t s) {
  seg_pair_reduce_kernel<<<1, 1024, 0, s>>>(part, n, inv_pix, out);
  return check_launch(fn);
}

}  // namespace
}  // namespace ucd
