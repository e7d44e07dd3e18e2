// Fused full-resolution BINARY cross entropy losses of the --bce / --icarl / --method LWF-MC runs (include/ucd_hip.h,
// DESIGN.md section 3.5.4): bilinear up-sampling of the student and teacher logits (segmentation_module.py:133) +
// BCEWithLogitsLossWithIgnoreIndex(reduction='none')(...).mean() (utils/loss.py:31-54, train.py:112/116) + the combined iCaRL
// term K * BCEWithLogitsLoss(mean)(out[:, :K], sigmoid(out_old)) (train.py:119-124) + their gradient w.r.t. the LOW-resolution
// student logits.
//
// There is no soft-max: every (pixel, class) term stands alone, so the gradient can be GATHERED.  One wave owns one
// low-resolution cell (b, i, j).  It walks the pixels whose bilinear footprint can contain the cell (a conservative rectangle;
// outside the footprint the pixel's weight on the cell is zero and the pixel is skipped), rebuilds z_pc from the 3 x 3 cells
// around its own (staged in LDS, read only), takes the pixel's weight on its own cell from the interpolation function
// itself and sums weight * dL/dz_pc per class in registers.  A pixel is re-evaluated by each of its (up to) four cells; in
// return nothing is ever added to memory that another unit owns: no atomics, no fixed point, no LDS adds, each element of
// d_sem is written once (no memset) and the same inputs give the same bits.  A pixel's LOSS is counted by the cell of its
// (y0, x0) corner alone; the per-cell pairs are added in index order by a second launch.
#include "common.h"
#include "upsample_index.h"

namespace ucd {
namespace {

constexpr int kChunk = 24;        // classes whose gradient sums a lane keeps in registers; more classes: the pixels are walked again
constexpr float kL2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

// scan_range (the pixels of one dimension that can touch a cell): upsample_index.h

// e = exp(-|z|): sigmoid(z) = z >= 0 ? 1 / (1 + e) : e / (1 + e), softplus(-|z|) = log1p(e); nothing overflows at any z
__device__ __forceinline__ float exp_neg_abs(float z) { return __builtin_amdgcn_exp2f(-fabsf(z) * kL2e); }

// part: [B * h * w][2] (hard sum, soft sum) of the pixels whose (y0, x0) cell this is; d_sem (may be NULL): the cell's row
__global__ __launch_bounds__(kWave) void seg_bce_kernel(
    const float* __restrict__ sem_s, int ld_s, const float* __restrict__ sem_t, int ld_t, const int64_t* __restrict__ labels,
    int H, int W, int h, int w, int Ctot, int K, int ignore_index, float scale_h, float scale_w, float inv_scale_h,
    float inv_scale_w, float hard_scale, float soft_scale, float* __restrict__ part, float* __restrict__ d_sem, int ld_d) {
  extern __shared__ float smem[];
  const int cell = blockIdx.x, lane = threadIdx.x;
  const int j = cell % w, i = (cell / w) % h, b = cell / (w * h);
  // the 3 x 3 cells around (i, j): [9][CS] student, [9][KS] teacher logits; odd strides keep the nine rows on different banks
  const int CS = Ctot | 1, KS = sem_t ? (K | 1) : 0;
  float* s_log = smem;
  float* t_log = smem + 9 * CS;
  for (int n = lane; n < 9 * Ctot; n += kWave) {
    const int q = n / Ctot, c = n - q * Ctot;
    const int cy = i - 1 + q / 3, cx = j - 1 + q % 3;
    const bool in = cy >= 0 && cy < h && cx >= 0 && cx < w;
    s_log[q * CS + c] = in ? sem_s[((size_t)(b * h + cy) * w + cx) * ld_s + c] : 0.f;
  }
  if (sem_t)
    for (int n = lane; n < 9 * K; n += kWave) {
      const int q = n / K, c = n - q * K;
      const int cy = i - 1 + q / 3, cx = j - 1 + q % 3;
      const bool in = cy >= 0 && cy < h && cx >= 0 && cx < w;
      t_log[q * KS + c] = in ? sem_t[((size_t)(b * h + cy) * w + cx) * ld_t + c] : 0.f;
    }
  __syncthreads();

  int ylo, yhi, xlo, xhi;
  scan_range(i, H, inv_scale_h, ylo, yhi);
  scan_range(j, W, inv_scale_w, xlo, xhi);
  const int ncol = xhi - xlo + 1, npix = (yhi - ylo + 1) * ncol;
  const bool want_grad = d_sem != nullptr;
  float hard_sum = 0.f, soft_sum = 0.f;
  for (int c0 = 0; c0 < Ctot; c0 += kChunk) {
    float acc[kChunk];
#pragma unroll
    for (int k = 0; k < kChunk; ++k) acc[k] = 0.f;
    for (int p = lane; p < npix; p += kWave) {
      const int ry = p / ncol;
      const int Y = ylo + ry, X = xlo + (p - ry * ncol);
      int y0, y1, x0, x1;
      float ly0, ly1, lx0, lx1;
      up_src(Y, h, scale_h, y0, y1, ly0, ly1);
      up_src(X, w, scale_w, x0, x1, lx0, lx1);
      // the pixel's weight on this cell, from the interpolation itself (at the clamped last row y0 == y1: the parts add to 1)
      const float wy = (y0 == i ? ly0 : 0.f) + (y1 == i ? ly1 : 0.f);
      const float wx = (x0 == j ? lx0 : 0.f) + (x1 == j ? lx1 : 0.f);
      const float wgt = wy * wx;
      const bool owner = y0 == i && x0 == j;          // this cell counts the pixel's loss
      if (!(owner || (want_grad && wgt != 0.f))) continue;
      // from here on y0, y1 in [i - 1, i + 1] and x0, x1 in [j - 1, j + 1]: rows 0 .. 8 of the staged neighbourhood
      const int q00 = (y0 - i + 1) * 3 + (x0 - j + 1), q01 = (y0 - i + 1) * 3 + (x1 - j + 1);
      const int q10 = (y1 - i + 1) * 3 + (x0 - j + 1), q11 = (y1 - i + 1) * 3 + (x1 - j + 1);
      const int64_t lab64 = labels[((size_t)b * H + Y) * W + X];
      // a label outside [0, Ctot) counts as ignored, ignore_index or not (include/ucd_hip.h)
      const bool valid = lab64 != ignore_index && lab64 >= 0 && lab64 < Ctot;
      const int lab = valid ? (int)lab64 : -1;
      const float hw = valid ? hard_scale : 0.f;
      float hard_pix = 0.f, soft_pix = 0.f;
#pragma unroll
      for (int k = 0; k < kChunk; ++k) {
        const int c = c0 + k;
        if (c < Ctot) {                                // wave-uniform
          // torch's up-sampling arithmetic: h0*(w0*v00 + w1*v01) + h1*(w0*v10 + w1*v11)
          const float z = ly0 * (lx0 * s_log[q00 * CS + c] + lx1 * s_log[q01 * CS + c]) +
                          ly1 * (lx0 * s_log[q10 * CS + c] + lx1 * s_log[q11 * CS + c]);
          const float e = exp_neg_abs(z);
          const float r = __builtin_amdgcn_rcpf(1.f + e);
          const float sig = z >= 0.f ? r : e * r;
          // max(z, 0) + log1p(e); below 2^-12 log1p(e) = e - e^2 / 2 + ... is e to fp32
          const float sp = fmaxf(z, 0.f) + (e < 2.44140625e-4f ? e : kLn2 * __builtin_amdgcn_logf(1.f + e));
          const float hot = c == lab ? 1.f : 0.f;
          hard_pix += sp - hot * z;
          float g = hw * (sig - hot);
          if (sem_t && c < K) {                        // wave-uniform
            const float zt = ly0 * (lx0 * t_log[q00 * KS + c] + lx1 * t_log[q01 * KS + c]) +
                             ly1 * (lx0 * t_log[q10 * KS + c] + lx1 * t_log[q11 * KS + c]);
            const float et = exp_neg_abs(zt);
            const float rt = __builtin_amdgcn_rcpf(1.f + et);
            const float tgt = zt >= 0.f ? rt : et * rt;     // the sigmoid is applied AFTER the up-sampling (train.py:123-124)
            soft_pix += sp - tgt * z;
            g += soft_scale * (sig - tgt);
          }
          acc[k] += wgt * g;
        }
      }
      if (owner) {
        if (valid) hard_sum += hard_pix;
        soft_sum += soft_pix;
      }
    }
    if (want_grad) {
      // lanes, in the fixed order of the butterfly; lane k keeps class c0 + k and writes it: one store per element
      float mine = 0.f;
#pragma unroll
      for (int k = 0; k < kChunk; ++k) {
        const float v = wave_sum(acc[k]);
        mine = lane == k ? v : mine;
      }
      if (lane < kChunk && c0 + lane < Ctot) d_sem[(size_t)cell * ld_d + c0 + lane] = mine;
    }
  }
  hard_sum = wave_sum(hard_sum);
  soft_sum = wave_sum(soft_sum);
  if (lane == 0) {
    part[2 * cell + 0] = hard_sum;
    part[2 * cell + 1] = soft_sum;
  }
}

// the per-cell pairs in index order (as seg_losses_reduce_kernel adds its per-tile pairs): a fixed order, the same bits
__global__ __launch_bounds__(1024) void seg_bce_reduce_kernel(const float* __restrict__ part, int n, float inv_pix,
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
    out[0] = (float)(sa * inv_pix);   // mean over ALL pixels, ignored ones count as 0 (train.py:116 .mean())
    out[1] = (float)(sb * inv_pix);   // K * BCEWithLogitsLoss(mean) over [B, K, H, W]: the class sum's mean over the pixels
  }
}

}  // namespace
}  // namespace ucd

using namespace ucd;

extern "C" {

size_t ucd_seg_bce_workspace_bytes(int B, int h, int w) {
  if (B <= 0 || h <= 0 || w <= 0) return 0;
  return (size_t)B * h * w * 2 * sizeof(float);       // one (hard, soft) pair per low-resolution cell
}

int ucd_seg_bce(const float* sem_s, int ld_s, const float* sem_t, int ld_t, const int64_t* labels, int B, int H, int W, int h,
                int w, int Ctot, int K, int ignore_index, float hard_weight, float soft_weight, float* loss_out, float* d_sem,
                int ld_d, void* workspace, size_t workspace_bytes, ucd_stream_t stream) {
  static const char* fn = "ucd_seg_bce";
  UCD_REQUIRE(sem_s && labels && loss_out && workspace, UCD_EINVAL, "%s: NULL argument (sem_s, labels, loss_out or workspace)", fn);
  UCD_REQUIRE(B > 0 && H > 0 && W > 0 && h > 0 && w > 0 && Ctot > 0, UCD_EINVAL,
              "%s: bad sizes (B %d, H %d, W %d, h %d, w %d, Ctot %d must be positive)", fn, B, H, W, h, w, Ctot);
  UCD_REQUIRE(K >= 1 && K <= Ctot, UCD_EINVAL, "%s: K = %d is outside [1, Ctot = %d]", fn, K, Ctot);
  UCD_REQUIRE(ld_s >= Ctot, UCD_EINVAL, "%s: bad leading dimension (ld_s = %d below Ctot = %d)", fn, ld_s, Ctot);
  UCD_REQUIRE(!sem_t || ld_t >= K, UCD_EINVAL, "%s: bad leading dimension (ld_t = %d below K = %d)", fn, ld_t, K);
  UCD_REQUIRE(!d_sem || ld_d >= Ctot, UCD_EINVAL, "%s: bad leading dimension (ld_d = %d below Ctot = %d)", fn, ld_d, Ctot);
  UCD_REQUIRE(H >= h && W >= w, UCD_EINVAL, "%s: bad scale (the label map %d x %d is smaller than the logits %d x %d)", fn, H, W, h, w);
  UCD_REQUIRE((long long)B * h * w <= 0x3fffffffLL, UCD_EINVAL, "%s: %lld low-resolution cells exceed the grid", fn, (long long)B * h * w);
  UCD_REQUIRE(workspace_bytes >= ucd_seg_bce_workspace_bytes(B, h, w), UCD_EWORKSPACE,
              "%s: workspace too small (%zu bytes, %zu needed)", fn, workspace_bytes, ucd_seg_bce_workspace_bytes(B, h, w));
  const size_t lds = (size_t)9 * ((Ctot | 1) + (sem_t ? (K | 1) : 0)) * sizeof(float);
  UCD_REQUIRE(lds <= 64 * 1024, UCD_EUNSUPPORTED, "%s: %d + %d classes exceed the LDS of a cell's neighbourhood", fn, Ctot, K);
  hipStream_t s = (hipStream_t)stream;
  const int cells = B * h * w;
  const float inv_pix = 1.f / ((float)B * H * W);
  float* part = (float*)workspace;
  // torch computes the up-sampling scale as float(in) / out
  seg_bce_kernel<<<cells, kWave, lds, s>>>(sem_s, ld_s, sem_t, ld_t, labels, H, W, h, w, Ctot, K, ignore_index, (float)h / (float)H,
                                           (float)w / (float)W, (float)H / (float)h, (float)W / (float)w, hard_weight * inv_pix,
                                           soft_weight * inv_pix, part, d_sem, ld_d);
  int rc = check_launch(fn);
  if (rc) return rc;
  seg_bce_reduce_kernel<<<1, 1024, 0, s>>>(part, cells, inv_pix, loss_out);
  return check_launch(fn);
}

}  // extern "C"
