// The train transform of a whole batch in ONE launch, for samples that already live in HBM (ucd_amd/datacache.py): crop +
// Pillow BILINEAR resize + flip + ToTensor + Normalize of the images and crop + NEAREST resize + flip + the step's table of the
// labels - what ucd_image_path and ucd_label_path (datapipe.hip) compute with five launches, two table workspaces and a
// [B][hmax][S][3] intermediate in HBM.  Same bits: the arithmetic is datapipe_rules.h in both files.
//
// A workgroup owns a tile of kTY x kTX output pixels of one sample and computes what it needs itself:
//   * the horizontal coefficient entries of its kTX columns and the vertical windows of its kTY rows (wave 0 / wave 1) and the
//     NEAREST source indices of the same columns and rows (waves 2 / 3; entry x is x dependent fp64 additions) go to LDS;
//   * the tile's source-row window [first row's ymin, last row's ymin + count) is streamed in chunks of kRows rows: the
//     horizontal pass writes the chunk's clipped 8-bit pixels of the tile's columns to LDS (what ucd_image_path keeps in
//     `tmp`), the vertical coefficients of (tile row, chunk row) are evaluated once per chunk into LDS, and every thread adds
//     the chunk's part of the vertical sums of its kTY * kTX / 256 pixels in registers.  The sums are integers, so the split
//     into chunks changes no bit, and no down-scaling factor outgrows LDS: a larger factor is more chunks;
//   * horizontal taps past the kTapsLds kept in LDS per column (factors above ~3.5) are evaluated where they are used.
// The tile's columns are columns of the un-flipped resize; a flipped sample stores them mirrored.
#include "common.h"
#include "datapipe_rules.h"

namespace ucd {
namespace {

constexpr int kThreads = 256;
constexpr int kTX = 64;                        // output columns of a tile = lanes of a wave
constexpr int kTY = 16;                        // output rows of a tile
constexpr int kPix = kTX * kTY / kThreads;     // output pixels per thread: consecutive rows of one column
constexpr int kRows = 32;                      // source rows per LDS chunk
constexpr int kTapsLds = 8;                    // horizontal taps per column kept in LDS
static_assert(kThreads == 4 * kTX && kThreads == 256 && kTY % (kThreads / kTX) == 0, "the set-up maps one wave to one table");

__device__ __forceinline__ bool batch_desc_ok(const int* d) {
  return d[2] >= 0 && d[3] >= 0 && d[4] > 0 && d[5] > 0 && (long long)d[2] + d[4] <= d[0] && (long long)d[3] + d[5] <= d[1];
}

__global__ __launch_bounds__(kThreads) void batch_path_kernel(const uint8_t* const* __restrict__ images,
                                                              const uint8_t* const* __restrict__ labels,
                                                              const int* __restrict__ desc, int S, const uint8_t* __restrict__ lut,
                                                              float m0, float m1, float m2, float d0, float d1, float d2,
                                                              float* __restrict__ out_images, int64_t* __restrict__ out_labels) {
  const int b = blockIdx.z;
  const int* d = desc + 8 * b;
  if (!batch_desc_ok(d)) return;                 // the whole workgroup: nothing of the sample is read or written
  const int W0 = d[1], i0 = d[2], j0 = d[3], h = d[4], w = d[5], flip = d[6];
  const int tx0 = blockIdx.x * kTX, ty0 = blockIdx.y * kTY;
  const int nx = S - tx0 < kTX ? S - tx0 : kTX, ny = S - ty0 < kTY ? S - ty0 : kTY;
  const int t = threadIdx.x;

  __shared__ CoeffWindow hwin[kTX], vwin[kTY];
  __shared__ double hww[kTX], vww[kTY];
  __shared__ int hk[kTapsLds][kTX];              // tap-major: a wave reads one tap of its 64 columns from 64 banks
  __shared__ int vk[kTY][kRows];                 // vertical coefficient of (tile row, chunk row); 0 outside the row's window
  __shared__ int xtab[kTX], ytab[kTY];
  __shared__ uint32_t hrow[kRows][kTX];          // the horizontal pass's pixel: r | g << 8 | b << 16
  __shared__ uint8_t lut_s[256];

  const int u = t & (kTX - 1), wave = t / kTX;
  if (wave == 0) {
    if (u < nx) {
      const CoeffWindow c = image_coeff_window(w, S, tx0 + u);
      const double ww = image_coeff_sum(c, c.count);
      hwin[u] = c;
      hww[u] = ww;
      for (int x = 0; x < kTapsLds; ++x) hk[x][u] = x < c.count ? image_coeff_fixed(c, ww, x) : 0;
    }
  } else if (wave == 1) {
    if (u < ny) {
      const CoeffWindow c = image_coeff_window(h, S, ty0 + u);
      vwin[u] = c;
      vww[u] = image_coeff_sum(c, c.count);
    }
  } else if (wave == 2) {
    if (u < nx) xtab[u] = nearest_index(w, S, tx0 + u);
  } else {
    if (u < ny) ytab[u] = nearest_index(h, S, ty0 + u);
  }
  lut_s[t] = lut[t];
  __syncthreads();

  const int sx = u, ybase = wave * kPix;         // this thread's pixels: column sx, tile rows ybase .. ybase + kPix - 1
  const bool col_ok = sx < nx;
  const uint8_t* img = images[b];
  int acc[kPix][3];
#pragma unroll
  for (int q = 0; q < kPix; ++q) acc[q][0] = acc[q][1] = acc[q][2] = 1 << (kPrecisionBits - 1);
  CoeffWindow hc = hwin[col_ok ? sx : 0];
  const double hsum = hww[col_ok ? sx : 0];

  const int r_lo = vwin[0].xmin, r_hi = vwin[ny - 1].xmin + vwin[ny - 1].count;   // both ends grow with the row
  for (int r0 = r_lo; r0 < r_hi; r0 += kRows) {
    const int nr = r_hi - r0 < kRows ? r_hi - r0 : kRows;
    if (col_ok) {
      for (int rr = wave; rr < nr; rr += kThreads / kTX) {
        const uint8_t* row = img + ((size_t)(i0 + r0 + rr) * W0 + j0 + hc.xmin) * 3;
        int s0 = 1 << (kPrecisionBits - 1), s1 = s0, s2 = s0;
        for (int x = 0; x < hc.count; ++x) {
          const int k = x < kTapsLds ? hk[x][sx] : image_coeff_fixed(hc, hsum, x);
          s0 += (int)row[3 * x + 0] * k;
          s1 += (int)row[3 * x + 1] * k;
          s2 += (int)row[3 * x + 2] * k;
        }
        hrow[rr][sx] = (uint32_t)clip8(s0) | (uint32_t)clip8(s1) << 8 | (uint32_t)clip8(s2) << 16;
      }
    }
    for (int e = t; e < kTY * kRows; e += kThreads) {
      const int yl = e / kRows, rr = e % kRows;
      int k = 0;
      if (yl < ny && rr < nr) {
        const int tap = r0 + rr - vwin[yl].xmin;
        if (tap >= 0 && tap < vwin[yl].count) k = image_coeff_fixed(vwin[yl], vww[yl], tap);
      }
      vk[yl][rr] = k;
    }
    __syncthreads();
    if (col_ok) {
#pragma unroll
      for (int q = 0; q < kPix; ++q) {
        const int yl = ybase + q;
        if (yl < ny) {
          const int ymin = vwin[yl].xmin, yend = ymin + vwin[yl].count;
          const int lo = (ymin > r0 ? ymin : r0) - r0, hi = (yend < r0 + nr ? yend : r0 + nr) - r0;
          for (int rr = lo; rr < hi; ++rr) {
            const uint32_t p = hrow[rr][sx];
            const int k = vk[yl][rr];
            acc[q][0] += (int)(p & 255u) * k;
            acc[q][1] += (int)((p >> 8) & 255u) * k;
            acc[q][2] += (int)((p >> 16) & 255u) * k;
          }
        }
      }
    }
    __syncthreads();
  }

  if (!col_ok) return;
  const int xx = flip ? S - 1 - (tx0 + sx) : tx0 + sx;
  const uint8_t* lab = labels[b] + j0 + xtab[sx];
#pragma unroll
  for (int q = 0; q < kPix; ++q) {
    const int yl = ybase + q;
    if (yl >= ny) continue;
    const size_t o = ((size_t)b * S + ty0 + yl) * S + xx;
    float* p = out_images + o * 3;
    p[0] = ((float)clip8(acc[q][0]) / 255.f - m0) / d0;
    p[1] = ((float)clip8(acc[q][1]) / 255.f - m1) / d1;
    p[2] = ((float)clip8(acc[q][2]) / 255.f - m2) / d2;
    out_labels[o] = (int64_t)lut_s[lab[(size_t)(i0 + ytab[yl]) * W0]];
  }
}

}  // namespace
}  // namespace ucd

using namespace ucd;

extern "C" int ucd_batch_path(const uint8_t* const* images, const uint8_t* const* labels, const int* desc, int B, int S,
                              const uint8_t* lut, float mean_r, float mean_g, float mean_b, float std_r, float std_g, float std_b,
                              float* out_images, int64_t* out_labels, ucd_stream_t stream) {
  static const char* fn = "ucd_batch_path";
  UCD_REQUIRE(images && labels && desc && lut && out_images && out_labels && B > 0 && S > 0, UCD_EINVAL, "%s: bad arguments", fn);
  UCD_REQUIRE(B <= 65535 && ceil_div(S, kTY) <= 65535, UCD_EINVAL, "%s: B and S / %d are grid extents (65535 at most)", fn, kTY);
  batch_path_kernel<<<dim3(ceil_div(S, kTX), ceil_div(S, kTY), B), kThreads, 0, (hipStream_t)stream>>>(
      images, labels, desc, S, lut, mean_r, mean_g, mean_b, std_r, std_g, std_b, out_images, out_labels);
  return check_launch(fn);
}
