// fp32 stride-1 convolutions (1x1 and 3x3 with padding = dilation) of the fp32 training mode (--opt_level O0) on the bf16
// matrix cores, by splitting every operand in two bf16 parts (reference call sites modules/residual.py:57-73 conv1 / conv2 /
// conv3, modules/deeplab.py:24-37,56-58 map_convs / red_conv).
//
// gfx950 has no xf32 MFMA, and v_mfma_f32_32x32x2_f32 runs at 1/16 of the bf16 rate.  Here x = hi + lo with hi = bf16_rn(x),
// lo = bf16_rn(x - hi) (x - hi is exact in fp32), and a product is accumulated in fp32 as hi.hi + hi.lo + lo.hi on
// v_mfma_f32_32x32x16_bf16: three bf16 MFMAs per product, i.e. up to 16 / 3 of the f32-MFMA ceiling.  Error per product: the
// rounding of lo (<= 2^-9 |x - hi| <= 2^-18 |x|) on either side plus the dropped lo.lo (<= 2^-18 |a b|): ~3 2^-18 ~ 1e-5
// relative, against ~4e-3 for a single bf16 product.  Inputs are assumed finite.
//
// Operands are fp32 channels-last row matrices with a row pitch.  Every staged element is split ONCE: a thread loads fp32 from
// global (buffer loads whose range check zero-fills rows past the end, 3x3 halo positions and channel tails - nothing outside an
// operand is read), splits in registers (v_cvt_pk_bf16_f32) and writes a hi and a lo plane to LDS; the wave fragments are then
// the plain bf16 reads of csrc/conv1x1.hip (lane l: 8 consecutive k of row l & 31, k group l >> 5).
//
//   ucd_conv_f32        Y[M, N] (+)= im2col(X)[M, taps K] . W[N, taps K]^T   (taps 1: 1x1; taps 9: 3x3 over the [B, H, W, K] map)
//   ucd_conv_f32_wgrad  dW[N, taps K] = sum_m dZ[m, n] X[shift_tap(m), k]: row chunks into fp32 slabs, summed in a fixed order
//                       (no atomics: bit-reproducible).  The reduction index m is the ROW index of both operands, so the staging
//                       writes the planes transposed ([channel][m]); the fragment reads stay the same.
//
// Tiling: 128 x 128 output tile per workgroup of 4 waves (2 x 2 wave tiles of 64 x 64 = 2 x 2 accumulators of 32 x 32), K step
// 32, two LDS stages of (A + B) x (hi + lo) planes [128][32 + 8 pad] bf16 (80 B rows: the 16 lanes of a ds_read_b128 group hit
// 16 disjoint 4-bank groups) = 80 KB, two workgroups per CU.  The fp32 loads of step k + 1 are issued before the MFMAs of step k
// and split into the other stage after them: one barrier per K step.
#include "common.h"

namespace ucd {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kBM = 128, kBN = 128, kBK = 32;
constexpr int kPitch = kBK + 8;                        // bf16 per LDS row (80 B)
constexpr int kPlane = kBM * kPitch;                   // bf16 per plane
constexpr int kStage = 4 * kPlane;                     // A hi, A lo, B hi, B lo
constexpr int kLdsBytes = 2 * kStage * 2;              // two stages: 80 KB
constexpr unsigned kOOB = 0x7FFFFFF0u;                 // voffset past every record count: the load returns zeros
constexpr int kSumThreads = 256;

struct FwdArgs {
  const float* A; int lda;
  const float* W; int ldw;
  float* Y; int ldy;
  int M, N, K, taps, H, Wd, dil;
  int a_bytes, w_bytes;                                // record counts of the two buffer descriptors
  int accumulate, tiles_n;
};

struct WgradArgs {
  const float* DZ; int ldz;
  const float* X; int ldx;
  float* out;                                          // dw (one chunk) or the slabs [chunks][N][taps K]
  int M, N, K, taps, H, Wd, dil;
  int z_bytes, x_bytes;
  int rows_per_chunk, tiles_n, tiles_k;
};

struct SumArgs {
  const float* slabs; float* dw; int chunks; int n4;   // n4: float4 per slab
};

__device__ __forceinline__ u32x4 load16(__amdgpu_buffer_rsrc_t rs, unsigned voff, int soff) {
  return __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff, soff, 0);
}

__device__ __forceinline__ void split4(u32x4 v, bf16x4& hi, bf16x4& lo) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float x = __uint_as_float(v[e]);
    const __bf16 h = (__bf16)x;
    hi[e] = h;
    lo[e] = (__bf16)(x - (float)h);
  }
}

// 16 x 3 MFMAs of one K step (two 16-deep slices) on the stage at S: wave tile (wm, wn) of 64 x 64
__device__ __forceinline__ void mma_step(const __bf16* S, int wm, int wn, int lane, f32x16 (&acc)[2][2]) {
  const __bf16* Ah = S;
  const __bf16* Al = S + kPlane;
  const __bf16* Bh = S + 2 * kPlane;
  const __bf16* Bl = S + 3 * kPlane;
  const int fr = lane & 31, fh = lane >> 5;
#pragma unroll
  for (int kk = 0; kk < kBK / 16; ++kk) {
    bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int o = (wm * 64 + a * 32 + fr) * kPitch + kk * 16 + fh * 8;
      ah[a] = *reinterpret_cast<const bf16x8*>(Ah + o);
      al[a] = *reinterpret_cast<const bf16x8*>(Al + o);
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int o = (wn * 64 + b * 32 + fr) * kPitch + kk * 16 + fh * 8;
      bh[b] = *reinterpret_cast<const bf16x8*>(Bh + o);
      bl[b] = *reinterpret_cast<const bf16x8*>(Bl + o);
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bh[b], acc[a][b], 0, 0, 0);
        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bl[b], acc[a][b], 0, 0, 0);
        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[a], bh[b], acc[a][b], 0, 0, 0);
      }
  }
}

// ---- forward / input gradient ---------------------------------------------------------------------------------------------------
// Staging: thread -> 16-byte k quad q = tid & 7 of tile rows r + 32 i (i < 4), for A (shifted by the tap) and W alike.
__global__ __launch_bounds__(kThreads, 2) void conv_f32_kernel(FwdArgs p) {
  extern __shared__ __attribute__((aligned(16))) __bf16 lds[];
  const int tm = blockIdx.x / p.tiles_n, tn = blockIdx.x - tm * p.tiles_n;
  const int m0 = tm * kBM, n0 = tn * kBN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int q = tid & 7, r = tid >> 3;

  const auto rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, p.a_bytes, 0x00020000);
  const auto rsW = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, p.w_bytes, 0x00020000);
  const int HW = p.H * p.Wd;
  int py[4], px[4];                                    // taps 9: pixel of each staged row (py < 0: past M)
  unsigned aoff[4], woff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + r + 32 * i, n = n0 + r + 32 * i;
    aoff[i] = m < p.M ? (unsigned)(((size_t)m * p.lda + 4 * q) * 4) : kOOB;
    woff[i] = n < p.N ? (unsigned)(((size_t)n * p.ldw + 4 * q) * 4) : kOOB;
    py[i] = -(1 << 20); px[i] = 0;
    if (p.taps == 9 && m < p.M) {
      const int rem = m % HW;
      py[i] = rem / p.Wd;
      px[i] = rem - py[i] * p.Wd;
    }
  }
  const int kpt = p.K / kBK, nk = p.taps * kpt;
  int cur_tap = -1;
  u32x4 ra[4], rb[4];
  auto load = [&](int kb) {
    const int tap = kb / kpt, k0 = (kb - tap * kpt) * kBK;
    if (p.taps == 9 && tap != cur_tap) {               // shifted source rows of this tap, halo -> out of range
      const int dy = (tap / 3 - 1) * p.dil, dx = (tap % 3 - 1) * p.dil;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int yy = py[i] + dy, xx = px[i] + dx;
        const bool ok = (unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.Wd;
        const int m = m0 + r + 32 * i;
        aoff[i] = ok ? (unsigned)(((size_t)(m + dy * p.Wd + dx) * p.lda + 4 * q) * 4) : kOOB;
      }
      cur_tap = tap;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = load16(rsA, aoff[i], k0 * 4);
      rb[i] = load16(rsW, woff[i], (tap * p.K + k0) * 4);
    }
  };
  auto stage = [&](__bf16* S) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bf16x4 h, l;
      const int o = (r + 32 * i) * kPitch + 4 * q;
      split4(ra[i], h, l);
      *reinterpret_cast<bf16x4*>(S + o) = h;
      *reinterpret_cast<bf16x4*>(S + kPlane + o) = l;
      split4(rb[i], h, l);
      *reinterpret_cast<bf16x4*>(S + 2 * kPlane + o) = h;
      *reinterpret_cast<bf16x4*>(S + 3 * kPlane + o) = l;
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

  load(0);
  stage(lds);
  __syncthreads();
  for (int kb = 0; kb < nk; ++kb) {
    if (kb + 1 < nk) load(kb + 1);
    mma_step(lds + (kb & 1) * kStage, wm, wn, lane, acc);
    if (kb + 1 < nk) stage(lds + ((kb + 1) & 1) * kStage);
    __syncthreads();
  }

  // epilogue: lane -> column n0 + wn 64 + b 32 + (lane & 31), rows of the 32 x 32 accumulator layout; 32 lanes store 128 B of a row
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int col = n0 + wn * 64 + b * 32 + (lane & 31);
      if (col >= p.N) continue;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * 64 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (row < p.M) {
          float* y = p.Y + (size_t)row * p.ldy + col;
          *y = p.accumulate ? *y + acc[a][b][e] : acc[a][b][e];
        }
      }
    }
}

// ---- weight gradient ------------------------------------------------------------------------------------------------------------
// Workgroup (tile t, chunk c): output rows n0.. of dW, columns k0.. of tap `tap`, over the rows [c rows_per_chunk, ...) of the
// chunk.  Staging: thread -> rows 4 g .. 4 g + 3 of the 32-row step (g = lane & 7) and the channel quad cq = (lane >> 3) + 8 wave:
// four 16-byte loads per operand, written transposed as 8-byte runs of 4 m per channel (32 lanes of a ds_write_b64 cover all 64
// banks once).
__global__ __launch_bounds__(kThreads, 2) void conv_f32_wgrad_kernel(WgradArgs p) {
  extern __shared__ __attribute__((aligned(16))) __bf16 lds[];
  const int per_tap = p.tiles_n * p.tiles_k;
  const int tap = blockIdx.x / per_tap, t = blockIdx.x - tap * per_tap;
  const int tn = t / p.tiles_k, tk = t - tn * p.tiles_k;
  const int n0 = tn * kBN, k0 = tk * kBN;
  const int mbeg = blockIdx.y * p.rows_per_chunk, mend = min(p.M, mbeg + p.rows_per_chunk);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int g = lane & 7, cq = (lane >> 3) + 8 * wave;

  const auto rsZ = __builtin_amdgcn_make_buffer_rsrc((void*)p.DZ, 0, p.z_bytes, 0x00020000);
  const auto rsX = __builtin_amdgcn_make_buffer_rsrc((void*)p.X, 0, p.x_bytes, 0x00020000);
  const bool nok = n0 + 4 * cq < p.N, kok = k0 + 4 * cq < p.K;
  const int dy = p.taps == 9 ? (tap / 3 - 1) * p.dil : 0, dx = p.taps == 9 ? (tap % 3 - 1) * p.dil : 0;
  // pixel (y, x) of row mbeg + 4 g + j, advanced by 32 rows per step
  int yy[4], xx[4];
  const int HW = p.H * p.Wd;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    yy[j] = xx[j] = 0;
    if (p.taps == 9) {
      const int rem = (mbeg + 4 * g + j) % HW;
      yy[j] = rem / p.Wd;
      xx[j] = rem - yy[j] * p.Wd;
    }
  }
  u32x4 rz[4], rx[4];
  int mstep = mbeg;
  auto load = [&]() {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = mstep + 4 * g + j;
      const bool live = m < mend;
      const unsigned zo = live && nok ? (unsigned)(((size_t)m * p.ldz + n0 + 4 * cq) * 4) : kOOB;
      bool inside = live && kok;
      int src = m;
      if (p.taps == 9) {
        const int y2 = yy[j] + dy, x2 = xx[j] + dx;
        inside = inside && (unsigned)y2 < (unsigned)p.H && (unsigned)x2 < (unsigned)p.Wd;
        src = m + dy * p.Wd + dx;
        // next step: 32 rows on
        int x3 = xx[j] + 32, y3 = yy[j];
        while (x3 >= p.Wd) { x3 -= p.Wd; if (++y3 == p.H) y3 = 0; }
        xx[j] = x3; yy[j] = y3;
      }
      const unsigned xo = inside ? (unsigned)(((size_t)src * p.ldx + k0 + 4 * cq) * 4) : kOOB;
      rz[j] = load16(rsZ, zo, 0);
      rx[j] = load16(rsX, xo, 0);
    }
    mstep += kBK;
  };
  auto stage = [&](__bf16* S) {
    bf16x4 zh[4], zl[4], xh[4], xl[4];                 // [j] = row 4 g + j, 4 channels
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      split4(rz[j], zh[j], zl[j]);
      split4(rx[j], xh[j], xl[j]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {                      // channel 4 cq + c: the 4 rows as one 8-byte run
      const int o = (4 * cq + c) * kPitch + 4 * g;
      *reinterpret_cast<bf16x4*>(S + o) = bf16x4{zh[0][c], zh[1][c], zh[2][c], zh[3][c]};
      *reinterpret_cast<bf16x4*>(S + kPlane + o) = bf16x4{zl[0][c], zl[1][c], zl[2][c], zl[3][c]};
      *reinterpret_cast<bf16x4*>(S + 2 * kPlane + o) = bf16x4{xh[0][c], xh[1][c], xh[2][c], xh[3][c]};
      *reinterpret_cast<bf16x4*>(S + 3 * kPlane + o) = bf16x4{xl[0][c], xl[1][c], xl[2][c], xl[3][c]};
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

  const int nk = (mend - mbeg + kBK - 1) / kBK;
  load();
  stage(lds);
  __syncthreads();
  for (int kb = 0; kb < nk; ++kb) {
    if (kb + 1 < nk) load();
    mma_step(lds + (kb & 1) * kStage, wm, wn, lane, acc);
    if (kb + 1 < nk) stage(lds + ((kb + 1) & 1) * kStage);
    __syncthreads();
  }

  const int ld = p.taps * p.K;
  float* out = p.out + (size_t)blockIdx.y * p.N * ld;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int k = k0 + wn * 64 + b * 32 + (lane & 31);
      if (k >= p.K) continue;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int n = n0 + wm * 64 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (n < p.N) out[(size_t)n * ld + tap * p.K + k] = acc[a][b][e];
      }
    }
}

// dw = sum of the slabs in chunk order (fixed: bit-reproducible)
__global__ __launch_bounds__(kSumThreads) void conv_f32_wgrad_sum_kernel(SumArgs p) {
  const int i = blockIdx.x * kSumThreads + threadIdx.x;
  if (i >= p.n4) return;
  const float4* s = reinterpret_cast<const float4*>(p.slabs);
  float4 v = s[i];
  for (int c = 1; c < p.chunks; ++c) {
    const float4 u = s[(size_t)c * p.n4 + i];
    v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
  }
  reinterpret_cast<float4*>(p.dw)[i] = v;
}

// Row chunks of a weight gradient: enough workgroups for two per CU on 256 CUs, chunks of at least 1024 rows (32 K steps)
struct WgradPlan { int chunks, rows_per_chunk, tiles_n, tiles_k; };
WgradPlan wgrad_plan(int M, int N, int K, int taps) {
  WgradPlan pl;
  pl.tiles_n = ceil_div(N, kBN);
  pl.tiles_k = ceil_div(K, kBN);
  const int tiles = pl.tiles_n * pl.tiles_k * taps;
  int chunks = ceil_div(512, tiles);
  chunks = max(1, min(chunks, M / 1024));
  pl.rows_per_chunk = ceil_div(ceil_div(M, chunks), kBK) * kBK;
  pl.chunks = ceil_div(M, pl.rows_per_chunk);
  return pl;
}

// byte extent of a row matrix, -1 when it does not fit a 31-bit buffer offset
long long extent(int rows, int ld, int width) {
  const long long b = ((long long)(rows - 1) * ld + width) * 4;
  return b < (long long)kOOB - (1 << 20) ? b : -1;
}

bool map_ok(int M, int taps, int H, int W, int dil) {
  if (taps == 1) return true;
  return taps == 9 && H > 0 && W > 0 && dil >= 1 && M % (H * W) == 0;
}

}  // namespace
}  // namespace ucd

using namespace ucd;

extern "C" {

int ucd_conv_f32(const float* a, int lda, const float* w, int ldw, float* y, int ldy, int M, int N, int K, int taps, int H, int W,
                 int dilation, int accumulate, ucd_stream_t stream) {
  static const char* fn = "ucd_conv_f32";
  UCD_REQUIRE(a && w && y, UCD_EINVAL, "%s: NULL argument", fn);
  UCD_REQUIRE(M > 0 && N > 0 && K > 0 && K % kBK == 0 && N % 32 == 0, UCD_EINVAL,
              "%s: M (%d) > 0, K (%d) and N (%d) multiples of 32 required", fn, M, K, N);
  UCD_REQUIRE(taps == 1 || taps == 9, UCD_EINVAL, "%s: taps must be 1 or 9", fn);
  UCD_REQUIRE(map_ok(M, taps, H, W, dilation), UCD_EINVAL, "%s: M (%d) is not a whole number of %d x %d maps", fn, M, H, W);
  UCD_REQUIRE(aligned16(a) && aligned16(w) && lda % 4 == 0 && ldw % 4 == 0 && lda >= K && ldw >= taps * K && ldy >= N,
              UCD_EINVAL, "%s: operands need 16-byte aligned bases and pitches covering their rows", fn);
  const long long ab = extent(M, lda, K), wb = extent(N, ldw, taps * K);
  UCD_REQUIRE(ab > 0 && wb > 0 && extent(M, ldy, N) > 0, UCD_EINVAL, "%s: operand larger than 2 GB", fn);
  FwdArgs p{a, lda, w, ldw, y, ldy, M, N, K, taps, taps == 9 ? H : 1, taps == 9 ? W : 1, taps == 9 ? dilation : 0,
            (int)ab, (int)wb, accumulate ? 1 : 0, ceil_div(N, kBN)};
  UCD_TRY_LDS(conv_f32_kernel, kLdsBytes);
  conv_f32_kernel<<<ceil_div(M, kBM) * p.tiles_n, kThreads, kLdsBytes, (hipStream_t)stream>>>(p);
  return check_launch(fn);
}

size_t ucd_conv_f32_wgrad_workspace_bytes(int M, int N, int K, int taps) {
  if (M <= 0 || N <= 0 || K <= 0 || N % 32 || K % 32 || (taps != 1 && taps != 9)) return 0;
  const WgradPlan pl = wgrad_plan(M, N, K, taps);
  return pl.chunks > 1 ? (size_t)pl.chunks * N * taps * K * sizeof(float) : 0;
}

int ucd_conv_f32_wgrad(const float* dz, int ld_dz, const float* x, int ld_x, int M, int N, int K, int taps, int H, int W,
                       int dilation, float* dw, void* workspace, size_t workspace_bytes, ucd_stream_t stream) {
  static const char* fn = "ucd_conv_f32_wgrad";
  UCD_REQUIRE(dz && x && dw, UCD_EINVAL, "%s: NULL argument", fn);
  UCD_REQUIRE(M > 0 && N > 0 && K > 0 && N % 32 == 0 && K % 32 == 0, UCD_EINVAL,
              "%s: M (%d) > 0, N (%d) and K (%d) multiples of 32 required", fn, M, N, K);
  UCD_REQUIRE(taps == 1 || taps == 9, UCD_EINVAL, "%s: taps must be 1 or 9", fn);
  UCD_REQUIRE(map_ok(M, taps, H, W, dilation), UCD_EINVAL, "%s: M (%d) is not a whole number of %d x %d maps", fn, M, H, W);
  UCD_REQUIRE(aligned16(dz) && aligned16(x) && aligned16(dw) && ld_dz % 4 == 0 && ld_x % 4 == 0 && ld_dz >= N && ld_x >= K,
              UCD_EINVAL, "%s: operands need 16-byte aligned bases and pitches covering their rows", fn);
  const long long zb = extent(M, ld_dz, N), xb = extent(M, ld_x, K);
  UCD_REQUIRE(zb > 0 && xb > 0 && extent(N, taps * K, taps * K) > 0, UCD_EINVAL, "%s: operand larger than 2 GB", fn);
  const WgradPlan pl = wgrad_plan(M, N, K, taps);
  const size_t need = pl.chunks > 1 ? (size_t)pl.chunks * N * taps * K * sizeof(float) : 0;
  UCD_REQUIRE(workspace_bytes >= need && (need == 0 || (workspace && aligned16(workspace))), UCD_EINVAL,
              "%s: workspace of %zu bytes needed", fn, need);
  WgradArgs p{dz, ld_dz, x, ld_x, pl.chunks > 1 ? (float*)workspace : dw, M, N, K, taps, taps == 9 ? H : 1, taps == 9 ? W : 1,
              taps == 9 ? dilation : 0, (int)zb, (int)xb, pl.rows_per_chunk, pl.tiles_n, pl.tiles_k};
  UCD_TRY_LDS(conv_f32_wgrad_kernel, kLdsBytes);
  conv_f32_wgrad_kernel<<<dim3(pl.tiles_n * pl.tiles_k * taps, pl.chunks), kThreads, kLdsBytes, (hipStream_t)stream>>>(p);
  int rc = check_launch(fn);
  if (rc || pl.chunks == 1) return rc;
  SumArgs s{(const float*)workspace, dw, pl.chunks, N * taps * K / 4};
  conv_f32_wgrad_sum_kernel<<<ceil_div(s.n4, kSumThreads), kSumThreads, 0, (hipStream_t)stream>>>(s);
  return check_launch(fn);
}

}  // extern "C"
