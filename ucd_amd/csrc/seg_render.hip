// The output side of an evaluation run (the reference's test.py and Trainer.test, train.py:271-375): what a user looks at after a step
// is trained.  The reference keeps fp32 images, int64 labels and int64 predictions of the whole test set on the host and colours them
// there; here one pass over the full-resolution pixel grid writes everything that leaves the device, as uint8:
//   pred_u8   arg-max of the bilinearly up-sampled logits (the arithmetic, and the bits, of seg_confusion_kernel's pred)
//   pred_rgb  cmap[pred]          label_rgb  cmap[label & 255]
//   image_u8  the de-normalised image, trunc(clamp((x * std + mean) * 255, 0, 255))
//   att       (fp32) a low-resolution attention map up-sampled bilinearly, on a source grid of its own
// The tiling is seg_confusion_kernel's (seglogit_loss.hip): a block owns a 64 x 64 pixel tile, the low-resolution cells under it are
// staged in LDS, a thread walks 16 consecutive rows of one pixel column and interpolates its pixel's logits in registers.  A wave
// therefore holds one tile row of 64 pixels at a time: 192 bytes of each RGB output.  Its lanes exchange their packed pixels by
// shuffles so that a lane stores a whole aligned dword of the row; the (at most three) bytes before the first and after the last
// aligned dword are byte stores - at W = 513 the row starts are not dword-aligned.
//
// ucd_attn_energy is the attention map itself (train.py:339-342): a[b, p] = sum_c x[b, p, c]^2 over the channels-last rows of a raw
// map, divided by the Frobenius norm of its image's map.  Two launches, no float atomics, every sum in a fixed order.
#include "common.h"
#include "upsample_index.h"

namespace ucd {
namespace {

constexpr int kThreads = 256;
constexpr int kTileY = 64, kTileX = 64;     // seg_confusion_kernel's tile: a thread walks kRows consecutive rows of one pixel column
constexpr int kRows = kTileY / 4;
constexpr int kCmap = 256;                  // palette entries, staged as packed r | g << 8 | b << 16 words in front of the cells

struct RenderArgs {
  const float* sem; int ld_s;
  const int64_t* labels;
  const float* image; long long sb, sc, sh, sw;
  float mean[3], std[3];
  const uint8_t* cmap;
  const float* att_low; int ha, wa;
  int H, W, h, w, Ctot;
  float scale_h, scale_w, scale_ha, scale_wa;
  uint8_t *pred_u8, *pred_rgb, *label_rgb, *image_u8;
  float* att;
};

// bytes o .. o + 3 of a wave's row of packed 24-bit pixels (lane l holds pixel l): they lie in the pixels o / 3 and o / 3 + 1.
// Every lane of the wave calls it (shuffles); a lane whose o is past the row gets bytes it never stores.
__device__ __forceinline__ uint32_t row_bytes4(uint32_t v, int o) {
  const int p0 = o / 3, r = o - 3 * p0;
  const uint32_t a = __shfl(v, p0 & 63, 64), b = __shfl(v, (p0 + 1) & 63, 64);
  return (uint32_t)((((uint64_t)b << 24) | (uint64_t)a) >> (8 * r));
}

// One tile row of an RGB output: npx pixels = 3 npx bytes at g.  Aligned dwords by the lanes 0 .. nd - 1, the bytes before the first
// one by the lanes 0 .. 2, the bytes after the last one by the lanes 3 .. 5.  Nothing outside [g, g + 3 npx) is written.
__device__ __forceinline__ void store_rgb_row(uint8_t* g, int npx, uint32_t v, int lane) {
  const int nbytes = 3 * npx;
  int head = (int)((4u - (uint32_t)(reinterpret_cast<uintptr_t>(g) & 3u)) & 3u);
  head = head < nbytes ? head : nbytes;
  const int nd = (nbytes - head) >> 2;
  const int o = head + 4 * lane;
  const uint32_t d = row_bytes4(v, o);
  if (lane < nd) *reinterpret_cast<uint32_t*>(g + o) = d;
  const int k = lane < 3 ? lane : head + 4 * nd + (lane - 3);
  const bool live = lane < 3 ? lane < head : (lane < 6 && k < nbytes);
  const uint32_t e = row_bytes4(v, live ? k : 0);
  if (live) g[k] = (uint8_t)e;
}

__global__ __launch_bounds__(kThreads) void seg_render_kernel(const RenderArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  uint32_t* s_cmap = reinterpret_cast<uint32_t*>(smem);         // [kCmap]
  float* s_log = smem + kCmap;                                  // [ncell][Ctot]
  const int H = p.H, W = p.W, Ctot = p.Ctot;
  const int b = blockIdx.z, ty0 = blockIdx.y * kTileY, tx0 = blockIdx.x * kTileX;
  const bool need_pred = p.pred_u8 || p.pred_rgb;
  int ya, ny, xa, nx;
  tile_span(ty0, kTileY, H, p.h, p.scale_h, ya, ny);
  tile_span(tx0, kTileX, W, p.w, p.scale_w, xa, nx);
  for (int i = threadIdx.x; i < kCmap; i += kThreads)
    s_cmap[i] = (uint32_t)p.cmap[3 * i] | ((uint32_t)p.cmap[3 * i + 1] << 8) | ((uint32_t)p.cmap[3 * i + 2] << 16);
  if (need_pred)
    for (int i = threadIdx.x; i < ny * nx * Ctot; i += kThreads) {
      const int cell = i / Ctot, c = i - cell * Ctot;
      const int cy = ya + cell / nx, cx = xa + cell % nx;
      s_log[i] = p.sem[((size_t)(b * p.h + cy) * p.w + cx) * p.ld_s + c];
    }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int X = tx0 + lane;
  const bool inx = X < W;
  const int npx = W - tx0 < kTileX ? W - tx0 : kTileX;
  int x0 = 0, x1 = 0, ax0 = 0, ax1 = 0;
  float lx0 = 0.f, lx1 = 0.f, alx0 = 0.f, alx1 = 0.f;
  if (inx) up_src(X, p.w, p.scale_w, x0, x1, lx0, lx1);
  if (inx && p.att) up_src(X, p.wa, p.scale_wa, ax0, ax1, alx0, alx1);
  for (int it = 0; it < kRows; ++it) {
    const int Y = ty0 + (threadIdx.x >> 6) * kRows + it;
    if (Y >= H) break;                                          // wave-uniform: the lanes of a wave share the row
    const size_t row = ((size_t)b * H + Y) * W;                 // every lane stays in the loop body for the shuffles below
    int arg = 0;
    if (need_pred && inx) {
      int y0, y1;
      float ly0, ly1;
      up_src(Y, p.h, p.scale_h, y0, y1, ly0, ly1);
      const int c00 = (y0 - ya) * nx + (x0 - xa), c01 = (y0 - ya) * nx + (x1 - xa);
      const int c10 = (y1 - ya) * nx + (x0 - xa), c11 = (y1 - ya) * nx + (x1 - xa);
      // seg_confusion_kernel's expression, written again (-ffp-contract=off: equal expressions, equal bits); first maximum wins
      float best = -INFINITY;
      for (int c = 0; c < Ctot; ++c) {
        const float z = ly0 * (lx0 * s_log[c00 * Ctot + c] + lx1 * s_log[c01 * Ctot + c]) +
                        ly1 * (lx0 * s_log[c10 * Ctot + c] + lx1 * s_log[c11 * Ctot + c]);
        if (z > best) { best = z; arg = c; }
      }
      if (p.pred_u8) p.pred_u8[row + X] = (uint8_t)arg;
    }
    if (p.pred_rgb) store_rgb_row(p.pred_rgb + (row + tx0) * 3, npx, s_cmap[arg], lane);
    if (p.label_rgb) {
      const int64_t lab = inx ? p.labels[row + X] : 0;
      store_rgb_row(p.label_rgb + (row + tx0) * 3, npx, s_cmap[(int)(lab & 255)], lane);
    }
    if (p.image_u8) {
      uint32_t v = 0;
      if (inx) {
        const float* px = p.image + (long long)b * p.sb + (long long)Y * p.sh + (long long)X * p.sw;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          float f = (px[c * p.sc] * p.std[c] + p.mean[c]) * 255.f;
          f = fminf(fmaxf(f, 0.f), 255.f);                      // the reference's astype(uint8) wraps; a NaN reads as 0
          v |= (uint32_t)(int)f << (8 * c);
        }
      }
      store_rgb_row(p.image_u8 + (row + tx0) * 3, npx, v, lane);
    }
    if (p.att && inx) {
      int y0, y1;
      float ly0, ly1;
      up_src(Y, p.ha, p.scale_ha, y0, y1, ly0, ly1);
      const float* al = p.att_low + (size_t)b * p.ha * p.wa;
      p.att[row + X] = ly0 * (alx0 * al[y0 * p.wa + ax0] + alx1 * al[y0 * p.wa + ax1]) +
                       ly1 * (alx0 * al[y1 * p.wa + ax0] + alx1 * al[y1 * p.wa + ax1]);
    }
  }
}

// ---- attention energy ----------------------------------------------------------------------------------------------------------
constexpr int kAeRows = kThreads / 64;      // one wave per cell

__device__ __forceinline__ float ae_get(const float* p) { return *p; }
__device__ __forceinline__ float ae_get(const __hip_bfloat16* p) { return __bfloat162float(*p); }

// a[r] = sum_c x[r, c]^2: 16-byte loads over the first Cv channels (Cv = 0 when base or pitch are off the 16-byte grid), a lane-strided
// tail for the rest; a lane over its channels, then the wave by shuffles - a fixed order
template <typename T>
__global__ __launch_bounds__(kThreads) void attn_rowsq_kernel(const T* __restrict__ x, int ld, int M, int C, int Cv, float* __restrict__ a) {
  constexpr int VEC = Vec<T>::N;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = blockIdx.x * kAeRows + wave;
  if (r >= M) return;
  const T* row = x + (size_t)r * ld;
  float s = 0.f;
  for (int c = lane * VEC; c < Cv; c += 64 * VEC) {
    Vec<T> v;
    v.load(row + c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) s += v.get(i) * v.get(i);
  }
  for (int c = Cv + lane; c < C; c += 64) {
    const float v = ae_get(row + c);
    s += v * v;
  }
  s = wave_sum(s);
  if (lane == 0) a[r] = s;
}

// a[b, :] /= || a[b, :] ||_2, one block per image: thread t adds the cells t, t + 256, ..., then the shuffles, then the four waves
__global__ __launch_bounds__(kThreads) void attn_unit_kernel(float* __restrict__ a, int HW) {
  __shared__ float red[kAeRows];
  float* ab = a + (size_t)blockIdx.x * HW;
  float s = 0.f;
  for (int q = threadIdx.x; q < HW; q += kThreads) s += ab[q] * ab[q];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  const float norm = sqrtf((red[0] + red[1]) + (red[2] + red[3]));
  for (int q = threadIdx.x; q < HW; q += kThreads) ab[q] = ab[q] / norm;
}

}  // namespace
}  // namespace ucd

using namespace ucd;

extern "C" {

int ucd_seg_render(const float* sem, int ld_s, const int64_t* labels, const float* image, long long sb, long long sc, long long sh,
                   long long sw, float mean_r, float mean_g, float mean_b, float std_r, float std_g, float std_b, const uint8_t* cmap,
                   const float* att_low, int ha, int wa, int B, int H, int W, int h, int w, int Ctot, uint8_t* pred_u8,
                   uint8_t* pred_rgb, uint8_t* label_rgb, uint8_t* image_u8, float* att, ucd_stream_t stream) {
  static const char* fn = "ucd_seg_render";
  UCD_REQUIRE(sem, UCD_EINVAL, "%s: NULL argument (sem)", fn);
  UCD_REQUIRE(cmap, UCD_EINVAL, "%s: NULL argument (cmap)", fn);
  UCD_REQUIRE(B > 0 && H > 0 && W > 0 && h > 0 && w > 0 && Ctot > 0, UCD_EINVAL,
              "%s: bad sizes (B = %d, H = %d, W = %d, h = %d, w = %d, Ctot = %d: each must be at least 1)", fn, B, H, W, h, w, Ctot);
  UCD_REQUIRE(ld_s >= Ctot, UCD_EINVAL, "%s: ld_s = %d is below Ctot = %d", fn, ld_s, Ctot);
  UCD_REQUIRE(Ctot <= 255, UCD_EINVAL, "%s: Ctot = %d classes do not fit the uint8 prediction map (at most 255)", fn, Ctot);
  UCD_REQUIRE(pred_u8 || pred_rgb || label_rgb || image_u8 || att, UCD_EINVAL,
              "%s: every output is NULL (pred_u8, pred_rgb, label_rgb, image_u8, att)", fn);
  UCD_REQUIRE(!label_rgb || labels, UCD_EINVAL, "%s: label_rgb needs labels", fn);
  UCD_REQUIRE(!image_u8 || image, UCD_EINVAL, "%s: image_u8 needs image", fn);
  UCD_REQUIRE(!att || att_low, UCD_EINVAL, "%s: att needs att_low", fn);
  UCD_REQUIRE(!att || (ha > 0 && wa > 0), UCD_EINVAL, "%s: bad sizes (ha = %d, wa = %d: each must be at least 1 with att)", fn, ha, wa);
  UCD_REQUIRE((float)H / h >= 4.f && (float)W / w >= 4.f, UCD_EUNSUPPORTED,
              "%s: built for up-sampling factors >= 4 (the model's is 16)", fn);
  const int tiles_x = ceil_div(W, kTileX), tiles_y = ceil_div(H, kTileY);
  const int ny = (int)(kTileY * (float)h / H) + 3, nx = (int)(kTileX * (float)w / W) + 3;      // ucd_seg_confusion's bound
  const size_t lds = ((size_t)ny * nx * Ctot + kCmap) * sizeof(float);
  UCD_REQUIRE(lds <= 150 * 1024, UCD_EUNSUPPORTED, "%s: %d classes exceed the LDS budget", fn, Ctot);
  RenderArgs p;
  p.sem = sem; p.ld_s = ld_s; p.labels = labels;
  p.image = image; p.sb = sb; p.sc = sc; p.sh = sh; p.sw = sw;
  p.mean[0] = mean_r; p.mean[1] = mean_g; p.mean[2] = mean_b;
  p.std[0] = std_r; p.std[1] = std_g; p.std[2] = std_b;
  p.cmap = cmap; p.att_low = att_low; p.ha = att ? ha : 1; p.wa = att ? wa : 1;
  p.H = H; p.W = W; p.h = h; p.w = w; p.Ctot = Ctot;
  p.scale_h = (float)h / (float)H; p.scale_w = (float)w / (float)W;
  p.scale_ha = (float)p.ha / (float)H; p.scale_wa = (float)p.wa / (float)W;
  p.pred_u8 = pred_u8; p.pred_rgb = pred_rgb; p.label_rgb = label_rgb; p.image_u8 = image_u8; p.att = att;
  UCD_TRY_LDS(seg_render_kernel, 150 * 1024);
  seg_render_kernel<<<dim3(tiles_x, tiles_y, B), kThreads, lds, (hipStream_t)stream>>>(p);
  return check_launch(fn);
}

int ucd_attn_energy(const void* x, int ld, int dtype, int B, int HW, int C, float* a, ucd_stream_t stream) {
  static const char* fn = "ucd_attn_energy";
  UCD_REQUIRE(x, UCD_EINVAL, "%s: NULL argument (x)", fn);
  UCD_REQUIRE(a, UCD_EINVAL, "%s: NULL argument (a)", fn);
  UCD_REQUIRE(dtype == UCD_F32 || dtype == UCD_BF16, UCD_EINVAL, "%s: unknown dtype %d", fn, dtype);
  UCD_REQUIRE(B > 0 && HW > 0 && C > 0, UCD_EINVAL, "%s: bad sizes (B = %d, HW = %d, C = %d: each must be at least 1)", fn, B, HW, C);
  UCD_REQUIRE((long long)B * HW <= 0x7FFFFFFF / 4, UCD_EINVAL, "%s: B * HW = %lld rows are more than the kernels index", fn,
              (long long)B * HW);
  UCD_REQUIRE(ld >= C, UCD_EINVAL, "%s: ld = %d is below C = %d", fn, ld, C);
  hipStream_t s = (hipStream_t)stream;
  const int M = B * HW, blocks = ceil_div(M, kAeRows);
  const int es = dtype == UCD_BF16 ? 2 : 4, vec = 16 / es;
  const int Cv = (aligned16(x) && ((size_t)ld * es) % 16 == 0) ? C / vec * vec : 0;
  if (dtype == UCD_BF16)
    attn_rowsq_kernel<__hip_bfloat16><<<blocks, kThreads, 0, s>>>((const __hip_bfloat16*)x, ld, M, C, Cv, a);
  else
    attn_rowsq_kernel<float><<<blocks, kThreads, 0, s>>>((const float*)x, ld, M, C, Cv, a);
  int rc = check_launch(fn);
  if (rc) return rc;
  attn_unit_kernel<<<B, kThreads, 0, s>>>(a, HW);
  return check_launch(fn);
}

}  // extern "C"
