// PLOP's pseudo-labelling (include/ucd_hip.h): at an incremental step a pixel labelled background takes the
// class the frozen teacher predicts there when the teacher is confident, and leaves the cross entropy when it is not.  As a torch
// composition that is interpolate -> softmax -> log -> sum -> max -> masked writes on a [B, K, H, W] tensor; here a full-resolution
// teacher logit only ever exists in a register.
// One device pixel walk serves both passes: a workgroup owns a tile of pixels, the low-resolution teacher cells under it are staged
// in LDS, one lane per pixel (consecutive lanes along x: the 8-byte label loads and stores of a wave are one contiguous run)
// rebuilds z_c from four LDS reads per class - the arithmetic of seg_confusion_kernel, torch's - and only for CANDIDATE pixels
// (0 <= label < K, label != ignore_index).  Two class loops: the first maximum (torch's tie rule), then the entropy around it.
//   pseudo_hist_kernel   hist[c*, bin(u)] += 1, summed per workgroup in LDS where K x bins words fit beside the cells, else per
//                        wave (equal keys of a wave are added once); 64-bit integer adds in global memory: exact, no order
//   pseudo_label_kernel  labels_out, the optional uncertainty map, per-image (passed, candidates) counts: lanes, waves through
//                        LDS, one pair of 32-bit integer adds per workgroup
//   pseudo_factor_kernel the adaptive factor of each image from its counts (the last launch of ucd_pseudo_label)
#include "common.h"
#include "upsample_index.h"

namespace ucd {
namespace {

constexpr int kMaxThreads = 256;
constexpr float kL2e = 1.4426950408889634f;

// what the teacher says about one pixel: the first arg-max of the up-sampled logits and u = H(softmax z) / log K
struct TeacherView { int arg; float u; };

struct PseudoTile {
  int b, ty0, tx0, ya, xa, nx, KS;
  float scale_h, scale_w;
};

// stage the cells under the tile: cells[cell][KS], KS = K | 1 (an odd stride: at small factors the lanes of a wave read different
// cells at one class)
__device__ __forceinline__ PseudoTile pseudo_stage(float* cells, const float* __restrict__ sem_t, int ld_t, int H, int W, int h, int w,
                                                   int K, int tile_y, int tile_x, float scale_h, float scale_w) {
  PseudoTile t;
  t.b = blockIdx.z; t.ty0 = blockIdx.y * tile_y; t.tx0 = blockIdx.x * tile_x;
  t.scale_h = scale_h; t.scale_w = scale_w; t.KS = K | 1;
  int ny;
  tile_span(t.ty0, tile_y, H, h, scale_h, t.ya, ny);
  tile_span(t.tx0, tile_x, W, w, scale_w, t.xa, t.nx);
  const int n = ny * t.nx * K;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int cell = i / K, c = i - cell * K;
    const int cy = t.ya + cell / t.nx, cx = t.xa + cell % t.nx;
    cells[cell * t.KS + c] = sem_t[((size_t)(t.b * h + cy) * w + cx) * ld_t + c];
  }
  return t;
}

__device__ __forceinline__ TeacherView pseudo_view(const float* cells, const PseudoTile& t, int Y, int X, int h, int w, int K,
                                                  float log2K) {
  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
  up_src(Y, h, t.scale_h, y0, y1, ly0, ly1);
  up_src(X, w, t.scale_w, x0, x1, lx0, lx1);
  const float* r00 = cells + ((y0 - t.ya) * t.nx + (x0 - t.xa)) * t.KS;
  const float* r01 = cells + ((y0 - t.ya) * t.nx + (x1 - t.xa)) * t.KS;
  const float* r10 = cells + ((y1 - t.ya) * t.nx + (x0 - t.xa)) * t.KS;
  const float* r11 = cells + ((y1 - t.ya) * t.nx + (x1 - t.xa)) * t.KS;
  float best = -INFINITY;
  int arg = 0;
  for (int c = 0; c < K; ++c) {
    const float z = ly0 * (lx0 * r00[c] + lx1 * r01[c]) + ly1 * (lx0 * r10[c] + lx1 * r11[c]);
    if (z > best) { best = z; arg = c; }
  }
  if (K == 1) return {0, 0.f};
  // in base 2: H / ln 2 = log2 S - T / S with d_c = (z_c - m) log2 e, S = sum 2^d_c, T = sum d_c 2^d_c; u = that / log2 K.
  // K equal logits give S = K, T = 0 and u = 1 exactly
  float S = 0.f, T = 0.f;
  for (int c = 0; c < K; ++c) {
    const float z = ly0 * (lx0 * r00[c] + lx1 * r01[c]) + ly1 * (lx0 * r10[c] + lx1 * r11[c]);
    const float d = (z - best) * kL2e;
    const float e = __builtin_amdgcn_exp2f(d);
    S += e;
    T = __builtin_fmaf(d, e, T);
  }
  const float u = (__builtin_amdgcn_logf(S) - T / S) / log2K;
  return {arg, fminf(fmaxf(u, 0.f), 1.f)};
}

__device__ __forceinline__ bool pseudo_candidate(int64_t lab, int K, int ignore_index) {
  return lab >= 0 && lab < K && lab != ignore_index;
}

// hist: [K][bins] int64, accumulated.  lds_hist: K * bins words behind the cells
__global__ __launch_bounds__(kMaxThreads) void pseudo_hist_kernel(const float* __restrict__ sem_t, int ld_t,
                                                                 const int64_t* __restrict__ labels, int H, int W, int h, int w, int K,
                                                                 int ignore_index, int bins, int tile_y, int tile_x_log2, int ncell_max,
                                                                 float scale_h, float scale_w, int lds_hist,
                                                                 unsigned long long* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tile_x = 1 << tile_x_log2;
  unsigned int* l_hist = reinterpret_cast<unsigned int*>(smem + (size_t)ncell_max * (K | 1));
  const PseudoTile t = pseudo_stage(smem, sem_t, ld_t, H, W, h, w, K, tile_y, tile_x, scale_h, scale_w);
  if (lds_hist)
    for (int i = threadIdx.x; i < K * bins; i += blockDim.x) l_hist[i] = 0u;
  __syncthreads();
  const float log2K = __builtin_amdgcn_logf((float)K);
  for (int p = threadIdx.x; p < tile_y * tile_x; p += blockDim.x) {      // every lane of a wave takes the same number of turns
    const int Y = t.ty0 + (p >> tile_x_log2), X = t.tx0 + (p & (tile_x - 1));
    int key = -1;
    if (Y < H && X < W && pseudo_candidate(labels[((size_t)t.b * H + Y) * W + X], K, ignore_index)) {
      const TeacherView v = pseudo_view(smem, t, Y, X, h, w, K, log2K);
      const int bin = min((int)floorf(v.u * (float)bins), bins - 1);
      key = v.arg * bins + bin;
    }
    if (lds_hist) {
      if (key >= 0) atomicAdd(&l_hist[key], 1u);
    } else {
      // the lanes of a wave that hold one key add once: the first live lane names the key, a ballot counts its holders
      for (unsigned long long live = __ballot(key >= 0); live;) {
        const int k = __builtin_amdgcn_readlane(key, __builtin_ctzll(live));
        const unsigned long long same = __ballot(key == k);
        if ((threadIdx.x & 63) == __builtin_ctzll(live)) atomicAdd(&hist[k], (unsigned long long)__popcll(same));
        live &= ~same;
      }
    }
  }
  if (lds_hist) {
    __syncthreads();
    for (int i = threadIdx.x; i < K * bins; i += blockDim.x) {
      const unsigned int v = l_hist[i];
      if (v) atomicAdd(&hist[i], (unsigned long long)v);
    }
  }
}

// counts: [B][2] (passed, candidates), cleared by the call; uncertainty may be NULL
__global__ __launch_bounds__(kMaxThreads) void pseudo_label_kernel(const float* __restrict__ sem_t, int ld_t,
                                                                  const int64_t* __restrict__ labels, int H, int W, int h, int w, int K,
                                                                  int ignore_index, const float* __restrict__ thresholds, int tile_y,
                                                                  int tile_x_log2, int ncell_max, float scale_h, float scale_w,
                                                                  int64_t* __restrict__ labels_out, int* __restrict__ counts,
                                                                  float* __restrict__ uncertainty) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tile_x = 1 << tile_x_log2;
  int* s_cnt = reinterpret_cast<int*>(smem + (size_t)ncell_max * (K | 1));      // the workgroup's (passed, candidates)
  const PseudoTile t = pseudo_stage(smem, sem_t, ld_t, H, W, h, w, K, tile_y, tile_x, scale_h, scale_w);
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const float log2K = __builtin_amdgcn_logf((float)K);
  int num = 0, den = 0;
  for (int p = threadIdx.x; p < tile_y * tile_x; p += blockDim.x) {
    const int Y = t.ty0 + (p >> tile_x_log2), X = t.tx0 + (p & (tile_x - 1));
    if (Y >= H || X >= W) continue;
    const size_t pix = ((size_t)t.b * H + Y) * W + X;
    int64_t lab = labels[pix];
    float u = 0.f;
    if (pseudo_candidate(lab, K, ignore_index)) {
      const TeacherView v = pseudo_view(smem, t, Y, X, h, w, K, log2K);
      const bool pass = v.u < thresholds[v.arg];
      u = v.u;
      lab = pass ? v.arg : ignore_index;
      num += pass;
      den += 1;
    }
    labels_out[pix] = lab;
    if (uncertainty) uncertainty[pix] = u;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { num += __shfl_xor(num, off, 64); den += __shfl_xor(den, off, 64); }
  if ((threadIdx.x & 63) == 0 && den) { atomicAdd(&s_cnt[0], num); atomicAdd(&s_cnt[1], den); }
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt[1]) {
    if (s_cnt[0]) atomicAdd(&counts[2 * t.b + 0], s_cnt[0]);
    atomicAdd(&counts[2 * t.b + 1], s_cnt[1]);
  }
}

// f_b = max(num / (den + 1e-6), f_min), max(0, f_min) for an image without candidates; in fp64, rounded once
__global__ __launch_bounds__(kMaxThreads) void pseudo_factor_kernel(const int* __restrict__ counts, int B, float f_min,
                                                                   float* __restrict__ factor) {
  const int b = blockIdx.x * kMaxThreads + threadIdx.x;
  if (b >= B) return;
  const int num = counts[2 * b], den = counts[2 * b + 1];
  const double f = den ? (double)num / ((double)den + 1e-6) : 0.0;
  factor[b] = (float)fmax(f, (double)f_min);
}

}  // namespace
}  // namespace ucd

using namespace ucd;

namespace {

constexpr size_t kPseudoLds = 160 * 1024;

struct PseudoPlan { int tile_y, tile_x, tile_x_log2, grid_y, grid_x, threads, ncell, lds_hist; size_t lds; };

// The tile: 64 x 64 pixels, the larger side halved (y first) until the cells under it - the bound (tile_y h / H + 3) x (tile_x w / W
// + 3), rows of K | 1 floats - fit the LDS, down to 8 x 8 (one wave).  bins: 0 for the label pass
int pseudo_plan(const char* fn, int H, int W, int h, int w, int K, int bins, PseudoPlan* p) {
  UCD_REQUIRE(H > 0 && W > 0 && h > 0 && w > 0, UCD_EINVAL, "%s: bad sizes (H %d, W %d, h %d, w %d must be positive)", fn, H, W, h, w);
  UCD_REQUIRE(K >= 1, UCD_EINVAL, "%s: bad sizes (K = %d is below 1)", fn, K);
  UCD_REQUIRE(bins == 0 || (bins >= 2 && bins <= 1024), UCD_EINVAL, "%s: bins = %d is outside [2, 1024]", fn, bins);
  UCD_REQUIRE(H >= h && W >= w, UCD_EINVAL, "%s: bad scale (the label map H x W = %d x %d is smaller than the logits h x w = %d x %d)", fn,
              H, W, h, w);
  const size_t KS = (size_t)K | 1;
  int ty = 64, tx = 64;
  size_t ncell = 0, lds = 0;
  for (;;) {
    ncell = (size_t)((int)(ty * (float)h / H) + 3) * ((int)(tx * (float)w / W) + 3);
    lds = ncell * KS * sizeof(float);
    if (lds + 2 * sizeof(int) <= kPseudoLds || (ty == 8 && tx == 8)) break;
    if (ty >= tx) ty /= 2; else tx /= 2;
  }
  UCD_REQUIRE(lds + 2 * sizeof(int) <= kPseudoLds, UCD_EUNSUPPORTED,
              "%s: the cells under the smallest tile (8 x 8 pixels at factors %.4g x %.4g) take %zu bytes of LDS for K = %d classes, over "
              "the %zu there are", fn, (double)H / h, (double)W / w, lds, K, kPseudoLds);
  p->tile_y = ty; p->tile_x = tx;
  p->tile_x_log2 = __builtin_ctz(tx);
  p->grid_y = ceil_div(H, ty); p->grid_x = ceil_div(W, tx);
  UCD_REQUIRE(p->grid_y <= 65535, UCD_EUNSUPPORTED, "%s: H = %d gives %d tile rows, over the 65535 of a grid", fn, H, p->grid_y);
  p->threads = ty * tx < kMaxThreads ? ty * tx : kMaxThreads;
  p->ncell = (int)ncell;
  const size_t hist_bytes = (size_t)K * bins * sizeof(unsigned int);
  p->lds_hist = bins && lds + hist_bytes <= kPseudoLds;
  // behind the cells: the workgroup's histogram, or (label pass) its two counters
  p->lds = lds + (bins ? (p->lds_hist ? hist_bytes : 0) : 2 * sizeof(int));
  return 0;
}

// the argument rules the two passes share, under the name of the entry that was called
int pseudo_prologue(const char* fn, const float* sem_t, int ld_t, const int64_t* labels, int B, int H, int W, int h, int w, int K,
                    int bins, PseudoPlan* p) {
  UCD_REQUIRE(sem_t && labels, UCD_EINVAL, "%s: NULL argument (%s)", fn, !sem_t ? "sem_t" : "labels");
  UCD_REQUIRE(B > 0 && B <= 65535, UCD_EINVAL, "%s: bad sizes (B = %d is outside [1, 65535])", fn, B);
  const int rc = pseudo_plan(fn, H, W, h, w, K, bins, p);
  if (rc) return rc;
  UCD_REQUIRE(ld_t >= K, UCD_EINVAL, "%s: bad leading dimension (ld_t = %d below K = %d)", fn, ld_t, K);
  UCD_REQUIRE((long long)B * h * w <= 0x7fffffffLL, UCD_EINVAL, "%s: %lld low-resolution cells exceed an int", fn, (long long)B * h * w);
  return 0;
}

}  // namespace

extern "C" {

int ucd_pseudo_plan(int H, int W, int h, int w, int K, int bins, int* tile_y, int* tile_x, int* grid_y, int* grid_x, int* threads,
                    size_t* lds_bytes, int* lds_hist) {
  PseudoPlan p;
  const int rc = pseudo_plan("ucd_pseudo_plan", H, W, h, w, K, bins, &p);
  if (rc) return rc;
  if (tile_y) *tile_y = p.tile_y;
  if (tile_x) *tile_x = p.tile_x;
  if (grid_y) *grid_y = p.grid_y;
  if (grid_x) *grid_x = p.grid_x;
  if (threads) *threads = p.threads;
  if (lds_bytes) *lds_bytes = p.lds;
  if (lds_hist) *lds_hist = p.lds_hist;
  return 0;
}

int ucd_pseudo_hist(const float* sem_t, int ld_t, const int64_t* labels, int B, int H, int W, int h, int w, int K, int ignore_index,
                    int bins, int64_t* hist, ucd_stream_t stream) {
  static const char* fn = "ucd_pseudo_hist";
  PseudoPlan p;
  UCD_REQUIRE(hist, UCD_EINVAL, "%s: NULL argument (hist)", fn);
  UCD_REQUIRE(bins != 0, UCD_EINVAL, "%s: bins = 0 is outside [2, 1024]", fn);
  const int rc = pseudo_prologue(fn, sem_t, ld_t, labels, B, H, W, h, w, K, bins, &p);
  if (rc) return rc;
  UCD_TRY_LDS(pseudo_hist_kernel, (int)kPseudoLds);
  pseudo_hist_kernel<<<dim3(p.grid_x, p.grid_y, B), p.threads, p.lds, (hipStream_t)stream>>>(
      sem_t, ld_t, labels, H, W, h, w, K, ignore_index, bins, p.tile_y, p.tile_x_log2, p.ncell, (float)h / (float)H, (float)w / (float)W,
      p.lds_hist, (unsigned long long*)hist);
  return check_launch(fn);
}

int ucd_pseudo_label(const float* sem_t, int ld_t, const int64_t* labels, int B, int H, int W, int h, int w, int K, int ignore_index,
                     const float* thresholds, float f_min, int64_t* labels_out, int* counts, float* factor, float* uncertainty,
                     ucd_stream_t stream) {
  static const char* fn = "ucd_pseudo_label";
  PseudoPlan p;
  UCD_REQUIRE(thresholds && labels_out && counts && factor, UCD_EINVAL, "%s: NULL argument (%s)", fn,
              !thresholds ? "thresholds" : !labels_out ? "labels_out" : !counts ? "counts" : "factor");
  UCD_REQUIRE(labels_out != labels, UCD_EINVAL, "%s: labels_out may not alias labels", fn);
  UCD_REQUIRE(f_min >= 0.f && f_min <= 1.f, UCD_EINVAL, "%s: f_min = %g is outside [0, 1]", fn, (double)f_min);
  const int rc = pseudo_prologue(fn, sem_t, ld_t, labels, B, H, W, h, w, K, 0, &p);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  UCD_TRY_LDS(pseudo_label_kernel, (int)kPseudoLds);
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)B * 2 * sizeof(int), s);
  if (e != hipSuccess) { set_error("%s: %s", fn, hipGetErrorString(e)); return (int)e; }
  pseudo_label_kernel<<<dim3(p.grid_x, p.grid_y, B), p.threads, p.lds, s>>>(sem_t, ld_t, labels, H, W, h, w, K, ignore_index, thresholds,
                                                                          p.tile_y, p.tile_x_log2, p.ncell, (float)h / (float)H,
                                                                          (float)w / (float)W, labels_out, counts, uncertainty);
  int rc2 = check_launch(fn);
  if (rc2) return rc2;
  pseudo_factor_kernel<<<ceil_div(B, kMaxThreads), kMaxThreads, 0, s>>>(counts, B, f_min, factor);
  return check_launch(fn);
}

}  // extern "C"
