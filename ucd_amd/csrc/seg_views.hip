// Evaluation with test-time views: the image is run at several scales, optionally mirrored, and the per-view
// class distributions are fused into one prediction per full-resolution pixel.  The torch composition builds one fp32 [B, Ctot, H, W]
// soft-max per view (158 MB per image and view at ADE); here a view's full-resolution logit only ever exists in a register.
//
// Per pixel, l_v(c) is view v's logit up-sampled bilinearly (align_corners = False: up_src, and seg_confusion_kernel's expression in
// its order; a mirrored view is sampled at column W - 1 - X) and p_v = softmax_c(l_v), shifted by the view's own maximum, in fp32:
//   mean    score(c) = sum_v p_v(c)          max    score(c) = max_v p_v(c)          voting    score(c) = #{v : argmax l_v = c}
// and the prediction is the smallest c with the largest score.  No per-class accumulators (Ctot reaches 151): one walk over the
// classes per view leaves (max_v, 1 / Z_v) - two registers per view - from a running maximum and a rescaled sum; a second walk forms
// the score of each class across the views and keeps the running arg-max.  Voting needs the first walk only, with the arg-max kept
// per view.  A block owns a pixel tile and stages the cells of all V views under it in LDS; neighbouring pixels read the same cells,
// so most reads are broadcasts.  (label, prediction) pairs are counted as integers (LDS histogram for n <= 64, global atomics above):
// the same bits on every run.  ucd_seg_views_plan is the one copy of the sizing arithmetic, on the host, without a device call.
#include "common.h"
#include "upsample_index.h"

namespace ucd {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxViews = 16;
constexpr size_t kLdsBudget = 150 * 1024;        // ucd_seg_confusion's
constexpr int kTabFloats = 4 * (kMaxViews + 1);  // per view (first cell row, first cell column, cells per row, offset of its cells); entry V: the end
// pixel tiles, largest first: seg_losses_wide_kernel's 32 x 64, halved in turn
constexpr int kTiles[][2] = {{32, 64}, {32, 32}, {16, 32}, {16, 16}, {8, 16}, {8, 8}};
constexpr int kNumTiles = sizeof(kTiles) / sizeof(kTiles[0]);

// the view table, by value in the kernel's arguments (640 bytes): nothing is uploaded
struct ViewTab {
  const float* sem[kMaxViews];
  int ld[kMaxViews], h[kMaxViews], w[kMaxViews], flip[kMaxViews];
  float scale_h[kMaxViews], scale_w[kMaxViews];    // torch's float(in) / out
};

// the cell columns under the pixel columns [t0, min(t0 + tile, W)) of a view: a mirrored view is sampled at W - 1 - X, so its span is
// taken over the mirrored range.  Host (the plan) and device (the kernel's staging): one copy
__host__ __device__ __forceinline__ void view_span_x(int t0, int tile, int W, int w, float scale, int flip, int& first, int& count) {
  const int end = t0 + tile < W ? t0 + tile : W;
  if (flip) tile_span(W - end, end - t0, W, w, scale, first, count);
  else tile_span(t0, tile, W, w, scale, first, count);
}

// a view's up-sampled logit walk for one pixel: where its four corners lie in LDS and with which weights (four registers per view)
struct Corner {
  int o00; unsigned d;        // LDS index of corner (y0, x0), class 0; distance to the x1 corner | distance to the y1 corner << 16
  float lx1, ly1;             // up_src's weights of the x1 / y1 corners; those of x0 / y0 are 1 - l1, as up_src forms them
};
__device__ __forceinline__ Corner view_corner(const ViewTab& t, int v, const int4 e, int Y, int X, int W, int Ctot) {
  Corner k;
  int y0, y1, x0, x1;
  float lx0, ly0;
  up_src(Y, t.h[v], t.scale_h[v], y0, y1, ly0, k.ly1);
  up_src(t.flip[v] ? W - 1 - X : X, t.w[v], t.scale_w[v], x0, x1, lx0, k.lx1);
  k.o00 = e.w + ((y0 - e.x) * e.z + (x0 - e.y)) * Ctot;
  k.d = (unsigned)((x1 - x0) * Ctot) | ((unsigned)((y1 - y0) * e.z * Ctot) << 16);     // both below 2^16: the LDS holds 150 KB of floats
  return k;
}
// seg_confusion_kernel's expression, written again (-ffp-contract=off: equal expressions, equal bits)
__device__ __forceinline__ float corner_logit(const float* __restrict__ s, const Corner& k, int c) {
  const float* p = s + k.o00 + c;
  const int dx = (int)(k.d & 0xffffu), dy = (int)(k.d >> 16);
  const float lx0 = 1.f - k.lx1, ly0 = 1.f - k.ly1;
  return ly0 * (lx0 * p[0] + k.lx1 * p[dx]) + k.ly1 * (lx0 * p[dy] + k.lx1 * p[dy + dx]);
}

// MODE 0: mean, 1: max, 2: voting
template <int MODE>
__global__ __launch_bounds__(kThreads) void seg_views_kernel(const ViewTab t, int V, const int64_t* __restrict__ labels, int H, int W,
                                                             int Ctot, int n_classes, int tile_y, int tile_x,
                                                             unsigned long long* __restrict__ hist, int use_lds_hist,
                                                             int64_t* __restrict__ pred) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr float kL2e = 1.4426950408889634f;
  int4* s_tab = reinterpret_cast<int4*>(smem);       // [kMaxViews + 1] (ya, xa, nx, offset)
  float* s_log = smem + kTabFloats;                  // view after view: [ncell_v][Ctot]
  const int b = blockIdx.z, ty0 = blockIdx.y * tile_y, tx0 = blockIdx.x * tile_x;
  if (threadIdx.x == 0) {
    int off = 0;
    for (int v = 0; v < V; ++v) {
      int ya, ny, xa, nx;
      tile_span(ty0, tile_y, H, t.h[v], t.scale_h[v], ya, ny);
      view_span_x(tx0, tile_x, W, t.w[v], t.scale_w[v], t.flip[v], xa, nx);
      s_tab[v] = make_int4(ya, xa, nx, off);
      off += ny * nx * Ctot;
    }
    s_tab[V] = make_int4(0, 0, 0, off);
  }
  __syncthreads();
  for (int v = 0; v < V; ++v) {
    const int4 e = s_tab[v];
    const int n = s_tab[v + 1].w - e.w;
    const float* __restrict__ src = t.sem[v];
    const int h = t.h[v], w = t.w[v], ld = t.ld[v];
    for (int i = threadIdx.x; i < n; i += kThreads) {
      const int cell = i / Ctot, c = i - cell * Ctot;
      const int cy = e.x + cell / e.z, cx = e.y + cell % e.z;
      s_log[e.w + i] = src[((size_t)(b * h + cy) * w + cx) * ld + c];
    }
  }
  unsigned int* l_hist = reinterpret_cast<unsigned int*>(s_log + s_tab[V].w);      // [n][n] when use_lds_hist
  if (use_lds_hist)
    for (int i = threadIdx.x; i < n_classes * n_classes; i += kThreads) l_hist[i] = 0u;
  __syncthreads();

  for (int p = threadIdx.x; p < tile_y * tile_x; p += kThreads) {
    const int py = p / tile_x;
    const int Y = ty0 + py, X = tx0 + (p - py * tile_x);
    if (Y >= H || X >= W) continue;
    int arg = 0;
    if (MODE == 2) {
      // one walk per view: its arg-max (first maximum); then the class most views name, the smallest on a tie
      int av[kMaxViews];
#pragma unroll
      for (int v = 0; v < kMaxViews; ++v) {
        av[v] = -1;
        if (v < V) {
          const Corner k = view_corner(t, v, s_tab[v], Y, X, W, Ctot);
          float best = -INFINITY;
          int a = 0;
          for (int c = 0; c < Ctot; ++c) {
            const float z = corner_logit(s_log, k, c);
            if (z > best) { best = z; a = c; }
          }
          av[v] = a;
        }
      }
      int top = 0;
      arg = 0x7fffffff;
#pragma unroll
      for (int v = 0; v < kMaxViews; ++v)
        if (v < V) {
          int cnt = 0;
#pragma unroll
          for (int u = 0; u < kMaxViews; ++u) cnt += av[u] == av[v] ? 1 : 0;
          if (cnt > top || (cnt == top && av[v] < arg)) { top = cnt; arg = av[v]; }
        }
    } else {
      // first walk: the view's maximum and 1 / Z around it, one exponential per class (running maximum, rescaled sum)
      float mv[kMaxViews], iz[kMaxViews];
      Corner kc[kMaxViews];
#pragma unroll
      for (int v = 0; v < kMaxViews; ++v) {
        mv[v] = 0.f; iz[v] = 0.f; kc[v] = Corner{0, 0u, 0.f, 0.f};
        if (v < V) {
          const Corner k = kc[v] = view_corner(t, v, s_tab[v], Y, X, W, Ctot);
          float m = corner_logit(s_log, k, 0), s = 1.f;
          for (int c = 1; c < Ctot; ++c) {
            const float z = corner_logit(s_log, k, c);
            const float d = z - m;
            const float ex = __builtin_amdgcn_exp2f(-fabsf(d) * kL2e);
            s = d > 0.f ? s * ex + 1.f : s + ex;
            m = fmaxf(m, z);
          }
          mv[v] = m; iz[v] = 1.f / s;
        }
      }
      // second walk: the score of a class across the views, the first maximum wins
      float best = -INFINITY;
      for (int c = 0; c < Ctot; ++c) {
        float score = 0.f;
#pragma unroll
        for (int v = 0; v < kMaxViews; ++v)
          if (v < V) {
            const float pr = __builtin_amdgcn_exp2f((corner_logit(s_log, kc[v], c) - mv[v]) * kL2e) * iz[v];
            score = MODE == 0 ? score + pr : fmaxf(score, pr);
          }
        if (score > best) { best = score; arg = c; }
      }
    }
    const size_t pix = ((size_t)b * H + Y) * W + X;
    if (pred) pred[pix] = arg;
    const int64_t lab = labels[pix];
    if (lab >= 0 && lab < n_classes && arg < n_classes) {
      if (use_lds_hist) atomicAdd(&l_hist[(int)lab * n_classes + arg], 1u);
      else atomicAdd(&hist[(size_t)lab * n_classes + arg], 1ull);
    }
  }
  if (use_lds_hist) {
    __syncthreads();
    for (int i = threadIdx.x; i < n_classes * n_classes; i += kThreads) {
      const unsigned int v = l_hist[i];
      if (v) atomicAdd(&hist[i], (unsigned long long)v);
    }
  }
}

// the LDS bytes of one tile size: per view the largest footprint any tile of the grid has (the kernel's own tile_span, tile by tile)
size_t views_lds_bytes(int tile_y, int tile_x, int H, int W, int V, const int* h, const int* w, const int* flip, int Ctot, int n_classes) {
  size_t cells = 0;
  for (int v = 0; v < V; ++v) {
    const float sh = (float)h[v] / (float)H, sw = (float)w[v] / (float)W;
    int my = 1, mx = 1, first, count;
    for (int t0 = 0; t0 < H; t0 += tile_y) {
      tile_span(t0, tile_y, H, h[v], sh, first, count);
      if (count > my) my = count;
    }
    for (int t0 = 0; t0 < W; t0 += tile_x) {
      view_span_x(t0, tile_x, W, w[v], sw, flip[v] != 0, first, count);
      if (count > mx) mx = count;
    }
    cells += (size_t)my * mx;
  }
  return (cells * Ctot + kTabFloats) * sizeof(float) + (n_classes <= 64 ? (size_t)n_classes * n_classes * 4 : 0);
}

}  // namespace
}  // namespace ucd

using namespace ucd;

extern "C" {

int ucd_seg_views_plan(int H, int W, int V, const int* h, const int* w, const int* flip, int Ctot, int n_classes, int* tile_y,
                       int* tile_x, size_t* lds_bytes) {
  static const char* fn = "ucd_seg_views";
  UCD_REQUIRE(V >= 1 && V <= kMaxViews, UCD_EINVAL, "%s: V = %d views (1 .. %d are served)", fn, V, kMaxViews);
  UCD_REQUIRE(h && w && flip, UCD_EINVAL, "%s: NULL argument (h, w, flip)", fn);
  UCD_REQUIRE(H > 0 && W > 0 && Ctot > 0 && n_classes > 0, UCD_EINVAL,
              "%s: bad sizes (H = %d, W = %d, Ctot = %d, n_classes = %d: each must be at least 1)", fn, H, W, Ctot, n_classes);
  UCD_REQUIRE(Ctot <= 255, UCD_EINVAL, "%s: Ctot = %d classes (at most 255)", fn, Ctot);
  for (int v = 0; v < V; ++v) {
    UCD_REQUIRE(h[v] > 0 && w[v] > 0, UCD_EINVAL, "%s: bad sizes (view %d is %d x %d)", fn, v, h[v], w[v]);
    UCD_REQUIRE(H >= h[v] && W >= w[v], UCD_EINVAL, "%s: bad scale (the label map %d x %d is smaller than view %d's logits %d x %d)", fn,
                H, W, v, h[v], w[v]);
  }
  size_t lds = 0;
  for (int i = 0; i < kNumTiles; ++i) {
    lds = views_lds_bytes(kTiles[i][0], kTiles[i][1], H, W, V, h, w, flip, Ctot, n_classes);
    if (lds <= kLdsBudget) {
      if (tile_y) *tile_y = kTiles[i][0];
      if (tile_x) *tile_x = kTiles[i][1];
      if (lds_bytes) *lds_bytes = lds;
      return 0;
    }
  }
  set_error("%s: the cells of %d views under the smallest pixel tile (%d x %d) take %zu bytes of LDS for %d classes, over the budget "
              "of %zu - no tile serves these views", fn, V, kTiles[kNumTiles - 1][0], kTiles[kNumTiles - 1][1], lds, Ctot, kLdsBudget);
  return UCD_EUNSUPPORTED;
}

int ucd_seg_views(const float* const* sem, const int* ld, const int* h, const int* w, const int* flip, int V, const int64_t* labels,
                  int B, int H, int W, int Ctot, int n_classes, int mode, int64_t* hist, int64_t* pred, ucd_stream_t stream) {
  static const char* fn = "ucd_seg_views";
  UCD_REQUIRE(sem && ld && labels && hist, UCD_EINVAL, "%s: NULL argument", fn);
  UCD_REQUIRE(B > 0, UCD_EINVAL, "%s: bad sizes (B = %d)", fn, B);
  UCD_REQUIRE(mode >= 0 && mode <= 2, UCD_EINVAL, "%s: unknown mode %d (0 mean, 1 max, 2 voting)", fn, mode);
  int tile_y = 0, tile_x = 0;
  size_t lds = 0;
  int rc = ucd_seg_views_plan(H, W, V, h, w, flip, Ctot, n_classes, &tile_y, &tile_x, &lds);
  if (rc) return rc;
  ViewTab t = {};
  for (int v = 0; v < V; ++v) {
    UCD_REQUIRE(sem[v], UCD_EINVAL, "%s: NULL argument (sem[%d])", fn, v);
    UCD_REQUIRE(ld[v] >= Ctot, UCD_EINVAL, "%s: ld[%d] = %d is below Ctot = %d", fn, v, ld[v], Ctot);
    UCD_REQUIRE((long long)B * h[v] * w[v] <= 0x7FFFFFFF, UCD_EINVAL, "%s: view %d has more rows than the kernel indexes", fn, v);
    t.sem[v] = sem[v]; t.ld[v] = ld[v]; t.h[v] = h[v]; t.w[v] = w[v]; t.flip[v] = flip[v] != 0;
    t.scale_h[v] = (float)h[v] / (float)H; t.scale_w[v] = (float)w[v] / (float)W;
  }
  const dim3 grid(ceil_div(W, tile_x), ceil_div(H, tile_y), B);
  const int use_lds_hist = n_classes <= 64;
  hipStream_t s = (hipStream_t)stream;
#define UCD_VIEWS_LAUNCH(MODE)                                                                                                      \
  do {                                                                                                                              \
    UCD_TRY_LDS(seg_views_kernel<MODE>, (int)kLdsBudget);                                                                           \
    seg_views_kernel<MODE><<<grid, kThreads, lds, s>>>(t, V, labels, H, W, Ctot, n_classes, tile_y, tile_x, (unsigned long long*)hist, \
                                                       use_lds_hist, pred);                                                         \
  } while (0)
  if (mode == 0) UCD_VIEWS_LAUNCH(0);
  else if (mode == 1) UCD_VIEWS_LAUNCH(1);
  else UCD_VIEWS_LAUNCH(2);
#undef UCD_VIEWS_LAUNCH
  return check_launch(fn);
}

}  // extern "C"
