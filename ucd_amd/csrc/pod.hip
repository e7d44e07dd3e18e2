// Local POD feature distillation (PLOP's `_local_pod`, extended to non-square maps) for one level: a student and a teacher
// map [B, h, w, C] (channels-last rows, bf16 or fp32, row pitch >= C), a slope a in (0, 1] and scales s_1 < ... < s_n.
//   P = X >= 0 ? X : X / a,  Q = P^2                       (the map in front of the block's leaky-ReLU, squared)
//   scale s: kh = h / s, kw = w / s; region (i, j) = rows [i kh, (i+1) kh) x columns [j kw, (j+1) kw)
//     row pool  E[s][r][j][c] = mean over the region's columns of Q[r][x][c]      (r < s kh)
//     col pool  E[s][x][i][c] = mean over the region's rows    of Q[r][x][c]      (x < s kw)
//   E^ = E / max(|E|, 1e-12),  l_b = |E^_s - E^_t|,  level = mean_b l_b,
//   g_E = weight / B * (u - E^_s (E^_s . u)) / max(|E_s|, 1e-12),  u = (E^_s - E^_t) / l_b  (0 where l_b = 0)
//   dX = 2 P dQ (X >= 0 ? 1 : 1 / a),  dQ[r][x][c] = sum over the scales that cover (r, x) of g_row[r][j(x)][c] / kw + g_col[x][i(r)][c] / kh
//
// Tiling.  Rows are cut at every region boundary of every scale and then into pieces of at most kPodRows rows, columns likewise
// into pieces of at most kPodCols columns: inside a tile (row piece x column piece) the region indices i(r), j(x) and the "covered"
// predicate of EVERY scale are constants, so one pair of scale-free partial sums per tile serves all scales.  The tile pass gives a
// thread one tile and one 16-byte channel vector (lanes run over channels: every load is 16 bytes per lane, contiguous over the
// wave); it reads each element of the map once and writes the tile's row sums (one per row) and column sums (one per column).
// Three small launches per level then work on strips only: pool (partials -> E, |E|^2 partials), diff (l_b^2 and E^_s . (E^_s - E^_t)
// partials) and coef (g_E, pre-divided by kw / kh, and the level value).  The backward pass walks the same tiles: it adds the
// coefficient strips of the covering scales once per tile row / tile column, reads the student map once and writes dX once.
//
// Every sum has a fixed order (a thread over its elements, a wave by shuffles, a block over its waves, per-block partials in index
// order); the strip sums are fp32, the norms and dot products fp64.  No atomics: same inputs, same bits.
//
// The level on the logits (PLOP's last one: Ctot student against K teacher channels, fp32 rows of any pitch) has a tile pass and a
// backward pass of its own further down and shares the geometry and the three strip kernels.
#include "common.h"

namespace ucd {
namespace {

constexpr int kPodBlock = 256;
constexpr int kPodRows = 8, kPodCols = 16;                 // largest tile
constexpr int kPodMaxScales = 4, kPodMaxScale = 8, kPodMaxDim = 1024;
constexpr int kPodMaxCuts = kPodMaxDim / kPodRows + 40;    // pieces per direction: <= dim / piece + region boundaries (<= 26) + 1
constexpr int kPodChunkElems = kPodBlock * 8;              // strip elements per block of the strip kernels (before the cap)
constexpr int kPodMaxChunks = 256;

struct PodGeom {
  int h, w, C, n, n_E, nrs, ncs;
  int s[kPodMaxScales], kh[kPodMaxScales], kw[kPodMaxScales];
  int rowoff[kPodMaxScales], coloff[kPodMaxScales];        // element offsets of a scale's row / column pools inside a sample's strips
  short rcut[kPodMaxCuts + 1], ccut[kPodMaxCuts + 1];      // piece p covers [cut[p], cut[p + 1])
  short rfirst[kPodMaxScales][kPodMaxScale + 1];           // first row piece of region i (entry s: the piece behind the last region)
  short cfirst[kPodMaxScales][kPodMaxScale + 1];
};

int pod_cut(int dim, int piece, const int* s, const int* k, int n, short* cut, short (*first)[kPodMaxScale + 1]) {
  bool edge[kPodMaxDim + 1] = {};
  edge[0] = edge[dim] = true;
  for (int q = 0; q < n; ++q)
    for (int i = 0; i <= s[q]; ++i) edge[i * k[q]] = true;
  int np = 0, pos = 0;
  cut[0] = 0;
  while (pos < dim) {
    int next = pos + 1;
    while (!edge[next] && next - pos < piece) ++next;
    cut[++np] = (short)next;
    pos = next;
  }
  for (int q = 0; q < n; ++q)
    for (int i = 0; i <= s[q]; ++i) {
      int p = 0;
      while (p < np && cut[p] != i * k[q]) ++p;             // i k is an edge, so a piece starts there (or it is the end: np)
      first[q][i] = (short)p;
    }
  return np;
}

// Validates the geometry and fills g.  Pure host code.  cmult, cmax: the channel counts the caller's tile and backward kernels
// take (the strip kernels take any)
int pod_geom(const char* fn, int h, int w, int C, const int* scales, int n, PodGeom* g, int cmult = 8, int cmax = 8192) {
  UCD_REQUIRE(scales, UCD_EINVAL, "%s: NULL scales", fn);
  UCD_REQUIRE(n >= 1 && n <= kPodMaxScales, UCD_EINVAL, "%s: %d scales (1 to %d are taken)", fn, n, kPodMaxScales);
  for (int q = 0; q < n; ++q) {
    UCD_REQUIRE(scales[q] >= 1 && scales[q] <= kPodMaxScale, UCD_EINVAL, "%s: scale %d is outside 1 .. %d", fn, scales[q], kPodMaxScale);
    UCD_REQUIRE(q == 0 || scales[q] > scales[q - 1], UCD_EINVAL, "%s: the scales must increase strictly (%d follows %d)", fn, scales[q],
                scales[q - 1]);
  }
  UCD_REQUIRE(C >= 1, UCD_EINVAL, "%s: C = %d must be at least 1", fn, C);
  UCD_REQUIRE(h >= scales[n - 1] && w >= scales[n - 1], UCD_EINVAL, "%s: a %d x %d map is smaller than the largest scale %d", fn, h, w,
              scales[n - 1]);
  UCD_REQUIRE(C % cmult == 0, UCD_EUNSUPPORTED, "%s: C = %d is not a multiple of %d (a lane moves 16 bytes of channels)", fn, C, cmult);
  UCD_REQUIRE(C <= cmax, UCD_EUNSUPPORTED, "%s: C = %d is above %d", fn, C, cmax);
  UCD_REQUIRE(h <= kPodMaxDim && w <= kPodMaxDim, UCD_EUNSUPPORTED, "%s: a %d x %d map is above %d rows or columns", fn, h, w, kPodMaxDim);
  memset(g, 0, sizeof(*g));
  g->h = h, g->w = w, g->C = C, g->n = n;
  int off = 0;
  for (int q = 0; q < n; ++q) {
    const int s = scales[q];
    g->s[q] = s, g->kh[q] = h / s, g->kw[q] = w / s;
    g->rowoff[q] = off;
    off += s * g->kh[q] * s * C;
    g->coloff[q] = off;
    off += s * g->kw[q] * s * C;
  }
  g->n_E = off;
  g->nrs = pod_cut(h, kPodRows, g->s, g->kh, n, g->rcut, g->rfirst);
  g->ncs = pod_cut(w, kPodCols, g->s, g->kw, n, g->ccut, g->cfirst);
  return UCD_OK;
}

// Workgroups per sample of the strip kernels.  lanes: the threads that take one unit (C channels of a pool entry) in the pool and
// coef kernels - the whole workgroup for the feature maps; for the few channels of the logits the power of two that holds them,
// and then enough workgroups that each takes its kPodBlock / lanes units in one trip
inline int pod_chunks(const PodGeom& g, int lanes = kPodBlock) {
  int c = ceil_div(g.n_E, kPodChunkElems);
  if (lanes < kPodBlock) {
    const int u = ceil_div(g.n_E / g.C, kPodBlock / lanes);
    c = u > c ? u : c;
  }
  return c < kPodMaxChunks ? c : kPodMaxChunks;
}
inline int pod_logits_lanes(int K) {
  int lanes = kPodBlock;
  while (lanes / 2 >= K) lanes /= 2;
  return lanes;
}

// workspace: rowseg [2][B][h][ncs][C], colseg [2][B][nrs][w][C], E [2][B][n_E] floats; partN, partD [2][B][chunks] doubles
struct PodWs {
  size_t rowseg, colseg, E, partN, partD, bytes;
};
PodWs pod_ws(const PodGeom& g, int B, int lanes = kPodBlock) {
  PodWs o;
  size_t off = 0;
  o.rowseg = off, off += align_up((size_t)2 * B * g.h * g.ncs * g.C * sizeof(float), 16);
  o.colseg = off, off += align_up((size_t)2 * B * g.nrs * g.w * g.C * sizeof(float), 16);
  o.E = off, off += align_up((size_t)2 * B * g.n_E * sizeof(float), 16);
  o.partN = off, off += (size_t)2 * B * pod_chunks(g, lanes) * sizeof(double);
  o.partD = off, off += (size_t)2 * B * pod_chunks(g, lanes) * sizeof(double);
  o.bytes = off;
  return o;
}

inline long long pod_tile_items(const PodGeom& g, int B, int vec) { return (long long)B * g.nrs * g.ncs * (g.C / vec); }

// ---- device side -------------------------------------------------------------------------------------------------------------
// The geometry arrives by value; a block copies it to LDS once, so that the per-lane table reads are LDS reads
__device__ __forceinline__ void pod_stage(PodGeom* sg, const PodGeom& g) {
  static_assert(sizeof(PodGeom) % sizeof(int) == 0 && sizeof(PodGeom) / sizeof(int) <= kPodBlock, "one dword per thread");
  const int* src = reinterpret_cast<const int*>(&g);
  if (threadIdx.x < sizeof(PodGeom) / sizeof(int)) reinterpret_cast<int*>(sg)[threadIdx.x] = src[threadIdx.x];
  __syncthreads();
}

__device__ __forceinline__ void pod_store(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void pod_store(float* p, const float (&v)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
template <int N>
__device__ __forceinline__ void pod_add(float (&acc)[N], const float* p) {
#pragma unroll
  for (int q = 0; q < N; q += 4) {
    const float4 v = *reinterpret_cast<const float4*>(p + q);
    acc[q] += v.x, acc[q + 1] += v.y, acc[q + 2] += v.z, acc[q + 3] += v.w;
  }
}

struct PodTile {
  int b, r0, nr, x0, x1, rs, cs, c;
  bool live;
};
template <int VEC>
__device__ __forceinline__ PodTile pod_tile(const PodGeom& g, int B) {
  PodTile t;
  const int CV = g.C / VEC;
  long long item = (long long)blockIdx.x * kPodBlock + threadIdx.x;
  t.live = item < (long long)B * g.nrs * g.ncs * CV;
  if (!t.live) item = 0;
  t.c = (int)(item % CV) * VEC;
  item /= CV;
  t.cs = (int)(item % g.ncs);
  item /= g.ncs;
  t.rs = (int)(item % g.nrs);
  t.b = (int)(item / g.nrs);
  t.r0 = g.rcut[t.rs], t.nr = g.rcut[t.rs + 1] - t.r0;
  t.x0 = g.ccut[t.cs], t.x1 = g.ccut[t.cs + 1];
  return t;
}

// The tile pass: blockIdx.y = 0 the student map, 1 the teacher map
template <typename T>
__global__ __launch_bounds__(kPodBlock) void pod_tile_kernel(const T* __restrict__ x_s, int ld_s, const T* __restrict__ x_t, int ld_t,
                                                            float inv_a, int B, const PodGeom geom, float* __restrict__ rowseg,
                                                            float* __restrict__ colseg) {
  constexpr int VEC = Vec<T>::N;
  __shared__ PodGeom g;
  pod_stage(&g, geom);
  const PodTile t = pod_tile<VEC>(g, B);
  if (!t.live) return;
  const int net = blockIdx.y;
  const T* x = net ? x_t : x_s;
  const size_t ld = net ? ld_t : ld_s;
  const T* base = x + ((size_t)t.b * g.h + t.r0) * g.w * ld + t.c;
  const size_t nb = (size_t)net * B + t.b;
  float* crow = colseg + ((nb * g.nrs + t.rs) * g.w) * g.C + t.c;
  float racc[kPodRows][VEC];
#pragma unroll
  for (int rr = 0; rr < kPodRows; ++rr)
#pragma unroll
    for (int q = 0; q < VEC; ++q) racc[rr][q] = 0.f;
  for (int xx = t.x0; xx < t.x1; ++xx) {
    Vec<T> v[kPodRows];
#pragma unroll
    for (int rr = 0; rr < kPodRows; ++rr)
      if (rr < t.nr) v[rr].load(base + ((size_t)rr * g.w + xx) * ld);
    float csum[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) csum[q] = 0.f;
#pragma unroll
    for (int rr = 0; rr < kPodRows; ++rr)
      if (rr < t.nr) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
          const float e = v[rr].get(q);
          const float p = e >= 0.f ? e : e * inv_a;
          const float sq = p * p;
          racc[rr][q] += sq;
          csum[q] += sq;
        }
      }
    pod_store(crow + (size_t)xx * g.C, csum);
  }
#pragma unroll
  for (int rr = 0; rr < kPodRows; ++rr)
    if (rr < t.nr) pod_store(rowseg + ((nb * g.h + t.r0 + rr) * g.ncs + t.cs) * g.C + t.c, racc[rr]);
}

// One strip entry: which scale, which pool, and its two coordinates
struct PodUnit {
  int k, col, a, b;       // col = 0: row pool of row a, column region b; col = 1: column pool of column a, row region b
};
__device__ __forceinline__ PodUnit pod_unit(const PodGeom& g, int u) {
  PodUnit o = {0, 0, 0, 0};
  for (int k = 0; k < g.n; ++k) {
    const int ro = g.rowoff[k] / g.C, co = g.coloff[k] / g.C, s = g.s[k];
    if (u < co) {
      o.k = k, o.col = 0, o.a = (u - ro) / s, o.b = (u - ro) % s;
      return o;
    }
    if (u < co + s * g.kw[k] * s) {
      o.k = k, o.col = 1, o.a = (u - co) / s, o.b = (u - co) % s;
      return o;
    }
  }
  return o;
}

__device__ __forceinline__ double pod_block_sum(double v, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
// sum of part[0 .. chunks) (chunks <= kPodBlock) in a fixed order, on every thread
__device__ __forceinline__ double pod_partial_sum(const double* part, int chunks, double* red) {
  return pod_block_sum((int)threadIdx.x < chunks ? part[threadIdx.x] : 0.0, red);
}

// pool: tile partials -> E (one division per entry), per-block partials of |E|^2.  grid (chunks, B, 2)
__global__ __launch_bounds__(kPodBlock) void pod_pool_kernel(const PodGeom geom, int B, int lanes, const float* __restrict__ rowseg,
                                                            const float* __restrict__ colseg, float* __restrict__ E,
                                                            double* __restrict__ partN) {
  __shared__ PodGeom g;
  __shared__ double red[4];
  pod_stage(&g, geom);
  const int b = blockIdx.y, net = blockIdx.z, chunks = gridDim.x;
  const size_t nb = (size_t)net * B + b;
  double acc = 0.0;
  // a workgroup takes whole units (the C channels of one pool entry): the decode is uniform, the lanes run over channels.  With few
  // channels (the logits) `lanes` threads take a unit and the workgroup kPodBlock / lanes units at a time
  const int nsub = kPodBlock / lanes, lane = threadIdx.x % lanes;
  for (int un = blockIdx.x * nsub + threadIdx.x / lanes; un < g.n_E / g.C; un += chunks * nsub) {
    const PodUnit u = pod_unit(g, un);
    const float* p;
    size_t pitch;
    int q0, q1;
    float count;
    if (!u.col) {
      p = rowseg + (nb * g.h + u.a) * g.ncs * g.C, pitch = g.C;
      q0 = g.cfirst[u.k][u.b], q1 = g.cfirst[u.k][u.b + 1], count = (float)g.kw[u.k];
    } else {
      p = colseg + (nb * g.nrs * g.w + u.a) * g.C, pitch = (size_t)g.w * g.C;
      q0 = g.rfirst[u.k][u.b], q1 = g.rfirst[u.k][u.b + 1], count = (float)g.kh[u.k];
    }
    for (int c = lane; c < g.C; c += lanes) {
      float sum = 0.f;
      for (int q = q0; q < q1; ++q) sum += p[q * pitch + c];
      const float val = sum / count;
      E[nb * g.n_E + (size_t)un * g.C + c] = val;
      acc += (double)val * val;
    }
  }
  acc = pod_block_sum(acc, red);
  if (threadIdx.x == 0) partN[nb * chunks + blockIdx.x] = acc;
}

__device__ __forceinline__ float pod_inv_norm(double sumsq) { return (float)(1.0 / fmax(sqrt(sumsq), 1e-12)); }

// diff: per-block partials of |E^_s - E^_t|^2 and E^_s . (E^_s - E^_t).  grid (chunks, B).  normalize = 0 (the level on the logits
// only): E^ = E, the norms are not read
__global__ __launch_bounds__(kPodBlock) void pod_diff_kernel(int n_E, int B, int normalize, const float* __restrict__ E,
                                                            const double* __restrict__ partN, double* __restrict__ partD) {
  __shared__ double red[4];
  const int b = blockIdx.y, chunks = gridDim.x;
  const float inv_s = normalize ? pod_inv_norm(pod_partial_sum(partN + (size_t)b * chunks, chunks, red)) : 1.f;
  const float inv_t = normalize ? pod_inv_norm(pod_partial_sum(partN + ((size_t)B + b) * chunks, chunks, red)) : 1.f;
  const float* Es = E + (size_t)b * n_E;
  const float* Et = E + ((size_t)B + b) * n_E;
  double a1 = 0.0, a2 = 0.0;
  for (int e = blockIdx.x * kPodBlock + threadIdx.x; e < n_E; e += chunks * kPodBlock) {
    const float es = Es[e] * inv_s, et = Et[e] * inv_t, d = es - et;
    a1 += (double)d * d;
    a2 += (double)es * d;
  }
  a1 = pod_block_sum(a1, red);
  a2 = pod_block_sum(a2, red);
  if (threadIdx.x == 0) {
    partD[(size_t)b * chunks + blockIdx.x] = a1;
    partD[((size_t)B + b) * chunks + blockIdx.x] = a2;
  }
}

// coef: g_E (already divided by the pool's count) and, by block (0, 0), the level value.  grid (chunks, B).  normalize = 0:
// g_E = weight / B * (E_s - E_t) / l_b - the projection term and the division by |E_s| drop out
__global__ __launch_bounds__(kPodBlock) void pod_coef_kernel(const PodGeom geom, int B, int normalize, int lanes, float weight,
                                                            const float* __restrict__ E, const double* __restrict__ partN,
                                                            const double* __restrict__ partD, float* __restrict__ gE,
                                                            float* __restrict__ loss_out) {
  __shared__ PodGeom g;
  __shared__ double red[4];
  pod_stage(&g, geom);
  const int b = blockIdx.y, chunks = gridDim.x;
  const double nn_s = normalize ? pod_partial_sum(partN + (size_t)b * chunks, chunks, red) : 1.0;
  const float inv_s = normalize ? pod_inv_norm(nn_s) : 1.f;
  const float inv_t = normalize ? pod_inv_norm(pod_partial_sum(partN + ((size_t)B + b) * chunks, chunks, red)) : 1.f;
  const double l = sqrt(pod_partial_sum(partD + (size_t)b * chunks, chunks, red));
  const double dot = pod_partial_sum(partD + ((size_t)B + b) * chunks, chunks, red);
  const bool zero = !(l > 0.0);
  const float inv_l = zero ? 0.f : (float)(1.0 / l), kappa = zero || !normalize ? 0.f : (float)(dot / l);
  const float wn = (float)((double)weight / B / fmax(sqrt(nn_s), 1e-12));
  const float* Es = E + (size_t)b * g.n_E;
  const float* Et = E + ((size_t)B + b) * g.n_E;
  const int nsub = kPodBlock / lanes, lane = threadIdx.x % lanes;
  for (int un = blockIdx.x * nsub + threadIdx.x / lanes; un < g.n_E / g.C; un += chunks * nsub) {      // whole units, as in the pool kernel
    const PodUnit u = pod_unit(g, un);
    const float count = (float)(u.col ? g.kh[u.k] : g.kw[u.k]);
    for (int c = lane; c < g.C; c += lanes) {
      const size_t e = (size_t)un * g.C + c;
      const float es = Es[e] * inv_s, et = Et[e] * inv_t, d = es - et;
      const float ge = zero ? 0.f : wn * (d * inv_l - kappa * es);
      gE[(size_t)b * g.n_E + e] = ge / count;
    }
  }
  if (blockIdx.x == 0 && b == 0) {
    double total = 0.0;
    for (int q = 0; q < B; ++q) total += sqrt(pod_partial_sum(partD + (size_t)q * chunks, chunks, red));
    if (threadIdx.x == 0) loss_out[0] = (float)(total / B);
  }
}

// The backward pass over the tiles of the student map: dX = grad_out * 2 P (X >= 0 ? 1 : 1 / a) * dQ
template <typename T>
__global__ __launch_bounds__(kPodBlock) void pod_bwd_kernel(const T* __restrict__ x, int ldx, float inv_a, int B, const PodGeom geom,
                                                           const float* __restrict__ gE, const float* __restrict__ grad_out,
                                                           T* __restrict__ dx, int ldd) {
  constexpr int VEC = Vec<T>::N;
  __shared__ PodGeom g;
  pod_stage(&g, geom);
  const PodTile t = pod_tile<VEC>(g, B);
  if (!t.live) return;
  const float go = grad_out[0];
  const float* gb = gE + (size_t)t.b * g.n_E + t.c;
  // the scales that cover this tile, and the tile's region in each
  bool cover[kPodMaxScales];
  int ri[kPodMaxScales], cj[kPodMaxScales];
#pragma unroll
  for (int k = 0; k < kPodMaxScales; ++k) {
    cover[k] = k < g.n && t.r0 < g.s[k] * g.kh[k] && t.x0 < g.s[k] * g.kw[k];
    ri[k] = cover[k] ? t.r0 / g.kh[k] : 0;
    cj[k] = cover[k] ? t.x0 / g.kw[k] : 0;
  }
  float rco[kPodRows][VEC];
#pragma unroll
  for (int rr = 0; rr < kPodRows; ++rr) {
#pragma unroll
    for (int q = 0; q < VEC; ++q) rco[rr][q] = 0.f;
    if (rr < t.nr) {
#pragma unroll
      for (int k = 0; k < kPodMaxScales; ++k)
        if (cover[k]) pod_add(rco[rr], gb + g.rowoff[k] + ((size_t)(t.r0 + rr) * g.s[k] + cj[k]) * g.C);
    }
  }
  const T* xbase = x + ((size_t)t.b * g.h + t.r0) * g.w * (size_t)ldx + t.c;
  T* dbase = dx + ((size_t)t.b * g.h + t.r0) * g.w * (size_t)ldd + t.c;
  for (int xx = t.x0; xx < t.x1; ++xx) {
    Vec<T> v[kPodRows];
#pragma unroll
    for (int rr = 0; rr < kPodRows; ++rr)
      if (rr < t.nr) v[rr].load(xbase + ((size_t)rr * g.w + xx) * ldx);
    float cco[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) cco[q] = 0.f;
#pragma unroll
    for (int k = 0; k < kPodMaxScales; ++k)
      if (cover[k]) pod_add(cco, gb + g.coloff[k] + ((size_t)xx * g.s[k] + ri[k]) * g.C);
#pragma unroll
    for (int rr = 0; rr < kPodRows; ++rr)
      if (rr < t.nr) {
        Vec<T> o;
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
          const float e = v[rr].get(q);
          const float f = e >= 0.f ? 2.f * e : 2.f * e * inv_a * inv_a;
          o.set(q, go * f * (rco[rr][q] + cco[q]));
        }
        o.store(dbase + ((size_t)rr * g.w + xx) * ldd);
      }
  }
}

// ---- the level on the logits --------------------------------------------------------------------------------------------------
// Student rows [h, w, Ctot], teacher rows [h, w, K], fp32, any 4-byte aligned base and pitch.  M[0] = S[0] + sum_{c >= K} S[c] (the
// sum first, in ascending c, then the addition), M[k] = S[k]; Q = M^2 against T^2, slope 1, strips of K channels.
// Lanes.  A pixel's channels are cut into slots of VEC consecutive floats (VEC = 4, 2 or 1: the widest that the base pointer, the
// pitch and the channel count of THAT map allow, chosen per call); slot v lies on lane v % G of a group of G lanes (the power of
// two that holds the slots, at most 64) as its chunk v / G, so a group's load instruction covers one contiguous stretch of the
// row and a wave holds 64 / G tiles.  A group walks one tile, as a thread of the feature kernels does.  The new-class sum is taken
// from the lanes that loaded the channels: every lane of the group adds the same values in the same order (one cross-lane read
// per value), nobody loads a second time and the result is on lane 0 (and everywhere else) without a reduction tree, whose order
// would not be the ascending one.
constexpr int kPodLogitsMaxC = 256;
constexpr int kPodSlotFloats = kPodLogitsMaxC / 64;        // floats of a pixel that a lane holds

inline int podl_vec(const void* p, int ld, int C) {
  for (int v = 4; v > 1; v >>= 1)
    if (reinterpret_cast<uintptr_t>(p) % (4u * v) == 0 && ld % v == 0 && C % v == 0) return v;
  return 1;
}
inline int podl_vec2(const void* p, int ld, const void* q, int ldq, int C) {
  const int a = podl_vec(p, ld, C), b = podl_vec(q, ldq, C);
  return a < b ? a : b;
}
inline int podl_group(int C, int vec) {
  int G = 1;
  while (G < C / vec && G < 64) G *= 2;
  return G;
}
inline long long podl_items(const PodGeom& g, int B, int G) { return (long long)B * g.nrs * g.ncs * G; }

struct PodlTile {
  int b, r0, nr, x0, x1, rs, cs, j;
  bool live;
};
__device__ __forceinline__ PodlTile podl_tile(const PodGeom& g, int B, int G) {
  PodlTile t;
  long long item = ((long long)blockIdx.x * kPodBlock + threadIdx.x) / G;      // G divides the block: a group never straddles two
  t.j = threadIdx.x & (G - 1);
  t.live = item < (long long)B * g.nrs * g.ncs;
  if (!t.live) item = 0;
  t.cs = (int)(item % g.ncs);
  item /= g.ncs;
  t.rs = (int)(item % g.nrs);
  t.b = (int)(item / g.nrs);
  t.r0 = g.rcut[t.rs], t.nr = g.rcut[t.rs + 1] - t.r0;
  t.x0 = g.ccut[t.cs], t.x1 = g.ccut[t.cs + 1];
  return t;
}

// register i * VEC + q of a lane holds channel (i * G + j) * VEC + q
template <int VEC>
__device__ __forceinline__ int podl_channel(int reg, int j, int G) {
  return ((reg / VEC) * G + j) * VEC + reg % VEC;
}

// the C channels of the pixel at p (C is a multiple of VEC: a slot is inside the row or outside)
template <int VEC>
__device__ __forceinline__ void podl_load(float (&v)[kPodSlotFloats], const float* __restrict__ p, int j, int G, int C) {
#pragma unroll
  for (int i = 0; i < kPodSlotFloats / VEC; ++i) {
    const int c = (i * G + j) * VEC;
    if (c < C) {
      if (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p + c);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
      } else if (VEC == 2) {
        const float2 q = *reinterpret_cast<const float2*>(p + c);
        v[i * 2] = q.x, v[i * 2 + 1] = q.y;
      } else {
        v[i] = p[c];
      }
    } else {
#pragma unroll
      for (int q = 0; q < VEC; ++q) v[i * VEC + q] = 0.f;
    }
  }
}
template <int VEC>
__device__ __forceinline__ void podl_store(float* __restrict__ p, const float (&v)[kPodSlotFloats], int j, int G, int C) {
#pragma unroll
  for (int i = 0; i < kPodSlotFloats / VEC; ++i) {
    const int c = (i * G + j) * VEC;
    if (c < C) {
      if (VEC == 4)
        *reinterpret_cast<float4*>(p + c) = make_float4(v[0], v[1], v[2], v[3]);
      else if (VEC == 2)
        *reinterpret_cast<float2*>(p + c) = make_float2(v[i * 2], v[i * 2 + 1]);
      else
        p[c] = v[i];
    }
  }
}

// e[rr] = sum over c in [K, C) of the row's channel c, in ascending c, on every lane of the group.  The trip counts depend on
// (K, C, G) alone: uniform over the wave, and every lane of a live group takes part (rows outside the tile hold zeros).
template <int VEC>
__device__ __forceinline__ void podl_extra(const float (&v)[kPodRows][kPodSlotFloats], float (&e)[kPodRows], int G, int K, int C) {
#pragma unroll
  for (int rr = 0; rr < kPodRows; ++rr) e[rr] = 0.f;
#pragma unroll
  for (int i = 0; i < kPodSlotFloats / VEC; ++i) {
    const int lo = K / VEC - i * G, hi = C / VEC - i * G;
    for (int jj = lo > 0 ? lo : 0; jj < (hi < G ? hi : G); ++jj) {
#pragma unroll
      for (int q = 0; q < VEC; ++q) {
        const bool take = (i * G + jj) * VEC + q >= K;
#pragma unroll
        for (int rr = 0; rr < kPodRows; ++rr) {
          const float s = __shfl(v[rr][i * VEC + q], jj, G);
          if (take) e[rr] += s;
        }
      }
    }
  }
}

// One map of the tile pass.  C: the map's channels (Ctot or K); the strips hold g.C = K of them.
template <int VEC, bool STUDENT>
__device__ __forceinline__ void podl_tile_pass(const PodGeom& g, const float* __restrict__ x, size_t ld, int C, int G, int B, size_t net,
                                               float* __restrict__ rowseg, float* __restrict__ colseg) {
  const PodlTile t = podl_tile(g, B, G);
  if (!t.live) return;
  const int K = g.C;
  const float* base = x + ((size_t)t.b * g.h + t.r0) * g.w * ld;
  const size_t nb = net * B + t.b;
  float* crow = colseg + ((nb * g.nrs + t.rs) * g.w) * K;
  float racc[kPodRows][kPodSlotFloats];
#pragma unroll
  for (int rr = 0; rr < kPodRows; ++rr)
#pragma unroll
    for (int q = 0; q < kPodSlotFloats; ++q) racc[rr][q] = 0.f;
  for (int xx = t.x0; xx < t.x1; ++xx) {
    float v[kPodRows][kPodSlotFloats];
#pragma unroll
    for (int rr = 0; rr < kPodRows; ++rr)
      podl_load<VEC>(v[rr], base + ((size_t)rr * g.w + xx) * ld, t.j, G, rr < t.nr ? C : 0);
    if (STUDENT && K < C) {
      float e[kPodRows];
      podl_extra<VEC>(v, e, G, K, C);
      if (t.j == 0) {
#pragma unroll
        for (int rr = 0; rr < kPodRows; ++rr) v[rr][0] += e[rr];
      }
    }
    float csum[kPodSlotFloats];
#pragma unroll
    for (int q = 0; q < kPodSlotFloats; ++q) csum[q] = 0.f;
#pragma unroll
    for (int rr = 0; rr < kPodRows; ++rr)
      if (rr < t.nr) {
#pragma unroll
        for (int q = 0; q < kPodSlotFloats; ++q) {
          const float sq = v[rr][q] * v[rr][q];
          racc[rr][q] += sq;
          csum[q] += sq;
        }
      }
    // the strips are 4-byte aligned only (K is free): one float per store, the lanes of a group over consecutive channels
#pragma unroll
    for (int q = 0; q < kPodSlotFloats; ++q) {
      const int c = podl_channel<VEC>(q, t.j, G);
      if (c < K) crow[(size_t)xx * K + c] = csum[q];
    }
  }
#pragma unroll
  for (int rr = 0; rr < kPodRows; ++rr)
    if (rr < t.nr) {
      float* rrow = rowseg + ((nb * g.h + t.r0 + rr) * g.ncs + t.cs) * K;
#pragma unroll
      for (int q = 0; q < kPodSlotFloats; ++q) {
        const int c = podl_channel<VEC>(q, t.j, G);
        if (c < K) rrow[c] = racc[rr][q];
      }
    }
}

struct PodlMap {
  const float* x;
  int ld, C, vec, G;
};

// The tile pass on the logits: blockIdx.y = 0 the student rows (Ctot channels, merged), 1 the teacher rows (K channels)
__global__ __launch_bounds__(kPodBlock) void pod_logits_tile_kernel(const PodlMap ms, const PodlMap mt, int B, const PodGeom geom,
                                                                   float* __restrict__ rowseg, float* __restrict__ colseg) {
  __shared__ PodGeom g;
  pod_stage(&g, geom);
  if (blockIdx.y == 0) {
    if (ms.vec == 4)
      podl_tile_pass<4, true>(g, ms.x, ms.ld, ms.C, ms.G, B, 0, rowseg, colseg);
    else if (ms.vec == 2)
      podl_tile_pass<2, true>(g, ms.x, ms.ld, ms.C, ms.G, B, 0, rowseg, colseg);
    else
      podl_tile_pass<1, true>(g, ms.x, ms.ld, ms.C, ms.G, B, 0, rowseg, colseg);
  } else {
    if (mt.vec == 4)
      podl_tile_pass<4, false>(g, mt.x, mt.ld, mt.C, mt.G, B, 1, rowseg, colseg);
    else if (mt.vec == 2)
      podl_tile_pass<2, false>(g, mt.x, mt.ld, mt.C, mt.G, B, 1, rowseg, colseg);
    else
      podl_tile_pass<1, false>(g, mt.x, mt.ld, mt.C, mt.G, B, 1, rowseg, colseg);
  }
}

// The backward pass on the logits: dS[c] = grad_out * 2 M[k(c)] dQ[k(c)], k(c) = c below K and 0 from K on - lane 0 of the group
// forms the value of channel 0 and the lanes of the new-class channels copy its bits
template <int VEC>
__global__ __launch_bounds__(kPodBlock) void pod_logits_bwd_kernel(const float* __restrict__ x, int ldx, int C, int G, int B,
                                                                  const PodGeom geom, const float* __restrict__ gE,
                                                                  const float* __restrict__ grad_out, float* __restrict__ dx, int ldd) {
  __shared__ PodGeom g;
  pod_stage(&g, geom);
  const PodlTile t = podl_tile(g, B, G);
  if (!t.live) return;
  const int K = g.C;
  const float go = grad_out[0];
  const float* gb = gE + (size_t)t.b * g.n_E;
  bool cover[kPodMaxScales];
  int ri[kPodMaxScales], cj[kPodMaxScales];
#pragma unroll
  for (int k = 0; k < kPodMaxScales; ++k) {
    cover[k] = k < g.n && t.r0 < g.s[k] * g.kh[k] && t.x0 < g.s[k] * g.kw[k];
    ri[k] = cover[k] ? t.r0 / g.kh[k] : 0;
    cj[k] = cover[k] ? t.x0 / g.kw[k] : 0;
  }
  int ch[kPodSlotFloats];
#pragma unroll
  for (int q = 0; q < kPodSlotFloats; ++q) ch[q] = podl_channel<VEC>(q, t.j, G);
  float rco[kPodRows][kPodSlotFloats];
#pragma unroll
  for (int rr = 0; rr < kPodRows; ++rr) {
#pragma unroll
    for (int q = 0; q < kPodSlotFloats; ++q) rco[rr][q] = 0.f;
    if (rr < t.nr) {
#pragma unroll
      for (int k = 0; k < kPodMaxScales; ++k)
        if (cover[k]) {
          const float* p = gb + g.rowoff[k] + ((size_t)(t.r0 + rr) * g.s[k] + cj[k]) * K;
#pragma unroll
          for (int q = 0; q < kPodSlotFloats; ++q)
            if (ch[q] < K) rco[rr][q] += p[ch[q]];
        }
    }
  }
  const float* xbase = x + ((size_t)t.b * g.h + t.r0) * g.w * (size_t)ldx;
  float* dbase = dx + ((size_t)t.b * g.h + t.r0) * g.w * (size_t)ldd;
  for (int xx = t.x0; xx < t.x1; ++xx) {
    float v[kPodRows][kPodSlotFloats];
#pragma unroll
    for (int rr = 0; rr < kPodRows; ++rr)
      podl_load<VEC>(v[rr], xbase + ((size_t)rr * g.w + xx) * ldx, t.j, G, rr < t.nr ? C : 0);
    if (K < C) {
      float e[kPodRows];
      podl_extra<VEC>(v, e, G, K, C);
      if (t.j == 0) {
#pragma unroll
        for (int rr = 0; rr < kPodRows; ++rr) v[rr][0] += e[rr];
      }
    }
    float cco[kPodSlotFloats];
#pragma unroll
    for (int q = 0; q < kPodSlotFloats; ++q) cco[q] = 0.f;
#pragma unroll
    for (int k = 0; k < kPodMaxScales; ++k)
      if (cover[k]) {
        const float* p = gb + g.coloff[k] + ((size_t)xx * g.s[k] + ri[k]) * K;
#pragma unroll
        for (int q = 0; q < kPodSlotFloats; ++q)
          if (ch[q] < K) cco[q] += p[ch[q]];
      }
#pragma unroll
    for (int rr = 0; rr < kPodRows; ++rr) {
      float o[kPodSlotFloats];
#pragma unroll
      for (int q = 0; q < kPodSlotFloats; ++q) {
        const float f = 2.f * v[rr][q];
        o[q] = go * f * (rco[rr][q] + cco[q]);
      }
      const float d0 = __shfl(o[0], 0, G);                  // every lane of the group, whatever its row count: group-uniform
#pragma unroll
      for (int q = 0; q < kPodSlotFloats; ++q)
        if (ch[q] >= K) o[q] = d0;
      if (rr < t.nr) podl_store<VEC>(dbase + ((size_t)rr * g.w + xx) * ldd, o, t.j, G, C);
    }
  }
}

// The argument rules that the three calls on the logits share; fills g with the geometry of the K-channel strips
int podl_args(const char* fn, int h, int w, int Ctot, int K, const int* scales, int n, int B, PodGeom* g) {
  UCD_REQUIRE(B >= 1, UCD_EINVAL, "%s: B = %d must be at least 1", fn, B);
  UCD_REQUIRE(K >= 1, UCD_EINVAL, "%s: K = %d must be at least 1", fn, K);
  UCD_REQUIRE(K <= Ctot, UCD_EINVAL, "%s: K = %d is above Ctot = %d", fn, K, Ctot);
  UCD_REQUIRE(Ctot <= kPodLogitsMaxC, UCD_EUNSUPPORTED, "%s: Ctot = %d is above %d", fn, Ctot, kPodLogitsMaxC);
  return pod_geom(fn, h, w, K, scales, n, g, 1, kPodLogitsMaxC);
}
int podl_check_rows(const char* fn, const char* what, const void* p, int ld, int C, const char* cname) {
  UCD_REQUIRE(ld >= C, UCD_EINVAL, "%s: the row pitch of %s (%d) is below %s = %d", fn, what, ld, cname, C);
  UCD_REQUIRE(reinterpret_cast<uintptr_t>(p) % 4 == 0, UCD_EALIGN, "%s: %s must be 4-byte aligned", fn, what);
  return UCD_OK;
}

int pod_check_map(const char* fn, const char* what, const void* p, int ld, int C, int es) {
  UCD_REQUIRE(ld >= C, UCD_EINVAL, "%s: the row pitch of %s (%d) is below C = %d", fn, what, ld, C);
  UCD_REQUIRE(aligned16(p) && ((size_t)ld * es) % 16 == 0, UCD_EALIGN, "%s: %s must be 16-byte aligned with a 16-byte multiple row pitch", fn,
              what);
  return UCD_OK;
}

// The three strip launches behind a tile pass: pool, diff, coef
int pod_strips(const char* fn, const PodGeom& g, int B, int normalize, int lanes, float weight, char* wsp, const PodWs& ws, float* loss_out,
               float* g_E, hipStream_t s) {
  float *rowseg = (float*)(wsp + ws.rowseg), *colseg = (float*)(wsp + ws.colseg), *E = (float*)(wsp + ws.E);
  double *partN = (double*)(wsp + ws.partN), *partD = (double*)(wsp + ws.partD);
  const int chunks = pod_chunks(g, lanes);
  int rc;
  pod_pool_kernel<<<dim3(chunks, B, 2), kPodBlock, 0, s>>>(g, B, lanes, rowseg, colseg, E, partN);
  if ((rc = check_launch(fn))) return rc;
  pod_diff_kernel<<<dim3(chunks, B), kPodBlock, 0, s>>>(g.n_E, B, normalize, E, partN, partD);
  if ((rc = check_launch(fn))) return rc;
  pod_coef_kernel<<<dim3(chunks, B), kPodBlock, 0, s>>>(g, B, normalize, lanes, weight, E, partN, partD, g_E, loss_out);
  return check_launch(fn);
}

}  // namespace
}  // namespace ucd

using namespace ucd;

extern "C" {

int ucd_pod_plan(int h, int w, int C, const int* scales, int n, int B, int dtype, int* n_E, size_t* workspace_bytes, int* grid) {
  static const char* fn = "ucd_pod_plan";
  PodGeom g;
  const int rc = pod_geom(fn, h, w, C, scales, n, &g);
  if (rc) return rc;
  UCD_REQUIRE(B >= 1, UCD_EINVAL, "%s: B = %d must be at least 1", fn, B);
  UCD_REQUIRE(dtype == UCD_F32 || dtype == UCD_BF16, UCD_EINVAL, "%s: unknown dtype %d", fn, dtype);
  const long long items = pod_tile_items(g, B, dtype == UCD_BF16 ? 8 : 4);
  UCD_REQUIRE((items + kPodBlock - 1) / kPodBlock <= 0x7FFFFFFF, UCD_EUNSUPPORTED, "%s: %lld tile items are more than a grid holds", fn, items);
  if (n_E) *n_E = g.n_E;
  if (workspace_bytes) *workspace_bytes = pod_ws(g, B).bytes;
  if (grid) {
    grid[0] = (int)((items + kPodBlock - 1) / kPodBlock);     // workgroups of the tile pass (per map) and of the backward pass
    grid[1] = pod_chunks(g);                                  // workgroups per sample of the three strip kernels
    grid[2] = g.nrs;                                          // row pieces
    grid[3] = g.ncs;                                          // column pieces
  }
  return UCD_OK;
}

int ucd_pod_forward(const void* x_s, int ld_s, const void* x_t, int ld_t, int dtype, int B, int C, int h, int w, float slope,
                    const int* scales, int n, float weight, float* loss_out, float* g_E, void* workspace, size_t workspace_bytes,
                    ucd_stream_t stream) {
  static const char* fn = "ucd_pod_forward";
  UCD_REQUIRE(x_s && x_t && loss_out && g_E, UCD_EINVAL, "%s: NULL argument (x_s, x_t, loss_out and g_E are required)", fn);
  UCD_REQUIRE(B >= 1, UCD_EINVAL, "%s: B = %d must be at least 1", fn, B);
  UCD_REQUIRE(dtype == UCD_F32 || dtype == UCD_BF16, UCD_EINVAL, "%s: unknown dtype %d", fn, dtype);
  UCD_REQUIRE(slope > 0.f && slope <= 1.f, UCD_EINVAL, "%s: the slope %g is outside (0, 1]", fn, (double)slope);
  PodGeom g;
  int rc = pod_geom(fn, h, w, C, scales, n, &g);
  if (rc) return rc;
  const int es = dtype == UCD_BF16 ? 2 : 4, vec = 16 / es;
  if ((rc = pod_check_map(fn, "x_s", x_s, ld_s, C, es))) return rc;
  if ((rc = pod_check_map(fn, "x_t", x_t, ld_t, C, es))) return rc;
  UCD_REQUIRE(aligned16(g_E), UCD_EALIGN, "%s: g_E must be 16-byte aligned", fn);
  const long long items = pod_tile_items(g, B, vec);
  UCD_REQUIRE((items + kPodBlock - 1) / kPodBlock <= 0x7FFFFFFF && B <= 65535, UCD_EUNSUPPORTED, "%s: B = %d with %lld tile items is more than a grid holds",
              fn, B, items);
  const PodWs ws = pod_ws(g, B);
  UCD_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= ws.bytes, UCD_EWORKSPACE, "%s: workspace missing, unaligned or too small", fn);
  hipStream_t s = (hipStream_t)stream;
  char* wsp = (char*)workspace;
  float *rowseg = (float*)(wsp + ws.rowseg), *colseg = (float*)(wsp + ws.colseg);
  const float inv_a = (float)(1.0 / (double)slope);
  const int blocks = (int)((items + kPodBlock - 1) / kPodBlock);
  if (dtype == UCD_BF16)
    pod_tile_kernel<__hip_bfloat16><<<dim3(blocks, 2), kPodBlock, 0, s>>>((const __hip_bfloat16*)x_s, ld_s, (const __hip_bfloat16*)x_t, ld_t,
                                                                         inv_a, B, g, rowseg, colseg);
  else
    pod_tile_kernel<float><<<dim3(blocks, 2), kPodBlock, 0, s>>>((const float*)x_s, ld_s, (const float*)x_t, ld_t, inv_a, B, g, rowseg, colseg);
  if ((rc = check_launch(fn))) return rc;
  return pod_strips(fn, g, B, 1, kPodBlock, weight, wsp, ws, loss_out, g_E, s);
}

int ucd_pod_backward(const void* x_s, int ld_s, int dtype, int B, int C, int h, int w, float slope, const int* scales, int n,
                     const float* g_E, const float* grad_out, void* d_x, int ld_d, ucd_stream_t stream) {
  static const char* fn = "ucd_pod_backward";
  UCD_REQUIRE(x_s && g_E && grad_out && d_x, UCD_EINVAL, "%s: NULL argument (x_s, g_E, grad_out and d_x are required)", fn);
  UCD_REQUIRE(B >= 1, UCD_EINVAL, "%s: B = %d must be at least 1", fn, B);
  UCD_REQUIRE(dtype == UCD_F32 || dtype == UCD_BF16, UCD_EINVAL, "%s: unknown dtype %d", fn, dtype);
  UCD_REQUIRE(slope > 0.f && slope <= 1.f, UCD_EINVAL, "%s: the slope %g is outside (0, 1]", fn, (double)slope);
  PodGeom g;
  int rc = pod_geom(fn, h, w, C, scales, n, &g);
  if (rc) return rc;
  const int es = dtype == UCD_BF16 ? 2 : 4, vec = 16 / es;
  if ((rc = pod_check_map(fn, "x_s", x_s, ld_s, C, es))) return rc;
  if ((rc = pod_check_map(fn, "d_x", d_x, ld_d, C, es))) return rc;
  UCD_REQUIRE(aligned16(g_E), UCD_EALIGN, "%s: g_E must be 16-byte aligned", fn);
  const long long items = pod_tile_items(g, B, vec);
  UCD_REQUIRE((items + kPodBlock - 1) / kPodBlock <= 0x7FFFFFFF, UCD_EUNSUPPORTED, "%s: %lld tile items are more than a grid holds", fn, items);
  hipStream_t s = (hipStream_t)stream;
  const float inv_a = (float)(1.0 / (double)slope);
  const int blocks = (int)((items + kPodBlock - 1) / kPodBlock);
  if (dtype == UCD_BF16)
    pod_bwd_kernel<__hip_bfloat16><<<blocks, kPodBlock, 0, s>>>((const __hip_bfloat16*)x_s, ld_s, inv_a, B, g, g_E, grad_out,
                                                               (__hip_bfloat16*)d_x, ld_d);
  else
    pod_bwd_kernel<float><<<blocks, kPodBlock, 0, s>>>((const float*)x_s, ld_s, inv_a, B, g, g_E, grad_out, (float*)d_x, ld_d);
  return check_launch(fn);
}

int ucd_pod_logits_plan(int h, int w, int Ctot, int K, const int* scales, int n, int B, int normalize, int* n_E, size_t* workspace_bytes,
                        int* grid) {
  static const char* fn = "ucd_pod_logits_plan";
  UCD_REQUIRE(normalize == 0 || normalize == 1, UCD_EINVAL, "%s: normalize = %d is neither 0 nor 1", fn, normalize);
  PodGeom g;
  const int rc = podl_args(fn, h, w, Ctot, K, scales, n, B, &g);
  if (rc) return rc;
  if (n_E) *n_E = g.n_E;
  if (workspace_bytes) *workspace_bytes = pod_ws(g, B, pod_logits_lanes(K)).bytes;
  if (grid) {
    // with dense 16-byte aligned rows; the calls choose the vector width from the pointers and pitches they get
    const int Gs = podl_group(Ctot, podl_vec(nullptr, Ctot, Ctot)), Gt = podl_group(K, podl_vec(nullptr, K, K));
    grid[0] = (int)((podl_items(g, B, Gs > Gt ? Gs : Gt) + kPodBlock - 1) / kPodBlock);
    grid[1] = pod_chunks(g, pod_logits_lanes(K));
    grid[2] = g.nrs;
    grid[3] = g.ncs;
  }
  return UCD_OK;
}

int ucd_pod_logits_forward(const void* x_s, int ld_s, const void* x_t, int ld_t, int dtype, int B, int Ctot, int K, int h, int w,
                           const int* scales, int n, int normalize, float weight, float* loss_out, float* g_E, void* workspace,
                           size_t workspace_bytes, ucd_stream_t stream) {
  static const char* fn = "ucd_pod_logits_forward";
  UCD_REQUIRE(x_s && x_t && loss_out && g_E, UCD_EINVAL, "%s: NULL argument (x_s, x_t, loss_out and g_E are required)", fn);
  UCD_REQUIRE(dtype == UCD_F32, UCD_EUNSUPPORTED, "%s: dtype %d (the logits are fp32 rows, UCD_F32)", fn, dtype);
  UCD_REQUIRE(normalize == 0 || normalize == 1, UCD_EINVAL, "%s: normalize = %d is neither 0 nor 1", fn, normalize);
  PodGeom g;
  int rc = podl_args(fn, h, w, Ctot, K, scales, n, B, &g);
  if (rc) return rc;
  if ((rc = podl_check_rows(fn, "x_s", x_s, ld_s, Ctot, "Ctot"))) return rc;
  if ((rc = podl_check_rows(fn, "x_t", x_t, ld_t, K, "K"))) return rc;
  UCD_REQUIRE(reinterpret_cast<uintptr_t>(g_E) % 4 == 0 && reinterpret_cast<uintptr_t>(loss_out) % 4 == 0, UCD_EALIGN,
              "%s: g_E and loss_out must be 4-byte aligned", fn);
  UCD_REQUIRE(B <= 65535, UCD_EUNSUPPORTED, "%s: B = %d is more than a grid holds", fn, B);
  const int lanes = pod_logits_lanes(K);
  const PodWs ws = pod_ws(g, B, lanes);
  UCD_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= ws.bytes, UCD_EWORKSPACE, "%s: workspace missing, unaligned or too small", fn);
  PodlMap ms = {(const float*)x_s, ld_s, Ctot, podl_vec(x_s, ld_s, Ctot), 0};
  PodlMap mt = {(const float*)x_t, ld_t, K, podl_vec(x_t, ld_t, K), 0};
  ms.G = podl_group(ms.C, ms.vec), mt.G = podl_group(mt.C, mt.vec);
  // at most 65535 samples x kPodMaxCuts^2 tiles x 64 lanes: fewer workgroups than a grid holds
  const long long items = podl_items(g, B, ms.G > mt.G ? ms.G : mt.G);
  hipStream_t s = (hipStream_t)stream;
  char* wsp = (char*)workspace;
  pod_logits_tile_kernel<<<dim3((unsigned)((items + kPodBlock - 1) / kPodBlock), 2), kPodBlock, 0, s>>>(
      ms, mt, B, g, (float*)(wsp + ws.rowseg), (float*)(wsp + ws.colseg));
  if ((rc = check_launch(fn))) return rc;
  return pod_strips(fn, g, B, normalize, lanes, weight, wsp, ws, loss_out, g_E, s);
}

int ucd_pod_logits_backward(const void* x_s, int ld_s, int dtype, int B, int Ctot, int K, int h, int w, const int* scales, int n,
                            const float* g_E, const float* grad_out, float* d_x, int ld_d, ucd_stream_t stream) {
  static const char* fn = "ucd_pod_logits_backward";
  UCD_REQUIRE(x_s && g_E && grad_out && d_x, UCD_EINVAL, "%s: NULL argument (x_s, g_E, grad_out and d_x are required)", fn);
  UCD_REQUIRE(dtype == UCD_F32, UCD_EUNSUPPORTED, "%s: dtype %d (the logits are fp32 rows, UCD_F32)", fn, dtype);
  PodGeom g;
  int rc = podl_args(fn, h, w, Ctot, K, scales, n, B, &g);
  if (rc) return rc;
  if ((rc = podl_check_rows(fn, "x_s", x_s, ld_s, Ctot, "Ctot"))) return rc;
  if ((rc = podl_check_rows(fn, "d_x", d_x, ld_d, Ctot, "Ctot"))) return rc;
  UCD_REQUIRE(reinterpret_cast<uintptr_t>(g_E) % 4 == 0 && reinterpret_cast<uintptr_t>(grad_out) % 4 == 0, UCD_EALIGN,
              "%s: g_E and grad_out must be 4-byte aligned", fn);
  const int vec = podl_vec2(x_s, ld_s, d_x, ld_d, Ctot), G = podl_group(Ctot, vec);
  const unsigned blocks = (unsigned)((podl_items(g, B, G) + kPodBlock - 1) / kPodBlock);
  UCD_REQUIRE(podl_items(g, B, G) / kPodBlock < 0x7FFFFFFF, UCD_EUNSUPPORTED, "%s: B = %d is more than a grid holds", fn, B);
  hipStream_t s = (hipStream_t)stream;
  const float* x = (const float*)x_s;
  if (vec == 4)
    pod_logits_bwd_kernel<4><<<blocks, kPodBlock, 0, s>>>(x, ld_s, Ctot, G, B, g, g_E, grad_out, d_x, ld_d);
  else if (vec == 2)
    pod_logits_bwd_kernel<2><<<blocks, kPodBlock, 0, s>>>(x, ld_s, Ctot, G, B, g, g_E, grad_out, d_x, ld_d);
  else
    pod_logits_bwd_kernel<1><<<blocks, kPodBlock, 0, s>>>(x, ld_s, Ctot, G, B, g, g_E, grad_out, d_x, ld_d);
  return check_launch(fn);
}

}  // extern "C"
