// What the three contrastive-loss units (pixcon_loss.hip: fp32; pixcon_loss_f16.hip: fp16 fixed-split; pixcon_loss_f16p.hip:
// fp16 planned) share whatever their operand precision: the tile geometry, the accumulator layout helpers, the split count
// and workspace layout of the two fixed-split paths, and the combine kernel that turns the sweeps' partials into the per-row
// loss and gradient.
#pragma once
#include "common.h"
#include "pixcon.h"

namespace ucd {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kTI = 32;             // anchors per wave
constexpr int kBI = kWaves * kTI;   // anchors per workgroup
constexpr int kTJ = 32;             // contrast rows per tile
constexpr int kN = 256;             // padded feature dimension
constexpr int kMaxSplit = 16;

// contrast row of accumulator register `reg` on half-wave `half` (the k-pair order of one 32x32 MFMA step)
__device__ __forceinline__ int tile_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

struct TileList {  // two ranges of contrast tiles, addressed as one virtual list
  int t1a, n1, t2a, n2;
  __device__ __forceinline__ int count() const { return n1 + n2; }
  __device__ __forceinline__ int at(int v) const { return v < n1 ? t1a + v : t2a + (v - n1); }
};

// store the lane's 128 accumulator values of anchor row `dst` (n = 32 nt + 8 g + 4 half + 0..3)
__device__ __forceinline__ void store_values(const f32x16 (&acc)[8], float* __restrict__ dst, int half) {
#pragma unroll
  for (int nt = 0; nt < 8; ++nt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float4 v = {acc[nt][4 * g + 0], acc[nt][4 * g + 1], acc[nt][4 * g + 2], acc[nt][4 * g + 3]};
      *reinterpret_cast<float4*>(dst + 32 * nt + 8 * g + 4 * half) = v;
    }
}

// ---- fixed-split paths: split count and workspace ----------------------------------------------------------------
// grid.y of both sweeps: enough column ranges for ~1024 workgroups.  The split counts come from here and nowhere else.
inline int pixcon_split_count(int nt_i) {
  const int ns = ceil_div(1024, nt_i);
  return ns > kMaxSplit ? kMaxSplit : (ns < 1 ? 1 : ns);
}

// Workspace of a fixed-split path: per-split row vectors, then the per-split accumulators.  The fp16 form keeps one more
// row vector, the running maximum its negatives are scaled by (mrun).
struct SplitLayout {
  int nt_i, nsplit;
  size_t off_negp, off_mrunp, off_maxp, off_lossp, off_qsump, off_rowloss, off_Up, off_Vp, total;
  SplitLayout(int BHW, bool with_mrun) {
    nt_i = ceil_div(BHW, kBI);
    nsplit = pixcon_split_count(nt_i);
    const size_t rowvec = align_up((size_t)BHW * 4, 256);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += bytes; return at; };
    off_negp = take(rowvec * nsplit);
    off_mrunp = take(with_mrun ? rowvec * nsplit : 0);
    off_maxp = take(rowvec * nsplit);
    off_lossp = take(rowvec * nsplit);
    off_qsump = take(rowvec * nsplit);
    off_rowloss = take(rowvec);
    off_Up = take((size_t)nsplit * BHW * kN * 4);
    off_Vp = take((size_t)nsplit * BHW * kN * 4);
    total = o;
  }
};

// ---- combine: per-row loss and gradient --------------------------------------------------------------------------
// A policy names, for anchor row i, the partial slots either sweep left (slots sa..sb-1 of sweep 1 and of sweep 2; the
// row's value of slot s sits at s * stride + base) and the power of two a sweep-1 slot is scaled by:
enum CombineScale {
  kScaleNone,   // partials are true values (fp32)
  kScaleSlot,   // slot s is in units of 2^mrun[s]
  kScaleConst   // every slot is in units of 2^m_run
};
struct SlotRange {
  int base, stride, s1a, s1b, s2a, s2b;
};
// fixed split: slot s < nsplit of row i at s * maxA + i
template <CombineScale SCALE>
struct SplitSlots {
  static constexpr CombineScale kScale = SCALE;
  int nsplit1, nsplit2, maxA;
  const float* mrun;   // [nsplit1][maxA] (kScaleSlot; unused otherwise)
  __device__ __forceinline__ SlotRange row(int i) const { return {i, maxA, 0, nsplit1, 0, nsplit2}; }
};

// one wave per anchor row; the slots are summed in ascending order
template <class Policy>
__global__ __launch_bounds__(kThreads) void pixcon_combine_kernel(
    Policy pol, const uint8_t* __restrict__ row_label, const ucd_pixcon_meta* __restrict__ meta, float inv_T,
    const float* __restrict__ negp, const float* __restrict__ lossp, const float* __restrict__ qsump,
    const float* __restrict__ Up, const float* __restrict__ Vp, float* __restrict__ grad_a, int ldg,
    float* __restrict__ row_stats, int maxA, float* __restrict__ row_loss) {
  constexpr CombineScale kScale = Policy::kScale;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * (kThreads / 64) + wave;
  const int A = meta->A;
  if (i >= A) return;
  const SlotRange r = pol.row(i);
  auto at = [&](int s) { return (size_t)s * r.stride + r.base; };
  const int num = meta->label_count_c[row_label[i]] - 1;
  const float R = (float)meta->n_valid;
  float M = 0.f;   // the sums below are in units of 2^M
  if constexpr (kScale == kScaleSlot) {
    M = -1e30f;
    for (int s = r.s1a; s < r.s1b; ++s) M = fmaxf(M, pol.mrun[at(s)]);
  } else if constexpr (kScale == kScaleConst) {
    M = pol.m_run;
  }
  float neg = 0.f, la = 0.f, qs = 0.f;
  for (int s = r.s1a; s < r.s1b; ++s) {
    if constexpr (kScale == kScaleSlot) neg += negp[at(s)] * exp2f(pol.mrun[at(s)] - M);
    else neg += negp[at(s)];
  }
  for (int s = r.s2a; s < r.s2b; ++s) {
    la += lossp[at(s)];
    qs += qsump[at(s)];
  }
  const float coef = num > 0 ? inv_T / ((float)num * R) : 0.f;
  const float ratio = neg > 0.f ? qs / neg : 0.f;   // U is in the same 2^M units: the scale cancels
  const float rl = num > 0 ? -la / (float)num : 0.f;
  if (grad_a) {
    for (int c = lane * 4; c < ldg; c += 256) {
      float4 u = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
      if (c < kN) {
        for (int s = r.s1a; s < r.s1b; ++s) {
          const float4 t = *reinterpret_cast<const float4*>(Up + at(s) * kN + c);
          if constexpr (kScale == kScaleSlot) {
            const float w = exp2f(pol.mrun[at(s)] - M);
            u.x += w * t.x; u.y += w * t.y; u.z += w * t.z; u.w += w * t.w;
          } else {
            u.x += t.x; u.y += t.y; u.z += t.z; u.w += t.w;
          }
        }
        for (int s = r.s2a; s < r.s2b; ++s) {
          const float4 t = *reinterpret_cast<const float4*>(Vp + at(s) * kN + c);
          vv.x += t.x; vv.y += t.y; vv.z += t.z; vv.w += t.w;
        }
      }
      float4 g = {coef * (ratio * u.x - vv.x), coef * (ratio * u.y - vv.y), coef * (ratio * u.z - vv.z),
                  coef * (ratio * u.w - vv.w)};
      *reinterpret_cast<float4*>(grad_a + (size_t)i * ldg + c) = g;
    }
  }
  if (lane == 0) {
    row_loss[i] = rl;
    if (row_stats) {
      row_stats[i] = kScale == kScaleNone ? neg : (neg > 0.f ? neg * exp2f(M) : 0.f);
      row_stats[(size_t)maxA + i] = (float)num;
      row_stats[(size_t)2 * maxA + i] = rl;
    }
  }
}

}  // namespace
}  // namespace ucd
