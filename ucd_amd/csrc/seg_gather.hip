// The GATHER forms of the fused full-resolution logit losses (include/ucd_hip.h, DESIGN.md sections 3.5.4 and 3.5.5): one wave owns
// one low-resolution cell and walks it as seg_cell.h says.  A pixel is re-evaluated by each of its (up to) four cells; in return
// nothing is ever added to memory that another unit owns: no atomics, no fixed point, no LDS adds, each element of d_sem is written
// once (no memset) and the same inputs give the same bits.  The per-cell loss pairs are added in index order by a second launch
// (seg_loss_common.h).  Each kernel adds a lane layout, a label rule and its loss arithmetic:
// seg_bce_kernel (ucd_seg_bce), the BINARY cross entropy losses of the --bce / --icarl / --method LWF-MC runs - bilinear up-sampling
// of the student and teacher logits (segmentation_module.py:133) + BCEWithLogitsLossWithIgnoreIndex(reduction='none')(...).mean()
// (utils/loss.py:31-54, train.py:112/116) + the combined iCaRL term K * BCEWithLogitsLoss(mean)(out[:, :K], sigmoid(out_old))
// (train.py:119-124) + their gradient w.r.t. the LOW-resolution student logits.  No soft-max: every (pixel, class) term stands
// alone.  Lanes lie over PIXELS, a lane keeps 24 class sums, a butterfly per class.
// seg_losses_gather_kernel (ucd_seg_losses_gather), the soft-max losses of ucd_seg_losses_ex (seglogit_loss.hip) at the geometries
// whose tiles do not fit the LDS there.  Lanes lie over CLASSES, the wave visits the pixels one after another.
#include "common.h"
#include "seg_cell.h"
#include "seg_loss_common.h"

namespace ucd {
namespace {

constexpr int kChunk = 24;        // classes whose gradient sums a lane keeps in registers; more classes: the pixels are walked again
constexpr float kL2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

// e = exp(-|z|): sigmoid(z) = z >= 0 ? 1 / (1 + e) : e / (1 + e), softplus(-|z|) = log1p(e); nothing overflows at any z
__device__ __forceinline__ float exp_neg_abs(float z) { return __builtin_amdgcn_exp2f(-fabsf(z) * kL2e); }

// part: [B * h * w][2] (hard sum, soft sum) of the pixels whose (y0, x0) cell this is; d_sem (may be NULL): the cell's row
__global__ __launch_bounds__(kWave) void seg_bce_kernel(
    const float* __restrict__ sem_s, int ld_s, const float* __restrict__ sem_t, int ld_t, const int64_t* __restrict__ labels,
    int H, int W, int h, int w, int Ctot, int K, int ignore_index, float scale_h, float scale_w, float inv_scale_h,
    float inv_scale_w, float hard_scale, float soft_scale, float* __restrict__ part, float* __restrict__ d_sem, int ld_d) {
  extern __shared__ float smem[];
  const int cell = blockIdx.x, lane = threadIdx.x;
  const CellWalk walk(cell, H, W, h, w, scale_h, scale_w, inv_scale_h, inv_scale_w);
  // the 3 x 3 cells around (i, j): [9][CS] student, [9][KS] teacher logits; odd strides keep the nine rows on different banks
  const int CS = Ctot | 1, KS = sem_t ? (K | 1) : 0;
  float* s_log = smem;
  float* t_log = smem + 9 * CS;
  walk.stage(s_log, CS, sem_s, ld_s, Ctot, 1.f, lane);
  if (sem_t) walk.stage(t_log, KS, sem_t, ld_t, K, 1.f, lane);
  __syncthreads();

  const bool want_grad = d_sem != nullptr;
  float hard_sum = 0.f, soft_sum = 0.f;
  for (int c0 = 0; c0 < Ctot; c0 += kChunk) {
    float acc[kChunk];
#pragma unroll
    for (int k = 0; k < kChunk; ++k) acc[k] = 0.f;
    for (int p = lane; p < walk.npix; p += kWave) {
      const CellPixel px = walk.pixel(p);
      if (!px.matters(want_grad)) continue;
      const int64_t lab64 = labels[((size_t)walk.b * H + px.Y) * W + px.X];
      // a label outside [0, Ctot) counts as ignored, ignore_index or not (include/ucd_hip.h)
      const bool valid = lab64 != ignore_index && lab64 >= 0 && lab64 < Ctot;
      const int lab = valid ? (int)lab64 : -1;
      const float hw = valid ? hard_scale : 0.f;
      float hard_pix = 0.f, soft_pix = 0.f;
#pragma unroll
      for (int k = 0; k < kChunk; ++k) {
        const int c = c0 + k;
        if (c < Ctot) {                                // wave-uniform
          const float z = px.interp(s_log, CS, c);
          const float e = exp_neg_abs(z);
          const float r = __builtin_amdgcn_rcpf(1.f + e);
          const float sig = z >= 0.f ? r : e * r;
          // max(z, 0) + log1p(e); below 2^-12 log1p(e) = e - e^2 / 2 + ... is e to fp32
          const float sp = fmaxf(z, 0.f) + (e < 2.44140625e-4f ? e : kLn2 * __builtin_amdgcn_logf(1.f + e));
          const float hot = c == lab ? 1.f : 0.f;
          hard_pix += sp - hot * z;
          float g = hw * (sig - hot);
          if (sem_t && c < K) {                        // wave-uniform
            const float zt = px.interp(t_log, KS, c);
            const float et = exp_neg_abs(zt);
            const float rt = __builtin_amdgcn_rcpf(1.f + et);
            const float tgt = zt >= 0.f ? rt : et * rt;     // the sigmoid is applied AFTER the up-sampling (train.py:123-124)
            soft_pix += sp - tgt * z;
            g += soft_scale * (sig - tgt);
          }
          acc[k] += px.wgt * g;
        }
      }
      if (px.owner) {
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

// ---- the soft-max form (ucd_seg_losses_gather) --------------------------------------------------------------
// The tiled forms (seglogit_loss.hip) scatter: a pixel tile stages every low-resolution cell under it plus per-cell accumulators,
// which at small up-sampling factors (ADE at --output_stride 8: 207 456 bytes) no longer fits the LDS.  The cell walk serves any
// factor >= 1.  A pixel's normalisers are formed again by each of its (up to) four cells: that is the price (section 3.5.4), paid
// only where nothing else runs.
// Lanes lie over CLASSES (lane l keeps classes l, 64 + l, ... of NR rounds), not over pixels: the wave walks the pixels one after
// another, so labels, corners and weights are wave-uniform, lane c rebuilds z_pc from four conflict-free LDS reads (consecutive
// lanes, consecutive words), the normalisers are wave reductions (butterfly: a fixed order) and a lane keeps one gradient sum per
// round.  The pixels of the footprint are prepared 64 at a time, one per lane (source index, weight, label: the label loads of a
// chunk are in flight together), and the wave then visits only those a ballot found to matter.
// The arithmetic per pixel is that of seg_losses_wide_kernel: the same constants, the same kSubsetTiny rescue.
__device__ __forceinline__ int lane_get(int v, int k) { return __builtin_amdgcn_readlane(v, k); }
__device__ __forceinline__ float lane_get(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }
// a value every lane holds alike (the result of a butterfly), moved to a scalar register
__device__ __forceinline__ float uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// part: [B * h * w][2] (ce sum, kd sum) of the pixels whose (y0, x0) cell this is; d_sem (may be NULL): the cell's row
// SW: image walk.b weighs its cross entropy with ce_sw[walk.b] (ucd_seg_losses_gather_w; a cell lies in one image)
template <int NR, bool SW, bool FO>
__global__ __launch_bounds__(kWave) void seg_losses_gather_kernel(
    const float* __restrict__ sem_s, int ld_s, const float* __restrict__ sem_t, int ld_t, const int64_t* __restrict__ labels,
    int H, int W, int h, int w, int Ctot, int K, int ignore_index, float scale_h, float scale_w, float inv_scale_h,
    float inv_scale_w, float ce_scale, float kd_scale, float* __restrict__ part, float* __restrict__ d_sem, int ld_d, int kce,
    int kd_plain, float alpha, const float* __restrict__ ce_sw, float fo_gamma, float fo_alpha) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr float kNegBig = -1e30f;
  const int cell = blockIdx.x, lane = threadIdx.x;
  const CellWalk walk(cell, H, W, h, w, scale_h, scale_w, inv_scale_h, inv_scale_w);
  // FO (ucd_seg_losses_gather_focal) is built with SW and takes a NULL weight as ones
  const float sw = SW ? ((FO && !ce_sw) ? 1.f : ce_sw[walk.b]) : 1.f;
  // the 3 x 3 cells around (i, j): [9][Ctot] student, [9][K] teacher logits times alpha (the up-sampling is linear); dense rows
  float* s_log = smem;
  float* t_log = smem + 9 * Ctot;
  walk.stage(s_log, Ctot, sem_s, ld_s, Ctot, 1.f, lane);
  if (sem_t) walk.stage(t_log, K, sem_t, ld_t, K, alpha, lane);
  __syncthreads();

  const bool want_grad = d_sem != nullptr;
  const bool plain = kd_plain != 0, pool = kce == K;
  const int q_lo = plain ? 0 : 1;                 // first class whose teacher probability enters the per-class KD terms
  const float invK = 1.f / (float)K;
  const float kdw = sem_t ? kd_scale * invK : 0.f;
  float ce_sum = 0.f, kd_sum = 0.f;               // wave-uniform: every lane adds the same numbers
  float acc[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) acc[r] = 0.f;

  for (int p0 = 0; p0 < walk.npix; p0 += kWave) {
    // ---- one pixel per lane: where it reads, what it weighs, its label ---------------------------------------------------------
    const int p = p0 + lane;
    int code = 0, lab = 0;
    float ly0 = 0.f, ly1 = 0.f, lx0 = 0.f, lx1 = 0.f, wgt = 0.f;
    bool act = false;
    if (p < walk.npix) {
      const CellPixel px = walk.pixel(p);
      ly0 = px.ly0; ly1 = px.ly1; lx0 = px.lx0; lx1 = px.lx1; wgt = px.wgt;
      act = px.matters(want_grad);
      if (act) {
        const int64_t lab64 = labels[((size_t)walk.b * H + px.Y) * W + px.X];
        const bool ignored = lab64 == ignore_index;
        // as the scatter kernels read a label (include/ucd_hip.h): negative -> background, Ctot and above -> no class
        lab = ignored ? 0 : (int)(lab64 < 0 ? 0 : lab64 > Ctot ? Ctot : lab64);
        if (lab < kce) lab = 0;                       // loss.py:104-105
        code = px.q00 | (px.q01 << 4) | (px.q10 << 8) | (px.q11 << 12) | ((int)px.owner << 16) | ((int)ignored << 17);
      }
    }
    // ---- the wave visits the pixels that matter, one after another: everything about the pixel is uniform -------------------------
    for (unsigned long long todo = __ballot(act); todo; todo &= todo - 1) {
      const int k = __builtin_ctzll(todo);
      const int pc = lane_get(code, k), plab = lane_get(lab, k);
      const float pw = want_grad ? lane_get(wgt, k) : 0.f;
      const bool owner = (pc >> 16) & 1, ignored = (pc >> 17) & 1;
      const CellCorners u{pc & 15, (pc >> 4) & 15, (pc >> 8) & 15, (pc >> 12) & 15,
                          lane_get(ly0, k), lane_get(ly1, k), lane_get(lx0, k), lane_get(lx1, k)};
      float z[NR], e[NR];
      float m = kNegBig;
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int c = r * kWave + lane;
        z[r] = c < Ctot ? u.interp(s_log, Ctot, c) : kNegBig;      // classes past Ctot: exponentials that are exact zeros
        m = fmaxf(m, z[r]);
      }
      const float mz = uniform(wave_max(m)), mzl = mz * kL2e;
      float so = 0.f, sn = 0.f;
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int c = r * kWave + lane;
        e[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(z[r], kL2e, -mzl));
        so += c < K ? e[r] : 0.f;
        sn += c < K ? 0.f : e[r];
      }
      const float s_old = uniform(wave_sum(so)), s_new = uniform(wave_sum(sn)), e0 = lane_get(e[0], 0);
      const float s_all = s_old + s_new, s_bn = s_new + e0;
      const float den = mz + kLn2 * __builtin_amdgcn_logf(s_all);
      float lse_old = mz + kLn2 * __builtin_amdgcn_logf(s_old), lse_bn = mz + kLn2 * __builtin_amdgcn_logf(s_bn);
      float inv_old = 1.f / s_old, inv_bn = 1.f / s_bn, m_o = 0.f, m_b = 0.f, r_o = 0.f, r_b = 0.f;
      const bool rescue = s_old < kSubsetTiny || s_bn < kSubsetTiny;
      if (rescue) {                                  // a class subset ~87 below the leader: its sums again around its own maximum
        float mo = kNegBig, mb = kNegBig;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int c = r * kWave + lane;
          mo = c < K ? fmaxf(mo, z[r]) : mo;
          mb = (c == 0 || c >= K) ? fmaxf(mb, z[r]) : mb;
        }
        m_o = uniform(wave_max(mo));
        m_b = uniform(wave_max(mb));
        float so2 = 0.f, sb2 = 0.f;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int c = r * kWave + lane;
          so2 += c < K ? __builtin_amdgcn_exp2f((z[r] - m_o) * kL2e) : 0.f;
          sb2 += (c == 0 || c >= K) ? __builtin_amdgcn_exp2f((z[r] - m_b) * kL2e) : 0.f;
        }
        const float so_r = uniform(wave_sum(so2)), sb_r = uniform(wave_sum(sb2));
        lse_old = m_o + kLn2 * __builtin_amdgcn_logf(so_r);
        lse_bn = m_b + kLn2 * __builtin_amdgcn_logf(sb_r);
        r_o = 1.f / so_r; r_b = 1.f / sb_r;
        inv_old = 0.f; inv_bn = 0.f;                 // the subset terms of the gradient come from r_o / r_b below
      }
      const bool lab0 = pool && plab == 0;           // the label is the pooled background (plain CE: a one-hot like any)
      float fo_g = 1.f;
      if (FO) {
        // focal: every visiting cell needs the pixel's cross entropy for fo_g, the factor on its share of the gradient; the owner counts F
        // the label's logit is in a register of lane (plab & 63) already: a lane read instead of four more LDS reads per visit
        float z_lab = 0.f;
        if (plab < Ctot) {
#pragma unroll
          for (int r = 0; r < NR; ++r)
            if ((plab >> 6) == r) z_lab = lane_get(z[r], plab & 63);
        }
        const float fv = focal_pixel(-(lab0 ? lse_old - den : z_lab - den), fo_gamma, fo_alpha, fo_g);
        if (owner && !ignored) ce_sum += fv;
      } else if (owner && !ignored) {
        const float z_lab = plab < Ctot ? u.interp(s_log, Ctot, plab) : 0.f;       // a label that is no class: as the scatter kernels
        ce_sum += -(lab0 ? lse_old - den : z_lab - den);
      }
      // teacher soft-max over the old classes; q_c = te_c / sum te
      float te[NR];
      float inv_st = 0.f, q0 = 0.f;
      if (sem_t) {
        float tz[NR];
        float mt = kNegBig;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int c = r * kWave + lane;
          tz[r] = c < K ? u.interp(t_log, K, c) : kNegBig;
          mt = fmaxf(mt, tz[r]);
        }
        const float mtl = uniform(wave_max(mt)) * kL2e;
        float st = 0.f;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          te[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(tz[r], kL2e, -mtl));
          st += te[r];
        }
        inv_st = 1.f / uniform(wave_sum(st));
        q0 = lane_get(te[0], 0) * inv_st;
        if (owner) {
          // unbiased: q_0 (LSE_bn - den) + sum_{1<=c<K} q_c (z_c - den); plain: sum_{c<K} q_c (z_c - LSE_old)
          const float kd_ref = plain ? lse_old : den;
          float t1 = 0.f;
#pragma unroll
          for (int r = 0; r < NR; ++r) {
            const int c = r * kWave + lane;
            t1 = __builtin_fmaf((c >= q_lo && c < K) ? te[r] : 0.f, z[r] - kd_ref, t1);
          }
          const float kd_pix = (plain ? 0.f : q0 * (lse_bn - den)) + inv_st * uniform(wave_sum(t1));
          kd_sum += -kd_pix * invK;
        }
      } else {
#pragma unroll
        for (int r = 0; r < NR; ++r) te[r] = 0.f;
      }
      if (pw != 0.f) {
        // g_c = e_c (a_all - a_old [c<K] - b_bn [c in bkg/new]) - hot [c == label] - b_q te_c [q_lo<=c<K]  (seg_losses_wide_kernel)
        const float ce_w = ignored ? 0.f : FO ? fo_g * (sw * ce_scale) : (SW ? sw * ce_scale : ce_scale);
        const float a_all = (ce_w + (plain ? 0.f : kdw)) / s_all;
        const float a_old = (lab0 ? ce_w * inv_old : 0.f) - (plain ? kdw * inv_old : 0.f);
        const float b_bn = plain ? 0.f : kdw * q0 * inv_bn;
        const float hot = lab0 ? 0.f : ce_w, b_q = kdw * inv_st;
        const float rco = (lab0 ? ce_w * r_o : 0.f) - (plain ? kdw * r_o : 0.f), rcb = plain ? 0.f : kdw * q0 * r_b;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int c = r * kWave + lane;
          const float coef = a_all - (c < K ? a_old : 0.f) - ((c == 0 || c >= K) ? b_bn : 0.f);
          float g = e[r] * coef - (c == plab ? hot : 0.f);
          g = __builtin_fmaf(-b_q, (c >= q_lo && c < K) ? te[r] : 0.f, g);
          if (rescue) {
            if (c < K) g -= rco * __builtin_amdgcn_exp2f((z[r] - m_o) * kL2e);
            if (c == 0 || c >= K) g -= rcb * __builtin_amdgcn_exp2f((z[r] - m_b) * kL2e);
          }
          acc[r] = __builtin_fmaf(pw, g, acc[r]);
        }
      }
    }
  }
  if (want_grad) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int c = r * kWave + lane;
      if (c < Ctot) d_sem[(size_t)cell * ld_d + c] = acc[r];     // one store per element
    }
  }
  if (lane == 0) {
    part[2 * cell + 0] = SW ? sw * ce_sum : ce_sum;
    part[2 * cell + 1] = kd_sum;
  }
}

}  // namespace
}  // namespace ucd

using namespace ucd;

namespace {

// one (loss, loss) pair per low-resolution cell
size_t cell_pairs_bytes(int B, int h, int w) { return B <= 0 || h <= 0 || w <= 0 ? 0 : (size_t)B * h * w * 2 * sizeof(float); }

// what a launch takes from the geometry: the grid, the LDS of the staged rows, the means' divisor, the up-sampling scales
struct GatherLaunch { int cells; size_t lds; float inv_pix, scale_h, scale_w, inv_scale_h, inv_scale_w; };

// The argument rules the two entries share, in the order they always had, under the name of the entry that was called.  ex_rules
// are the rules an entry adds between the sizes and the limits (ucd_seg_losses_gather: seg_ex_check); row_floats is what one of the
// nine staged rows takes at the kernel's strides.
template <typename ExRules>
int gather_prologue(const char* fn, const float* sem_s, int ld_s, const float* sem_t, int ld_t, const int64_t* labels, int B, int H,
                    int W, int h, int w, int Ctot, int K, const float* loss_out, const float* d_sem, int ld_d, const void* workspace,
                    size_t workspace_bytes, ExRules ex_rules, int row_floats, GatherLaunch* g) {
  UCD_REQUIRE(sem_s && labels && loss_out && workspace, UCD_EINVAL, "%s: NULL argument (%s)", fn,
              !sem_s ? "sem_s" : !labels ? "labels" : !loss_out ? "loss_out" : "workspace");
  UCD_REQUIRE(B > 0 && H > 0 && W > 0 && h > 0 && w > 0 && Ctot > 0, UCD_EINVAL,
              "%s: bad sizes (B %d, H %d, W %d, h %d, w %d, Ctot %d must be positive)", fn, B, H, W, h, w, Ctot);
  UCD_REQUIRE(K >= 1 && K <= Ctot, UCD_EINVAL, "%s: bad sizes (K = %d is outside [1, Ctot = %d])", fn, K, Ctot);
  UCD_REQUIRE(ld_s >= Ctot, UCD_EINVAL, "%s: bad leading dimension (ld_s = %d below Ctot = %d)", fn, ld_s, Ctot);
  UCD_REQUIRE(!sem_t || ld_t >= K, UCD_EINVAL, "%s: bad leading dimension (ld_t = %d below K = %d)", fn, ld_t, K);
  UCD_REQUIRE(!d_sem || ld_d >= Ctot, UCD_EINVAL, "%s: bad leading dimension (ld_d = %d below Ctot = %d)", fn, ld_d, Ctot);
  UCD_REQUIRE(H >= h && W >= w, UCD_EINVAL, "%s: bad scale (the label map H x W = %d x %d is smaller than the logits h x w = %d x %d)", fn,
              H, W, h, w);
  const int rc = ex_rules();
  if (rc) return rc;
  UCD_REQUIRE((long long)B * h * w <= 0x3fffffffLL, UCD_EINVAL, "%s: %lld low-resolution cells exceed the grid", fn, (long long)B * h * w);
  UCD_REQUIRE(workspace_bytes >= cell_pairs_bytes(B, h, w), UCD_EWORKSPACE, "%s: workspace too small (workspace_bytes = %zu, %zu needed)",
              fn, workspace_bytes, cell_pairs_bytes(B, h, w));
  const size_t lds = (size_t)9 * row_floats * sizeof(float);
  UCD_REQUIRE(lds <= 64 * 1024, UCD_EUNSUPPORTED,
              "%s: the 3 x 3 neighbourhood of a cell takes %zu bytes of LDS for %d + %d classes, over the 65536 the gather form has", fn,
              lds, Ctot, sem_t ? K : 0);
  // torch computes the up-sampling scale as float(in) / out
  *g = {B * h * w, lds, 1.f / ((float)B * H * W), (float)h / (float)H, (float)w / (float)W, (float)H / (float)h, (float)W / (float)w};
  return 0;
}

}  // namespace

extern "C" {

size_t ucd_seg_bce_workspace_bytes(int B, int h, int w) { return cell_pairs_bytes(B, h, w); }
size_t ucd_seg_losses_gather_workspace_bytes(int B, int h, int w) { return cell_pairs_bytes(B, h, w); }

int ucd_seg_bce(const float* sem_s, int ld_s, const float* sem_t, int ld_t, const int64_t* labels, int B, int H, int W, int h,
                int w, int Ctot, int K, int ignore_index, float hard_weight, float soft_weight, float* loss_out, float* d_sem,
                int ld_d, void* workspace, size_t workspace_bytes, ucd_stream_t stream) {
  static const char* fn = "ucd_seg_bce";
  GatherLaunch g;
  int rc = gather_prologue(fn, sem_s, ld_s, sem_t, ld_t, labels, B, H, W, h, w, Ctot, K, loss_out, d_sem, ld_d, workspace, workspace_bytes,
                           [] { return 0; }, (Ctot | 1) + (sem_t ? (K | 1) : 0), &g);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)workspace;
  seg_bce_kernel<<<g.cells, kWave, g.lds, s>>>(sem_s, ld_s, sem_t, ld_t, labels, H, W, h, w, Ctot, K, ignore_index, g.scale_h, g.scale_w,
                                               g.inv_scale_h, g.inv_scale_w, hard_weight * g.inv_pix, soft_weight * g.inv_pix, part,
                                               d_sem, ld_d);
  rc = check_launch(fn);
  return rc ? rc : seg_pair_reduce(fn, part, g.cells, g.inv_pix, loss_out, s);
}

}  // extern "C"

namespace {

// ucd_seg_losses_gather and ucd_seg_losses_gather_w: one body under the name of the entry that was called; ce_sw NULL: no weight
int seg_losses_gather_impl(const char* fn, const float* sem_s, int ld_s, const float* sem_t, int ld_t, const int64_t* labels, int B, int H,
                           int W, int h, int w, int Ctot, int K, int ce_old_cl, int kd_mode, float alpha, int ignore_index,
                           float ce_weight, float kd_weight, const float* ce_sw, float* loss_out, float* d_sem, int ld_d, void* workspace,
                           size_t workspace_bytes, ucd_stream_t stream, bool focal = false, float fo_gamma = 0.f, float fo_alpha = 1.f) {
  GatherLaunch g;
  int rc = gather_prologue(fn, sem_s, ld_s, sem_t, ld_t, labels, B, H, W, h, w, Ctot, K, loss_out, d_sem, ld_d, workspace, workspace_bytes,
                           [&] { return seg_ex_check(fn, Ctot, K, ce_old_cl, kd_mode, alpha, sem_t != nullptr); },
                           Ctot + (sem_t ? K : 0), &g);
  if (rc) return rc;
  // without a teacher the only class split is the cross entropy's (as seg_losses_impl)
  if (!sem_t) K = ce_old_cl;
  hipStream_t s = (hipStream_t)stream;
  const int kd_plain = kd_mode == UCD_KD_PLAIN;
  float* part = (float*)workspace;
#define UCD_SEG_GATHER_SW(NR, SW, FO)                                                                                                    \
  seg_losses_gather_kernel<NR, SW, FO><<<g.cells, kWave, g.lds, s>>>(sem_s, ld_s, sem_t, ld_t, labels, H, W, h, w, Ctot, K, ignore_index, \
                                                                    g.scale_h, g.scale_w, g.inv_scale_h, g.inv_scale_w,                  \
                                                                    ce_weight * g.inv_pix, kd_weight * g.inv_pix, part, d_sem, ld_d,     \
                                                                    ce_old_cl, kd_plain, alpha, ce_sw, fo_gamma, fo_alpha)
  // the focal kernels are instantiations of their own, as the weighted ones are
#define UCD_SEG_GATHER(NR)                              \
  do {                                                  \
    if (focal) UCD_SEG_GATHER_SW(NR, true, true);       \
    else if (ce_sw) UCD_SEG_GATHER_SW(NR, true, false); \
    else UCD_SEG_GATHER_SW(NR, false, false);           \
  } while (0)
  const int rounds = ceil_div(Ctot, kWave);           // 64 KB of LDS hold 1820 classes: at most 29 rounds
  if (rounds <= 1) UCD_SEG_GATHER(1);
  else if (rounds <= 2) UCD_SEG_GATHER(2);
  else if (rounds <= 3) UCD_SEG_GATHER(3);
  else if (rounds <= 8) UCD_SEG_GATHER(8);
  else UCD_SEG_GATHER(29);
#undef UCD_SEG_GATHER
#undef UCD_SEG_GATHER_SW
  rc = check_launch(fn);
  return rc ? rc : seg_pair_reduce(fn, part, g.cells, g.inv_pix, loss_out, s);
}

}  // namespace

extern "C" {

int ucd_seg_losses_gather(const float* sem_s, int ld_s, const float* sem_t, int ld_t, const int64_t* labels, int B, int H, int W,
                          int h, int w, int Ctot, int K, int ce_old_cl, int kd_mode, float alpha, int ignore_index, float ce_weight,
                          float kd_weight, float* loss_out, float* d_sem, int ld_d, void* workspace, size_t workspace_bytes,
                          ucd_stream_t stream) {
  return seg_losses_gather_impl("ucd_seg_losses_gather", sem_s, ld_s, sem_t, ld_t, labels, B, H, W, h, w, Ctot, K, ce_old_cl, kd_mode,
                                alpha, ignore_index, ce_weight, kd_weight, nullptr, loss_out, d_sem, ld_d, workspace, workspace_bytes,
                                stream);
}

int ucd_seg_losses_gather_w(const float* sem_s, int ld_s, const float* sem_t, int ld_t, const int64_t* labels, int B, int H, int W,
                            int h, int w, int Ctot, int K, int ce_old_cl, int kd_mode, float alpha, int ignore_index, float ce_weight,
                            float kd_weight, const float* ce_sample_weight, float* loss_out, float* d_sem, int ld_d, void* workspace,
                            size_t workspace_bytes, ucd_stream_t stream) {
  return seg_losses_gather_impl("ucd_seg_losses_gather_w", sem_s, ld_s, sem_t, ld_t, labels, B, H, W, h, w, Ctot, K, ce_old_cl,
                                kd_mode, alpha, ignore_index, ce_weight, kd_weight, ce_sample_weight, loss_out, d_sem, ld_d, workspace,
                                workspace_bytes, stream);
}

int ucd_seg_losses_gather_focal(const float* sem_s, int ld_s, const float* sem_t, int ld_t, const int64_t* labels, int B, int H, int W,
                                int h, int w, int Ctot, int K, int ce_old_cl, int kd_mode, float alpha, int ignore_index, float ce_weight,
                                float kd_weight, const float* ce_sample_weight, float focal_gamma, float focal_alpha, float* loss_out,
                                float* d_sem, int ld_d, void* workspace, size_t workspace_bytes, ucd_stream_t stream) {
  static const char* fn = "ucd_seg_losses_gather_focal";
  const int rc = seg_focal_check(fn, focal_gamma, focal_alpha);
  if (rc) return rc;
  // gamma 0 at alpha 1 is no modulation: the launch, and the bits, of the call without focal
  const bool focal = !(focal_gamma == 0.f && focal_alpha == 1.f);
  return seg_losses_gather_impl(fn, sem_s, ld_s, sem_t, ld_t, labels, B, H, W, h, w, Ctot, K, ce_old_cl, kd_mode, alpha, ignore_index,
                                ce_weight, kd_weight, ce_sample_weight, loss_out, d_sem, ld_d, workspace, workspace_bytes, stream, focal,
                                focal_gamma, focal_alpha);
}

}  // extern "C"
