// PixelConLossV2 streaming kernels, fp16-operand path, FIXED-SPLIT form: every anchor block sweeps all contrast tiles in
// `nsplit` equal column ranges.  UCD_PIXCON_F16 runs the planned form (pixcon_loss_f16p.hip: device-built unit lists,
// pure-positive tiles skipped, pinned MFMA / LDS / VALU interleave) where it applies - T >= 0.06, at most 32 teacher
// classes, fewer than 1024 anchor blocks - and falls back to this file otherwise; UCD_PIXCON_F16_SPLIT selects this
// file explicitly (the A/B reference of the tests).
//
// Same two-sweep structure and the same math as pixcon_loss.hip (see the derivation there); what changes
// is the arithmetic of the two GEMM pairs: v_mfma_f32_32x32x16_f16 (16x the fp32-MFMA rate) with fp32
// accumulation.  Why fp16 and not bf16: the operands are L2-normalised rows (|x| <= 1), so fp16's
// 11-bit mantissa costs ~3e-4 absolute on S = cos/T where bf16 costs ~2.5e-3 - inside exp() that is the
// difference between meeting and missing the 1e-3 contract.
//
//   sweep 1, per 32x32 tile and wave:  16 MFMA  X = S^T tile (contrast rows x anchors)
//                                     epilogue  s2 = X*log2(e)/T; E = exp2(s2 - m_run)[negative]
//                                     16 MFMA  U^T += C_j^T . E
//   E must fit fp16: an online, thresholded running maximum m_run of the NEGATIVE logits per anchor keeps
//   E <= 2^8; when a tile raises the maximum by more than 2^8 the anchor's accumulators are rescaled
//   (flash-attention style).  Every lane owns one anchor, so the maximum, the rescale factor and the sums
//   are per-lane scalars - the only cross-lane traffic is one shfl_xor(32) per tile.
//   The E tile never leaves registers: accumulator registers 8s..8s+7 converted to fp16 are the B operand
//   of k-step s of the second GEMM; the matching A operand (C_j^T, k order permuted the same way) is
//   fetched with ds_read_b64_tr_b16 from the row-major LDS tile (hardware transpose, 4 rows x 16 columns
//   per 16-lane group).
//   Teacher joint probabilities P = p_i . p_j use a hi/lo fp16 split (3 MFMAs per 16 classes, ~2^-21).
//
// Shared: geometry, split count, workspace layout (SplitLayout with mrun) and the combine kernel (per-slot mrun scale) in
// pixcon_tiles.h; the tile staging and the MFMA fragment helpers in pixcon_f16_tiles.h.
#include "pixcon_f16_tiles.h"

namespace ucd {
namespace {

// ---- sweep 1 --------------------------------------------------------------------------------------------
// Software pipeline over the contrast tiles of one split (t = tile index), three LDS buffers:
//   block A:  x_next = S^T(tile t+1)   [16 MFMA + 16 ds_read_b128]   ||   s2 / masks / tile max of tile t  [VALU]
//   (rare, wave-uniform) rescale when the running negative maximum jumps by more than 2^8
//   block B:  E = exp2(s2 - m_run), row sums, fp16 pack [VALU]  ->  U^T += C_t^T . E   [16 MFMA + 32 tr reads]
//   commit tile t+2 (fetched into registers at the top) to the third buffer; one barrier per tile.
// The MFMAs of block A and the VALU work on the previous tile are independent, so the scheduler interleaves
// them in one basic block.
struct EpiA {
  float tmax, mx_all;
};

template <bool PURE_NEG>
__device__ __forceinline__ void epilogue_a(f32x16& x, const int* __restrict__ labs, int la, int half, float k2, float& tmax,
                                           float& mx_all) {
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const float s2 = x[reg] * k2;
    if (PURE_NEG) {  // every row of the tile is a valid negative for every anchor of this wave
      mx_all = fmaxf(mx_all, s2);
      tmax = fmaxf(tmax, s2);
      x[reg] = s2;
    } else {
      const int lc = labs[tile_row(reg, half)];
      const bool valid = lc != kPadLabel;
      mx_all = valid ? fmaxf(mx_all, s2) : mx_all;
      const float sn = (valid && lc != la) ? s2 : -INFINITY;
      tmax = fmaxf(tmax, sn);
      x[reg] = sn;
    }
  }
}

// FIXED: the rows are L2-normalised, so s2 = cos * log2(e)/T is bounded by k2 and a constant shift m = k2 - 14.5 keeps
// E = exp2(s2 - m) below 2^15 (fp16 range) for EVERY pair, with full fp16 precision down to cos = 1 - 28.5/k2 (-0.38
// at T = 0.07; smaller terms are below 2^-28 of the row's self term).  No running maximum, no conditional rescale -
// and therefore no VALU instruction that touches the 128 accumulator registers inside the loop: with the rescale
// branch present the register allocator moves all of them AGPR -> VGPR -> AGPR every iteration (~400 v_accvgpr_*
// per tile).  Used when k2 <= kFixedShiftMaxK2 (T >= 0.06); the running-maximum form stays for sharper temperatures.
template <bool FIXED>
__global__ __launch_bounds__(kThreads, 1) void pixcon16_neg_kernel(const _Float16* ch16, const uint8_t* row_label,
                                                                  const ucd_pixcon_meta* __restrict__ meta, float k2,
                                                                  int nsplit, int maxA, float* __restrict__ negp,
                                                                  float* __restrict__ mrunp, float* __restrict__ maxp,
                                                                  float* __restrict__ Up) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  _Float16* cs0 = reinterpret_cast<_Float16*>(smem_raw);                       // [3][32][kPitchH]
  int* labs0 = reinterpret_cast<int*>(smem_raw + 3 * kTJ * kPitchH * 2);       // [3][32 labels + min + max]
  constexpr int kLabStride = kTJ + 4;
  const int A = meta->A, Cpad = meta->Cpad;
  const int i_base = blockIdx.x * kBI;
  if (i_base >= A) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5;
  const int i_row = i_base + wave * kTI + (lane & 31);
  const bool row_ok = i_row < A;
  const bool wave_ok = i_base + wave * kTI < A;
  const int la = row_ok ? row_label[i_row] : -1;
  // label range of this wave's anchors (for the pure-negative fast path)
  int w_lo = row_ok ? la : 255, w_hi = row_ok ? la : -1;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    w_lo = min(w_lo, __shfl_xor(w_lo, off, 64));
    w_hi = max(w_hi, __shfl_xor(w_hi, off, 64));
  }
  const int ntiles = Cpad / kTJ;
  const int per = (ntiles + nsplit - 1) / nsplit;
  const int v_begin = blockIdx.y * per, v_end = min(ntiles, v_begin + per);
  const int nt_loc = v_end - v_begin;

  f16x8 a16[16];
  load_anchor_frags(a16, ch16, i_row, row_ok, half);
  f32x16 U[8];
#pragma unroll
  for (int nt = 0; nt < 8; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) U[nt][r] = 0.f;
  float neg = 0.f, m_run = FIXED ? k2 - 14.5f : -1e30f, mx_all = -INFINITY;

  auto commit_labels = [&](int buf, unsigned lab_byte) {
    if (threadIdx.x < 64) {   // wave 0: 32 labels + their min / max over the valid rows
      const int lc = threadIdx.x < kTJ ? (int)lab_byte : kPadLabel;
      int lo = lc == kPadLabel ? 256 : lc, hi = lc == kPadLabel ? 256 : lc;   // a padding row forces the slow path
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off, 64));
        hi = max(hi, __shfl_xor(hi, off, 64));
      }
      if (threadIdx.x < kTJ) labs0[buf * kLabStride + threadIdx.x] = lc;
      if (threadIdx.x == 0) { labs0[buf * kLabStride + kTJ] = lo; labs0[buf * kLabStride + kTJ + 1] = hi; }
    }
  };

  Stage stage;
  if (nt_loc > 0) {
    tile_fetch(stage, ch16, row_label, v_begin * kTJ);
    tile_commit(stage, cs0);
    commit_labels(0, stage.lab);
  }
  if (nt_loc > 1) {
    tile_fetch(stage, ch16, row_label, (v_begin + 1) * kTJ);
    tile_commit(stage, cs0 + kTJ * kPitchH);
    commit_labels(1, stage.lab);
  }
  __syncthreads();
  f32x16 x_cur;
  if (nt_loc > 0 && wave_ok) x_cur = gemm_scores(cs0, a16, lane);
  // unrolled by the three LDS buffers: buffer indices are compile-time constants, so every LDS address of a step is a
  // per-lane base plus an immediate offset (a rotating index costs ~100 address VALU instructions per tile)
  auto step = [&](auto bc_tag, int t) {
    constexpr int b_cur = decltype(bc_tag)::value, b_nxt = (b_cur + 1) % 3, b_new = (b_cur + 2) % 3;
    // unconditional (clamped) prefetch two tiles ahead: no branch inside the pipelined body; past the end it
    // re-fetches the last tile into a slot nobody reads again
    const int t_new = min(v_begin + t + 2, v_end - 1);
    tile_fetch(stage, ch16, row_label, t_new * kTJ);
    fetch_fence();
    const _Float16* cs = cs0 + b_cur * kTJ * kPitchH;
    const int* labs = labs0 + b_cur * kLabStride;
    if (wave_ok) {
      // ---- all LDS reads of the step, then block A
      ScoreFrags sf;
      ValueFrags vf;
      load_score_frags(sf, cs0 + b_nxt * kTJ * kPitchH, lane);   // past the last tile: stale rows, result unused
      if (FIXED) load_value_frags(vf, cs, lane);   // the running-maximum form has no registers to spare for them yet
      __builtin_amdgcn_sched_barrier(0);
      f32x16 x_next = mfma_scores(sf, a16);
      float tmax = -INFINITY;
      // wave-uniform (LDS broadcast values); hi == 256 marks a tile with padding rows
      const bool pure = labs[kTJ + 1] < 256 && (labs[kTJ] > w_hi || labs[kTJ + 1] < w_lo);
      if (pure) epilogue_a<true>(x_cur, labs, la, half, k2, tmax, mx_all);
      else epilogue_a<false>(x_cur, labs, la, half, k2, tmax, mx_all);
      if (!FIXED) {
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float m_new = tmax > m_run + kRescaleTh ? tmax : m_run;
        if (__any(m_new != m_run)) {   // rare: lanes that keep their maximum scale by 1
          const float sc = __builtin_amdgcn_exp2f(m_run - m_new);
          neg *= sc;
#pragma unroll
          for (int nt = 0; nt < 8; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) U[nt][r] *= sc;
          m_run = m_new;
        }
      }
      // ---- block B
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const float e = __builtin_amdgcn_exp2f(x_cur[reg] - m_run);   // exp2(-inf) = 0 for masked entries
        neg += e;
        x_cur[reg] = e;
      }
      if (FIXED) mfma_values(U, vf, x_cur);
      else gemm_values(U, cs, x_cur, lane);
      x_cur = x_next;
    }
    // keep the loop-carried accumulators in the AGPR half of the register file (the allocator otherwise parks other
    // values there and moves the accumulators in and out around them)
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) asm volatile("" : "+a"(U[nt]));
    tile_commit(stage, cs0 + b_new * kTJ * kPitchH);
    commit_labels(b_new, stage.lab);
    __syncthreads();
  };
  for (int t = 0; t < nt_loc; t += 3) {
    step(std::integral_constant<int, 0>{}, t);
    if (t + 1 < nt_loc) step(std::integral_constant<int, 1>{}, t + 1);
    if (t + 2 < nt_loc) step(std::integral_constant<int, 2>{}, t + 2);
  }
  neg += __shfl_xor(neg, 32, 64);
  mx_all = fmaxf(mx_all, __shfl_xor(mx_all, 32, 64));
  if (row_ok) {
    if (half == 0) {
      const size_t o = (size_t)blockIdx.y * maxA + i_row;
      negp[o] = neg;       // in units of 2^m_run
      mrunp[o] = m_run;    // log2 domain
      maxp[o] = mx_all;    // log2 domain
    }
    store_values(U, Up + ((size_t)blockIdx.y * maxA + i_row) * kN, half);
  }
}

// ---- sweep 2 --------------------------------------------------------------------------------------------
// p16: [Cpad][2][KP16] halfs (hi then lo) ; KP16 = K rounded up to 16
__global__ __launch_bounds__(kThreads, 1) void pixcon16_pos_kernel(
    const _Float16* ch16, const uint8_t* row_label, const _Float16* p16, int KP16,
    const ucd_pixcon_meta* __restrict__ meta, float k2, int shift_pos, int use_prob, int nsplit1, int nsplit2, int maxA,
    const float* __restrict__ negp, const float* __restrict__ mrunp, const float* __restrict__ maxp,
    float* __restrict__ lossp, float* __restrict__ qsump, float* __restrict__ Vp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int ppitch = 2 * KP16 + 8;                                              // halfs per row: hi | lo | pad
  _Float16* cs0 = reinterpret_cast<_Float16*>(smem_raw);                        // [3][32][kPitchH]
  int* labs0 = reinterpret_cast<int*>(smem_raw + 3 * kTJ * kPitchH * 2);        // [3][32]
  _Float16* ps0 = reinterpret_cast<_Float16*>(smem_raw + 3 * kTJ * kPitchH * 2 + 3 * kTJ * 4);  // [3][32][ppitch]
  const int A = meta->A, Apad = meta->Apad, Cpad = meta->Cpad, min_new = meta->min_new;
  const int i_base = blockIdx.x * kBI;
  if (i_base >= A) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5;
  const int i_row = i_base + wave * kTI + (lane & 31);
  const bool row_ok = i_row < A;
  const int la = row_ok ? row_label[i_row] : -1;
  const bool gt_i = la >= min_new;

  TileList tl;
  if (meta->sorted) {
    const int Lmin = row_label[i_base], Lmax = row_label[min(i_base + kBI, A) - 1];
    const int r1a = meta->label_start_a[Lmin], r1b = meta->label_start_a[Lmax + 1];
    const int r2a = Apad + meta->label_start_o[Lmin], r2b = Apad + meta->label_start_o[Lmax + 1];
    tl.t1a = r1a / kTJ; tl.n1 = (r1b + kTJ - 1) / kTJ - tl.t1a;
    tl.t2a = r2a / kTJ; tl.n2 = r2b > r2a ? (r2b + kTJ - 1) / kTJ - tl.t2a : 0;
  } else {
    tl.t1a = 0; tl.n1 = Cpad / kTJ; tl.t2a = 0; tl.n2 = 0;
  }
  const int nv = tl.count();
  const int per = (nv + nsplit2 - 1) / nsplit2;
  const int v_begin = blockIdx.y * per, v_end = min(nv, v_begin + per);

  // row constants from sweep 1: combine the split partials at a common scale
  float neg_true = 0.f, m2 = -INFINITY;
  if (row_ok) {
    float M = -1e30f;
    for (int s = 0; s < nsplit1; ++s) M = fmaxf(M, mrunp[(size_t)s * maxA + i_row]);
    float acc = 0.f;
    for (int s = 0; s < nsplit1; ++s) {
      acc += negp[(size_t)s * maxA + i_row] * exp2f(mrunp[(size_t)s * maxA + i_row] - M);
      m2 = fmaxf(m2, maxp[(size_t)s * maxA + i_row]);
    }
    neg_true = acc > 0.f ? acc * exp2f(M) : 0.f;
  }
  if (!shift_pos) m2 = 0.f;

  f16x8 a16[16];
  load_anchor_frags(a16, ch16, i_row, row_ok, half);
  f32x16 V[8];
#pragma unroll
  for (int nt = 0; nt < 8; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) V[nt][r] = 0.f;
  float lossacc = 0.f, qsum = 0.f;
  const int nk = KP16 / 16;

  // teacher-probability rows of a tile: 2*KP16 halfs per row = `chunks` 16-byte pieces; when the tile has at most one
  // piece per thread (K <= 32 classes) the piece travels with the tile prefetch, else it is copied at commit time
  const int chunks = use_prob ? (2 * KP16) / 8 : 0;
  const bool side_fast = use_prob && chunks * kTJ <= kThreads;
  const int s_idx = min((int)threadIdx.x, max(kTJ * chunks - 1, 0));
  const int s_row = chunks ? s_idx / chunks : 0, s_c = chunks ? s_idx - s_row * chunks : 0;
  Stage stage;
  auto fetch = [&](int j0) {
    tile_fetch(stage, ch16, row_label, j0);
    if (side_fast) side_fetch(stage, p16 + (size_t)(j0 + s_row) * 2 * KP16 + s_c * 8);
    fetch_fence();
  };
  auto commit = [&](int buf, int j0) {
    tile_commit(stage, cs0 + buf * kTJ * kPitchH);
    if (threadIdx.x < kTJ) labs0[buf * kTJ + threadIdx.x] = (int)stage.lab;
    if (side_fast) {
      if ((int)threadIdx.x < kTJ * chunks)
        *reinterpret_cast<u32x4*>(ps0 + (buf * kTJ + s_row) * ppitch + s_c * 8) = stage.side;
    } else if (use_prob) {
      for (int idx = threadIdx.x; idx < kTJ * chunks; idx += kThreads) {
        const int row = idx / chunks, c = idx - row * chunks;
        *reinterpret_cast<uint4*>(ps0 + (buf * kTJ + row) * ppitch + c * 8) =
            *reinterpret_cast<const uint4*>(p16 + (size_t)(j0 + row) * 2 * KP16 + c * 8);
      }
    }
  };

  // the anchors' own probability fragments do not change over the sweep: loaded once (two 16-class steps cover K <= 32)
  f16x8 pah[2], pal[2];
  {
    const _Float16* pa = p16 + (size_t)(row_ok ? i_row : 0) * 2 * KP16 + 8 * half;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      if (use_prob && kk < nk) {
        pah[kk] = *reinterpret_cast<const f16x8*>(pa + 16 * kk);
        pal[kk] = *reinterpret_cast<const f16x8*>(pa + KP16 + 16 * kk);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) { pah[kk][e] = (_Float16)0.f; pal[kk][e] = (_Float16)0.f; }
      }
    }
  }

  // P^T tile of contrast tile `buf`: pm[j][i] = sum_k pc[j][k] pa[i][k]  (hi/lo split: 3 MFMAs per 16 classes)
  auto prob_tile = [&](int buf) {
    f32x16 pm = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const _Float16* pc = ps0 + (buf * kTJ + (lane & 31)) * ppitch + 8 * half;
    if (nk <= 2) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        if (kk < nk) {
          const f16x8 ch = *reinterpret_cast<const f16x8*>(pc + 16 * kk);
          const f16x8 cl = *reinterpret_cast<const f16x8*>(pc + KP16 + 16 * kk);
          pm = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch, pah[kk], pm, 0, 0, 0);
          pm = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch, pal[kk], pm, 0, 0, 0);
          pm = __builtin_amdgcn_mfma_f32_32x32x16_f16(cl, pah[kk], pm, 0, 0, 0);
        }
      }
      return pm;
    }
    const _Float16* pa = p16 + (size_t)(row_ok ? i_row : 0) * 2 * KP16 + 8 * half;
    for (int kk = 0; kk < nk; ++kk) {
      const f16x8 ch = *reinterpret_cast<const f16x8*>(pc + 16 * kk);
      const f16x8 cl = *reinterpret_cast<const f16x8*>(pc + KP16 + 16 * kk);
      const f16x8 ah = *reinterpret_cast<const f16x8*>(pa + 16 * kk);
      const f16x8 al = *reinterpret_cast<const f16x8*>(pa + KP16 + 16 * kk);
      pm = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch, ah, pm, 0, 0, 0);
      pm = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch, al, pm, 0, 0, 0);
      pm = __builtin_amdgcn_mfma_f32_32x32x16_f16(cl, ah, pm, 0, 0, 0);
    }
    return pm;
  };

  // three-buffer software pipeline (same schedule as sweep 1): scores / probabilities of tile t+1 are issued
  // beside the epilogue of tile t; tile t+2 (rows, labels, probability rows) travels global -> registers -> LDS meanwhile
  const int nt_loc = v_end - v_begin;
  if (nt_loc > 0) {
    const int j0 = tl.at(v_begin) * kTJ;
    fetch(j0);
    commit(0, j0);
  }
  if (nt_loc > 1) {
    const int j0 = tl.at(v_begin + 1) * kTJ;
    fetch(j0);
    commit(1, j0);
  }
  __syncthreads();
  f32x16 x_cur, pm_cur;
  if (nt_loc > 0) {
    x_cur = gemm_scores(cs0, a16, lane);
    if (use_prob) pm_cur = prob_tile(0);
  }
  for (int t = 0; t < nt_loc; ++t) {
    const int b_cur = t % 3, b_nxt = (t + 1) % 3, b_new = (t + 2) % 3;
    const bool has_next = t + 1 < nt_loc;
    const int j0 = tl.at(v_begin + t) * kTJ;
    const int j0n = tl.at(min(v_begin + t + 2, v_end - 1)) * kTJ;
    fetch(j0n);
    const _Float16* cs = cs0 + b_cur * kTJ * kPitchH;
    const int* labs = labs0 + b_cur * kTJ;
    {
      const int bn = has_next ? b_nxt : b_cur;
      int lcs[16];
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) lcs[reg] = labs[tile_row(reg, half)];   // one batch of LDS reads, not 16 round trips
      ScoreFrags sf;
      ValueFrags vf;
      load_score_frags(sf, cs0 + bn * kTJ * kPitchH, lane);
      load_value_frags(vf, cs, lane);
      __builtin_amdgcn_sched_barrier(0);
      f32x16 x_next = mfma_scores(sf, a16);
      f32x16 pm_next;
      if (use_prob) pm_next = prob_tile(bn);
      // branch-free: every element is evaluated, non-positives contribute zero
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int jl = tile_row(reg, half);
        const int lc = lcs[reg];
        const bool pos = row_ok && lc == la && (j0 + jl) != i_row;
        const float pw = (use_prob && !(gt_i && lc >= min_new)) ? pm_cur[reg] : 1.f;
        const float sp2 = x_cur[reg] * k2 - m2;
        const float d = __builtin_amdgcn_exp2f(sp2) + neg_true;
        const float dd = pos ? d : 1.f;                       // keeps log / rcp finite on the unused lanes
        const float term = pw * (sp2 * kLn2 - __logf(dd));
        const float q = pos ? pw * (neg_true * __builtin_amdgcn_rcpf(dd)) : 0.f;
        lossacc += pos ? term : 0.f;
        qsum += q;
        x_cur[reg] = q;
      }
      mfma_values(V, vf, x_cur);
      x_cur = x_next;
      if (use_prob) pm_cur = pm_next;
    }
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) asm volatile("" : "+a"(V[nt]));   // accumulators stay in the AGPR half (see sweep 1)
    commit(b_new, j0n);
    __syncthreads();
  }
  lossacc += __shfl_xor(lossacc, 32, 64);
  qsum += __shfl_xor(qsum, 32, 64);
  if (row_ok) {
    if (half == 0) {
      lossp[(size_t)blockIdx.y * maxA + i_row] = lossacc;
      qsump[(size_t)blockIdx.y * maxA + i_row] = qsum;
    }
    store_values(V, Vp + ((size_t)blockIdx.y * maxA + i_row) * kN, half);
  }
}

}  // namespace

// Plan: the split count and the workspace are the fp32 path's (SplitLayout, pixcon_tiles.h) with the mrun row vector.
// LDS of sweep 2: three contrast tiles + labels + three tiles of probability rows (hi | lo | 8 halfs of padding), i.e.
// 54 144 + 192 (2 KP16 + 8) bytes: 153 984 at KP16 = 256, inside the 160 KiB of a workgroup, so every K <= 255 is served in
// one piece.  The kernel's class loop (nk = KP16 / 16 steps, anchors' fragments from global memory when nk > 2), the commit
// copy (16-byte pieces, KP16 / 4 per row) and the p16 row stride 2 KP16 hold for any multiple of 16.
void pixcon16_plan(int BHW, int KP16, PixconPlan* p) {
  const SplitLayout L(BHW, true);
  p->path = UCD_PIXCON_PATH_F16_SPLIT;
  p->class_chunk = 0;
  p->kp = KP16;
  p->nt_i = L.nt_i;
  p->nsplit1 = p->nsplit2 = L.nsplit;
  p->lds1 = (size_t)3 * kTJ * kPitchH * 2 + 3 * (kTJ + 4) * 4;
  p->lds2 = (size_t)3 * kTJ * kPitchH * 2 + 3 * kTJ * 4 + (size_t)3 * kTJ * (2 * KP16 + 8) * 2;
  p->workspace = L.total;
}

int pixcon16_launch(const _Float16* ch16, const uint8_t* row_label, const _Float16* p16, const ucd_pixcon_meta* meta, int BHW,
                    float temperature, int shift_pos, int use_prob, float* loss_out, float* grad_a, int ldg, float* row_stats,
                    void* workspace, const PixconPlan& p, hipStream_t s) {
  static const char* fn = "ucd_pixcon_loss[f16]";
  const SplitLayout L(BHW, true);
  const int nt_i = p.nt_i, ns = p.nsplit1;
  char* ws = (char*)workspace;
  float* negp = (float*)(ws + L.off_negp);
  float* mrunp = (float*)(ws + L.off_mrunp);
  float* maxp = (float*)(ws + L.off_maxp);
  float* lossp = (float*)(ws + L.off_lossp);
  float* qsump = (float*)(ws + L.off_qsump);
  float* rowloss = (float*)(ws + L.off_rowloss);
  float* Up = (float*)(ws + L.off_Up);
  float* Vp = (float*)(ws + L.off_Vp);
  const float k2 = kLog2e / temperature;
  const int maxA = BHW;
  // opt in to more than 64 KiB of dynamic LDS: per call (the attribute is per device; there is no process-wide state here)
  UCD_TRY_LDS(pixcon16_neg_kernel<true>, 160 * 1024);
  UCD_TRY_LDS(pixcon16_neg_kernel<false>, 160 * 1024);
  UCD_TRY_LDS(pixcon16_pos_kernel, 160 * 1024);
  if (k2 <= kFixedShiftMaxK2)
    pixcon16_neg_kernel<true><<<dim3(nt_i, ns), kThreads, p.lds1, s>>>(ch16, row_label, meta, k2, ns, maxA, negp, mrunp, maxp, Up);
  else
    pixcon16_neg_kernel<false><<<dim3(nt_i, ns), kThreads, p.lds1, s>>>(ch16, row_label, meta, k2, ns, maxA, negp, mrunp, maxp, Up);
  int rc = check_launch(fn);
  if (rc) return rc;
  pixcon16_pos_kernel<<<dim3(nt_i, ns), kThreads, p.lds2, s>>>(ch16, row_label, p16, p.kp, meta, k2, shift_pos, use_prob, ns, ns,
                                                              maxA, negp, mrunp, maxp, lossp, qsump, Vp);
  rc = check_launch(fn);
  if (rc) return rc;
  const SplitSlots<kScaleSlot> slots = {ns, ns, maxA, mrunp};
  pixcon_combine_kernel<<<ceil_div(BHW, kThreads / 64), kThreads, 0, s>>>(slots, row_label, meta, 1.f / temperature, negp, lossp,
                                                                          qsump, Up, Vp, grad_a, ldg, row_stats, maxA, rowloss);
  rc = check_launch(fn);
  if (rc) return rc;
  pixcon_launch_reduce(rowloss, meta, loss_out, s);
  return check_launch(fn);
}

}  // namespace ucd
