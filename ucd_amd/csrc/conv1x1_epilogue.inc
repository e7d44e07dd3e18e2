// Output side of the GEMM kernels of conv1x1.hip (OUT 0 .. 4), included TEXTUALLY into each kernel body (a function call, even
// force-inlined, changed the register allocation of the single-stage forms: +32 B of scratch per lane).  Expects in scope:
// BN, OUT, TN, WN (constexpr), p (Args), acc[2][TN], smem, tm, m0, n0, tid, lane, wm, wn; kThreads = the 256 threads that hold the
// 2 x 2 wave tiles.  Every __syncthreads() here is matched by kEpilogueBarriers<OUT> barriers in waves that only load.
// UCD_EPI_ACTIVE (default: true) - kernels whose MFMA waves outnumber the 256 epilogue threads define it as (tid < kThreads): the
// other threads then only put their accumulators into LDS and keep the barriers.  UCD_EPI_TILE_OK (default: true) - whether this
// 128-row tile has a row in the per-tile partial buffers (a 256-row workgroup tile's second half may lie past M).
#ifndef UCD_EPI_ACTIVE
#define UCD_EPI_ACTIVE true
#define UCD_EPI_ACTIVE_DEFAULTED
#endif
#ifndef UCD_EPI_TILE_OK
#define UCD_EPI_TILE_OK true
#define UCD_EPI_TILE_OK_DEFAULTED
#endif
// UCD_EPI_THREADS (default: kThreads = 256) / UCD_EPI_HALVES (default: 2) - the 64-row workgroup tiles of round 6 (two MFMA waves,
// one 64-row half): 128 epilogue threads, one pass.  kEpilogueBarriersH<OUT, halves> counts the barriers either way.
// UCD_EPI_ROW(r) (default: r) - the row of Y (and of the old y that OUT 0 accumulates into) that GEMM row r of the tile belongs to
// (a kernel that maps rows has OUT == 0: the only side input is that old y).
#ifndef UCD_EPI_ROW
#define UCD_EPI_ROW(r) (r)
#endif
#ifndef UCD_EPI_THREADS
#define UCD_EPI_THREADS kThreads
#define UCD_EPI_HALVES 2
#define UCD_EPI_THREADS_DEFAULTED
#endif
  constexpr int CP = BN + 4;           // fp32 pitch of the (half) output tile in LDS
  float* Cs = reinterpret_cast<float*>(smem);          // [64][CP] per epilogue half
  // ---- epilogue: accumulators -> LDS (fp32, [row][col], 64 rows at a time) -> row-contiguous 16-byte global accesses --
  constexpr int CPR = BN / 8;                       // 8-column chunks per row
  constexpr int RPT = 64 * CPR / (UCD_EPI_THREADS); // rows per thread and half (4 for BN = 128, 2 for BN = 64)
  constexpr int RSTEP = (UCD_EPI_THREADS) / CPR;    // row stride between a thread's chunks
  const int c8 = tid % CPR, r0 = tid / CPR;
  const int ncol = n0 + c8 * 8;
  // the row loop below runs on float PAIRS (common.h: Pack8 - packed-fp32 instructions, one v_cvt_pk_bf16_f32 per pair): written
  // per element it was ~15 VALU instructions per value and the slowest phase of the short-K products (profiles/r04_conv1x1_timeline.txt)
  Pack8 em, es, eb, ei;
  if (OUT == 3) {
    em = load_f8(p.out_mean + ncol);
    es = load_f8(p.out_scale + ncol);
    eb = load_f8(p.out_shift + ncol);
    ei = load_f8(p.out_invstd + ncol);
  }
  // OUT == 1 (frozen statistics: the teacher's layers, round 6): the affine part (acc - mean) * scale + shift is applied to the
  // accumulators IN REGISTERS on their way into LDS - a lane of the MFMA layout holds ONE output column per 32-wide tile, so it
  // needs 3 TN per-channel constants instead of the 24 registers of three 8-channel vectors in the row loop below (the form ran
  // at its 128-register cap with 12 - 16 B of scratch per lane; same operations on the same values: bit-identical results)
  float am[OUT == 1 ? TN : 1], as_[OUT == 1 ? TN : 1], ab[OUT == 1 ? TN : 1];
  if (OUT == 1) {
#pragma unroll
    for (int b = 0; b < TN; ++b) {
      const int col = n0 + wn * WN + b * 32 + (lane & 31);
      am[b] = p.out_mean[col];
      as_[b] = p.out_scale[col];
      ab[b] = p.out_shift[col];
    }
  }
  if (OUT == 4) {
    em = load_f8(p.out_mean + ncol);
    ei = load_f8(p.out_invstd + ncol);
  }
  Pack8 kshift, s1, s2;
#pragma unroll
  for (int j = 0; j < 4; ++j) { kshift.p[j] = f32x2{0.f, 0.f}; s1.p[j] = f32x2{0.f, 0.f}; s2.p[j] = f32x2{0.f, 0.f}; }
  const bool has_side = ((OUT == 0 || OUT == 4) && p.accumulate) || (OUT == 1 && p.R != nullptr) || OUT == 3;
  const bf16* sp = (OUT == 0 || OUT == 4) ? p.Y : p.R;
  const int lds_ = (OUT == 0 || OUT == 4) ? p.ldy : p.ldr;
#pragma unroll
  for (int half = 0; half < (UCD_EPI_HALVES); ++half) {
    // side input (residual / old y / x) of this half's rows: requested before the LDS round trip, rows past M clamped
    uint4 side[RPT], side_y[OUT == 4 ? RPT : 1], side_z[OUT == 4 ? RPT : 1];
    if (has_side && UCD_EPI_ACTIVE) {
#pragma unroll
      for (int i = 0; i < RPT; ++i)
        side[i] = *reinterpret_cast<const uint4*>(sp + (size_t)UCD_EPI_ROW(min(m0 + half * 64 + r0 + RSTEP * i, p.M - 1)) * lds_ + ncol);
    }
    if (OUT == 4) {
#pragma unroll
      for (int i = 0; i < RPT; ++i) {
        const size_t row = (size_t)min(m0 + half * 64 + r0 + RSTEP * i, p.M - 1);
        side_y[i] = *reinterpret_cast<const uint4*>(p.R + row * p.ldr + ncol);
        side_z[i] = *reinterpret_cast<const uint4*>(p.Z + row * p.ldz + ncol);
      }
    }
    __syncthreads();                                  // main loop reads / previous half's reads are done
    if (wm == half) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            Cs[row * CP + wn * WN + b * 32 + (lane & 31)] =
                OUT == 1 ? (acc[a][b][r] - am[OUT == 1 ? b : 0]) * as_[OUT == 1 ? b : 0] + ab[OUT == 1 ? b : 0] : acc[a][b][r];
          }
    }
    __syncthreads();
    if (OUT == 2 && half == 0 && p.stat_acc) {
      kshift = load_f8(p.stat_shift + ncol);   // atomic mode: one shift for every tile (the caller's estimate of the channel mean)
    } else if (OUT == 2 && half == 0) {   // shift = the tile's first row (rounded like the stored value): sums of small numbers
      const float4 k0 = *reinterpret_cast<const float4*>(Cs + c8 * 8), k1 = *reinterpret_cast<const float4*>(Cs + c8 * 8 + 4);
      Pack8 kf;
      kf.p[0] = f32x2{k0.x, k0.y}; kf.p[1] = f32x2{k0.z, k0.w}; kf.p[2] = f32x2{k1.x, k1.y}; kf.p[3] = f32x2{k1.z, k1.w};
      kshift = unpack8(pack8(kf));
    }
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int row = r0 + RSTEP * i;
      const int grow = m0 + half * 64 + row;
      const bool live = grow < p.M && UCD_EPI_ACTIVE;
      const float4 v0 = *reinterpret_cast<const float4*>(Cs + row * CP + c8 * 8);
      const float4 v1 = *reinterpret_cast<const float4*>(Cs + row * CP + c8 * 8 + 4);
      Pack8 v, o;
      v.p[0] = f32x2{v0.x, v0.y}; v.p[1] = f32x2{v0.z, v0.w}; v.p[2] = f32x2{v1.x, v1.y}; v.p[3] = f32x2{v1.z, v1.w};
      uint4 packed;
      if (OUT == 0) {
        if (p.accumulate) {
          const Pack8 sv = unpack8(side[i]);
#pragma unroll
          for (int j = 0; j < 4; ++j) v.p[j] += sv.p[j];
        }
        packed = pack8(v);
      } else if (OUT == 1) {
        // per element: this form (frozen statistics + residual: the teacher's layers) measured FASTER than the pair form at four
        // workgroups per CU (256 -> 1024 at M = 26 136: 31.9 vs 35.3 us; the pair form needs 134 registers against the cap of 128)
        Vec<bf16> ov, sv;
        sv.raw = side[i];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float z = v.p[e >> 1][e & 1];                 // the affine part was applied on the way into LDS (above)
          if (p.R) z += sv.get(e);
          ov.set(e, act_rt(z, p.out_slope));
        }
        packed = ov.raw;
      } else if (OUT == 2) {
        packed = pack8(v);
        if (live) {
          const Pack8 q = unpack8(packed);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const f32x2 d = q.p[j] - kshift.p[j];
            s1.p[j] += d;
            s2.p[j] += d * d;
          }
        }
      } else if (OUT == 3) {  // v = d a', x = the fused layer's pre-norm input
        const Pack8 sv = unpack8(side[i]);
        Pack8 xc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          xc.p[j] = sv.p[j] - em.p[j];
          o.p[j] = leaky_grad2(v.p[j], xc.p[j] * es.p[j] + eb.p[j], p.out_slope);
        }
        packed = pack8(o);
        if (live) {   // the stored (rounded) value is what the apply pass will read
          const Pack8 q = unpack8(packed);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            s1.p[j] += q.p[j];
            s2.p[j] += q.p[j] * (xc.p[j] * ei.p[j]);
          }
        }
      } else {  // OUT == 4: v (+ the shortcut's gradient) = d out of a residual block; sign from its output, x-hat from its z
        const Pack8 yv = unpack8(side_y[OUT == 4 ? i : 0]), zv = unpack8(side_z[OUT == 4 ? i : 0]);
        if (p.accumulate) {
          const Pack8 sv = unpack8(side[i]);
#pragma unroll
          for (int j = 0; j < 4; ++j) v.p[j] += sv.p[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) o.p[j] = leaky_grad2(v.p[j], yv.p[j], p.out_slope);
        packed = pack8(o);
        if (live) {
          const Pack8 q = unpack8(packed);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            s1.p[j] += q.p[j];
            s2.p[j] += q.p[j] * ((zv.p[j] - em.p[j]) * ei.p[j]);
          }
        }
      }
      if (live) *reinterpret_cast<uint4*>(p.Y + (size_t)UCD_EPI_ROW(grow) * p.ldy + ncol) = packed;
    }
  }
  if (OUT >= 2) {
    // reduce over the RSTEP threads that share a column chunk: through LDS (the output tile is consumed)
    __syncthreads();
    float* red = Cs;                                  // [RSTEP][2][BN]
    if (UCD_EPI_ACTIVE) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        *reinterpret_cast<f32x2*>(red + (r0 * 2 + 0) * BN + c8 * 8 + 2 * j) = s1.p[j];
        *reinterpret_cast<f32x2*>(red + (r0 * 2 + 1) * BN + c8 * 8 + 2 * j) = s2.p[j];
      }
    }
    __syncthreads();
    if (tid < 2 * BN && UCD_EPI_TILE_OK) {
      const int which = tid / BN, col = tid % BN;
      float t = 0.f;
#pragma unroll 8
      for (int q = 0; q < RSTEP; ++q) t += red[(q * 2 + which) * BN + col];
      if (p.stat_acc) {
        // one accumulator per layer: 2 N floats that every row tile adds to (no-return atomics, executed at the memory side)
        const size_t ro = (size_t)(tm & (p.stat_rep - 1)) * 2 * p.N;      // this tile's replica
        atomicAdd(p.stat_acc + ro + which * p.N + n0 + col, t);
        if (p.stat_acc2) atomicAdd(p.stat_acc2 + ro + which * p.N + n0 + col, t);
      } else if (OUT == 2) {
        float* dst = p.partial + (size_t)tm * 3 * p.N + n0 + col;
        dst[(1 + which) * p.N] = t;
      } else {
        p.partial[(size_t)tm * 2 * p.N + which * p.N + n0 + col] = t;
      }
    }
    if (OUT == 2 && p.stat_acc) {
      if (tm == 0 && r0 == 0 && UCD_EPI_TILE_OK) {   // the snapshot of the shift (partial[0 .. N)) the finalising apply pass reads
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x2*>(p.partial + ncol + 2 * j) = kshift.p[j];
      }
    } else if (OUT == 2 && r0 == 0 && UCD_EPI_TILE_OK) {
#pragma unroll
      for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x2*>(p.partial + (size_t)tm * 3 * p.N + ncol + 2 * j) = kshift.p[j];
    }
  }
#ifdef UCD_EPI_ACTIVE_DEFAULTED
#undef UCD_EPI_ACTIVE
#undef UCD_EPI_ACTIVE_DEFAULTED
#endif
#ifdef UCD_EPI_TILE_OK_DEFAULTED
#undef UCD_EPI_TILE_OK
#undef UCD_EPI_TILE_OK_DEFAULTED
#endif
#ifdef UCD_EPI_THREADS_DEFAULTED
#undef UCD_EPI_THREADS
#undef UCD_EPI_HALVES
#undef UCD_EPI_THREADS_DEFAULTED
#endif
