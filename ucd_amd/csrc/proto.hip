// SDR's class-prototype feature losses (Michieli and Zanuttigh, CVPR 2021: prototype matching, feature clustering, prototype
// repulsion) on the raw pre-logits X [M = B h w rows][C channels] (channels-last, bf16 or fp32, row pitch >= C), T classes of the
// step, K teacher classes.
//   cls_p   class of a low-resolution pixel: the nearest down-sampled label; -1 where ignored or outside [0, T); with a teacher a
//           background pixel takes the first arg-max of the teacher's row
//   n_c = #{p : cls_p = c},  S_c = sum_{cls_p = c} X_p,  mu_c = S_c / n_c
//   R_c = state_sum_c / state_n_c (the running prototype, valid where state_n_c > 0),  O_c (the previous step's, where valid_c)
//   L_match = 1/|A|  sum_{c in A}  |mu_c - O_c|                                  A  = {c < K : n_c > 0, valid_c}
//   L_attr  = 1/|Bs| sum_{c in Bs} 1/n_c sum_{cls_p = c} |X_p - R_c|^2           Bs = {c : n_c > 0, state_n_c > 0}
//   L_rep   = 1/|P|  sum_{c in P}  sum_{k in P, k != c} 1 / (|mu_c - mu_k| + 1e-6)   P = {c : n_c > 0}; 0 for |P| < 2
//   d_x[p]  = grad_out (a_c (X_p - R_c) + G_c / n_c),  a_c = 2 w_a / (|Bs| n_c),  G_c = d(w_m L_match + w_r L_rep) / d mu_c
//
// Forward, three launches behind the classify launch:
//   accum   the one pass over X.  The rows are cut into pieces of 64.  A group of C / VEC threads owns a piece, a thread one 16-byte
//           channel vector of it (lanes over channels: 16-byte loads, contiguous over the group).  The piece's rows are ordered by
//           class in LDS (a stable rank of 64 keys), so a thread meets each class of the piece as one run of rows: it keeps the
//           run's sum and its sum of (x - R_c)^2 in registers - R_c is known before the pass - and writes them once per run into
//           the piece's slot for that class.  Only the classes present in a piece are written (at most min(64, T), typically 1 - 4);
//           slot_of[c][piece] says where.  No LDS tables, no atomics.
//   class   one workgroup per class adds the piece slots that hold the class, in piece order (the present pieces are compacted in
//           LDS 256 at a time, a group of threads takes every G-th entry, the groups are added in index order): S_c and the squared
//           distances in fp64, n_c in int64, mu_c in fp64.
//   proto   one workgroup per class on [T, C]: R_c, the distances to the old prototype and to every other present mean (fp64, a
//           wave per pair, fixed shuffle order), a_c, G_c / n_c and the class's three partial values; the workgroup that finishes
//           last (an INTEGER ticket) adds the partials in class order and writes the four values.  |A|, |Bs| and |P| are counted
//           on the device by every workgroup for itself.
// Backward, one launch: a thread per row and 16-byte channel vector reads X once, the tables from L2, and writes d_x once.
// Every sum has a fixed order: same inputs, same bits.  Nothing allocates, nothing synchronises with the host.
#include "common.h"

namespace ucd {
namespace {

constexpr int kProtoBlock = 256;
constexpr int kProtoPiece = 64;                 // rows of a piece
constexpr int kProtoMaxGroups = 16;             // pieces of one accum workgroup (a group of C / VEC threads each)
constexpr int kProtoMaxC = 512, kProtoMaxT = 256;
constexpr int kProtoAbsent = 0x7fffffff;        // sort key of a row without a class
constexpr int kProtoPrefetch = 8;               // rows a thread has in flight

// static LDS of the three forward kernels (what ucd_proto_plan reports)
constexpr int kProtoAccumLds = kProtoMaxGroups * kProtoPiece * (4 + 4 + 1) + kProtoMaxGroups * 4 + kProtoMaxGroups * kProtoMaxT * 2;
constexpr int kProtoClassLds = kProtoBlock * 4 + 4 * 4 + 4 * 8 + 4 * 8 + 8 + 1024 * 8;
constexpr int kProtoProtoLds = kProtoMaxT * (4 + 8 + 8) + 4 * 8 + 4 * 4 + 8;

struct ProtoWs {
  size_t piece_s, piece_d, piece_n, slot_of, mu, dsum, part, ticket, bytes;
  int pieces, slots, lanes, groups;
};

// lanes = 16-byte vectors of a row, groups = pieces of one accum workgroup
ProtoWs proto_ws(long long M, int C, int T, int dtype) {
  ProtoWs w;
  w.pieces = (int)((M + kProtoPiece - 1) / kProtoPiece);
  w.slots = T < kProtoPiece ? T : kProtoPiece;
  w.lanes = C / (dtype == UCD_BF16 ? 8 : 4);
  const int g = kProtoBlock / w.lanes;
  w.groups = g > kProtoMaxGroups ? kProtoMaxGroups : g;
  size_t off = 0;
  const size_t cells = (size_t)w.pieces * w.slots;
  w.piece_s = off; off = align_up(off + cells * C * sizeof(float), 16);
  w.piece_d = off; off = align_up(off + cells * w.lanes * sizeof(float), 16);
  w.piece_n = off; off = align_up(off + cells * sizeof(int), 16);
  w.slot_of = off; off = align_up(off + (size_t)T * w.pieces * sizeof(short), 16);
  w.mu = off;      off = align_up(off + (size_t)T * C * sizeof(double), 16);
  w.dsum = off;    off = align_up(off + (size_t)T * sizeof(double), 16);
  w.part = off;    off = align_up(off + (size_t)T * 3 * sizeof(double), 16);
  w.ticket = off;  off += 16;
  w.bytes = off;
  return w;
}

// ---- classify ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kProtoBlock) void proto_classify_kernel(const int64_t* __restrict__ labels, int B, int H, int W, int h, int w,
                                                                    float fy, float fx, int T, int K, int ignore_index,
                                                                    const float* __restrict__ sem_t, int ld_t, int* __restrict__ cls) {
  const int p = blockIdx.x * kProtoBlock + threadIdx.x;
  if (p >= B * h * w) return;
  const int j = p % w, i = (p / w) % h, b = p / (w * h);
  int sy = (int)floorf(i * fy), sx = (int)floorf(j * fx);           // F.interpolate(mode='nearest'): floor(dst * (float)in / out)
  sy = sy < H - 1 ? sy : H - 1;
  sx = sx < W - 1 ? sx : W - 1;
  const int64_t y = labels[((size_t)b * H + sy) * W + sx];
  int c = (y == (int64_t)ignore_index || y < 0 || y >= (int64_t)T) ? -1 : (int)y;
  if (c == 0 && sem_t != nullptr) {
    const float* row = sem_t + (size_t)p * ld_t;
    float best = row[0];
    for (int k = 1; k < K; ++k) {                                    // torch's arg-max: the first maximum, a NaN counts as the largest
      const float v = row[k];
      if (v > best || (v != v && best == best)) { best = v; c = k; }
    }
  }
  cls[p] = c;
}

// ---- accum: the pass over X ----------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kProtoBlock) void proto_accum_kernel(const T* __restrict__ x, int ld, const int* __restrict__ cls, long long M,
                                                                 int C, int Tc, int lanes, int groups, int pieces, int slots,
                                                                 const double* __restrict__ state_sum, const int64_t* __restrict__ state_n,
                                                                 float* __restrict__ piece_s, float* __restrict__ piece_d,
                                                                 int* __restrict__ piece_n, short* __restrict__ slot_of) {
  constexpr int VEC = Vec<T>::N;
  __shared__ int key[kProtoMaxGroups][kProtoPiece];                 // class of a row of the piece (kProtoAbsent: none)
  __shared__ int skey[kProtoMaxGroups][kProtoPiece];                // the keys in ascending order
  __shared__ unsigned char srow[kProtoMaxGroups][kProtoPiece];      // the row behind a sorted position
  __shared__ int nvalid[kProtoMaxGroups];
  __shared__ short slotmap[kProtoMaxGroups][kProtoMaxT];
  const int tid = threadIdx.x;
  const int piece0 = blockIdx.x * groups;
  for (int idx = tid; idx < groups * kProtoPiece; idx += kProtoBlock) {
    const int g = idx / kProtoPiece, r = idx % kProtoPiece;
    const long long row = (long long)(piece0 + g) * kProtoPiece + r;
    int k = kProtoAbsent;
    if (piece0 + g < pieces && row < M) {
      const int c = cls[row];
      if (c >= 0 && c < Tc) k = c;
    }
    key[g][r] = k;
  }
  for (int idx = tid; idx < groups * Tc; idx += kProtoBlock) slotmap[idx / Tc][idx % Tc] = -1;
  __syncthreads();
  // a stable rank of the 64 keys: rows of one class stay in ascending order
  for (int idx = tid; idx < groups * kProtoPiece; idx += kProtoBlock) {
    const int g = idx / kProtoPiece, r = idx % kProtoPiece;
    const int k = key[g][r];
    int rank = 0;
    for (int j = 0; j < kProtoPiece; ++j) {
      const int kj = key[g][j];
      rank += (kj < k || (kj == k && j < r)) ? 1 : 0;
    }
    skey[g][rank] = k;
    srow[g][rank] = (unsigned char)r;
  }
  __syncthreads();
  // the slot of a class: the number of run heads in front of its own
  for (int idx = tid; idx < groups * kProtoPiece; idx += kProtoBlock) {
    const int g = idx / kProtoPiece, s = idx % kProtoPiece;
    const int k = skey[g][s];
    if (k != kProtoAbsent && (s == 0 || skey[g][s - 1] != k)) {
      int slot = 0;
      for (int j = 1; j <= s; ++j) slot += skey[g][j] != skey[g][j - 1] ? 1 : 0;
      slotmap[g][k] = (short)slot;
    }
    if (s == 0) {
      int n = 0;
      for (int j = 0; j < kProtoPiece; ++j) n += skey[g][j] != kProtoAbsent ? 1 : 0;
      nvalid[g] = n;
    }
  }
  __syncthreads();
  for (int idx = tid; idx < groups * Tc; idx += kProtoBlock) {
    const int g = idx % groups, c = idx / groups;
    if (piece0 + g < pieces) slot_of[(size_t)c * pieces + piece0 + g] = slotmap[g][c];
  }
  const int g = tid / lanes, lane = tid % lanes;
  if (g >= groups || piece0 + g >= pieces) return;
  const int piece = piece0 + g, nv = nvalid[g], ch0 = lane * VEC;
  const T* base = x + (size_t)piece * kProtoPiece * ld + ch0;
  float acc[VEC], rv[VEC], dacc = 0.f;
  int cur = -1, slot = -1, cnt = 0;
  bool has_r = false;
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = rv[i] = 0.f;
  auto flush = [&]() {
    const size_t cell = (size_t)piece * slots + slot;
    float* out = piece_s + cell * C + ch0;
#pragma unroll
    for (int i = 0; i < VEC; i += 4) *reinterpret_cast<float4*>(out + i) = make_float4(acc[i], acc[i + 1], acc[i + 2], acc[i + 3]);
    piece_d[cell * lanes + lane] = dacc;
    if (lane == 0) piece_n[cell] = cnt;
  };
  for (int s0 = 0; s0 < nv; s0 += kProtoPrefetch) {
    Vec<T> v[kProtoPrefetch];
#pragma unroll
    for (int u = 0; u < kProtoPrefetch; ++u)
      if (s0 + u < nv) v[u].load(base + (size_t)srow[g][s0 + u] * ld);
#pragma unroll
    for (int u = 0; u < kProtoPrefetch; ++u) {
      if (s0 + u >= nv) break;
      const int k = skey[g][s0 + u];
      if (k != cur) {
        if (cur >= 0) flush();
        cur = k;
        ++slot;
        cnt = 0;
        dacc = 0.f;
        const int64_t n = state_n[k];
        has_r = n > 0;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          acc[i] = 0.f;
          rv[i] = has_r ? (float)(state_sum[(size_t)k * C + ch0 + i] / (double)n) : 0.f;
        }
      }
      ++cnt;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float f = v[u].get(i);
        acc[i] += f;
        const float d = f - rv[i];                                    // formed per element: X_p == R_c gives exactly 0
        dacc += has_r ? d * d : 0.f;
      }
    }
  }
  if (cur >= 0) flush();
}

// ---- class: the piece slots of one class, in piece order --------------------------------------------------------------------
__global__ __launch_bounds__(kProtoBlock) void proto_class_kernel(int C, int pieces, int slots, int lanes_x, const float* __restrict__ piece_s,
                                                                 const float* __restrict__ piece_d, const int* __restrict__ piece_n,
                                                                 const short* __restrict__ slot_of, double* __restrict__ batch_sums,
                                                                 int64_t* __restrict__ batch_n, double* __restrict__ mu,
                                                                 double* __restrict__ dsum, unsigned int* __restrict__ ticket) {
  __shared__ unsigned int list[kProtoBlock];                        // piece * 64 + slot of the present pieces of a chunk, in order
  __shared__ int wave_cnt[4];
  __shared__ double wred[4];
  __shared__ long long nred[4];
  __shared__ long long n_all;
  __shared__ double comb[1024];                                     // [group][C]: groups * C <= 1024
  const int c = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lanes = C / 4, groups = kProtoBlock / lanes;            // a group of C / 4 threads: a float4 each
  const int g = tid / lanes, gl = tid % lanes;
  const bool adder = g < groups;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  double dtot = 0.0;                                                // thread 0 only
  long long ntot = 0;
  const short* so = slot_of + (size_t)c * pieces;
  for (int p0 = 0; p0 < pieces; p0 += kProtoBlock) {
    const int p = p0 + tid;
    const int slot = p < pieces ? (int)so[p] : -1;
    const unsigned long long mask = __ballot(slot >= 0);
    if (lane == 0) wave_cnt[wave] = __popcll(mask);
    __syncthreads();
    int off = __popcll(mask & ((1ull << lane) - 1ull)), E = 0;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) off += wave_cnt[w];
      E += wave_cnt[w];
    }
    if (slot >= 0) list[off] = (unsigned int)p * kProtoPiece + (unsigned int)slot;
    __syncthreads();
    if (adder) {
#pragma unroll 4
      for (int e = g; e < E; e += groups) {
        const unsigned int ent = list[e];
        const size_t cell = (size_t)(ent / kProtoPiece) * slots + ent % kProtoPiece;
        const float4 v = *reinterpret_cast<const float4*>(piece_s + cell * C + gl * 4);
        acc[0] += (double)v.x; acc[1] += (double)v.y; acc[2] += (double)v.z; acc[3] += (double)v.w;
      }
    }
    // the squared distances and the count of entry `tid`, then the chunk's sum in a fixed order
    double d = 0.0;
    long long n = 0;
    if (tid < E) {
      const unsigned int ent = list[tid];
      const size_t cell = (size_t)(ent / kProtoPiece) * slots + ent % kProtoPiece;
      for (int l = 0; l < lanes_x; ++l) d += (double)piece_d[cell * lanes_x + l];
      n = piece_n[cell];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      d += __shfl_xor(d, o, 64);
      n += __shfl_xor(n, o, 64);
    }
    if (lane == 0) { wred[wave] = d; nred[wave] = n; }
    __syncthreads();
    if (tid == 0) {
      dtot += (wred[0] + wred[1]) + (wred[2] + wred[3]);
      ntot += (nred[0] + nred[1]) + (nred[2] + nred[3]);
    }
  }
  if (adder) {
#pragma unroll
    for (int i = 0; i < 4; ++i) comb[g * C + gl * 4 + i] = acc[i];
  }
  if (tid == 0) {
    n_all = ntot;
    batch_n[c] = ntot;
    dsum[c] = dtot;
    if (c == 0) *ticket = 0u;                                       // of the launch that follows
  }
  __syncthreads();
  const long long n = n_all;
  for (int ch = tid; ch < C; ch += kProtoBlock) {
    double s = 0.0;
    for (int q = 0; q < groups; ++q) s += comb[q * C + ch];
    batch_sums[(size_t)c * C + ch] = s;
    mu[(size_t)c * C + ch] = n > 0 ? s / (double)n : 0.0;
  }
}

// ---- proto: the prototype level, one workgroup per class ---------------------------------------------------------------------
__device__ __forceinline__ double proto_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(kProtoBlock) void proto_level_kernel(int C, int T, int K, const double* __restrict__ mu, const double* __restrict__ dsum,
                                                                 const int64_t* __restrict__ batch_n, const double* __restrict__ state_sum,
                                                                 const int64_t* __restrict__ state_n, const float* __restrict__ old_proto,
                                                                 const unsigned char* __restrict__ old_valid, float w_m, float w_a, float w_r,
                                                                 float* __restrict__ tables, double* __restrict__ part,
                                                                 unsigned int* __restrict__ ticket, float* __restrict__ loss_out) {
  __shared__ int plist[kProtoMaxT];                                 // the present classes, ascending
  __shared__ double coef[kProtoMaxT];                               // d L_rep / d |mu_c - mu_k| / |mu_c - mu_k|, per present k
  __shared__ double inv[kProtoMaxT];                                // 1 / (|mu_c - mu_k| + 1e-6)
  __shared__ double wred[4];
  __shared__ int counts[4];                                         // |A|, |Bs|, |P|, last
  __shared__ double rowsum;
  const int c = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float* tab_a = tables;
  float* tab_r = tables + T;
  float* tab_g = tables + T + (size_t)T * C;
  if (tid == 0) {
    int nA = 0, nB = 0, nP = 0;
    for (int t = 0; t < T; ++t) {
      if (batch_n[t] <= 0) continue;
      plist[nP++] = t;
      nB += state_n[t] > 0 ? 1 : 0;
      nA += (t < K && old_valid[t]) ? 1 : 0;
    }
    counts[0] = nA; counts[1] = nB; counts[2] = nP;
  }
  __syncthreads();
  const int nA = counts[0], nB = counts[1], nP = counts[2];
  const long long n_c = batch_n[c], N_c = state_n[c];
  const bool in_p = n_c > 0, in_b = in_p && N_c > 0, in_a = in_p && c < K && old_valid[c] != 0;
  for (int ch = tid; ch < C; ch += kProtoBlock)
    tab_r[(size_t)c * C + ch] = N_c > 0 ? (float)(state_sum[(size_t)c * C + ch] / (double)N_c) : 0.f;
  double m_c = 0.0, t_c = 0.0, r_c = 0.0;
  if (!in_p) {
    for (int ch = tid; ch < C; ch += kProtoBlock) tab_g[(size_t)c * C + ch] = 0.f;
    if (tid == 0) tab_a[c] = 0.f;
  } else {
    const double* mc = mu + (size_t)c * C;
    // a wave per pair: |mu_c - mu_k| in fp64, lanes over channels, the fixed shuffle order - both workgroups of a pair get the same bits
    for (int j = wave; j < nP; j += 4) {
      const int k = plist[j];
      double s = 0.0;
      if (k != c) {
        const double* mk = mu + (size_t)k * C;
        for (int ch = lane; ch < C; ch += 64) {
          const double d = mc[ch] - mk[ch];
          s += d * d;
        }
        s = proto_wave_sum(s);
      }
      if (lane == 0) {
        const double d = sqrt(s), e = d + 1e-6;
        inv[j] = k != c ? 1.0 / e : 0.0;
        // d/d mu_c of (1 / (d + eps)) counted for (c, k) and (k, c): -2 (mu_c - mu_k) / (d (d + eps)^2); 0 at d = 0
        coef[j] = (k != c && d > 0.0 && nP >= 2) ? -2.0 * (double)w_r / ((double)nP * d * e * e) : 0.0;
      }
    }
    // the distance to the old prototype
    double sm = 0.0;
    if (in_a) {
      const float* oc = old_proto + (size_t)c * C;
      for (int ch = tid; ch < C; ch += kProtoBlock) {
        const double d = mc[ch] - (double)oc[ch];
        sm += d * d;
      }
    }
    sm = proto_wave_sum(sm);
    if (lane == 0) wred[wave] = sm;
    __syncthreads();
    const double dm = sqrt((wred[0] + wred[1]) + (wred[2] + wred[3]));
    const double cm = (in_a && dm > 0.0) ? (double)w_m / ((double)nA * dm) : 0.0;      // the gradient of a zero distance is 0
    if (tid == 0) {
      double r = 0.0;
      for (int j = 0; j < nP; ++j) r += inv[j];
      rowsum = nP >= 2 ? r : 0.0;
      tab_a[c] = in_b ? (float)(2.0 * (double)w_a / ((double)nB * (double)n_c)) : 0.f;
    }
    for (int ch = tid; ch < C; ch += kProtoBlock) {
      const double m = mc[ch];
      double gsum = in_a ? cm * (m - (double)old_proto[(size_t)c * C + ch]) : 0.0;
      for (int j = 0; j < nP; ++j) gsum += coef[j] * (m - mu[(size_t)plist[j] * C + ch]);
      tab_g[(size_t)c * C + ch] = (float)(gsum / (double)n_c);
    }
    __syncthreads();
    m_c = in_a ? dm : 0.0;
    t_c = in_b ? dsum[c] / (double)n_c : 0.0;
    r_c = rowsum;
  }
  if (tid == 0) {
    part[3 * c] = m_c;
    part[3 * c + 1] = t_c;
    part[3 * c + 2] = r_c;
    __threadfence();                                                // the partials are visible before the ticket is
    counts[3] = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1 : 0;
  }
  __syncthreads();
  if (!counts[3]) return;
  __threadfence();
  if (tid == 0) {                                                   // the last workgroup: at most 256 classes, in class order
    const volatile double* vp = part;
    double lm = 0.0, la = 0.0, lr = 0.0;
    for (int t = 0; t < T; ++t) {
      lm += vp[3 * t];
      la += vp[3 * t + 1];
      lr += vp[3 * t + 2];
    }
    lm = nA > 0 ? lm / (double)nA : 0.0;
    la = nB > 0 ? la / (double)nB : 0.0;
    lr = nP >= 2 ? lr / (double)nP : 0.0;
    loss_out[0] = (float)((double)w_m * lm + (double)w_a * la + (double)w_r * lr);
    loss_out[1] = (float)lm;
    loss_out[2] = (float)la;
    loss_out[3] = (float)lr;
  }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kProtoBlock) void proto_bwd_kernel(const T* __restrict__ x, int ld, const int* __restrict__ cls, long long M, int C,
                                                               int Tc, int lanes, const float* __restrict__ tables,
                                                               const float* __restrict__ grad_out, T* __restrict__ d_x, int ld_d) {
  constexpr int VEC = Vec<T>::N;
  const long long item = (long long)blockIdx.x * kProtoBlock + threadIdx.x;
  const long long row = item / lanes;
  if (row >= M) return;
  const int ch0 = (int)(item % lanes) * VEC;
  const int c = cls[row];
  Vec<T> out;
  if (c < 0 || c >= Tc) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) out.set(i, 0.f);
  } else {
    const float go = grad_out[0], a = tables[c];
    const float* r = tables + Tc + (size_t)c * C + ch0;
    const float* g = tables + Tc + (size_t)Tc * C + (size_t)c * C + ch0;
    Vec<T> v;
    v.load(x + (size_t)row * ld + ch0);
#pragma unroll
    for (int i = 0; i < VEC; ++i) out.set(i, go * (a * (v.get(i) - r[i]) + g[i]));
  }
  out.store(d_x + (size_t)row * ld_d + ch0);
}

__global__ __launch_bounds__(kProtoBlock) void proto_update_kernel(double* __restrict__ state_sum, int64_t* __restrict__ state_n,
                                                                  const double* __restrict__ batch_sums, const int64_t* __restrict__ batch_n,
                                                                  int T, int C) {
  const int i = blockIdx.x * kProtoBlock + threadIdx.x;
  if (i < T * C) state_sum[i] += batch_sums[i];
  if (i < T) state_n[i] += batch_n[i];
}

// the shape rules shared by the plan and the calls
int proto_shape(const char* fn, long long M, int C, int T, int dtype) {
  UCD_REQUIRE(M >= 1 && C >= 1 && T >= 1, UCD_EINVAL, "%s: bad sizes (M = %lld, C = %d, T = %d)", fn, M, C, T);
  UCD_REQUIRE(dtype == UCD_F32 || dtype == UCD_BF16, UCD_EINVAL, "%s: unknown dtype %d", fn, dtype);
  UCD_REQUIRE(C % 8 == 0 && C <= kProtoMaxC, UCD_EUNSUPPORTED, "%s: C = %d must be a multiple of 8 up to %d", fn, C, kProtoMaxC);
  UCD_REQUIRE(T <= kProtoMaxT, UCD_EUNSUPPORTED, "%s: T = %d is above %d classes", fn, T, kProtoMaxT);
  UCD_REQUIRE(M < (1ll << 31), UCD_EUNSUPPORTED, "%s: M = %lld rows are more than 2^31 - 1", fn, M);
  return UCD_OK;
}

int proto_check_map(const char* fn, const char* what, const void* p, int ld, int C, int es) {
  UCD_REQUIRE(ld >= C, UCD_EINVAL, "%s: the row pitch of %s (%d) is below C = %d", fn, what, ld, C);
  UCD_REQUIRE(aligned16(p) && ((size_t)ld * es) % 16 == 0, UCD_EALIGN, "%s: %s must be 16-byte aligned with a 16-byte multiple row pitch", fn,
              what);
  return UCD_OK;
}

long long proto_bwd_blocks(long long M, int lanes) { return (M * lanes + kProtoBlock - 1) / kProtoBlock; }

}  // namespace
}  // namespace ucd

using namespace ucd;

extern "C" {

int ucd_proto_plan(long long M, int C, int T, int dtype, size_t* workspace_bytes, int* grid, int* lds_bytes, int* pieces) {
  static const char* fn = "ucd_proto_plan";
  const int rc = proto_shape(fn, M, C, T, dtype);
  if (rc) return rc;
  const ProtoWs ws = proto_ws(M, C, T, dtype);
  if (workspace_bytes) *workspace_bytes = ws.bytes;
  if (grid) {
    grid[0] = ceil_div(ws.pieces, ws.groups);                  // accum
    grid[1] = T;                                               // class
    grid[2] = T;                                               // proto
    grid[3] = (int)proto_bwd_blocks(M, ws.lanes);              // backward
  }
  if (lds_bytes) {
    lds_bytes[0] = kProtoAccumLds;
    lds_bytes[1] = kProtoClassLds;
    lds_bytes[2] = kProtoProtoLds;
  }
  if (pieces) *pieces = ws.pieces;
  return UCD_OK;
}

int ucd_proto_classify(const int64_t* labels, int B, int H, int W, int h, int w, int T, int K, int ignore_index, const float* sem_t,
                       int ld_t, int32_t* cls, ucd_stream_t stream) {
  static const char* fn = "ucd_proto_classify";
  UCD_REQUIRE(labels && cls, UCD_EINVAL, "%s: NULL argument (labels and cls are required)", fn);
  UCD_REQUIRE(B >= 1 && H >= 1 && W >= 1 && h >= 1 && w >= 1 && T >= 1 && K >= 0, UCD_EINVAL,
              "%s: bad sizes (B = %d, H = %d, W = %d, h = %d, w = %d, T = %d, K = %d)", fn, B, H, W, h, w, T, K);
  UCD_REQUIRE(K <= T, UCD_EINVAL, "%s: K = %d teacher classes are more than T = %d", fn, K, T);
  UCD_REQUIRE(sem_t == nullptr || (K >= 1 && ld_t >= K), UCD_EINVAL, "%s: teacher rows need K >= 1 and a row pitch (%d) of at least K = %d", fn,
              ld_t, K);
  UCD_REQUIRE(T <= kProtoMaxT, UCD_EUNSUPPORTED, "%s: T = %d is above %d classes", fn, T, kProtoMaxT);
  UCD_REQUIRE((long long)B * h * w < (1ll << 31) && (long long)B * H * W < (1ll << 40), UCD_EUNSUPPORTED,
              "%s: B h w = %lld rows are more than 2^31 - 1", fn, (long long)B * h * w);
  UCD_REQUIRE(((uintptr_t)labels & 7u) == 0 && ((uintptr_t)cls & 3u) == 0 && ((uintptr_t)sem_t & 3u) == 0, UCD_EALIGN,
              "%s: labels, cls and sem_t must be aligned to their element size", fn);
  const int Mlow = B * h * w;
  proto_classify_kernel<<<ceil_div(Mlow, kProtoBlock), kProtoBlock, 0, (hipStream_t)stream>>>(labels, B, H, W, h, w, (float)H / (float)h,
                                                                                             (float)W / (float)w, T, K, ignore_index,
                                                                                             sem_t, ld_t, cls);
  return check_launch(fn);
}

int ucd_proto_forward(const void* x, int ld_x, int dtype, const int32_t* cls, long long M, int C, int T, int K, const double* state_sum,
                      const int64_t* state_n, const float* old_proto, const unsigned char* old_valid, float w_m, float w_a, float w_r,
                      float* loss_out, float* tables, double* batch_sums, int64_t* batch_n, void* workspace, size_t workspace_bytes,
                      ucd_stream_t stream) {
  static const char* fn = "ucd_proto_forward";
  UCD_REQUIRE(x && cls && state_sum && state_n && loss_out && tables && batch_sums && batch_n, UCD_EINVAL,
              "%s: NULL argument (x, cls, state_sum, state_n, loss_out, tables, batch_sums and batch_n are required)", fn);
  UCD_REQUIRE(K >= 0, UCD_EINVAL, "%s: K = %d must not be negative", fn, K);
  int rc = proto_shape(fn, M, C, T, dtype);
  if (rc) return rc;
  UCD_REQUIRE(K <= T, UCD_EINVAL, "%s: K = %d teacher classes are more than T = %d", fn, K, T);
  UCD_REQUIRE(K == 0 || (old_proto && old_valid), UCD_EINVAL, "%s: NULL old_proto / old_valid with K = %d", fn, K);
  const int es = dtype == UCD_BF16 ? 2 : 4;
  if ((rc = proto_check_map(fn, "x", x, ld_x, C, es))) return rc;
  UCD_REQUIRE(((uintptr_t)cls & 3u) == 0 && ((uintptr_t)state_sum & 7u) == 0 && ((uintptr_t)state_n & 7u) == 0 &&
                  ((uintptr_t)batch_sums & 7u) == 0 && ((uintptr_t)batch_n & 7u) == 0 && ((uintptr_t)old_proto & 3u) == 0 &&
                  ((uintptr_t)tables & 3u) == 0 && ((uintptr_t)loss_out & 3u) == 0,
              UCD_EALIGN, "%s: cls, the state, the batch sums, old_proto, tables and loss_out must be aligned to their element size", fn);
  const ProtoWs ws = proto_ws(M, C, T, dtype);
  UCD_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= ws.bytes, UCD_EWORKSPACE, "%s: workspace missing, unaligned or too small",
              fn);
  hipStream_t s = (hipStream_t)stream;
  char* wsp = (char*)workspace;
  float *piece_s = (float*)(wsp + ws.piece_s), *piece_d = (float*)(wsp + ws.piece_d);
  int* piece_n = (int*)(wsp + ws.piece_n);
  short* slot_of = (short*)(wsp + ws.slot_of);
  double *mu = (double*)(wsp + ws.mu), *dsum = (double*)(wsp + ws.dsum), *part = (double*)(wsp + ws.part);
  unsigned int* ticket = (unsigned int*)(wsp + ws.ticket);
  const int blocks = ceil_div(ws.pieces, ws.groups);
  if (dtype == UCD_BF16)
    proto_accum_kernel<__hip_bfloat16><<<blocks, kProtoBlock, 0, s>>>((const __hip_bfloat16*)x, ld_x, cls, M, C, T, ws.lanes, ws.groups, ws.pieces,
                                                                     ws.slots, state_sum, state_n, piece_s, piece_d, piece_n, slot_of);
  else
    proto_accum_kernel<float><<<blocks, kProtoBlock, 0, s>>>((const float*)x, ld_x, cls, M, C, T, ws.lanes, ws.groups, ws.pieces, ws.slots,
                                                            state_sum, state_n, piece_s, piece_d, piece_n, slot_of);
  if ((rc = check_launch(fn))) return rc;
  proto_class_kernel<<<T, kProtoBlock, 0, s>>>(C, ws.pieces, ws.slots, ws.lanes, piece_s, piece_d, piece_n, slot_of, batch_sums, batch_n, mu, dsum,
                                               ticket);
  if ((rc = check_launch(fn))) return rc;
  proto_level_kernel<<<T, kProtoBlock, 0, s>>>(C, T, K, mu, dsum, batch_n, state_sum, state_n, old_proto, old_valid, w_m, w_a, w_r, tables, part,
                                               ticket, loss_out);
  return check_launch(fn);
}

int ucd_proto_backward(const void* x, int ld_x, int dtype, const int32_t* cls, long long M, int C, int T, const float* tables,
                       const float* grad_out, void* d_x, int ld_d, ucd_stream_t stream) {
  static const char* fn = "ucd_proto_backward";
  UCD_REQUIRE(x && cls && tables && grad_out && d_x, UCD_EINVAL, "%s: NULL argument (x, cls, tables, grad_out and d_x are required)", fn);
  int rc = proto_shape(fn, M, C, T, dtype);
  if (rc) return rc;
  const int es = dtype == UCD_BF16 ? 2 : 4;
  if ((rc = proto_check_map(fn, "x", x, ld_x, C, es))) return rc;
  if ((rc = proto_check_map(fn, "d_x", d_x, ld_d, C, es))) return rc;
  UCD_REQUIRE(((uintptr_t)cls & 3u) == 0 && ((uintptr_t)tables & 3u) == 0 && ((uintptr_t)grad_out & 3u) == 0, UCD_EALIGN,
              "%s: cls, tables and grad_out must be 4-byte aligned", fn);
  const int lanes = C / (16 / es);
  const long long blocks = proto_bwd_blocks(M, lanes);
  UCD_REQUIRE(blocks <= 0x7FFFFFFF, UCD_EUNSUPPORTED, "%s: %lld workgroups are more than a grid holds", fn, blocks);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == UCD_BF16)
    proto_bwd_kernel<__hip_bfloat16><<<(unsigned int)blocks, kProtoBlock, 0, s>>>((const __hip_bfloat16*)x, ld_x, cls, M, C, T, lanes, tables,
                                                                                 grad_out, (__hip_bfloat16*)d_x, ld_d);
  else
    proto_bwd_kernel<float><<<(unsigned int)blocks, kProtoBlock, 0, s>>>((const float*)x, ld_x, cls, M, C, T, lanes, tables, grad_out,
                                                                        (float*)d_x, ld_d);
  return check_launch(fn);
}

int ucd_proto_update(double* state_sum, int64_t* state_n, const double* batch_sums, const int64_t* batch_n, int T, int C,
                     ucd_stream_t stream) {
  static const char* fn = "ucd_proto_update";
  UCD_REQUIRE(state_sum && state_n && batch_sums && batch_n, UCD_EINVAL, "%s: NULL argument (the state and the batch sums are required)", fn);
  UCD_REQUIRE(T >= 1 && C >= 1, UCD_EINVAL, "%s: bad sizes (T = %d, C = %d)", fn, T, C);
  UCD_REQUIRE(T <= kProtoMaxT && C <= kProtoMaxC, UCD_EUNSUPPORTED, "%s: T = %d, C = %d are above %d classes or %d channels", fn, T, C,
              kProtoMaxT, kProtoMaxC);
  UCD_REQUIRE((((uintptr_t)state_sum | (uintptr_t)state_n | (uintptr_t)batch_sums | (uintptr_t)batch_n) & 7u) == 0, UCD_EALIGN,
              "%s: the state and the batch sums must be 8-byte aligned", fn);
  proto_update_kernel<<<ceil_div(T * C, kProtoBlock), kProtoBlock, 0, (hipStream_t)stream>>>(state_sum, state_n, batch_sums, batch_n, T, C);
  return check_launch(fn);
}

}  // extern "C"
