// The weight-space regularisers of the EWC / PI / RW baselines (reference utils/regularizer.py, train.py:139-145) as ONE pass
// over every trainable tensor, between the gradient all-reduce and the optimiser step.  The reference runs update(), builds the
// penalty as an autograd graph and back-propagates it a second time; here the penalty's gradient is added analytically to the
// reduced gradient buckets, and the state (Fisher matrix, path-integral delta, RW score, theta at the last update) is updated
// in the same pass.
//
// HBM-bound, like sgd.hip: one workgroup per 4096-element chunk of one tensor (block table built once by the host), 16-byte
// accesses when every pointer of the chunk allows.  Bytes per element: EWC 28 (read g, p, p_old, omega, F; write F, g), PI 36
// (+ delta, temp read and written, no F), RW 44 (EWC + score, temp read and written).
//
// Arithmetic: the reference's fp32 torch ops, one rounding per operation (the Makefile compiles with -ffp-contract=off), IEEE
// division (hipcc's default), in the reference's order.  The penalty gradient is what autograd produces for
// lambda * sum(omega * (p - p_old) ** 2): MulBackward (lambda * omega), PowBackward (* (2 * d)), AccumulateGrad (g + .).
// The penalty sum is accumulated in fp64 per block and reduced in a fixed order by a second launch: bit-reproducible.
#include "common.h"

namespace ucd {
namespace {

constexpr int kRegThreads = 256;
constexpr int kRegChunk = 4096;
constexpr int kRegFinishThreads = 256;

struct RegCtl {
  float alpha, beta, lam;
  bool has_temp;    // a previous update stored temp (PI / RW: counter > 0)
  bool boundary;    // RW: counter % iterations == 0
};

template <int kMethod>
__device__ __forceinline__ void reg_elem(const RegCtl& c, bool pen, float p, float& g, float old, float om, float& f,
                                         float& s, float& t, double& acc) {
  const float g0 = g;
  if (kMethod == UCD_REG_EWC) {
    f = c.alpha * (g0 * g0) + c.beta * f;                                   // regularizer.py:106
  } else if (kMethod == UCD_REG_PI) {
    if (c.has_temp) s = s + g0 * (t - p);                                   // :169-170
    t = p;                                                                  // :172
  } else {
    if (c.boundary) {
      if (c.has_temp) {                                                     // :265-269, F before this step's update
        const float delta = g0 * (t - p);
        const float d = p - t;
        const float den = (0.5f * f) * (d * d) + (float)1e-8;
        s = s + delta / den;
      }
      t = p;                                                                // :271
    }
    f = c.alpha * (g0 * g0) + c.beta * f;                                   // :278
  }
  if (pen) {
    const float d = p - old;
    acc += (double)(om * (d * d));
    g = g0 + (c.lam * om) * (2.0f * d);
  }
}

template <int kMethod>
__global__ __launch_bounds__(kRegThreads) void reg_step_kernel(const ucd_reg_tensor* __restrict__ table,
                                                               const int* __restrict__ blocks,
                                                               const ucd_reg_hyper* __restrict__ hyper,
                                                               double* __restrict__ partials) {
  const int t = blocks[2 * blockIdx.x], chunk = blocks[2 * blockIdx.x + 1];
  const ucd_reg_tensor e = table[t];
  const int counter = hyper->counter;
  RegCtl c;
  c.alpha = hyper->alpha; c.beta = hyper->one_minus_alpha; c.lam = hyper->lambda_f;
  c.has_temp = counter > 0;
  c.boundary = hyper->iterations > 0 && counter % hyper->iterations == 0;
  const bool pen = e.penalize != 0;
  // score / delta and temp are read (and the score written) only when this update accumulates into them; temp is rewritten
  // on every PI update and on RW's boundary updates
  const bool write_temp = kMethod == UCD_REG_PI || (kMethod == UCD_REG_RW && c.boundary);
  const bool read_st = write_temp && c.has_temp;
  const long long begin = (long long)chunk * kRegChunk;
  const int n = (int)(e.n - begin < kRegChunk ? e.n - begin : kRegChunk);
  const float* p = e.p + begin;
  float* g = e.g + begin;
  const float* po = pen ? e.p_old + begin : nullptr;
  const float* om = pen ? e.omega + begin : nullptr;
  float* f = kMethod != UCD_REG_PI ? e.fisher + begin : nullptr;
  float* s = kMethod != UCD_REG_EWC ? e.score + begin : nullptr;
  float* tp = kMethod != UCD_REG_EWC ? e.temp + begin : nullptr;
  double acc = 0.0;
  const uintptr_t bits = (uintptr_t)p | (uintptr_t)g | (uintptr_t)po | (uintptr_t)om | (uintptr_t)f | (uintptr_t)s |
                         (uintptr_t)tp;
  int scalar_from = 0;
  if ((bits & 15u) == 0) {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = threadIdx.x * 4; i + 4 <= n; i += kRegThreads * 4) {
      const float4 pv = *(const float4*)(p + i);
      float4 gv = *(const float4*)(g + i);
      const float4 ov = pen ? *(const float4*)(po + i) : z, mv = pen ? *(const float4*)(om + i) : z;
      float4 fv = f ? *(const float4*)(f + i) : z, sv = z, tv = z;
      if (read_st) { sv = *(const float4*)(s + i); tv = *(const float4*)(tp + i); }
      reg_elem<kMethod>(c, pen, pv.x, gv.x, ov.x, mv.x, fv.x, sv.x, tv.x, acc);
      reg_elem<kMethod>(c, pen, pv.y, gv.y, ov.y, mv.y, fv.y, sv.y, tv.y, acc);
      reg_elem<kMethod>(c, pen, pv.z, gv.z, ov.z, mv.z, fv.z, sv.z, tv.z, acc);
      reg_elem<kMethod>(c, pen, pv.w, gv.w, ov.w, mv.w, fv.w, sv.w, tv.w, acc);
      if (pen) *(float4*)(g + i) = gv;
      if (f) *(float4*)(f + i) = fv;
      if (read_st) *(float4*)(s + i) = sv;
      if (write_temp) *(float4*)(tp + i) = tv;
    }
    scalar_from = n & ~3;
  }
  for (int i = scalar_from + threadIdx.x; i < n; i += kRegThreads) {
    float gv = g[i], fv = f ? f[i] : 0.f, sv = 0.f, tv = 0.f;
    if (read_st) { sv = s[i]; tv = tp[i]; }
    reg_elem<kMethod>(c, pen, p[i], gv, pen ? po[i] : 0.f, pen ? om[i] : 0.f, fv, sv, tv, acc);
    if (pen) g[i] = gv;
    if (f) f[i] = fv;
    if (read_st) s[i] = sv;
    if (write_temp) tp[i] = tv;
  }
  // fixed-order block reduction of the fp64 partial
  __shared__ double red[kRegThreads];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = kRegThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

// One workgroup: partials summed in a fixed order -> penalty; the update counter advances (stream order: after the pass).
__global__ __launch_bounds__(kRegFinishThreads) void reg_finish_kernel(const double* __restrict__ partials, int n_blocks,
                                                                       ucd_reg_hyper* __restrict__ hyper,
                                                                       float* __restrict__ penalty) {
  __shared__ double red[kRegFinishThreads];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_blocks; i += kRegFinishThreads) acc += partials[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = kRegFinishThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    penalty[0] = (float)(hyper->reg_importance * red[0]);
    hyper->counter = hyper->counter + 1;
  }
}

__global__ void reg_hyper_store_kernel(ucd_reg_hyper* dst, ucd_reg_hyper value) { *dst = value; }

}  // namespace
}  // namespace ucd

using namespace ucd;

extern "C" {

int ucd_reg_chunk(void) { return kRegChunk; }

int ucd_reg_hyper_store(ucd_reg_hyper* device_hyper, const ucd_reg_hyper* hyper, ucd_stream_t stream) {
  static const char* fn = "ucd_reg_hyper_store";
  UCD_REQUIRE(device_hyper && hyper, UCD_EINVAL, "%s: device_hyper / hyper is NULL", fn);
  UCD_REQUIRE(hyper->iterations > 0 && hyper->counter >= 0, UCD_EINVAL, "%s: iterations = %d, counter = %d", fn,
              hyper->iterations, hyper->counter);
  reg_hyper_store_kernel<<<1, 1, 0, (hipStream_t)stream>>>(device_hyper, *hyper);     // the values travel as a kernel argument
  return check_launch(fn);
}

int ucd_reg_step(const ucd_reg_tensor* table, const int* blocks, int n_blocks, int method, ucd_reg_hyper* device_hyper,
                 double* partials, float* penalty, ucd_stream_t stream) {
  static const char* fn = "ucd_reg_step";
  UCD_REQUIRE(n_blocks >= 0, UCD_EINVAL, "%s: n_blocks = %d", fn, n_blocks);
  UCD_REQUIRE(method == UCD_REG_EWC || method == UCD_REG_PI || method == UCD_REG_RW, UCD_EINVAL, "%s: unknown method %d", fn,
              method);
  if (n_blocks == 0) return 0;
  UCD_REQUIRE(table && blocks && device_hyper && partials && penalty, UCD_EINVAL,
              "%s: table / blocks / hyper / partials / penalty is NULL", fn);
  hipStream_t s = (hipStream_t)stream;
  if (method == UCD_REG_EWC)
    reg_step_kernel<UCD_REG_EWC><<<(unsigned)n_blocks, kRegThreads, 0, s>>>(table, blocks, device_hyper, partials);
  else if (method == UCD_REG_PI)
    reg_step_kernel<UCD_REG_PI><<<(unsigned)n_blocks, kRegThreads, 0, s>>>(table, blocks, device_hyper, partials);
  else
    reg_step_kernel<UCD_REG_RW><<<(unsigned)n_blocks, kRegThreads, 0, s>>>(table, blocks, device_hyper, partials);
  int rc = check_launch(fn);
  if (rc) return rc;
  reg_finish_kernel<<<1, kRegFinishThreads, 0, s>>>(partials, n_blocks, device_hyper, penalty);
  return check_launch(fn);
}

}  // extern "C"
