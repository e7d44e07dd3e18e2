// ILT's encoder distillation term as one operation (train.py:129 of the reference, segmentation_module.py:86-94):
//   att(x) = a.detach() * x,  a[b, p] = sum_c x[b, p, c]^2 / || sum_c x[b, :, c]^2 ||_2   (one norm per image)
//   loss = mean over B HW C of (a_s x_s - a_t x_t)^2,   d_x = weight * 2 a_s (a_s x_s - a_t x_t) / (B HW C)
// on the channels-last rows [B HW, C] of the student and the teacher map, bf16 or fp32.  The torch composition builds both
// attention-weighted maps, casts them to fp32 and runs MSELoss with its autograd nodes (~10 passes over [B, C, h, w] fp32);
// here: one launch for the per-pixel sums of squares of BOTH maps, one for the per-image norms, one streaming pass that reads
// both maps once more, writes d_x and reduces the loss.  HBM traffic: 2 reads of each map + 1 write, nothing else of that size.
//
// The loss is summed in a fixed order: a lane over its vectors, a wave by shuffles, a block over its waves, each block's partial
// into the workspace; the block that finishes last (an INTEGER ticket, no atomics on floats) adds the partials in index order.
// Same inputs, same bits.
#include "common.h"

namespace ucd {
namespace {

constexpr int kFdBlock = 256, kFdRows = kFdBlock / 64;      // one wave per pixel row

template <typename T>
__device__ __forceinline__ float fd_get(const T* p) { return (float)*p; }
template <>
__device__ __forceinline__ float fd_get<__hip_bfloat16>(const __hip_bfloat16* p) { return __bfloat162float(*p); }
__device__ __forceinline__ void fd_put(float* p, float v) { *p = v; }
__device__ __forceinline__ void fd_put(__hip_bfloat16* p, float v) { *p = __float2bfloat16(v); }

// a[which][r] = sum_c x[r, c]^2 for the student (blockIdx.y == 0) and the teacher (1).  16-byte loads over the first
// C / VEC * VEC channels, a scalar tail for the rest (C need not be a multiple of the vector; the row pitch is)
template <typename T>
__global__ __launch_bounds__(kFdBlock) void fd_rowsq_kernel(const T* __restrict__ x_s, int ld_s, const T* __restrict__ x_t, int ld_t,
                                                           int M, int C, float* __restrict__ a) {
  constexpr int VEC = Vec<T>::N;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = blockIdx.x * kFdRows + wave;
  if (r >= M) return;
  const T* row = blockIdx.y ? x_t + (size_t)r * ld_t : x_s + (size_t)r * ld_s;
  const int Cv = C / VEC * VEC;
  float s = 0.f;
  for (int c = lane * VEC; c < Cv; c += 64 * VEC) {
    Vec<T> v;
    v.load(row + c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) s += v.get(i) * v.get(i);
  }
  for (int c = Cv + lane; c < C; c += 64) {
    const float v = fd_get(row + c);
    s += v * v;
  }
  s = wave_sum(s);
  if (lane == 0) a[(size_t)blockIdx.y * M + r] = s;
}

// inv[which][b] = 1 / || a[which][b, :] ||_2 ; block (0, 0) also clears the ticket of the pass that follows
__global__ __launch_bounds__(kFdBlock) void fd_norm_kernel(const float* __restrict__ a, int M, int HW, int B, float* __restrict__ inv,
                                                          unsigned int* __restrict__ ticket) {
  __shared__ float lds[kFdRows];
  const int b = blockIdx.x, which = blockIdx.y;
  float s = 0.f;
  for (int p = threadIdx.x; p < HW; p += kFdBlock) {
    const float v = a[(size_t)which * M + (size_t)b * HW + p];
    s += v * v;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < kFdRows; ++i) t += lds[i];
    inv[which * B + b] = 1.f / sqrtf(t);
    if (b == 0 && which == 0) *ticket = 0u;
  }
}

template <typename T>
__global__ __launch_bounds__(kFdBlock) void fd_loss_kernel(const T* __restrict__ x_s, int ld_s, const T* __restrict__ x_t, int ld_t,
                                                          int M, int HW, int B, int C, const float* __restrict__ a,
                                                          const float* __restrict__ inv, float grad_scale, double inv_count,
                                                          T* __restrict__ d_x, int ld_d, float* __restrict__ part,
                                                          unsigned int* __restrict__ ticket, float* __restrict__ loss_out) {
  constexpr int VEC = Vec<T>::N;
  __shared__ float lds[kFdRows];
  __shared__ double dred[kFdRows];
  __shared__ int last;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = blockIdx.x * kFdRows + wave;
  float s = 0.f;
  if (r < M) {
    const int b = r / HW;
    const float f_s = a[r] * inv[b], f_t = a[(size_t)M + r] * inv[B + b];
    const float g = grad_scale * f_s;
    const T *rs = x_s + (size_t)r * ld_s, *rt = x_t + (size_t)r * ld_t;
    T* rd = d_x + (size_t)r * ld_d;
    const int Cv = C / VEC * VEC;
    for (int c = lane * VEC; c < Cv; c += 64 * VEC) {
      Vec<T> vs, vt, o;
      vs.load(rs + c);
      vt.load(rt + c);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float d = f_s * vs.get(i) - f_t * vt.get(i);
        s += d * d;
        o.set(i, g * d);
      }
      o.store(rd + c);
    }
    for (int c = Cv + lane; c < C; c += 64) {
      const float d = f_s * fd_get(rs + c) - f_t * fd_get(rt + c);
      s += d * d;
      fd_put(rd + c, g * d);
    }
  }
  s = wave_sum(s);
  if (lane == 0) lds[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    part[blockIdx.x] = (lds[0] + lds[1]) + (lds[2] + lds[3]);
    __threadfence();                                             // the partial is visible before the ticket is
    last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  // the last block: every partial in index order (thread t takes t, t + 256, ...; then the fixed shuffle and wave order)
  const volatile float* vp = part;
  double t = 0.0;
  for (unsigned int i = threadIdx.x; i < gridDim.x; i += kFdBlock) t += (double)vp[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
  if (lane == 0) dred[wave] = t;
  __syncthreads();
  if (threadIdx.x == 0) loss_out[0] = (float)(((dred[0] + dred[1]) + (dred[2] + dred[3])) * inv_count);
}

}  // namespace
}  // namespace ucd

using namespace ucd;

extern "C" {

// a [2][B HW], inv [2][B], one partial per block of the loss pass, the ticket
size_t ucd_attn_mse_workspace_bytes(int B, int HW) {
  if (B < 1 || HW < 1) return 0;
  const size_t M = (size_t)B * HW;
  return (2 * M + 2 * (size_t)B + (M + kFdRows - 1) / kFdRows + 4) * sizeof(float);
}

int ucd_attn_mse(const void* x_s, int ld_s, const void* x_t, int ld_t, int dtype, int B, int HW, int C, float weight,
                 float* loss_out, void* d_x, int ld_d, void* workspace, size_t workspace_bytes, ucd_stream_t stream) {
  static const char* fn = "ucd_attn_mse";
  UCD_REQUIRE(x_s && x_t && loss_out && d_x, UCD_EINVAL, "%s: NULL argument (x_s, x_t, loss_out and d_x are required)", fn);
  UCD_REQUIRE(dtype == UCD_F32 || dtype == UCD_BF16, UCD_EINVAL, "%s: unknown dtype %d", fn, dtype);
  UCD_REQUIRE(B > 0 && HW > 0, UCD_EINVAL, "%s: bad sizes (B = %d, HW = %d)", fn, B, HW);
  UCD_REQUIRE(C >= 1, UCD_EINVAL, "%s: C = %d must be at least 1", fn, C);
  UCD_REQUIRE((long long)B * HW <= 0x7FFFFFFF / 4, UCD_EINVAL, "%s: B * HW = %lld rows are more than the kernels index", fn,
              (long long)B * HW);
  UCD_REQUIRE(ld_s >= C && ld_t >= C && ld_d >= C, UCD_EINVAL, "%s: a leading dimension is below C = %d", fn, C);
  const int es = dtype == UCD_BF16 ? 2 : 4;
  UCD_REQUIRE(aligned16(x_s) && aligned16(x_t) && aligned16(d_x) && ((size_t)ld_s * es) % 16 == 0 && ((size_t)ld_t * es) % 16 == 0 &&
                  ((size_t)ld_d * es) % 16 == 0,
              UCD_EALIGN, "%s: the maps must be 16-byte aligned with 16-byte multiple row pitches", fn);
  UCD_REQUIRE(workspace && workspace_bytes >= ucd_attn_mse_workspace_bytes(B, HW), UCD_EWORKSPACE, "%s: workspace too small", fn);
  hipStream_t s = (hipStream_t)stream;
  const int M = B * HW, blocks = ceil_div(M, kFdRows);
  float* a = (float*)workspace;
  float* inv = a + 2 * (size_t)M;
  float* part = inv + 2 * (size_t)B;
  unsigned int* ticket = reinterpret_cast<unsigned int*>(part + blocks);
  const double count = (double)B * HW * C;
  const float grad_scale = (float)(2.0 * (double)weight / count);
  if (dtype == UCD_BF16)
    fd_rowsq_kernel<__hip_bfloat16><<<dim3(blocks, 2), kFdBlock, 0, s>>>((const __hip_bfloat16*)x_s, ld_s, (const __hip_bfloat16*)x_t,
                                                                         ld_t, M, C, a);
  else
    fd_rowsq_kernel<float><<<dim3(blocks, 2), kFdBlock, 0, s>>>((const float*)x_s, ld_s, (const float*)x_t, ld_t, M, C, a);
  int rc = check_launch(fn);
  if (rc) return rc;
  fd_norm_kernel<<<dim3(B, 2), kFdBlock, 0, s>>>(a, M, HW, B, inv, ticket);
  rc = check_launch(fn);
  if (rc) return rc;
  if (dtype == UCD_BF16)
    fd_loss_kernel<__hip_bfloat16><<<blocks, kFdBlock, 0, s>>>((const __hip_bfloat16*)x_s, ld_s, (const __hip_bfloat16*)x_t, ld_t, M, HW,
                                                               B, C, a, inv, grad_scale, 1.0 / count, (__hip_bfloat16*)d_x, ld_d, part,
                                                               ticket, loss_out);
  else
    fd_loss_kernel<float><<<blocks, kFdBlock, 0, s>>>((const float*)x_s, ld_s, (const float*)x_t, ld_t, M, HW, B, C, a, inv, grad_scale,
                                                      1.0 / count, (float*)d_x, ld_d, part, ticket, loss_out);
  return check_launch(fn);
}

}  // extern "C"
