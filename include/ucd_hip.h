/*
 * ucd_hip.h - C ABI of libucd_hip.so: the MI355X (gfx950) kernels of the UCD train-step hot path.
 *
 * The reference (ygjwd12345/UCD) has no FFI layer of its own: its native work enters through the
 * third-party wheels inplace-abn / apex and through ~40 stock PyTorch kernels per loss.  Each entry
 * point below names the reference call site (file:line under the reference tree) whose device work
 * it replaces; INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch); nothing is allocated, freed or
 *     retained past the call; workspaces are caller-provided and sized by the *_workspace_bytes calls;
 *   - every call is asynchronous on the given hipStream_t (passed as void*), re-entrant, and makes
 *     no host synchronisation (data-dependent sizes such as the anchor count stay on the device);
 *   - return 0 on success, a negative UCD_E* code for argument errors, or the positive hipError_t of
 *     a failed launch; ucd_last_error() returns the thread-local message; no C++ exception crosses;
 *   - activations ("act" tensors) are channels-last: a [B,C,H,W] map is the row-major matrix
 *     [M = B*H*W rows][C channels] with a leading dimension `ld` in ELEMENTS (ld >= C, so a channel
 *     slice of a wider buffer can be addressed); dtype is UCD_F32 or UCD_BF16; base pointers and
 *     ld*sizeof(elem) must be 16-byte aligned and C a multiple of 16/sizeof(elem);
 *   - per-channel parameters and statistics are float32.
 */
#ifndef UCD_HIP_H
#define UCD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UCD_VERSION 100 /* 0.1.0 */

typedef void* ucd_stream_t; /* hipStream_t */
typedef void* ucd_comm_t;   /* communicator owned by this library (ucd_comm_init: RCCL, optionally with an IPC mailbox) */

enum ucd_dtype { UCD_F32 = 0, UCD_BF16 = 1 };
enum ucd_act { UCD_ACT_IDENTITY = 0, UCD_ACT_LEAKY_RELU = 1, UCD_ACT_ELU = 2 /* slope = alpha */ };
/* Flag bits OR-ed into an `act` (or `flags`) argument.  UCD_NORM_ABS_GAMMA selects the parameterisation of
 * inplace_abn's InPlaceABN / InPlaceABNSync, gamma~ = |weight| + eps in place of weight (their published forward;
 * d weight = sign(weight) * sum dz*xhat, sign(0) = +1); without it the layer is F.batch_norm (inplace_abn.ABN). */
#define UCD_ACT_MASK 0xff
#define UCD_NORM_ABS_GAMMA 0x100
/* UCD_PIXCON_F16_SPLIT: the fp16 path forced onto its fixed-split kernels (what UCD_PIXCON_F16 falls back to for
 * T < 0.06, more than 32 teacher classes or more than 1023 anchor blocks); kept selectable as the A/B reference. */
enum ucd_pixcon_precision { UCD_PIXCON_F32 = 0, UCD_PIXCON_F16 = 1, UCD_PIXCON_F16_SPLIT = 2 };
enum ucd_error {
  UCD_OK = 0,
  UCD_EINVAL = -1,      /* bad argument (null pointer, negative size, unknown enum) */
  UCD_EALIGN = -2,      /* pointer / leading dimension / channel count not 16-byte friendly */
  UCD_EWORKSPACE = -3,  /* workspace too small */
  UCD_EUNSUPPORTED = -4, /* shape outside what the kernels are built for */
  UCD_ETIMEOUT = -5     /* a mailbox exchange of the communicator timed out earlier (a rank never wrote): the communicator is dead */
#define UCD_ERCCL_BASE 100000 /* RCCL failures are returned as UCD_ERCCL_BASE + ncclResult_t */
#define UCD_EBLAS_BASE 200000 /* hipBLASLt failures are returned as UCD_EBLAS_BASE + hipblasStatus_t */
};

int ucd_version(void);
const char* ucd_last_error(void);
/* `bytes` zero bytes at `ptr`, in stream order (one memset node when the stream is being captured): the per-step fill of the
 * statistics arena (ucd_conv1x1_desc.stat_acc; csrc/abn_node.cpp) - a plain memset, so no tensor version counter moves. */
int ucd_fill_zero(void* ptr, size_t bytes, ucd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * ABN: fused BatchNorm + LeakyReLU(slope) / identity.  Replaces the inplace-abn==1.0.7 CUDA extension
 * behind every norm_act(...) instance: models/resnet.py:60, modules/residual.py:51,56,64,68,71,81,
 * modules/deeplab.py:30,33,37 (selected at segmentation_module.py:15-20), plus the glue the reference
 * runs as separate kernels around it: residual add + activation (modules/residual.py:90-97), channel
 * concatenation (modules/deeplab.py:56) and the pooled-branch broadcast add (modules/deeplab.py:65-68).
 *
 *   z = (x [+ plane_bias[b, c]] - mean[c]) * scale[c] + shift[c] [+ residual]      y = act(z)
 * ---------------------------------------------------------------------------------------------- */

/* bytes of scratch needed by ucd_abn_stats / ucd_abn_bwd_reduce for an [M, C] map */
size_t ucd_abn_workspace_bytes(int M, int C);

/* Per-channel sums over the M rows, taken about k[c] = x'[row 0, c] ("shifted data": E[x^2] - E[x]^2
 * cancels catastrophically in float32 when |mean| >> std):
 *   sums[0:C] = sum (x' - k), sums[C:2C] = sum (x' - k)^2, kshift[0:C] = k,
 * with x' = x + plane_bias[row / HW, c] (plane_bias may be NULL).  Deterministic two-stage reduction. */
int ucd_abn_stats(const void* x, int ld_x, int dtype, int M, int C,
                  const float* plane_bias, int HW,
                  float* sums /* [2*C] */, float* kshift /* [C] */,
                  void* workspace, size_t workspace_bytes, ucd_stream_t stream);

/* ucd_abn_stats followed by ucd_abn_finalize with count = M, in one launch sequence less (the stage-2
 * reduction finalises its own channels): the single-process training forward. */
int ucd_abn_stats_finalize(const void* x, int ld_x, int dtype, int M, int C, const float* plane_bias, int HW,
                           float* sums, float* kshift, const float* weight,
                           float* running_mean, float* running_var, float momentum, float eps,
                           float* mean, float* invstd, float* scale, int flags /* 0 or UCD_NORM_ABS_GAMMA */,
                           void* workspace, size_t workspace_bytes, ucd_stream_t stream);

/* Batch statistics -> normalisation constants.  With d = sums[c]/count:
 *   mean = kshift + d,  var = (sums[C+c] - sums[c]*d)/count (biased),  invstd = 1/sqrt(var + eps),
 *   scale = weight * invstd ((|weight| + eps) * invstd with flags = UCD_NORM_ABS_GAMMA);  running_mean / running_var
 *   are updated in place with `momentum` (unbiased variance) unless NULL.  kshift NULL means 0; weight NULL means 1.
 * For statistics combined across ranks pass kshift = global mean, sums[0:C] = 0, sums[C:2C] = global M2. */
int ucd_abn_finalize(const float* sums, const float* kshift, float count, int C, const float* weight,
                     float* running_mean, float* running_var, float momentum, float eps,
                     float* mean, float* invstd, float* scale, int flags, ucd_stream_t stream);

/* Evaluation mode (teacher; --fix_bn): invstd = 1/sqrt(running_var + eps), scale = weight * invstd; the
 * mean is running_mean itself. */
int ucd_abn_eval_params(const float* weight, const float* running_var, float eps, int C,
                        float* invstd, float* scale, int flags /* 0 or UCD_NORM_ABS_GAMMA */, ucd_stream_t stream);

/* y = act((x + plane_bias - mean) * scale + shift + residual); shift is the affine bias (NULL = 0);
 * y may alias x (in place) or be a channel slice of a wider buffer (ld_y > C); residual / plane_bias
 * may be NULL.  Subtracting the mean first keeps the result exact when x is close to it.
 * This call, ucd_abn_bwd_reduce and ucd_abn_bwd_apply run on packed fp32 pairs for every dtype, activation and plane-bias form
 * (the operations of a per-element loop in the same order: bit-identical to one). */
int ucd_abn_apply(const void* x, int ld_x, void* y, int ld_y, const void* residual, int ld_r,
                  int dtype, int M, int C, const float* plane_bias, int HW,
                  const float* mean, const float* scale, const float* shift, int act, float slope,
                  ucd_stream_t stream);

/* Backward, stage 1: dz = dy * act'(z) and the two per-channel sums
 *   sums[0:C] = sum dz            (= d bias)
 *   sums[C:2C] = sum dz * xhat    (= d weight),   xhat = (x' - mean) * invstd.
 * The sign of z is taken from y when y != NULL (needed when a residual was fused), else z =
 * (x' - mean) * scale + shift is recomputed from x (shift = the affine bias, NULL = 0).  With UCD_NORM_ABS_GAMMA in
 * `act`, sums[C:2C] is multiplied by sign(weight[c]) (d weight of gamma~ = |weight| + eps); ucd_abn_bwd_apply with the
 * same flag undoes the sign, so the pair stays consistent (also across an all-reduce: the sign is rank-independent). */
int ucd_abn_bwd_reduce(const void* x, int ld_x, const void* dy, int ld_dy, const void* y, int ld_y,
                       int dtype, int M, int C, const float* plane_bias, int HW,
                       const float* mean, const float* invstd, const float* scale, const float* shift,
                       const float* weight /* read only with UCD_NORM_ABS_GAMMA */, int act, float slope,
                       float* sums /* [2*C] */, void* workspace, size_t workspace_bytes, ucd_stream_t stream);

/* Backward, stage 2: dx = (dz - sums[0]/count - xhat * sums[1]/count) * weight * invstd
 * (training statistics) or dx = dz * scale when frozen != 0 (running statistics).  dz_out, when not
 * NULL, receives dz (the gradient of the fused residual input).  dx may alias dy. */
int ucd_abn_bwd_apply(const void* x, int ld_x, const void* dy, int ld_dy, const void* y, int ld_y,
                      void* dx, int ld_dx, void* dz_out, int ld_dz,
                      int dtype, int M, int C, const float* plane_bias, int HW,
                      const float* mean, const float* invstd, const float* scale, const float* shift,
                      const float* weight, const float* sums, float count, int frozen,
                      int act, float slope, ucd_stream_t stream);

/* Apply pass that FINALISES the statistics itself (round 5, bf16 activations, leaky_relu / identity): acc[0..C) = sum (x - k),
 * acc[C..2C) = sum (x - k)^2 over `count` rows (the atomic accumulator of ucd_conv1x1's statistics epilogue, all-reduced over the
 * ranks under SyncBN; `reps` replicas of [2 C], summed here), kshift[c] = k.  Every workgroup derives mean / invstd / scale of its channels in its prologue (2C loads);
 * the first row band also stores them to mean / invstd / scale (saved for the backward) and updates the running statistics
 * (momentum, unbiased variance) - what ucd_conv1x1_stats_finalize did in a launch of its own.  flags: UCD_NORM_ABS_GAMMA. */
int ucd_abn_apply_stats(const void* x, int ld_x, void* y, int ld_y, const void* residual, int ld_r, int M, int C,
                        const float* acc, int reps, const float* kshift, float count, const float* weight, const float* bias,
                        float* running_mean, float* running_var, float momentum, float eps, float* mean, float* invstd,
                        float* scale, int act, float slope, ucd_stream_t stream);

/* Backward apply on RAW sums (round 5, bf16): sums[0..C) = sum dz, sums[C..2C) = sum dz * xhat as accumulated by ucd_conv1x1's
 * out_mode 3 / 4 epilogues with stat_acc (no sign applied, all-reduced over the ranks under SyncBN; count = rows over all ranks).
 * grad_out (optional): [d bias | d weight] of the layer is written by the first row band from grad_sums (this rank's sums; NULL:
 * sums; both `reps` replicas of [2 C], summed in the prologue), d weight with the sign of weight under UCD_NORM_ABS_GAMMA - what ucd_abn_reduce_partials did in a launch of its own.
 * Arguments otherwise as ucd_abn_bwd_apply (training statistics; identity / leaky_relu). */
int ucd_abn_bwd_apply_raw(const void* x, int ld_x, const void* dy, int ld_dy, const void* y, int ld_y, void* dx, int ld_dx,
                          void* dz_out, int ld_dz, int M, int C, const float* mean, const float* invstd, const float* scale,
                          const float* shift, const float* weight, const float* sums, const float* grad_sums, int reps,
                          float* grad_out, float count, int act, float slope, ucd_stream_t stream);

/* Whole-layer forward in one call (single process): training != 0 -> ucd_abn_stats_finalize + ucd_abn_apply with
 * buf = [sums(2C) | kshift(C) | mean(C) | invstd(C) | scale(C)] (kept for the backward); training == 0 ->
 * running statistics, with [invstd | scale] taken from eval_consts when given (frozen teacher) or computed into buf. */
int ucd_abn_forward(const void* x, int ld_x, void* y, int ld_y, const void* residual, int ld_r,
                    int dtype, int M, int C, const float* plane_bias, int HW,
                    const float* weight, const float* bias, float* running_mean, float* running_var,
                    float momentum, float eps, int training, float* buf, const float* eval_consts,
                    int act, float slope, void* workspace, size_t workspace_bytes, ucd_stream_t stream);

/* Whole-layer backward in one call: ucd_abn_bwd_reduce (when training or need_sums) + ucd_abn_bwd_apply.
 * sums[0:C] = d bias, sums[C:2C] = d weight on return. */
int ucd_abn_backward(const void* x, int ld_x, const void* dy, int ld_dy, const void* y, int ld_y,
                     void* dx, int ld_dx, void* dz_out, int ld_dz, int dtype, int M, int C,
                     const float* plane_bias, int HW, const float* mean, const float* invstd,
                     const float* scale, const float* bias, const float* weight, float* sums, float count,
                     int training, int need_sums, int act, float slope,
                     void* workspace, size_t workspace_bytes, ucd_stream_t stream);

/* SyncBN across one-process-per-GPU ranks (InPlaceABNSync, segmentation_module.py:17; the inplace-abn
 * extension all-reduces the statistics of every layer in forward and backward).  The collectives stay with the
 * caller (torch.distributed / RCCL); these are the library calls around them, equal row counts per rank:
 *
 *   forward   ucd_abn_sync_stats    pack[0:C] = mean_r, pack[C:2C] = M2_r = sum (x' - mean_r)^2 of this rank
 *             all_gather(pack)   -> gathered[world][2C]
 *             ucd_abn_sync_forward  Chan's combination (mean = avg mean_r, M2 = sum M2_r + M sum (mean_r - mean)^2),
 *                                   finalize with count = world * M into buf = [. . . | mean | invstd | scale]
 *                                   (same layout as ucd_abn_forward), running statistics update, then apply
 *   backward  ucd_abn_sync_bwd_reduce  sums = local_sums = [sum dz | sum dz xhat] of this rank
 *             all_reduce(sums)
 *             ucd_abn_bwd_apply with count = world * M    (local_sums are the rank's d bias / d weight) */
int ucd_abn_sync_stats(const void* x, int ld_x, int dtype, int M, int C, const float* plane_bias, int HW,
                       float* sums /* [2*C] scratch */, float* kshift /* [C] scratch */, float* pack /* [2*C] */,
                       void* workspace, size_t workspace_bytes, ucd_stream_t stream);
int ucd_abn_sync_forward(const void* x, int ld_x, void* y, int ld_y, const void* residual, int ld_r,
                         int dtype, int M, int C, const float* plane_bias, int HW,
                         const float* gathered /* [world][2*C] */, int world,
                         const float* weight, const float* bias, float* running_mean, float* running_var,
                         float momentum, float eps, float* buf /* [6*C] */, int act, float slope, ucd_stream_t stream);
int ucd_abn_sync_bwd_reduce(const void* x, int ld_x, const void* dy, int ld_dy, const void* y, int ld_y,
                            int dtype, int M, int C, const float* plane_bias, int HW,
                            const float* mean, const float* invstd, const float* scale, const float* shift,
                            const float* weight, int act, float slope, float* sums /* [2*C] */, float* local_sums /* [2*C] */,
                            void* workspace, size_t workspace_bytes, ucd_stream_t stream);

/* ---- row-major bf16 GEMMs of the wide 1x1 convolutions (modules/residual.py:57-63 builds them as nn.Conv2d(k=1);
 * on the channels-last row matrix [B*H*W, C] they are plain GEMMs), fp32 accumulation, bf16 output, through hipBLASLt
 * with the algorithm picked once per shape by timing the library's candidates (tune != 0) and cached:
 *   mode 0:  C[M,N] = A[M,K] . B[N,K]^T     forward          rows x weight^T
 *   mode 1:  C[M,N] = A[M,K] . B[K,N]       input gradient   dY x weight
 *   mode 2:  C[M,N] = A[K,M]^T . B[K,N]     weight gradient  dY^T x rows   (K = B*H*W)
 * lda/ldb/ldc = row pitch in elements.  ucd_gemm_load binds hipBLASLt from the shared object the process already uses. */
int ucd_gemm_load(const char* hipblaslt_path);
size_t ucd_gemm_workspace_bytes(void);
int ucd_gemm_bf16(int mode, int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C, int ldc,
                  void* workspace, size_t workspace_bytes, int tune, ucd_stream_t stream);
/* C += op(A) op(B) with the plan ucd_gemm_bf16 holds for the shape (the residual-branch gradient folded into the input
 * gradient of a block's first 1x1 convolution); never tunes - warm the shape through ucd_gemm_bf16 first
 * (ucd_gemm_has_plan tells) or it takes the library's first suggestion */
int ucd_gemm_bf16_acc(int mode, int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C, int ldc,
                      void* workspace, size_t workspace_bytes, ucd_stream_t stream);
int ucd_gemm_has_plan(int mode, int M, int N, int K, int lda, int ldb, int ldc);
float ucd_gemm_last_tuned_us(void);
int ucd_gemm_last_candidates(void);

/* ---- library-owned RCCL communicator (one process per GPU) ------------------------------------------
 * Replaces the per-layer torch.distributed collectives of InPlaceABNSync (the reference reaches NCCL through the
 * inplace-abn extension, segmentation_module.py:17): the exchange runs on the caller's stream inside the layer call.
 *   ucd_comm_load(path)      bind RCCL from the shared object the process already uses (NULL/"" = default search)
 *   rank 0: ucd_comm_unique_id(id, 128); every rank receives the 128 bytes (e.g. one torch.distributed broadcast)
 *   every rank: ucd_comm_init(id, 128, nranks, rank, &comm)         (collective; current HIP device = the rank's GPU) */
int ucd_comm_load(const char* rccl_path);
int ucd_comm_unique_id(void* id_out, size_t bytes);
int ucd_comm_init(const void* id, size_t bytes, int nranks, int rank, ucd_comm_t* comm_out);
int ucd_comm_destroy(ucd_comm_t comm);
int ucd_comm_all_gather(ucd_comm_t comm, const float* send, float* recv /* [nranks*count] */, size_t count,
                        ucd_stream_t stream);
int ucd_comm_all_reduce_sum(ucd_comm_t comm, float* buf, size_t count, ucd_stream_t stream);

/* One-shot mailbox exchange for the small collectives (round 5; SURVEY section 7 hard part 1): every rank owns a mailbox in device
 * memory shared through hipIpcMemHandle; ucd_comm_all_gather / ucd_comm_all_reduce_sum of at most `slot_floats` floats then run as
 * ONE kernel of one workgroup on the caller's stream - peer stores, system-scope fence, sequence flags, bounded spin, sum in rank
 * order (bit-identical on every rank) - instead of an RCCL call; larger messages keep RCCL.  Set-up (every rank, collective):
 *   ucd_comm_init (RCCL underneath) or ucd_comm_init_local (no RCCL: mailbox only - several ranks on ONE GPU, which RCCL refuses)
 *   ucd_comm_ipc_create(comm, slot_floats, timeout_ms, handle)  -> exchange the ucd_comm_ipc_handle_bytes() bytes of every rank
 *   ucd_comm_ipc_connect(comm, handles)      handles = [nranks][handle bytes] in rank order
 * A peer that never writes makes the kernel give up after timeout_ms (<= 0: 2 s).  It then (round 6) writes NaN into its output,
 * latches a word in pinned host memory (ucd_comm_ipc_timeouts; every later host-issued collective on the communicator returns
 * UCD_ETIMEOUT) and poisons the mailbox of EVERY rank: all later exchange kernels of the communicator - replayed graphs included -
 * return NaN at once instead of waiting.  The mailbox lives in fine-grained device memory; where that cannot be allocated
 * ucd_comm_ipc_create fails (no coarse-grained fallback) and the caller keeps RCCL.  ucd_comm_ipc_drop removes the mailbox
 * (the collectives go back to RCCL).  ONE stream at a time per communicator: exchanges of one mailbox must be stream-ordered. */
int ucd_comm_init_local(int nranks, int rank, ucd_comm_t* comm_out);
size_t ucd_comm_ipc_handle_bytes(void);
int ucd_comm_ipc_create(ucd_comm_t comm, int slot_floats, int timeout_ms, void* handle_out);
int ucd_comm_ipc_connect(ucd_comm_t comm, const void* handles);
int ucd_comm_ipc_drop(ucd_comm_t comm);
unsigned ucd_comm_ipc_timeouts(ucd_comm_t comm);

/* Whole SyncBN layer in one call each way, collectives included (comm from ucd_comm_init, world = its size):
 *   forward   ucd_abn_sync_stats -> all-gather -> ucd_abn_sync_forward; buf = [6*C | pack 2*C | gathered world*2*C]
 *   backward  ucd_abn_sync_bwd_reduce -> all-reduce -> ucd_abn_bwd_apply(count = world*M);
 *             sums [2*C] = the global sums on return, local_sums [2*C] = this rank's [d bias | d weight]
 *             (may point straight at the parameters' gradient storage) */
int ucd_abn_sync_forward_comm(ucd_comm_t comm, int world, const void* x, int ld_x, void* y, int ld_y,
                              const void* residual, int ld_r, int dtype, int M, int C, const float* plane_bias, int HW,
                              const float* weight, const float* bias, float* running_mean, float* running_var,
                              float momentum, float eps, float* buf, int act, float slope,
                              void* workspace, size_t workspace_bytes, ucd_stream_t stream);
int ucd_abn_sync_backward_comm(ucd_comm_t comm, int world, const void* x, int ld_x, const void* dy, int ld_dy,
                               const void* y, int ld_y, void* dx, int ld_dx, void* dz_out, int ld_dz, int dtype, int M,
                               int C, const float* plane_bias, int HW, const float* mean, const float* invstd,
                               const float* scale, const float* bias, const float* weight, float* sums,
                               float* local_sums, int act, float slope, void* workspace, size_t workspace_bytes,
                               ucd_stream_t stream);

/* Per-(image, channel) reduction over the HW rows of each image: out[b, c] = alpha * sum_hw x.
 * Global average pooling of the ASPP image-level branch (modules/deeplab.py:72-76) with alpha = 1/HW,
 * and the gradient of a plane_bias (sum of dz over the plane) with alpha = 1. */
int ucd_plane_sum(const void* x, int ld_x, int dtype, int B, int HW, int C, float alpha,
                  float* out /* [B, C] */, ucd_stream_t stream);

/* Sliding-window mean with stride 1 and no padding: out[b, oy, ox, c] = mean of the ph x pw window of x at (oy, ox);
 * out is [B, H-ph+1, W-pw+1, C] channels-last.  Replaces F.avg_pool2d(x, (ph, pw), stride=1) of the image-pooling branch in
 * evaluation mode (modules/deeplab.py:77-83; the teacher at 513^2 and 768^2, --pooling 32) with one read of the map. */
size_t ucd_window_mean_workspace_bytes(int B, int H, int W, int C, int ph);
int ucd_window_mean(const void* x, int ld_x, int dtype, int B, int H, int W, int C, int ph, int pw, void* out, int ld_out,
                    void* workspace, size_t workspace_bytes, ucd_stream_t stream);

/* Spatial attention map (segmentation_module.py:86-94): a[b,p] = sum_c x^2, normalised per image by
 * its Frobenius norm; y = a * x.  workspace: B*HW + B floats. */
size_t ucd_attmap_workspace_bytes(int B, int HW);
int ucd_attmap(const void* x, int ld_x, void* y, int ld_y, int dtype, int B, int HW, int C,
               void* workspace, size_t workspace_bytes, ucd_stream_t stream);

/* ILT's encoder distillation term (train.py:129 of the reference) on the RAW maps, the attention weighting of both included:
 *   att(x) = a * x with a as in ucd_attmap (detached);   loss_out[0] = mean over B HW C of (a_s x_s - a_t x_t)^2;
 *   d_x = weight * 2 a_s (a_s x_s - a_t x_t) / (B HW C)   in the input dtype (the gradient of weight * loss w.r.t. x_s).
 * x_s / x_t / d_x are channels-last rows [B*HW, C] (dtype UCD_F32 or UCD_BF16, the same for all three) with leading dimensions
 * in elements; base pointers and row pitches 16-byte aligned, C itself is free (a scalar tail follows the 16-byte vectors).
 * Three launches: per-pixel sums of squares of both maps, per-image norms, one pass that reads both maps once, writes d_x and
 * reduces the loss in a fixed order (per-workgroup partials in the workspace, added in index order by the workgroup that
 * finishes last; no float atomics): same inputs, same bits.  HBM traffic: 2 reads of each map + 1 write.
 * Errors (checked on the host before any device call): UCD_EINVAL (NULL x_s / x_t / loss_out / d_x, unknown dtype, B / HW / C
 * below 1, a leading dimension below C), UCD_EALIGN, UCD_EWORKSPACE (NULL or short workspace). */
size_t ucd_attn_mse_workspace_bytes(int B, int HW);
int ucd_attn_mse(const void* x_s, int ld_s, const void* x_t, int ld_t, int dtype, int B, int HW, int C, float weight,
                 float* loss_out, void* d_x, int ld_d, void* workspace, size_t workspace_bytes, ucd_stream_t stream);

/* Local POD feature distillation (PLOP) for one level: a student and a teacher map [B, h, w, C] as channels-last rows (dtype
 * UCD_F32 or UCD_BF16, the same for both; row pitches in elements, at least C; base pointers and row pitches 16-byte aligned), a
 * slope in (0, 1] and n scales, 1 <= n <= 4, each in 1 .. 8, strictly increasing, h and w at least the largest (csrc/pod.hip).
 *   P = X >= 0 ? X : X / slope,  Q = P^2;  per scale s, kh = h / s, kw = w / s, region (i, j) = rows [i kh, (i+1) kh) x columns
 *   [j kw, (j+1) kw): the mean of Q over the region's columns per (channel, row) and over its rows per (channel, column);
 *   E_b = all of them, n_E = sum_s s^2 C (kh + kw) values;  E^ = E / max(|E|, 1e-12);  l_b = |E^_s - E^_t|;
 *   loss_out[0] = mean_b l_b;  g_E [B][n_E] = d(weight * loss_out) / d E_s, each entry already divided by its pool's count.
 * The forward pass is four launches: one trip over both maps (16-byte loads, lanes over channels) that leaves scale-free partial
 * row and column sums per tile, then three strip kernels (pool, difference, coefficients).  The backward pass is one launch:
 *   d_x = grad_out[0] * 2 P dQ (X >= 0 ? 1 : 1 / slope),  dQ = the g_E entries of the pools that hold the element, summed,
 * one read of the student map and one write of d_x (map dtype).  grad_out is a device scalar.  Strip sums are fp32, norms and dot
 * products fp64, every sum in a fixed order, no atomics: same inputs, same bits.  No allocation, no host synchronisation: the
 * calls capture into graphs.  l_b = 0 and E = 0 give a zero loss term and zero coefficients.
 * The plan is a pure host function (no device is touched): n_E, the workspace bytes of the forward pass for B samples and
 * grid[4] = {workgroups of the tile pass per map (and of the backward pass), workgroups per sample of the strip kernels, row
 * pieces, column pieces}; output pointers may be NULL.
 * Supported C: every multiple of 8 up to 8192; h, w up to 1024.
 * Checked on the host before any device call, the message names the argument: UCD_EINVAL (a NULL pointer; B or C below 1; n
 * outside 1 .. 4; a scale outside 1 .. 8 or not above the one before; h or w below the largest scale; a slope outside (0, 1]; an
 * unknown dtype; a row pitch below C), UCD_EUNSUPPORTED (C not a multiple of 8 or above 8192; h or w above 1024), UCD_EALIGN,
 * UCD_EWORKSPACE (NULL, unaligned or short workspace); else the hipError_t of a failed launch. */
int ucd_pod_plan(int h, int w, int C, const int* scales, int n, int B, int dtype, int* n_E, size_t* workspace_bytes, int* grid);
int ucd_pod_forward(const void* x_s, int ld_s, const void* x_t, int ld_t, int dtype, int B, int C, int h, int w, float slope,
                    const int* scales, int n, float weight, float* loss_out, float* g_E, void* workspace, size_t workspace_bytes,
                    ucd_stream_t stream);
int ucd_pod_backward(const void* x_s, int ld_s, int dtype, int B, int C, int h, int w, float slope, const int* scales, int n,
                     const float* g_E, const float* grad_out, void* d_x, int ld_d, ucd_stream_t stream);

/* Local POD on the logits (PLOP's last level, `extra_channels: "sum"`): student rows [B, h, w, Ctot] and teacher rows [B, h, w, K],
 * 1 <= K <= Ctot <= 256, channels-last fp32 (dtype must be UCD_F32), row pitches in elements, at least the channel count; base
 * pointers need 4-byte alignment only and the pitches are free (a dense row of 21 logits is 84 bytes).
 *   M[0] = S[0] + sum_{c >= K} S[c] (the sum first, in ascending c, fp32), M[k] = S[k] for 1 <= k < K; K == Ctot: M = S;
 *   Q_s = M^2, Q_t = T^2; the pools, E and g_E are those of ucd_pod_forward with C = K and slope 1: n_E = sum_s s^2 K (kh + kw);
 *   normalize = 1: E^, l_b and g_E as above;  normalize = 0: l_b = |E_s - E_t|, g_E = weight / B * (E_s - E_t) / l_b (0 where
 *   l_b = 0), each entry divided by its pool's count;  loss_out[0] = mean_b l_b.
 *   d_x[c] = grad_out[0] * 2 M[k(c)] dQ[k(c)], k(c) = c below K and 0 from K on: channel 0 and every new-class channel of a pixel
 *   receive the same bits.  d_x is fp32 with its own pitch ld_d >= Ctot.  The backward call takes no normalize: g_E carries it.
 * Four launches forward (a tile pass of its own, then the three strip kernels of ucd_pod_forward on K-channel strips; normalize = 0
 * is an arm of the last two), one backward.  Each call picks its load width - 16, 8 or 4 bytes per lane - per map from the base
 * pointer, the pitch and the channel count it is given; a group of lanes (the power of two that holds a pixel's channels, at most
 * 64) walks one tile, its load covering one contiguous stretch of a row, and every lane of the group adds the new-class channels
 * in ascending order from the lanes that loaded them.  Each element of both maps is read once forward; backward reads each
 * student element once and writes each d_x element once.  Fixed summation order, no atomics: same inputs, same bits.  No
 * allocation, no host synchronisation: the calls capture into graphs.
 * The plan is a pure host function: n_E, the forward workspace bytes for B samples and grid[4] = {workgroups of the tile pass per
 * map for dense 16-byte aligned rows, workgroups per sample of the strip kernels, row pieces, column pieces}; output pointers may
 * be NULL.
 * Checked on the host before any device call, the message names the argument: UCD_EINVAL (a NULL pointer; B or K below 1; K above
 * Ctot; a row pitch below its channel count; n outside 1 .. 4, a scale outside 1 .. 8 or not above the one before, h or w below
 * the largest scale; normalize neither 0 nor 1), UCD_EUNSUPPORTED (Ctot above 256; a dtype other than UCD_F32; h or w above 1024),
 * UCD_EALIGN (a pointer that is not 4-byte aligned), UCD_EWORKSPACE (NULL, not 16-byte aligned or short workspace); else the
 * hipError_t of a failed launch. */
int ucd_pod_logits_plan(int h, int w, int Ctot, int K, const int* scales, int n, int B, int normalize, int* n_E,
                        size_t* workspace_bytes, int* grid);
int ucd_pod_logits_forward(const void* x_s, int ld_s, const void* x_t, int ld_t, int dtype, int B, int Ctot, int K, int h, int w,
                           const int* scales, int n, int normalize, float weight, float* loss_out, float* g_E, void* workspace,
                           size_t workspace_bytes, ucd_stream_t stream);
int ucd_pod_logits_backward(const void* x_s, int ld_s, int dtype, int B, int Ctot, int K, int h, int w, const int* scales, int n,
                            const float* g_E, const float* grad_out, float* d_x, int ld_d, ucd_stream_t stream);

/* SDR's class-prototype feature losses (Michieli and Zanuttigh, CVPR 2021: prototype matching, feature clustering, prototype
 * repulsion) on one feature level: the raw pre-logits X [M = B h w rows][C] as channels-last rows (UCD_F32 or UCD_BF16, row pitch in
 * elements, at least C; base pointer and pitch 16-byte aligned), T classes of the step, K <= T teacher classes (csrc/proto.hip).
 *   classify: cls[p] of the low-resolution pixel p = (b, i, j): y = labels[b, sy, sx], sy = min((int)floorf(i * ((float)H / h)), H - 1)
 *     and sx likewise (F.interpolate(mode='nearest')); -1 where y == ignore_index or y outside [0, T); with teacher rows (sem_t [B h w]
 *     [K] fp32, pitch ld_t >= K; NULL: no teacher) and y == 0 the first arg-max of sem_t[p, 0..K) (torch's rule; may be 0); else y.
 *   n_c = #{p : cls_p = c}, S_c = sum_{cls_p = c} X_p, mu_c = S_c / n_c;  R_c = state_sum_c / state_n_c where state_n_c > 0 (the
 *   running prototypes as they stood before this batch: state_sum [T, C] fp64, state_n [T] int64);  O [K, C] fp32 with old_valid [K]
 *   bytes (non-zero: valid), the previous step's prototypes (both may be NULL for K = 0).  Every |.| is the L2 norm over C:
 *     L_match = 1/|A|  sum_{c in A}  |mu_c - O_c|,                                  A  = {c < K : n_c > 0, valid_c}
 *     L_attr  = 1/|Bs| sum_{c in Bs} 1/n_c sum_{cls_p = c} |X_p - R_c|^2,           Bs = {c : n_c > 0, state_n_c > 0}
 *     L_rep   = 1/|P|  sum_{c in P}  sum_{k in P, k != c} 1 / (|mu_c - mu_k| + 1e-6),  P = {c : n_c > 0}; 0 for |P| < 2
 *   an empty index set gives 0 and no gradient, and so does a zero distance.  X_p - R_c is formed per element: X_p == R_c on every row
 *   gives L_attr == 0 exactly.
 *   forward: loss_out[4] = {w_m L_match + w_a L_attr + w_r L_rep, L_match, L_attr, L_rep};  batch_sums [T, C] fp64 = S, batch_n [T]
 *     int64 = n (what ucd_proto_update adds to the state, in a call of its own: the loss is a pure function of its arguments);
 *     tables = a[T] | R[T, C] | G[T, C] fp32, (2 C + 1) T floats: a_c = 2 w_a / (|Bs| n_c) for c in Bs, R_c (0 where state_n_c = 0) and
 *     G_c = d(w_m L_match + w_r L_rep) / d mu_c ALREADY divided by n_c; rows of absent classes are 0.
 *   backward: d_x[p] = grad_out[0] * (a_c (X_p - R_c) + G_c) for c = cls_p in [0, T), 0 otherwise; d_x has the map's dtype and its own
 *     pitch ld_d >= C.  grad_out is a device scalar.
 *   update: state_sum += batch_sums, state_n += batch_n, element by element (fp64 and int64, no atomics).
 * Launches: classify one; forward three - one pass over X (16-byte loads, lanes over channels; each element read once; rows in pieces
 * of 64, ordered by class inside a piece, per-piece per-class sums of X and of (X - R_c)^2 and counts, only for the classes a piece
 * holds), one workgroup per class that adds the pieces in index order (fp64), one workgroup per class on [T, C] (fp64 distances; the
 * workgroup that finishes last, an integer ticket, adds the per-class values in class order); backward one (one read of X, one write
 * of d_x, the tables from L2); update one.  |A|, |Bs| and |P| stay on the device.  Every sum has a fixed order and there is no
 * floating-point atomic: same inputs, same bits.  No allocation, no host synchronisation: the calls capture into graphs.
 * The plan is a pure host function (no device is touched): the forward workspace bytes (per-piece slots for min(64, T) classes: at
 * most about 6 M C bytes, reached from T = 64 on), grid[4] = {workgroups of the pass over X, of the class kernel, of the prototype kernel, of the backward pass},
 * lds_bytes[3] = static LDS of the three forward kernels, pieces = ceil(M / 64); output pointers may be NULL.
 * Checked on the host before any device call, the message names the argument: UCD_EINVAL (a NULL pointer; a size below 1; a negative
 * K; K above T; an unknown dtype; a row pitch below C, or ld_t below K), UCD_EUNSUPPORTED (C not a multiple of 8 or above 512; T above
 * 256; M = B h w of 2^31 or more), UCD_EALIGN (x / d_x or their pitch not 16-byte aligned; another pointer not aligned to its
 * element), UCD_EWORKSPACE (NULL, not 16-byte aligned or short workspace); else the hipError_t of a failed launch. */
int ucd_proto_plan(long long M, int C, int T, int dtype, size_t* workspace_bytes, int* grid, int* lds_bytes, int* pieces);
int ucd_proto_classify(const int64_t* labels, int B, int H, int W, int h, int w, int T, int K, int ignore_index, const float* sem_t,
                       int ld_t, int32_t* cls, ucd_stream_t stream);
int ucd_proto_forward(const void* x, int ld_x, int dtype, const int32_t* cls, long long M, int C, int T, int K, const double* state_sum,
                      const int64_t* state_n, const float* old_proto, const unsigned char* old_valid, float w_m, float w_a, float w_r,
                      float* loss_out, float* tables, double* batch_sums, int64_t* batch_n, void* workspace, size_t workspace_bytes,
                      ucd_stream_t stream);
int ucd_proto_backward(const void* x, int ld_x, int dtype, const int32_t* cls, long long M, int C, int T, const float* tables,
                       const float* grad_out, void* d_x, int ld_d, ucd_stream_t stream);
int ucd_proto_update(double* state_sum, int64_t* state_n, const double* batch_sums, const int64_t* batch_n, int T, int C,
                     ucd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Uncertainty-weighted pixel-contrastive distillation.  Replaces pre_contractive_pixel
 * (utils/utils.py:256-393; twin utils/loss.py:258-395) and PixelConLossV2.forward
 * (utils/loss.py:412-466) - and, with shift_pos = 0, no teacher and no joint-probability weight,
 * PixelConLoss.forward of the dead file utils/loss_new.py:359-400.
 * ---------------------------------------------------------------------------------------------- */

/* Device-resident description of one batch's anchor / contrast sets, written by ucd_pixcon_prep and
 * read by the loss kernels (the host never needs it; tests copy it back). */
typedef struct ucd_pixcon_meta {
  int32_t A;        /* anchors: pixels with mixed label > 0                      (utils.py:358) */
  int32_t Co;       /* teacher-only contrast rows: kept pixels that are not new (utils.py:359) */
  int32_t min_new;  /* smallest down-sampled ground-truth label > 0              (utils.py:353) */
  int32_t n_new;    /* pixels with a ground-truth (new-class) label              (utils.py:352) */
  int32_t Apad;     /* A rounded up to the contrast tile (row offset of the teacher segment) */
  int32_t Cpad;     /* Apad + Co rounded up to the tile: rows of the contrast matrix */
  int32_t n_valid;  /* anchors with at least one positive (rows of the final mean, loss.py:465) */
  int32_t sorted;   /* rows grouped by label (sort_by_label) */
  /* with sorted != 0: rows [label_start_a[L], label_start_a[L+1]) of the anchor segment and rows
     Apad + [label_start_o[L], label_start_o[L+1]) of the teacher segment carry label L */
  int32_t label_start_a[257];
  int32_t label_start_o[257];
  int32_t label_count_a[256]; /* anchors per label */
  int32_t label_count_c[256]; /* contrast rows per label (anchors + teacher rows): num_i + 1 */
  int32_t reserved[2];
} ucd_pixcon_meta;

size_t ucd_pixcon_prep_workspace_bytes(int BHW, int K);

/* Stage 1 (utils/utils.py:264-268,352-359,367-371): per low-resolution pixel p of the [B,h,w] grid
 *   label_ds = trunc(bilinear(labels)) kept when in [0, max_label] else 0   (bit-exact float32
 *              arithmetic of torch's one-channel bilinear kernel, align_corners = False);
 *   mix      = label_ds, or the teacher arg-max where label_ds == 0;
 *   keep     = mix > 0;  keep_o = keep && label_ds == 0;
 * then order-preserving stream compaction.  sort_by_label != 0 additionally groups anchors and
 * teacher rows by label (stable), which is what the fused loss wants; 0 keeps the reference's pixel
 * order.  Outputs (all device):
 *   anchor_pix[BHW], old_pix[BHW]  : pixel index of anchor row r / teacher row r
 *   row_label[2*BHW + 2*tile]      : label of contrast row r (anchors first, teacher rows from
 *                                    meta->Apad), 255 for padding rows
 *   prob[BHW, K]                   : softmax of the teacher logits per pixel (float32)
 *   meta                           : counts, see above
 * teacher_logits is the [B*h*w, K] channels-last low-resolution teacher output ("sem",
 * segmentation_module.py:136) in float32 or bf16 with leading dimension ld_t. */
int ucd_pixcon_prep(const int64_t* labels, int B, int H, int W, int h, int w, int max_label,
                    const void* teacher_logits, int ld_t, int dtype_t, int K, int sort_by_label,
                    int32_t* anchor_pix, int32_t* old_pix, uint8_t* row_label, float* prob,
                    ucd_pixcon_meta* meta, void* workspace, size_t workspace_bytes, ucd_stream_t stream);

/* Stage 2 (utils/utils.py:361-364,372-375): gather the kept rows of the student (anchors) and teacher
 * (teacher-only rows) pre-logit maps, L2-normalise each row (F.normalize, eps 1e-12) and write the
 * contrast matrix chat[Cpad, ldc] (float32): rows [0, A) anchors, [Apad, Apad+Co) teacher rows,
 * zeros elsewhere (also columns N..ldc); inv_norm[r] = 1 / max(||row||, eps) for the anchors (needed
 * by the backward).  When pcat != NULL the teacher probabilities of the same pixels are gathered in
 * the same row order into pcat[Cpad, ldp] (columns K..ldp zero).
 * f_n / f_o are [B*h*w, N] channels-last maps (float32 or bf16). */
int ucd_pixcon_gather(const void* f_n, int ld_n, const void* f_o, int ld_o, int dtype, int BHW, int N,
                      const int32_t* anchor_pix, const int32_t* old_pix, const float* prob, int K,
                      const ucd_pixcon_meta* meta, float* chat, int ldc, float* pcat, int ldp,
                      void* ch16 /* fp16 [Cpad, ldc] copy of chat, or NULL */,
                      void* p16 /* fp16 [Cpad, 2, K rounded up to 16]: hi | lo split of pcat, or NULL */,
                      float* inv_norm, ucd_stream_t stream);

/* Enough for every path a call of this size can take (any precision, temperature and K): >= the workspace_bytes that
 * ucd_pixcon_loss_plan reports for it. */
size_t ucd_pixcon_loss_workspace_bytes(int BHW, int N, int K);

/* Which kernels serve a ucd_pixcon_loss call, and with what launch.  Touches no device (it answers on a machine without a
 * GPU); ucd_pixcon_loss takes its launch parameters from the same function.  For BHW pixels, K teacher classes, a
 * precision, use_prob and the temperature it returns the code ucd_pixcon_loss would return for these arguments and, on 0:
 *   path            enum ucd_pixcon_path
 *                   F32       K <= 110 (or use_prob == 0): the anchor block's probability rows are staged in LDS;
 *                   F32_WIDE  110 < K <= 255: they are read from pcat in global memory inside the class loop (same order of
 *                             the MFMA accumulation), so that the LDS holds two contrast tiles' rows only;
 *                   F16_PLANNED  UCD_PIXCON_F16 with T >= 0.06, at most 32 classes and fewer than 1024 anchor blocks;
 *                   F16_SPLIT    every other fp16 call, K <= 255
 *   class_chunk     classes per staged piece of the probability product; 0: no path chunks the classes
 *   nsplit1/2       grid.y of the negatives / positives sweep (grid.x = ceil(BHW / 128)); 0 for F16_PLANNED, whose persistent
 *                   grid is the device's CU count
 *   lds_sweep1/2    bytes of dynamic LDS of the two sweeps (at most 160 KiB)
 *   workspace_bytes what the path lays out in the workspace
 * Output pointers may be NULL.  Errors: UCD_EINVAL (BHW < 1, temperature <= 0, unknown precision, K < 0, K < 1 with use_prob),
 * UCD_EUNSUPPORTED (K > 255: row labels are bytes and 255 marks padding rows); the message states the bound. */
enum ucd_pixcon_path {
  UCD_PIXCON_PATH_F32 = 1,
  UCD_PIXCON_PATH_F32_WIDE = 2,
  UCD_PIXCON_PATH_F16_PLANNED = 3,
  UCD_PIXCON_PATH_F16_SPLIT = 4
};
int ucd_pixcon_loss_plan(int BHW, int K, int precision, int use_prob, float temperature, int* path, int* class_chunk,
                         int* nsplit1, int* nsplit2, size_t* lds_sweep1, size_t* lds_sweep2, size_t* workspace_bytes);

/* Loss and its gradient w.r.t. the normalised anchors in one launch sequence (utils/loss.py:435-466):
 *   S_ij = a_i . c_j / T;  neg_i = sum_j [la_i != lc_j] exp(S_ij)                     (un-shifted)
 *   m_i = max_j S_ij (shift_pos != 0) or 0;  S' = S - m_i;  pos_ij = [la_i == lc_j] - [j == i]
 *   P_ij = 1 when use_prob == 0 or (la_i >= min_new and lc_j >= min_new), else p_i . p_j
 *   loss = mean_{i: num_i != 0} ( - sum_j pos_ij P_ij (S'_ij - log(exp S'_ij + neg_i)) / num_i )
 *   grad_a[i, :] = d loss / d a_i  (closed form); grad_a may be NULL.
 * chat [Cpad, ldc] / pcat [Cpad, ldp] / row_label are the outputs of ucd_pixcon_prep + ucd_pixcon_gather
 * (ldc must be 256: feature rows zero-padded to 256 columns; ldp >= K rounded up to even).
 * loss_out[0] = loss, loss_out[1] = number of valid rows.  row_stats (optional, [3, BHW]) receives
 * neg_i, num_i and the per-row loss for inspection.
 * precision = UCD_PIXCON_F32: exact float32 MFMA (v_mfma_f32_32x32x2_f32) on chat / pcat - the parity
 * mode; UCD_PIXCON_F16: fp16 operands ch16 / p16 (from ucd_pixcon_gather), fp32 accumulation
 * (v_mfma_f32_32x32x16_f16, 16x the rate) with an online rescale of the negative sums - the
 * performance mode; loss within ~1e-4, gradients within ~1e-3 of the float32 path.
 * 1 <= K <= 255 with use_prob in every precision (ucd_pixcon_loss_plan names the kernels and their LDS). */
int ucd_pixcon_loss(const float* chat, int ldc, int N, const uint8_t* row_label,
                    const float* pcat, int ldp, int K, const void* ch16, const void* p16, int precision,
                    const ucd_pixcon_meta* meta, int BHW,
                    float temperature, int shift_pos, int use_prob,
                    float* loss_out, float* grad_a /* [BHW, ldg] */, int ldg, float* row_stats,
                    void* workspace, size_t workspace_bytes, ucd_stream_t stream);

/* The same loss with the weight matrix P MATERIALISED by the caller: the literal signature of the reference's
 * PixelConLossV2.forward(anchor_features, contrast_feature, anchor_labels, contrast_labels, P) (utils/loss.py:412), for
 * callers that hold plain tensors instead of a prepared batch.  chat [Cpad, 256] holds the anchors in rows [0, A) and the
 * remaining contrast rows (contrast_feature[A:]) in rows [meta->Apad, meta->Apad + Co); contrast_feature[:A] must be the
 * anchors themselves (the reference's construction, utils/utils.py:362; its self-pair mask `mask_p[:, :A] -= eye`
 * assumes it).  P is [A, A + Co] row-major in the reference's column order with leading dimension ld_P, or NULL for
 * P = 1; rows need not be normalised (the row maximum of S is computed, not assumed).  meta: A, Co, Apad, Cpad,
 * n_valid, sorted = 0 and label_count_c must be filled (device memory); max_anchors sizes the workspace
 * (ucd_pixcon_loss_workspace_bytes(max_anchors, N, 0)) and must be >= A.  float32 MFMA path only. */
int ucd_pixcon_loss_given_p(const float* chat, int ldc, int N, const uint8_t* row_label, const float* P, int ld_P,
                            const ucd_pixcon_meta* meta, int max_anchors, float temperature, int shift_pos,
                            float* loss_out, float* grad_a, int ldg, float* row_stats,
                            void* workspace, size_t workspace_bytes, ucd_stream_t stream);

/* Chain rule through F.normalize and scatter to the student map:
 *   d f_n[pix(r), :] = grad_scale[0] * inv_norm[r] * (g_r - (g_r . a_r) a_r),  zero for unkept pixels.
 * grad_scale is a device scalar (the upstream gradient of the loss).  d_f_n has dtype `dtype`. */
int ucd_pixcon_scatter_grad(const float* grad_a, const float* chat, int ldc, const float* inv_norm,
                            const int32_t* anchor_pix, const ucd_pixcon_meta* meta,
                            const float* grad_scale, void* d_f_n, int ld_d, int dtype, int BHW, int N,
                            ucd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fused full-resolution logit losses.  Replaces, in one pass over the label map,
 * the bilinear up-sampling of the student and teacher logits (segmentation_module.py:133),
 * UnbiasedCrossEntropy (utils/loss.py:96-109; reduction 'none' then .mean() over ALL pixels, train.py:116)
 * and UnbiasedKnowledgeDistillationLoss (utils/loss.py:148-184, alpha = 1, reduction 'mean').
 *   sem_s [B*h*w, Ctot] / sem_t [B*h*w, K] : low-resolution student / teacher logits, float32 rows
 *   (sem_t may be NULL: cross entropy only; K = number of old classes incl. background, >= 1)
 *   loss_out[0] = mean CE, loss_out[1] = mean KD
 *   d_sem [B*h*w, ld_d] = d(ce_weight * CE + kd_weight * KD) / d sem_s   (overwritten)
 * Rows may be column slices of wider buffers: ld_s >= Ctot, ld_t >= K, ld_d >= Ctot in elements; columns past the class
 * counts are never read, and those of d_sem come back as zeros (the whole [B*h*w, ld_d] block is cleared first).
 *
 * Forms (ucd_seg_losses_plan names the one a call gets; enum ucd_seg_form):
 *   packed, Ctot <= 24:  (K <= 16, Ctot - K <= 8), (K <= 20, Ctot - K <= 4) or (K <= 12, Ctot - K <= 12), 64 x 64 pixel tiles;
 *   register, Ctot <= 24: any other split, a d_sem that is not 16-byte aligned, UCD_SEG_PK=0 (environment, read once per
 *            process), or a geometry whose packed form does not fit the LDS while this one does (21 classes at factor 8);
 *   many-class, Ctot > 24: 32 x 64 pixel tiles.
 * Gradient arithmetic.  The packed and the many-class form add every tile's contribution to a low-resolution cell as a 32-bit
 * FIXED-POINT word: integer addition has no order, so d_sem has the same bits on every run.  The quantum of a word is
 *   q = gmax / 2^17,  gmax = (|ce_weight| + 2 |kd_weight| / K) / (B H W)   (the largest gradient one pixel can contribute);
 *   (gmax is the same in every mode of ucd_seg_losses_ex: the plain distillation's per-pixel gradient |softmax_K(z)_c - q_c| / K is
 *   below |kd_weight| / (K B H W) per element, inside the 2 |kd_weight| / K that the unbiased form needs, and alpha only changes q)
 * a tile sums its pixels in fp64, rounds ONCE to the nearest word (error <= q / 2) and adds it; a cell receives one add from each
 * tile that touches it, at most n_tiles = (ceil(2 f_y / tile_y) + 1) (ceil(2 f_x / 64) + 1) for up-sampling factors f_y, f_x
 * (a cell's bilinear support is 2 f pixels wide).  The fixed-point error of an element is therefore at most (q / 2) n_tiles
 * (4 q / 2 at factor 16), on top of the fp32 rounding of the per-pixel terms.  A cell collects bilinear weights of at most
 * f_y f_x pixels: 64^2 x 2^17 = 2^29 < 2^31, which is why factors above 64 are refused.
 * The register form, and the many-class form when d_sem is not 16-byte aligned, add with fp32 atomics instead (LDS, then
 * global): no quantum, but the last bits depend on the execution order.  The loss values are summed in a fixed order always.
 *
 * Supported up-sampling factors: H / h and W / w in [4, 64], and the low-resolution cells under one tile must fit 150 KB of LDS
 * in some form (at a 512-pixel crop: 21 classes down to about factor 7.5, 151 student + 101 teacher classes down to about 10;
 * the count of cells depends on how the tiles fall on the source grid, so ask ucd_seg_losses_plan).
 * Returns UCD_EINVAL (NULL sem_s / labels / loss_out / d_sem / workspace; a size < 1; K < 1 or K > Ctot; a leading dimension
 * below its class count; H < h or W < w), UCD_EUNSUPPORTED (a factor below 4 or above 64; no form fits the LDS - the message
 * names the factors and the bytes asked for; ucd_seg_losses_gather below serves those geometries), UCD_EWORKSPACE (workspace_bytes
 * below ucd_seg_losses_workspace_bytes), or the hipError_t of a failed launch.  On a negative code nothing was launched and no
 * output was written.
 *
 * ucd_seg_losses_plan touches no device (it answers on a machine without a GPU): for a geometry, a class split, has_teacher
 * (sem_t != NULL), d_sem_aligned (16-byte) and pk (1 / 0: the packed forms allowed / not; -1: as UCD_SEG_PK says) it returns
 * the code ucd_seg_losses would return for these arguments and, on 0, the form, the low-resolution cells ny x nx staged per
 * tile and the bytes of dynamic LDS of the launch.  Output pointers may be NULL. */
enum ucd_seg_form {
  UCD_SEG_PK_16_8 = 1,   /* seg_losses_pk_kernel<16, 8>,  fixed-point words */
  UCD_SEG_PK_20_4 = 2,   /* seg_losses_pk_kernel<20, 4>,  fixed-point words */
  UCD_SEG_PK_12_12 = 3,  /* seg_losses_pk_kernel<12, 12>, fixed-point words */
  UCD_SEG_REG_24_16 = 4, /* seg_losses_kernel<24, 16> (K <= 16), fp32 atomics */
  UCD_SEG_REG_24_24 = 5, /* seg_losses_kernel<24, 24> (K > 16),  fp32 atomics */
  UCD_SEG_WIDE_FIXED = 6, /* seg_losses_wide_kernel, fixed-point words */
  UCD_SEG_WIDE_F32 = 7   /* seg_losses_wide_kernel, fp32 atomics (d_sem not 16-byte aligned) */
};
int ucd_seg_losses_plan(int H, int W, int h, int w, int Ctot, int K, int has_teacher, int d_sem_aligned, int pk, int* form,
                        int* ny, int* nx, size_t* lds_bytes);
size_t ucd_seg_losses_workspace_bytes(int B, int H, int W);
int ucd_seg_losses(const float* sem_s, int ld_s, const float* sem_t, int ld_t, const int64_t* labels,
                   int B, int H, int W, int h, int w, int Ctot, int K, int ignore_index,
                   float ce_weight, float kd_weight, float* loss_out, float* d_sem, int ld_d,
                   void* workspace, size_t workspace_bytes, ucd_stream_t stream);

/* The same kernels for the other loss pairs of the reference's --method table (LWF, ILT, MiB / UCD at --alpha != 1, mixed pairs).
 * ucd_seg_losses is this call with ce_old_cl = K, kd_mode = UCD_KD_UNBIASED, alpha = 1 (same launch, same bits).
 *   ce_old_cl  the cross entropy pools the classes [0, ce_old_cl) into the background and maps labels below it to 0
 *              (utils/loss.py:96-109); 1 is plain nn.CrossEntropyLoss.  With a teacher it must be 1 or K; without one it is the only
 *              class split of the call and K is not used beyond its range check.
 *   kd_mode    UCD_KD_UNBIASED, or UCD_KD_PLAIN: KnowledgeDistillationLoss (utils/loss.py:118-136),
 *                KD = mean over pixels of -sum_{c<K} softmax(alpha t)_c log_softmax(z[:K])_c / K
 *              - the student's soft-max is over the first K classes only; dKD/dz_c = (softmax_K(z)_c - q_c) / (K B H W) for
 *              c < K and zero for the new classes.
 *   alpha      multiplies the teacher logits (utils/loss.py:122, :158) - applied to the staged low-resolution rows, bilinear
 *              up-sampling being linear.  Finite and non-zero.
 * Every form serves every legal combination; form, cells and LDS bytes do not depend on kd_mode or alpha (ucd_seg_losses_plan_ex
 * answers as ucd_seg_losses_plan does for the split the kernels use: K with a teacher, ce_old_cl without).
 * Additional UCD_EINVAL: kd_mode not one of the two, alpha zero / NaN / infinite, ce_old_cl outside [1, Ctot], ce_old_cl not in
 * {1, K} with a teacher - checked on the host before any device call; the message names the argument. */
enum ucd_seg_kd_mode { UCD_KD_UNBIASED = 0, UCD_KD_PLAIN = 1 };
int ucd_seg_losses_plan_ex(int H, int W, int h, int w, int Ctot, int K, int ce_old_cl, int kd_mode, int has_teacher,
                           int d_sem_aligned, int pk, int* form, int* ny, int* nx, size_t* lds_bytes);
int ucd_seg_losses_ex(const float* sem_s, int ld_s, const float* sem_t, int ld_t, const int64_t* labels,
                      int B, int H, int W, int h, int w, int Ctot, int K, int ce_old_cl, int kd_mode, float alpha,
                      int ignore_index, float ce_weight, float kd_weight, float* loss_out, float* d_sem, int ld_d,
                      void* workspace, size_t workspace_bytes, ucd_stream_t stream);

/* The GATHER form of the same losses (csrc/seg_gather.hip): for the geometries no tiled form above
 * serves - ADE at --output_stride 8 (151 + 101 classes on 64 x 64 cells under a 512-pixel crop: 207 456 bytes of LDS), any
 * up-sampling factor below 4 - and for a caller that wants a gradient with the same bits on every run where the tiled form adds with
 * fp32 atomics.  Arguments, loss_out[0], loss_out[1] and d_sem[:, :Ctot] mean exactly what they mean for ucd_seg_losses_ex: unbiased
 * or plain cross entropy through ce_old_cl, unbiased or plain distillation through kd_mode, any finite non-zero alpha (applied to
 * the staged teacher rows), sem_t == NULL for the cross entropy alone.
 * One wave owns one low-resolution cell: it stages the 3 x 3 cells around it (9 (Ctot + K) floats of LDS, K counted with a teacher
 * only), walks the pixels whose bilinear footprint contains the cell (lanes over classes, the pixels one after another; the
 * normalisers are wave reductions) and keeps weight * dL/dz per class in registers.  A pixel's normalisers are formed by each of its
 * (up to) four cells; a pixel's LOSS is counted by the cell of its (y0, x0) corner alone, and a second launch adds the per-cell pairs
 * in index order.  No atomics, no fixed point, reductions in a fixed order: the same inputs give the same bits on every run.
 *   d_sem      may be NULL: only the losses are formed, and loss_out has the same bits.  Otherwise every row is written, columns
 *              < Ctot, each element ONCE: the call does not accumulate, needs no memset and does not touch columns Ctot .. ld_d - 1
 *              (ucd_seg_losses clears them; as ucd_seg_bce).
 *   labels     ignore_index: the pixel adds nothing to the cross entropy (it still distils).  A label that is no class is read as
 *              the tiled kernels read it: a negative one is the background (class 0, pooled with [0, ce_old_cl) like a real 0); one
 *              in [Ctot, ...) matches no class - the pixel's cross entropy is LSE(z) (the label's logit counts as 0) and its gradient
 *              softmax(z), no class being subtracted.  (The tiled forms pad their class rows to a multiple of 4 and their packed
 *              slot groups with -1e30 and give that rule from the end of the padding on; the reference raises for such a label.)
 *   factors    any H / h >= 1, W / w >= 1.
 *   classes    any Ctot (and K) whose neighbourhood 9 (Ctot + K) floats fits 64 KB of LDS (1820 classes); beyond that
 *              UCD_EUNSUPPORTED, the message states the bytes asked for.
 * workspace: ucd_seg_losses_gather_workspace_bytes(B, h, w) bytes (one pair of floats per cell; 0 for a size below 1).
 * Checked on the host before any device call, the message names the argument: UCD_EINVAL as ucd_seg_losses_ex (NULL sem_s / labels /
 * loss_out / workspace; a size < 1; K < 1 or K > Ctot; ld_s < Ctot; ld_t < K with a teacher; ld_d < Ctot with d_sem; H < h or W < w;
 * kd_mode, alpha, ce_old_cl as there), UCD_EWORKSPACE (a short workspace), UCD_EUNSUPPORTED; else the hipError_t of a failed launch.
 * On a negative code nothing was launched and no output was written.  No allocation, no host synchronisation: the call captures
 * into graphs. */
size_t ucd_seg_losses_gather_workspace_bytes(int B, int h, int w);
int ucd_seg_losses_gather(const float* sem_s, int ld_s, const float* sem_t, int ld_t, const int64_t* labels,
                          int B, int H, int W, int h, int w, int Ctot, int K, int ce_old_cl, int kd_mode, float alpha,
                          int ignore_index, float ce_weight, float kd_weight, float* loss_out /*[2]*/,
                          float* d_sem /* NULL: losses only */, int ld_d,
                          void* workspace, size_t workspace_bytes, ucd_stream_t stream);

/* The same two calls with a PER-IMAGE weight on the cross entropy (the adaptive factor of the pseudo-labelling below):
 *   loss_out[0] = 1 / (B H W) sum_b f_b sum_{p in image b} CE_p,   f_b = ce_sample_weight[b]
 * and d_sem the gradient of ce_weight loss_out[0] + kd_weight loss_out[1]; the distillation term is untouched.
 *   ce_sample_weight  [B] fp32 ON THE DEVICE, each in [0, 1] (the fixed-point gradient words of the packed and many-class forms
 *                     are scaled for a pixel gradient of at most ce_weight / (B H W): a weight above 1 could wrap them; the host
 *                     cannot check device values).  NULL: the unweighted call, launch for launch.
 * A tile of the tiled forms and a cell of the gather form lie in one image: the weight multiplies ce_scale where a pixel's
 * gradient coefficient is formed and the tile's or cell's cross entropy partial.  The weighted kernels are template
 * instantiations of their own (the packed 16 + 8 and the many-class form sit at 256 VGPRs): ucd_seg_losses_ex and
 * ucd_seg_losses_gather keep their code and their bits, and a weight of ones gives those bits too.  Plan, workspace, errors and
 * every other argument: as the call without _w. */
int ucd_seg_losses_ex_w(const float* sem_s, int ld_s, const float* sem_t, int ld_t, const int64_t* labels,
                        int B, int H, int W, int h, int w, int Ctot, int K, int ce_old_cl, int kd_mode, float alpha,
                        int ignore_index, float ce_weight, float kd_weight, const float* ce_sample_weight /*[B], NULL = 1*/,
                        float* loss_out, float* d_sem, int ld_d, void* workspace, size_t workspace_bytes, ucd_stream_t stream);
int ucd_seg_losses_gather_w(const float* sem_s, int ld_s, const float* sem_t, int ld_t, const int64_t* labels,
                            int B, int H, int W, int h, int w, int Ctot, int K, int ce_old_cl, int kd_mode, float alpha,
                            int ignore_index, float ce_weight, float kd_weight, const float* ce_sample_weight /*[B], NULL = 1*/,
                            float* loss_out /*[2]*/, float* d_sem /* NULL: losses only */, int ld_d,
                            void* workspace, size_t workspace_bytes, ucd_stream_t stream);

/* The same two calls with FOCAL modulation of the cross entropy (the reference's FocalLoss, utils/loss.py:6-28; DESIGN.md
 * section 3.5.10).  Write ce_p >= 0 for pixel p's cross entropy as the calls above define it (plain, or unbiased through ce_old_cl;
 * 0 for an ignored pixel) and w_b for ce_sample_weight[b] (NULL: 1):
 *   p   = exp(-ce_p),   u = clamp(1 - p, 0, 1)
 *   F_p = focal_alpha u^focal_gamma ce_p
 *   loss_out[0] = 1 / (B H W) sum_b w_b sum_p F_p          (ignored pixels count as 0: the reference's focal_loss.mean())
 *   dF_p/dz = focal_alpha g(ce_p) dce_p/dz,   g = u^gamma + gamma u^(gamma-1) p ce_p
 * so a pixel's coefficient on the cross-entropy gradient is multiplied by focal_alpha g(ce_p); nothing else in the gradient
 * arithmetic changes and the distillation term is untouched.
 * Zero rule.  Where u rounds to 0 (ce_p below about 6e-8, an ignored pixel, or the negative "cross entropy" LSE(z) of a label
 * >= Ctot, which the clamp catches) F_p = 0 and g = 0 for gamma > 0; for gamma == 0, F_p = focal_alpha ce_p and g = 1.
 * 0^(gamma-1) ce is never formed: the power is taken of max(u, 2^-24), the smallest u that is not 0, and the zero case is selected.
 * focal_gamma == 2 runs without exp2 / log; any other value goes through exp2(gamma log2 u).
 * Bound for the fixed-point forms.  ln(1/p) <= 1/p - 1 gives p ce <= 1 - p = u, so gamma u^(gamma-1) p ce <= gamma u^gamma <= gamma
 * and g <= 1 + gamma for every gamma >= 0 (u <= 1).  A focal call therefore scales its gradient words with
 *   gmax = (focal_alpha (1 + focal_gamma) |ce_weight| + 2 |kd_weight| / K) / (B H W);
 * the quantum q = gmax / 2^17, the 2^29 < 2^31 argument and the error statement of ucd_seg_losses follow from it unchanged.
 * Additional UCD_EINVAL, checked on the host before anything else, the message names the argument: focal_gamma negative, NaN or
 * infinite; focal_alpha zero, negative, NaN or infinite.  focal_gamma == 0 with focal_alpha == 1 is the call without focal
 * (_ex / _ex_w, _gather / _gather_w): same kernel, same bits.  ce_sample_weight may be NULL, and a weight of ones gives the bits of
 * NULL.  The focal kernels are template instantiations of their own (all tiled forms and the gather form), as the weighted ones
 * are: the calls above keep their code, registers and bits.  Plan, workspace, errors and every other argument: as the call
 * without focal. */
int ucd_seg_losses_focal(const float* sem_s, int ld_s, const float* sem_t, int ld_t, const int64_t* labels,
                         int B, int H, int W, int h, int w, int Ctot, int K, int ce_old_cl, int kd_mode, float alpha,
                         int ignore_index, float ce_weight, float kd_weight, const float* ce_sample_weight /*[B], NULL = 1*/,
                         float focal_gamma, float focal_alpha, float* loss_out, float* d_sem, int ld_d, void* workspace,
                         size_t workspace_bytes, ucd_stream_t stream);
int ucd_seg_losses_gather_focal(const float* sem_s, int ld_s, const float* sem_t, int ld_t, const int64_t* labels,
                                int B, int H, int W, int h, int w, int Ctot, int K, int ce_old_cl, int kd_mode, float alpha,
                                int ignore_index, float ce_weight, float kd_weight, const float* ce_sample_weight /*[B], NULL = 1*/,
                                float focal_gamma, float focal_alpha, float* loss_out /*[2]*/, float* d_sem /* NULL: losses only */,
                                int ld_d, void* workspace, size_t workspace_bytes, ucd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * PLOP's pseudo-labelling (csrc/pseudo_label.hip).  sem_t [B*h*w, ld_t >= K] fp32: the frozen teacher's
 * low-resolution logits as rows (as ucd_seg_losses takes them), labels int64 [B, H, W].  With z = up(sem_t)[b, :, y, x] (up:
 * bilinear, align_corners=False, as F.interpolate and the loss kernels compute it), per pixel
 *   c* = argmax_c z_c                       the first maximum (torch's rule, as ucd_seg_confusion)
 *   u  = H(softmax z) / log K in [0, 1]     H = log S - T / S, m = max z, S = sum exp(z_c - m), T = sum (z_c - m) exp(z_c - m);
 *                                           no epsilon; 0 for K = 1; K equal logits give exactly 1
 *   candidate: 0 <= label < K and label != ignore_index.  Only candidates do class work.
 * ucd_pseudo_hist   hist[c*, min(floor(u bins), bins - 1)] += 1 over the candidates.  hist [K, bins] int64 is ACCUMULATED into
 *                   (zero it before the first batch); integer adds: exact, independent of order.  Summed per workgroup in LDS
 *                   where K x bins words fit beside the cells (ucd_pseudo_plan says), else per wave; never one global add per pixel.
 * ucd_pseudo_label  labels_out = c* where a candidate has u < thresholds[c*], ignore_index for any other candidate, the label
 *                   itself elsewhere.  labels_out [B, H, W] int64 may not alias labels.  counts [B, 2] int32 = (candidates that
 *                   passed, candidates): the call clears them itself, integer adds.  factor [B] fp32 = max(num / (den + 1e-6),
 *                   f_min), max(0, f_min) for an image without candidates - a last small launch on the same stream (fp64, rounded
 *                   once).  uncertainty (may be NULL; tests, diagnosis) [B, H, W] fp32 = u for candidates, 0 elsewhere.
 *                   thresholds [K] fp32 on the device; 0 <= f_min <= 1.
 * ucd_pseudo_plan   host only, no device call: the pixel tile, the grid over one image, the threads of a workgroup, the bytes of
 *                   dynamic LDS and whether the histogram is summed in LDS.  bins = 0 plans the label pass.
 * One pixel walk for both: a workgroup owns a tile of pixels (64 x 64, the larger side halved until it fits, down to 8 x 8), the
 * teacher cells under it staged in LDS - (tile_y h / H + 3) x (tile_x w / W + 3) rows of K | 1 floats (the odd pitch spreads the
 * banks) - and one lane per pixel, consecutive lanes along x (8-byte label loads and stores in contiguous runs).
 * Limits: any factors H / h, W / w >= 1; K as the LDS allows - the smallest tile stages at most 11 x 11 cells, so 160 KB
 * (163840 bytes) serve K <= 337 at every factor (ADE at --output_stride 8: K = 141 on 64 x 64 tiles, 68 KB); 2 <= bins <= 1024;
 * B <= 65535 and H / tile_y <= 65535.
 * Checked on the host before any device call, the message names the argument: UCD_EINVAL (a NULL pointer other than uncertainty;
 * B, H, W, h, w or K below 1; H < h or W < w; ld_t < K; bins outside [2, 1024]; f_min outside [0, 1]; labels_out == labels),
 * UCD_EUNSUPPORTED (no tile fits the LDS - the message states the bytes asked for; a grid limit); else the hipError_t of a failed
 * launch.  On a negative code nothing was launched.  No allocation, no host synchronisation: the calls capture into graphs. */
int ucd_pseudo_plan(int H, int W, int h, int w, int K, int bins, int* tile_y, int* tile_x, int* grid_y, int* grid_x, int* threads,
                    size_t* lds_bytes, int* lds_hist);
int ucd_pseudo_hist(const float* sem_t, int ld_t, const int64_t* labels, int B, int H, int W, int h, int w, int K,
                    int ignore_index, int bins, int64_t* hist /*[K, bins], accumulated*/, ucd_stream_t stream);
int ucd_pseudo_label(const float* sem_t, int ld_t, const int64_t* labels, int B, int H, int W, int h, int w, int K,
                     int ignore_index, const float* thresholds /*[K]*/, float f_min, int64_t* labels_out,
                     int* counts /*[B, 2]: num, den*/, float* factor /*[B]*/, float* uncertainty /*[B, H, W] or NULL*/,
                     ucd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fused full-resolution BINARY cross entropy losses: --bce, --icarl, --method LWF-MC (csrc/seg_gather.hip).
 * Rows as for ucd_seg_losses: sem_s [B*h*w, ld_s >= Ctot] / sem_t [B*h*w, ld_t >= K] float32 (sem_t may be NULL), labels int64
 * [B, H, W].  With z = up(sem_s) [B, Ctot, H, W], zt = up(sem_t) [B, K, H, W] (up: bilinear, align_corners=False, as
 * F.interpolate computes it), y the labels, s() the logistic function and
 *   bce(z, t) = max(z, 0) - t z + log1p(exp(-|z|))                      (finite at any z; logits of +-90 are served)
 *   loss_out[0] = 1 / (B H W) sum_p [y_p valid] sum_c bce(z_pc, [c == y_p])
 *                 - BCEWithLogitsLossWithIgnoreIndex(reduction='none')(z, y).mean() (utils/loss.py:31-54, train.py:112/116);
 *                 an all-ignored batch gives exactly 0
 *   loss_out[1] = 1 / (B H W) sum_p sum_{c<K} bce(z_pc, s(zt_pc))
 *                 - K * nn.BCEWithLogitsLoss()(z[:, :K], sigmoid(zt)) (train.py:119-124; no ignore mask; the sigmoid is applied
 *                 AFTER the up-sampling); 0 with sem_t == NULL
 *   d_sem[b, i, j, c] = d(hard_weight loss_out[0] + soft_weight loss_out[1]) / d sem_s[b, i, j, c]
 *                 = 1 / (B H W) sum_p w_p(i, j) (hard_weight [y_p valid] (s(z_pc) - [c == y_p]) + soft_weight [c < K] (s(z_pc) - s(zt_pc)))
 *                 with w_p(i, j) the bilinear weight of cell (i, j) in pixel p.
 * d_sem may be NULL (losses only: the same loss_out bits).  Otherwise the call writes every row, columns < Ctot, each element
 * ONCE - it does not accumulate, needs no memset and does not touch columns Ctot .. ld_d - 1.
 * A label is valid when it is in [0, Ctot) and not ignore_index: any other value counts as ignored (the reference's F.one_hot
 * raises for a label in [Ctot, ...) other than 255).
 * Gather form: one wave per low-resolution cell re-evaluates the pixels under the cell's bilinear footprint and sums in
 * registers; a pixel's loss is counted by the cell of its (y0, x0) corner; a second launch adds the per-cell pairs in index
 * order.  No atomics, no fixed point: the same inputs give the same bits.  Any up-sampling factor >= 1 is served.
 * workspace: ucd_seg_bce_workspace_bytes(B, h, w) bytes (one pair of floats per cell).
 * Checked on the host before any device call: UCD_EINVAL (NULL sem_s / labels / loss_out / workspace; a size < 1; K < 1 or K >
 * Ctot; ld_s < Ctot; ld_t < K with a teacher; ld_d < Ctot with d_sem; H < h or W < w), UCD_EWORKSPACE (a short workspace),
 * UCD_EUNSUPPORTED (9 (Ctot + K) floats over 64 KB of LDS); else the hipError_t of a failed launch. */
size_t ucd_seg_bce_workspace_bytes(int B, int h, int w);
int ucd_seg_bce(const float* sem_s, int ld_s, const float* sem_t, int ld_t, const int64_t* labels,
                int B, int H, int W, int h, int w, int Ctot, int K, int ignore_index,
                float hard_weight, float soft_weight, float* loss_out /*[2]*/,
                float* d_sem /* NULL: losses only */, int ld_d,
                void* workspace, size_t workspace_bytes, ucd_stream_t stream);

/* Validation on the device: bilinear up-sampling of the low-resolution logits
 * (segmentation_module.py:133), arg-max over the classes (train.py:242 `outputs.max(dim=1)`) and the confusion matrix of
 * metrics/stream_metrics.py:65-71 (`bincount(n * label + pred)` over the pixels with 0 <= label < n_classes) in one pass;
 * the full-resolution logits never exist and nothing is copied to the host.  hist [n_classes, n_classes] int64 is
 * ACCUMULATED into (zero it before the first batch; integer atomics: exact, order-independent); pred (optional,
 * [B, H, W] int64) receives the arg-max map (first maximum, torch.max's rule). */
int ucd_seg_confusion(const float* sem, int ld_s, const int64_t* labels, int B, int H, int W, int h, int w, int Ctot,
                      int n_classes, int64_t* hist, int64_t* pred, ucd_stream_t stream);

/* Evaluation with test-time views: the image was run at V scales, some of them mirrored, and the per-view class distributions are
 * fused into one prediction per full-resolution pixel, counted into the confusion matrix of the call above - one pass, no
 * full-resolution logits or soft-max maps.
 *   sem[v]   fp32 rows [B*h[v]*w[v], ld[v] >= Ctot]: view v's low-resolution logits, laid out as the call above takes them
 *   flip[v]  != 0: the view was computed from the horizontally mirrored image; its value at output pixel (Y, X) is the view's
 *            bilinear sample at (Y, W - 1 - X)
 *   1 <= V <= 16, Ctot <= 255, H >= h[v] and W >= w[v] for every view (any up-sampling factor >= 1)
 * sem, ld, h, w and flip are HOST arrays: the view table travels to the kernel by value in its arguments, nothing is uploaded and
 * the call is asynchronous on `stream`.  The device memory behind sem[v] is read when the kernel runs.
 * Per pixel, l_v(c) is view v's logit up-sampled bilinearly (align_corners = False, the arithmetic of the call above, expression
 * by expression) and p_v = softmax_c(l_v), shifted by the view's own maximum, in fp32.  The score of class c is
 *   mode 0 (mean)    sum_v p_v(c)
 *   mode 1 (max)     max_v p_v(c)
 *   mode 2 (voting)  the number of views whose arg-max of l_v is c (first maximum per view)
 * and the prediction is the smallest c with the largest score.  Pairs (label, prediction) with 0 <= label < n_classes and
 * prediction < n_classes are ADDED to hist [n_classes, n_classes] int64 (zero it before the first batch) as integers - an LDS
 * histogram for n_classes <= 64, global atomics above; pred (optional, [B, H, W] int64) receives the prediction.  The same inputs
 * give the same bits of hist and pred on every run; voting over the single plain view is ucd_seg_confusion bit for bit.
 * A workgroup owns a pixel tile and stages the cells of all views under it in LDS.  The plan call (host only, no device call; the
 * one copy of the sizing arithmetic, which the launch itself asks) picks the largest tile of 32 x 64, 32 x 32, 16 x 32, 16 x 16,
 * 8 x 16, 8 x 8 pixels for which sum_v cells_v * Ctot * 4 bytes (cells_v: the largest footprint of view v over the tiles of the
 * grid, by the kernel's own index arithmetic; a mirrored view's columns over the mirrored pixel range), a 272-byte table and - for
 * n_classes <= 64 - the n_classes^2 * 4 bytes of the histogram fit 150 KB.
 * Checked on the host before any device call: UCD_EINVAL (V outside 1 .. 16; a NULL array; a size below 1; Ctot > 255; h[v] > H
 * or w[v] > W; and for the launch a NULL sem[v], labels or hist, ld[v] < Ctot, an unknown mode), UCD_EUNSUPPORTED (no tile fits:
 * the message names the bytes of the smallest one); else the hipError_t of a failed launch. */
int ucd_seg_views_plan(int H, int W, int V, const int* h, const int* w, const int* flip, int Ctot, int n_classes, int* tile_y,
                       int* tile_x, size_t* lds_bytes);
int ucd_seg_views(const float* const* sem, const int* ld, const int* h, const int* w, const int* flip, int V, const int64_t* labels,
                  int B, int H, int W, int Ctot, int n_classes, int mode, int64_t* hist, int64_t* pred, ucd_stream_t stream);

/* The output side of an evaluation run (the reference's test.py / Trainer.test, train.py:271-375) in one pass over the
 * full-resolution pixel grid of a batch; only uint8 maps (and the fp32 attention map) leave the device.  Inputs:
 *   sem      fp32 rows [B*h*w, ld_s >= Ctot], the low-resolution logits (as ucd_seg_confusion takes them); Ctot <= 255
 *   labels   int64 [B, H, W], may be NULL
 *   image    fp32, element (b, c, y, x) at image[b sb + c sc + y sh + x sw], c < 3: the normalised input in NCHW or channels-last
 *            (strides in elements, as ucd_stem_conv7x7 takes them); may be NULL
 *   mean_*, std_*   the normalisation that the data pipeline applied, by value
 *   cmap     uint8 [256][3] in device memory, the palette
 *   att_low  fp32 [B, ha, wa], may be NULL: a low-resolution map (ucd_attn_energy) on a grid independent of h x w
 * Outputs, each optional (NULL: not produced, and nothing of it is touched):
 *   pred_u8   [B, H, W]     arg-max over the classes of the bilinearly up-sampled logits (align_corners = False), first maximum
 *                           wins: the same arithmetic, and the same bits, as the pred of ucd_seg_confusion
 *   pred_rgb  [B, H, W, 3]  cmap[pred]
 *   label_rgb [B, H, W, 3]  cmap[label & 255]
 *   image_u8  [B, H, W, 3]  trunc(clamp((x * std + mean) * 255, 0, 255)) in fp32 (the reference's astype(uint8) wraps values
 *                           outside the range; the clamp is the one difference)
 *   att       [B, H, W] fp32  att_low up-sampled bilinearly with the same source-index arithmetic
 * Every byte of a requested output is written exactly once.  One launch, no allocation, no host synchronisation: the call can be
 * captured into a graph.  Tiling: ucd_seg_confusion's (64 x 64 pixel tiles, the cells under a tile in LDS); a wave exchanges the
 * packed pixels of a tile row by shuffles and stores aligned dwords of the RGB rows, bytes only at the ends of a row segment.
 * Checked on the host before any device call, the message names the argument: UCD_EINVAL (NULL sem or cmap; B, H, W, h, w or
 * Ctot below 1; ld_s < Ctot; Ctot > 255; every output NULL; label_rgb without labels; image_u8 without image; att without
 * att_low, or with ha / wa below 1), UCD_EUNSUPPORTED (an up-sampling factor H / h or W / w below 4; more than 150 KB of LDS for
 * the cells under a tile - the limits of ucd_seg_confusion); else the hipError_t of a failed launch.  On a negative code nothing
 * was launched. */
int ucd_seg_render(const float* sem, int ld_s, const int64_t* labels, const float* image, long long sb, long long sc, long long sh,
                   long long sw, float mean_r, float mean_g, float mean_b, float std_r, float std_g, float std_b, const uint8_t* cmap,
                   const float* att_low, int ha, int wa, int B, int H, int W, int h, int w, int Ctot, uint8_t* pred_u8,
                   uint8_t* pred_rgb, uint8_t* label_rgb, uint8_t* image_u8, float* att, ucd_stream_t stream);

/* The attention map of the reference's Trainer.test (train.py:339-342) from a RAW map: a[b, p] = sum_c x[b, p, c]^2, divided by
 * the Frobenius norm of its image's map (the factor ucd_attmap multiplies with, kept instead of applied).
 *   x  channels-last rows [B*HW, ld >= C], dtype UCD_F32 or UCD_BF16;  a  fp32 [B*HW], written in full
 * 16-byte loads when the base pointer and the row pitch are 16-byte aligned, element loads otherwise: no alignment is required.
 * Two launches (per-cell sums of squares; one workgroup per image for the norm and the division), no workspace, no float
 * atomics, every sum in a fixed order: same inputs, same bits.  An all-zero image divides by zero like the reference (NaN).
 * Checked on the host before any device call: UCD_EINVAL (NULL x or a, unknown dtype, B / HW / C below 1, ld < C, more than
 * 2^29 rows); else the hipError_t of a failed launch. */
int ucd_attn_energy(const void* x, int ld, int dtype, int B, int HW, int C, float* a, ucd_stream_t stream);

/* ---- label path of the training data pipeline on the device (first piece) ------------------------
 * Replaces, for the label maps of a batch, the reference's host-side RandomResizedCrop (crop + PIL NEAREST resize,
 * dataset/transform.py:481-553), RandomHorizontalFlip (:300-318) and the per-pixel Python lambda that remaps labels for
 * the incremental step (dataset/voc.py:176-203).  Bit-exact (index arithmetic of Pillow's NEAREST resize).
 *   src     B device pointers (array in device memory) to uint8 label maps, image b is [H0_b][W0_b] row-major
 *   desc    int32 [B][8] in device memory: {H0, W0, i, j, h, w, flip, 0}  (crop box top-left (i, j), size (h, w))
 *   lut     uint8 [256]: value after remapping for every stored label (inverted_order / masking_value)
 *   tables  int32 workspace [B][2][S];  out  int64 [B][S][S] (the labels tensor the train step takes) */
int ucd_label_path(const uint8_t* const* src, const int* desc, int B, int S, const uint8_t* lut, int* tables,
                   int64_t* out, ucd_stream_t stream);

/* Image half of the same pipeline: crop + Pillow BILINEAR resize (8-bit, separable, anti-aliased when down-scaling; the
 * fixed-point arithmetic of Pillow's Resample.c, bit-exact) + horizontal flip + ToTensor + Normalize
 * (dataset/transform.py:481-553, 300-318, 37-86; run.py:49-55).
 *   src   B device pointers to decoded uint8 RGB images [H0_b][W0_b][3];   desc as in ucd_label_path
 *   kmax  >= ceil(max(1, max crop extent / S)) * 2 + 1;   hmax >= max crop height of the batch
 *   mean_* / std_*  the Normalize constants;   coeff_ws int32 [B][2][S][kmax + 2];   tmp uint8 [B][hmax][S][3]
 *   out   float32 [B][S][S][3] = the channels-last storage of the [B, 3, S, S] batch */
int ucd_image_path(const uint8_t* const* src, const int* desc, int B, int S, int kmax, int hmax, float mean_r, float mean_g,
                   float mean_b, float std_r, float std_g, float std_b, int* coeff_ws, uint8_t* tmp, float* out,
                   ucd_stream_t stream);

/* Both halves for samples that are resident in HBM (ucd_amd/datacache.py), in ONE kernel launch with no workspace: the
 * coefficient entries and index tables are computed by the workgroup that needs them and the horizontal pass's 8-bit rows are
 * streamed through LDS in chunks, so any down-scaling factor works.
 *   images  B device pointers (array in device memory) to decoded uint8 RGB images [H0_b][W0_b][3], any alignment
 *   labels  B device pointers to the uint8 label maps [H0_b][W0_b] of the same samples
 *   desc    int32 [B][8] in device memory: {H0, W0, i, j, h, w, flip, 0}, as ucd_image_path / ucd_label_path take it.  The
 *           caller checks 0 <= i, 0 <= j, 0 < h, 0 < w, i + h <= H0 and j + w <= W0 (the descriptors are device memory: this
 *           library cannot); a sample whose descriptor fails that is skipped - nothing of it is read, its outputs stay unwritten
 *   lut     uint8 [256];   mean_* / std_*  the Normalize constants
 *   out_images  float32 [B][S][S][3], bit-identical to ucd_image_path's `out` for the same pointers and descriptors
 *   out_labels  int64 [B][S][S], bit-identical to ucd_label_path's `out`
 * UCD_EINVAL (a NULL pointer, B or S below 1, B or S / 16 above 65535) before the launch; else the hipError_t of a failed
 * launch. */
int ucd_batch_path(const uint8_t* const* images, const uint8_t* const* labels, const int* desc, int B, int S, const uint8_t* lut,
                   float mean_r, float mean_g, float mean_b, float std_r, float std_g, float std_b, float* out_images,
                   int64_t* out_labels, ucd_stream_t stream);

/* ---- the validation transforms on the device: Resize + CenterCrop, and full size (run.py:58-73) ------------------
 * The second geometry of the same pipeline: resize the WHOLE image [H0][W0] to (oh, ow), then cut the window
 * [i, i + out_h) x [j, j + out_w) out of the result - Pillow's resize((ow, oh)) followed by crop().  The tables belong to
 * the full axis H0 -> oh / W0 -> ow and are evaluated at the window's indices only; the horizontal pass runs over the
 * source rows the vertical window reads.  Full-size validation is oh = H0, ow = W0, i = j = 0, out_h = H0, out_w = W0: the
 * identity coefficients {1 << 22, 0} give the source byte back.  The output is rectangular and common to the batch.
 *   src   B device pointers to decoded uint8 RGB images [H0_b][W0_b][3]
 *   desc  int32 [B][8] in device memory: {H0, W0, oh, ow, i, j, 0, 0}.  The caller checks 0 <= i <= oh - out_h and
 *         0 <= j <= ow - out_w (the descriptors are device memory: this library cannot); an image whose descriptor fails
 *         that is skipped by every kernel - nothing of it is read and its part of the output is not written
 *   kmax  >= ceil(max(1, H0 / oh, W0 / ow over the batch)) * 2 + 1
 *   hmax  >= min(H0, floor((out_h - 1) * H0 / oh + 2 * max(1, H0 / oh)) + 2) over the batch: rows of the intermediate
 *   scale_mode  ToTensor as 0: v / 255.f (the expression of ucd_image_path), 1: v * (1.f / 255.f) (what torch computes for a
 *         tensor divided by the scalar 255 on the device); the two differ in the last bit for about half the byte values
 *   coeff_ws int32 [B][out_h + out_w][kmax + 2];   tmp uint8 [B][hmax][out_w][3]
 *   out   float32 [B][out_h][out_w][3] = the channels-last storage of the [B, 3, out_h, out_w] batch
 * Checked on the host before any launch: UCD_EINVAL (a NULL pointer, B / out_h / out_w / hmax below 1, kmax below 3, B,
 * out_h or hmax above 65535, an unknown scale_mode); else the hipError_t of a failed launch. */
int ucd_val_image_path(const uint8_t* const* src, const int* desc, int B, int out_h, int out_w, int kmax, int hmax, int scale_mode,
                       float mean_r, float mean_g, float mean_b, float std_r, float std_g, float std_b, int* coeff_ws, uint8_t* tmp,
                       float* out, ucd_stream_t stream);

/* Label half: Pillow's NEAREST resize((ow, oh)) + crop() + the step's table.  Pillow picks source indices by a running
 * double sum from output index 0 of the full axis (xo = a / 2; idx = (int)xo; xo += a with a = in / out_full), so the tables
 * are accumulated from 0 through off + out - 1 and kept from off on - not restarted at the window.
 *   src, desc  as above, label maps [H0_b][W0_b] uint8;   lut  uint8 [256]
 *   tables  int32 workspace [B][out_h + out_w];   out  int64 [B][out_h][out_w]
 * UCD_EINVAL (a NULL pointer, B / out_h / out_w below 1, B or out_h above 65535) before any launch. */
int ucd_val_label_path(const uint8_t* const* src, const int* desc, int B, int out_h, int out_w, const uint8_t* lut, int* tables,
                       int64_t* out, ucd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 1x1 convolutions as row-matrix GEMMs on the bf16 matrix cores with the neighbouring ABN work fused (SURVEY.md
 * section 8-f4).  Replaces the cuDNN 1x1 convolutions of the bottleneck blocks and of the head -
 * modules/residual.py:57-63 (conv1, conv3), :79-80 (proj_conv), modules/deeplab.py:25,35 (map_convs[0], red_conv) - plus,
 * fused into them, the inplace_abn passes around them (modules/residual.py:64-73,81-82,90-97; modules/deeplab.py:57,69).
 *
 *   y[M, N] = out( in(a)[M, K] . w[N, K]^T )      bf16 operands, fp32 accumulation, bf16 result
 *
 *   in(a)    a itself, or (in_scale != NULL) act_in((a - in_mean[k]) * in_scale[k] + in_shift[k]): the ABN apply of the
 *            layer that PRODUCED a, applied while the tile is staged - that layer's output never exists in memory;
 *   out_mode 0  y = acc (+ y when accumulate != 0: the identity shortcut's gradient, beta = 1)
 *            1  y = act_out((acc - out_mean[n]) * out_scale[n] + out_shift[n] + residual[m, n]): this layer's ABN with
 *               frozen statistics (evaluation mode / --fix_bn), the block's residual add and activation
 *            2  y = acc and partial[t][0..2][n] = (k, sum (y - k), sum (y - k)^2) over the rows of row tile t, k = the
 *               tile's first row: input of ucd_conv1x1_stats_finalize (training: the following ABN's statistics pass)
 *            3  acc is the gradient w.r.t. in'(x) of a layer whose input transform was fused in the forward; with
 *               x = residual[m, n] (its pre-norm input), z = (x - out_mean) * out_scale + out_shift:
 *               y = dz = acc * act_out'(z) and partial[t][0..1][n] = (sum dz, sum dz * (x - out_mean) * out_invstd): input
 *               of ucd_abn_reduce_partials (that ABN's backward reduction)
 *            4  (1x1 only) acc (+ y when accumulate != 0: the identity shortcut's gradient) is the gradient w.r.t. the
 *               OUTPUT out = act(norm(z) + shortcut) of the residual block in front (modules/residual.py:84-97): with
 *               residual = out (the sign of the activation) and side2 = z: y = d pre = (acc + y) * act_out'(out) and
 *               partial[t][0..1][n] = (sum d pre, sum d pre * (z - out_mean) * out_invstd) - the backward sums of the
 *               block's last norm; its backward is then ucd_abn_reduce_partials + ucd_abn_bwd_apply (identity activation)
 *               on d pre, and the shortcut's gradient is d pre itself
 * act_in / act_out: UCD_ACT_LEAKY_RELU or UCD_ACT_IDENTITY (elu layers keep the separate ucd_abn_* kernels); modes 1 and 3
 * need out_mean, out_scale and out_shift (pass zeros / ones for a missing term).
 * Shapes: K and N multiples of 64, any M; pointers 16-byte aligned, leading dimensions (elements) multiples of 8.
 * partial: out_mode 2 needs ucd_conv1x1_stats_partial_bytes(M, N) bytes (the row tiles' [3][N] triples); out_mode 3 needs
 * ucd_conv1x1_row_tiles(M) rows of [2][N].  The input gradient of the layer is the same call on (dY, W^T)
 * (ucd_transpose_bf16 builds W^T); the weight gradient is ucd_conv1x1_wgrad. */
typedef struct ucd_conv1x1_desc {
  const void* a;  int lda;
  const void* w;  int ldw;
  void* y;        int ldy;
  int M, N, K;
  const float* in_mean;  const float* in_scale;  const float* in_shift;  int in_act;  float in_slope;
  int out_mode;
  const float* out_mean;  const float* out_scale;  const float* out_shift;  const float* out_invstd;
  const void* residual;  int ldr;
  int out_act;  float out_slope;
  float* partial;
  int accumulate;
  /* taps = 9: a is the [B, H, W, K] map and the product is the 3x3 convolution with stride 1 and padding = dilation
   * (modules/residual.py:69 conv2, modules/deeplab.py:27-29 the ASPP branches) as an implicit GEMM over 9 K columns: w is
   * the channels-last 4-D weight [N][kh][kw][K] (ldw >= 9 K), M = B*H*W; no input transform, every out_mode.  The input
   * gradient of such a layer is the same call on (dY, w.flip(2, 3).transpose(0, 1)) (ucd_flip_weights_batched).
   * taps = 0 or 1: the 1x1 product above. */
  int taps, H, W, dilation;
  /* out_mode 4 only: the conv output z of the residual block whose OUTPUT is `residual` (x-hat of its last norm's sums) */
  const void* side2;  int ld2;
  /* stride > 1 (0 and 1: none): the strided layers of the first block of a stage (modules/residual.py:57-73 conv2 with
   * stride 2, :79 proj_conv 1x1 stride 2).  a is the [B, H, W, K] map, y the [B, OH, OW, N] one with OH = (H - 1) / stride + 1
   * (padding 0 for taps <= 1, padding = dilation for taps = 9), M = B*OH*OW; out_mode 0, 1 or 2, no input transform. */
  int stride;
  /* Atomic statistics (round 5; NULL: the per-tile partial rows above).  stat_acc != NULL: out_mode 2 / 3 / 4 add their
   * per-channel column sums with fp32 atomics into stat_acc[0..N) / stat_acc[N..2N) (zeroed by the caller before the launch; one
   * accumulator per layer and direction, see ucd_abn_apply_stats / ucd_abn_bwd_apply_raw, which finalise it in their prologue - no
   * second-stage reduction launch).  out_mode 2 then sums about the caller's shift stat_shift[n] (any value near the channel mean:
   * the layer's running mean; NOT the tile's first row) and row tile 0 stores a snapshot of that shift to partial[0..N) (the consumer
   * reads the snapshot, so the running mean may be updated meanwhile).  stat_acc2 (optional): a second accumulator receiving the same
   * adds (SyncBN: one is all-reduced, the other stays this rank's parameter gradient).  Sums are order dependent: results differ
   * in the last bits from run to run. */
  float* stat_acc;  const float* stat_shift;  float* stat_acc2;
  /* stat_rep (0 / 1: one): REPLICAS of the accumulator, a power of two - row tile t adds into replica t % stat_rep (stat_acc holds
   * stat_rep x [2 N] floats); adds to one address are serialised at the memory side (~25 ns each), so a launch of hundreds of row
   * tiles spreads them (ucd_conv1x1_stat_replicas(M) is the library's choice: <= 64 adds per address) and the finalising apply pass
   * sums the replicas in its prologue. */
  int stat_rep;
} ucd_conv1x1_desc;

/* Kernel forms behind ucd_conv1x1 (results do not depend on the choice - tests/test_conv1x1_fused_gpu.py::
 * test_every_pipeline_form... holds every form bit-exact on integers).  ucd_conv1x1_plan is the one statement of which form, tile,
 * grid and LDS a call gets, and ucd_conv1x1 launches with exactly its numbers (rules and the network's shapes: DESIGN.md section
 * 3.1.1; restated by tests/test_conv1x1_plan_cpu.py).  It reads only M, N, K, taps, stride, out_mode and whether in_scale and
 * stat_acc are NULL - no operand is dereferenced and no device touched, so it answers on a machine without a GPU - and returns
 * the code ucd_conv1x1 would return for these fields.
 * Three environment variables, read once per process, exist for probes and A/B runs: UCD_CONV_PIPE (2x64, lw64 = loader waves on
 * 128-row tiles, lw256; auto or unset = by the grid) forces one form for every double-buffer-eligible launch - any other value
 * makes the plan, and with it every ucd_conv1x1 call, fail with UCD_EINVAL; UCD_CONV_BN64_TILES (default 128, 0 = never) is the
 * largest grid of 128 x 128 tiles that runs on 128 x 64 tiles instead; UCD_CONV_LW64_TILES (default 128, 0 = never) is the largest
 * grid of 128 x 64 loader-wave tiles that runs on 64-row tiles instead. */
enum ucd_conv_form {
  UCD_CONV_SINGLE = 0,  /* conv1x1_kernel, one LDS stage, four workgroups per CU */
  UCD_CONV_DB = 1,      /* conv1x1_kernel, two LDS stages */
  UCD_CONV_LW128 = 2,   /* conv_lw_kernel, loader waves on 128-row tiles */
  UCD_CONV_LW256 = 3,   /* conv_lw_kernel, loader waves on 256-row tiles */
  UCD_CONV_LW64 = 4     /* conv_lw_kernel, loader waves on 64-row tiles */
};
#define UCD_CONV_FORM_NAMES {"single", "2x64", "lw/128", "lw/256", "lw/64"}   /* indexed by enum ucd_conv_form */
typedef struct ucd_conv1x1_plan_t {
  int form;                  /* enum ucd_conv_form */
  int tile_rows, tile_cols;  /* 64 / 128 / 256 rows, 64 / 128 columns */
  int tiles_m, tiles_n, grid, threads, lds_bytes;
  int param_off;             /* LDS byte offset of the input-transform constants (0 without an input transform) */
} ucd_conv1x1_plan_t;
int ucd_conv1x1_plan(const ucd_conv1x1_desc* desc, ucd_conv1x1_plan_t* plan);
int ucd_conv1x1_row_tiles(int M);
int ucd_conv1x1_stat_replicas(int M);   /* replicas of an atomic statistics accumulator for a product of M rows (1 .. 64) */
size_t ucd_conv1x1_stats_partial_bytes(int M, int C);
int ucd_conv1x1(const ucd_conv1x1_desc* desc, ucd_stream_t stream);

/* Class-ordered rows of the stand-alone dilated 3x3 products (taps = 9, stride 1, dilation > 1, out_mode 0: the ASPP branches,
 * forward and input gradient).  A pixel is classed by which of its four axis neighbours at distance `dilation` lie inside the map;
 * the kernels then take GEMM row r to be pixel perm[r] - class-major over the whole batch, the classes by falling number of live
 * taps, raster order inside a class - and every row tile walks only the taps of its 9-bit mask (bit kh * 3 + kw), the union of the
 * live taps of its rows.  Skipped steps would have added exact zeros and the live steps keep their order: the outputs are bit-identical
 * to those of the raster order.  The library builds the plan of a (device, B, H, W, dilation, tile rows) at the first ucd_conv1x1
 * call that needs it and keeps it in device memory; that takes blocking calls, so it happens only outside a stream capture - a call
 * that arrives under capture without its plan runs in raster order (run one eager step before capturing).
 * ucd_conv3_tap_plan: the host half - fills perm[B * H * W] and masks[ceil(B * H * W / tile_rows)] (tile_rows 64, 128 or 256) and
 *   reports the number of classes that occur (<= 16); no GPU needed.
 * ucd_conv3_tap_classes: mode = 0 / 1 / 2 sets the switch inside the process, mode < 0 only reads it; returns the value in force.
 *   The first use reads the environment variable UCD_CONV3_TAP_CLASSES (default 1; 0: exactly the launches without the plans).
 *   Mode 1 leaves one kind of launch in raster order: at most one 64-row workgroup per CU whose heaviest tile keeps its tap count
 *   in class order (such a launch lasts as long as that tile; measured 4 - 5 % slower with the row table).  Mode 2 takes the
 *   class order there too (tests, probes).
 * ucd_conv3_tap_plans_resident: number of plans in device memory (at most 64; further shapes run in raster order).
 * ucd_conv3_tap_stats: launches that took the class-ordered kernels so far, and for the latest stand-alone dilated 3x3 product
 *   the rows of its workgroup tile and whether it took them (any pointer may be NULL). */
int ucd_conv3_tap_plan(int B, int H, int W, int dilation, int tile_rows, int* perm, int* masks, int* n_classes);
int ucd_conv3_tap_classes(int mode);
int ucd_conv3_tap_plans_resident(void);
int ucd_conv3_tap_stats(long long* launches, int* last_tile_rows, int* last_class_ordered);

/* out_mode 2 partials -> batch statistics of the [M, C] product -> buf = [sums(2C) | kshift(C) | mean | invstd | scale]
 * (the layout ucd_abn_forward leaves for the backward) and the running statistics, like ucd_abn_stats_finalize; with
 * pack != NULL it writes this rank's [mean_r | M2_r] instead (SyncBN: all-gather, then ucd_abn_sync_forward). */
int ucd_conv1x1_stats_finalize(const float* partial, int M, int C, const float* weight, float* running_mean,
                               float* running_var, float momentum, float eps, float* buf, float* pack, int flags,
                               ucd_stream_t stream);

/* sums[0:C] / sums[C:2C] = sum over the `tiles` rows of partial[tiles][2][C] (fixed order); sums_copy (optional) receives
 * the same; with UCD_NORM_ABS_GAMMA in flags the second row is multiplied by sign(weight) (see ucd_abn_bwd_reduce). */
int ucd_abn_reduce_partials(const float* partial, int tiles, int C, float* sums, float* sums_copy, const float* weight,
                            int flags, ucd_stream_t stream);

/* dw[N, K] (bf16) = dy[M, N]^T . in(a)[M, K] with the forward's input transform re-applied to a (N, K multiples of 128).
 * workspace: ucd_conv1x1_wgrad_workspace_bytes(M, N, K) bytes of fp32 split-M partials, combined in a fixed order. */
size_t ucd_conv1x1_wgrad_workspace_bytes(int M, int N, int K);
int ucd_conv1x1_wgrad(const void* dy, int ld_dy, const void* a, int lda, int M, int N, int K,
                      const float* in_mean, const float* in_scale, const float* in_shift, int in_act, float in_slope,
                      void* dw, void* workspace, size_t workspace_bytes, ucd_stream_t stream);

/* The combination + finalize step of ucd_abn_sync_forward on its own (the stem's fused norm + pooling applies the result itself):
 * gathered [world][2C] = every rank's [mean_r | M2_r] -> buf = [.. | mean | invstd | scale] and the running statistics. */
int ucd_abn_sync_finalize(const float* gathered, int world, int M, int C, const float* weight, float* running_mean,
                          float* running_var, float momentum, float eps, float* buf, int flags, ucd_stream_t stream);

/* ---- stem: norm_act + MaxPool2d(3, stride 2, padding 1) as one pass (models/resnet.py:58-64, mod1.bn1 + mod1.pool1) -----------
 * z [B, H, W, C] dense channels-last bf16 (the 7x7 convolution's output), C a multiple of 8 that divides 2048.
 *   ucd_stem_apply_pool     out [B, PH, PW, C] = max over each 3x3 window of bf16(act((z - mean) scale + beta)) - bit for bit
 *                           max_pool2d(abn_apply(z)), first maximum wins; idx (optional, uint8 [B, PH, PW, C]) = window position
 *                           0..8 of the maximum, kept for the backward; PH = ucd_stem_pooled_size(H)
 *   ucd_stem_pool_backward  phase 1: sums [2C] = (sum dyact, sum dyact xhat) with dyact = dpool * act' at the arg-max positions
 *                           (the layer's d bias / d weight; the second row times sign(weight) for UCD_NORM_ABS_GAMMA layers);
 *                           phase 2: dz [B, H, W, C] = the norm's input gradient for every position (count = B H W x ranks);
 *                           phase 3: both.  SyncBN all-reduces sums between the phases.  workspace:
 *                           ucd_stem_pool_workspace_bytes(C).  leaky_relu / identity only. */
/* The stem's convolution itself (models/resnet.py:58: Conv2d(3, 64, 7, stride 2, padding 3, bias False)): x fp32 [B, 3, H, W] with
 * element strides (sb, sc, sh, sw) - the loader's image in either memory format, converted to bf16 while it is staged -, w the
 * bf16 weight in channels-last memory order [64][7][7][3], z [B, OH, OW, 64] dense channels-last bf16, OH = (H - 1) / 2 + 1. */
int ucd_stem_conv7x7(const float* x, long long sb, long long sc, long long sh, long long sw, int B, int H, int W, const void* w,
                     void* z, ucd_stream_t stream);

/* The same convolution followed by the frozen-statistics norm + activation + 3x3 / 2 max pool (models/resnet.py:58-64 in evaluation
 * mode: the teacher) in ONE kernel: out [B, PH, PW, 64] bf16 = max_pool2d(act((conv(x) - mean) * scale + beta), 3, 2, 1), the
 * convolution output rounded to bf16 in between as ucd_stem_conv7x7 stores it - bit-identical to ucd_stem_conv7x7 followed by
 * ucd_stem_apply_pool, without the 257 x 257 x 64 map in memory.  leaky_relu / identity; mean, scale, beta [64] fp32, 16-byte aligned. */
int ucd_stem_conv_pool(const float* x, long long sb, long long sc, long long sh, long long sw, int B, int H, int W, const void* w,
                       const float* mean, const float* scale, const float* beta, int act, float slope, void* out, ucd_stream_t stream);
int ucd_stem_pooled_size(int n);
size_t ucd_stem_pool_workspace_bytes(int C);
int ucd_stem_apply_pool(const void* z, int B, int H, int W, int C, const float* mean, const float* scale, const float* beta, int act,
                        float slope, void* out, uint8_t* idx, ucd_stream_t stream);
int ucd_stem_pool_backward(const void* z, const void* dpool, const uint8_t* idx, int B, int H, int W, int C, const float* mean,
                           const float* invstd, const float* scale, const float* beta, const float* weight, float* sums, float count,
                           int act, float slope, void* dz, void* workspace, size_t workspace_bytes, int phase, ucd_stream_t stream);

/* Weight gradient of a stride-1 convolution on channels-last maps (backward of modules/residual.py:57-73 conv1 / conv2 / conv3 /
 * proj_conv, modules/deeplab.py:24-37 map_convs / red_conv; replaces MIOpen's weight-gradient solvers and the batched split-M
 * library products on the train step):
 *     dw[n][t][k] = sum_m dz[m][n] * x[shift_t(m)][k]      taps = 1: the 1x1 product dz^T x;  taps = 9: the 3x3 convolution with
 *                                                          padding = dilation over the [B, H, W, K] map behind x (M = B*H*W)
 * dz [M][N] and x [M][K] bf16 row matrices (leading dimensions in elements), N and K multiples of 64.  The result is in the
 * weight's channels-last order [N][kh][kw][K]: dw (bf16, may be NULL) and / or dw32 (fp32, may be NULL; += when accumulate32,
 * e.g. straight into the fp32 gradient bucket).  workspace: ucd_conv_wgrad_workspace_bytes(M, N, K, taps) bytes of fp32 slabs
 * (one per row chunk), added in a fixed order (deterministic).  3x3 layers with 128-aligned channels, M >= 8192 and dilation <= 18
 * run the three-tap form (one kernel row per workgroup, round 4); UCD_WGRAD3=0 in the environment keeps the 9-tap form for them
 * (both are exact on integer operands and agree bit for bit there: tests/test_conv1x1_fused_gpu.py). */
size_t ucd_conv_wgrad_workspace_bytes(int M, int N, int K, int taps);
/* The entry point is ucd_conv_wgrad_ex (below), with stride <= 1 and flags 0 for the plain call described above.  stride > 1: the
 * strided layers (modules/residual.py:57-73 conv2 with stride 2, :79 proj_conv 1x1 stride 2): x is the [B, H, W, K] input map, dz
 * the [M = B*OH*OW][N] output gradient with OH = (H - 1) / stride + 1; N and K multiples of 128.
 *
 * Round 6: the slab sum of a weight gradient may be DEFERRED into the next weight-gradient launch on the same stream (it rides as
 * extra workgroups behind that product's own: no launch, no kernel boundary; bit-identical result).
 * flags: bit 0 = the caller does not read dw / dw32, nor reuses `workspace`, before the next ucd_conv_wgrad* call on
 * this stream or ucd_conv_wgrad_flush(stream).  Deferral happens only while ucd_conv_wgrad_defer(1) is in force (returns the
 * previous setting; the gradient-bucket wrapper switches it on for its backward passes and flushes in front of its bucket copies);
 * ucd_conv_wgrad_flush launches the stream's pending sum, ucd_conv_wgrad_drop forgets it (an aborted backward).  The autograd
 * nodes of this library replace one launch per convolution of the reference's backward (modules/residual.py:67-73) this way.
 *
 * SIDE STREAM (round 6, mode bit 1 / flags bit 1): nothing in a backward pass waits for a weight gradient before the optimiser, yet on
 * the caller's stream each one sits in the chain of input-gradient products - ~190 of the ~850 dependent launches of a step, which at
 * 3 - 6 images per GPU fill a quarter of the chip each.  Under ucd_conv_wgrad_defer(mode) with mode & 2, a call with flags & 2 runs
 * on a stream owned by the library (lowest priority, one per caller stream), forked behind `stream`
 * and joined back into `stream` by ucd_conv_wgrad_flush(stream) / ucd_conv_wgrad_drop(stream); under stream capture fork and join
 * become the graph's edges.  An accepted call records its fork point on `stream` at once, its launches go out at the NEXT accepted
 * call or at the flush: in a replayed graph the branch created first keeps the fork point's hardware queue and the other one hops
 * behind a cross-queue signal - launched at the fork, the weight gradients would make the CALLER's chain the one that hops, ~8 us
 * per call.  flags & 2 promises: dz, x, dw / dw32 and `workspace` stay allocated and untouched by other
 * streams until that flush, `workspace` is not the one of a call without the flag, and dw is not read before the flush; an error
 * of a launch made later is returned by the call that triggers it.  Results are the same bits either way (the same kernels on the
 * same operands).
 *
 * The library keeps one record per CALLER stream: its pending sum, its side stream with the armed call and that stream's pending
 * sum.  ucd_conv_wgrad_flush(stream) launches the armed call and the pending sums of the record and joins its side stream;
 * ucd_conv_wgrad_drop(stream) forgets the pending sums and the armed call and joins launched side work.
 * ucd_conv_wgrad_defer(mode): bit 0 deferral, bit 1 side stream; returns the previous mode (process-wide).  ucd_conv_wgrad_mode():
 * the mode. */
int ucd_conv_wgrad_ex(const void* dz, int ld_dz, const void* x, int ld_x, int M, int N, int K, int taps, int H, int W, int dilation,
                      int stride, void* dw, float* dw32, int accumulate32, void* workspace, size_t workspace_bytes, int flags,
                      ucd_stream_t stream);
int ucd_conv_wgrad_defer(int mode);
int ucd_conv_wgrad_mode(void);
int ucd_conv_wgrad_flush(ucd_stream_t stream);
int ucd_conv_wgrad_drop(ucd_stream_t stream);
/* ucd_conv_wgrad_drop on every caller stream the library holds state for (an aborted backward whose streams the caller no longer
 * knows, e.g. a failed capture); the mode is kept; returns the first error (a NULL stream cannot mean "all": it is the default stream). */
int ucd_conv_wgrad_drop_all(void);

/* Kernel forms behind ucd_conv_wgrad* (results do not depend on the choice: both 3x3 forms are exact on integers and agree bit
 * for bit there).  ucd_conv_wgrad_plan is the one statement of which form, tile, row chunks, grid, LDS and slab sum a call gets,
 * and ucd_conv_wgrad_ex launches with exactly its numbers - a side-stream call with the plan made AT the call (rules and the
 * network's layers: DESIGN.md section 3.2; restated by tests/test_wgrad_plan_cpu.py).  It reads its arguments and the environment
 * only - no operand is dereferenced and no device touched, so it answers on a machine without a GPU - and returns the code and
 * message ucd_conv_wgrad_ex gives for these arguments (N and K multiples of 64; taps 1 or 9; H, W, dilation and M = B*OH*OW for
 * the 3x3 / strided forms; 128-aligned channels when strided; M < 2^22), UCD_EINVAL for a NULL plan.
 * Three environment variables exist for probes and A/B runs and are read at EVERY call of the plan (a probe or a test changes
 * them inside one process; never cached): UCD_WGRAD_TARGET (workgroups aimed for by the tile and strided forms; unset or <= 0:
 * 256 / 512 for 1x1, 512 / 1024 for 3x3 by the tiles of a chunk), UCD_WGRAD3_TARGET (the same for the row-3 form, default 256),
 * UCD_WGRAD3=0 (3x3 layers keep the tile form).  ucd_conv_wgrad_workspace_bytes is the geometry-free upper bound of
 * plan.workspace_bytes under the same variables. */
enum ucd_wgrad_form {
  UCD_WGRAD_TILE = 0,     /* wgrad_kernel<BN, BK, T9>: one (tile, tap, chunk) per workgroup */
  UCD_WGRAD_STRIDED = 1,  /* wgrad_kernel<128, 128, T9, true> */
  UCD_WGRAD_ROW3 = 2      /* wgrad3_kernel<NX>: one kernel row (three taps) per workgroup */
};
#define UCD_WGRAD_FORM_NAMES {"tile", "strided", "row3"}   /* indexed by enum ucd_wgrad_form */
typedef struct ucd_conv_wgrad_plan_t {
  int form;                  /* enum ucd_wgrad_form */
  int tile_n, tile_k, tiles_n, tiles_k;
  int chunks, rows_per_chunk, ksplit;   /* row chunks of whole 64-row steps; k-tile groups of a chunk that go to different XCDs */
  int x_tile_rows;           /* ROW3: 96 or 128 (NX = 3 / 4); else 0 */
  int grid, threads, lds_bytes;
  int sum_lanes, sum_blocks; /* the slab sum this call launches or leaves pending: chunk lanes (1, 4, 16) and workgroups */
  size_t workspace_bytes;    /* exactly chunks * N * taps * K * 4 for THIS call */
} ucd_conv_wgrad_plan_t;
int ucd_conv_wgrad_plan(int M, int N, int K, int taps, int H, int W, int dilation, int stride, ucd_conv_wgrad_plan_t* plan);

/* The weights of the input-gradient convolutions of ALL stride-1 layers in one launch: for table entry e = {src offset,
 * dst offset, Co, Ci, KH*KW} (elements into the flat bf16 buffers; 4-D weights in channels-last memory order
 * [out][kh][kw][in]), dst_e = src_e.flip(2, 3).transpose(0, 1) in the same memory order.  blocks [n_blocks][4] (device,
 * int32) = {entry, spatial tap, out-channel tile of 32, in-channel tile of 32}, entries [n][5] (device, int64).  Replaces the
 * per-layer flip + copy of the "input gradient on the forward solver" trick (ucd_amd/blocks.py::_StrideOneConvFn). */
int ucd_flip_weights_batched(const void* src_flat, void* dst_flat, const int* blocks, int n_blocks, const long long* entries,
                             ucd_stream_t stream);
/* The same with blocks = {entry, spatial tap, out-channel tile of 64, in-channel tile of 64}: 16-byte accesses on both sides. */
int ucd_flip_weights_batched64(const void* src_flat, void* dst_flat, const int* blocks, int n_blocks, const long long* entries,
                               ucd_stream_t stream);

/* dst[cols, rows] = src[rows, cols]^T (bf16): the [K, N] weight of the input-gradient product. */
int ucd_transpose_bf16(const void* src, int rows, int cols, void* dst, ucd_stream_t stream);

/* ---- fp32 stride-1 convolutions (the fp32 training mode, --opt_level O0; csrc/conv_f32.hip) ---------------------------
 * PRECISION: every fp32 operand is split as x = hi + lo, hi = bf16_rn(x), lo = bf16_rn(x - hi), and each product is
 * accumulated in fp32 as hi*hi + hi*lo + lo*hi on the bf16 matrix cores (three MFMAs per product).  The error per product is
 * about 3 * 2^-18 ~ 1e-5 relative (the rounding of each lo part plus the dropped lo*lo term) - ~100x below a bf16 product.
 * Inputs are assumed finite (an inf makes its lo part NaN).  On integer-valued operands whose partial sums stay below 2^24 the
 * result is exact.
 * All operands are fp32 row matrices with a row pitch in elements (multiple of 4, 16-byte aligned bases); rows past the end,
 * 3x3 halo positions and channel tails are read as zeros through range-checked loads - nothing outside an operand is touched.
 * No allocation, no host synchronisation: the calls capture into graphs.  UCD_EINVAL for shapes the kernels do not take (K or
 * N not a multiple of 32, unaligned pitch or base, an operand beyond 2 GB).
 *
 * ucd_conv_f32:  y[M][N] (+)= im2col(a)[M][taps K] . w[N][taps K]^T.  taps = 1: the 1x1 product; taps = 9: the 3x3 convolution
 * (stride 1, padding = dilation) over the [B, H, W, K] map behind a (M = B*H*W), w the channels-last weight [N][kh][kw][K].
 * accumulate != 0: y += the product.  The input gradient is the same call on w^T (1x1) or on w.flip(2, 3).transpose(0, 1) (3x3).
 * ucd_conv_f32_wgrad:  dw[N][taps K] = sum_m dz[m][n] * x[shift_t(m)][k] (taps 1 / 9 as above, dw dense in the weight's
 * channels-last order), written (not accumulated).  Row chunks reduce into ucd_conv_f32_wgrad_workspace_bytes(M, N, K, taps)
 * bytes of fp32 slabs (0: none needed), summed in a fixed order on the same stream: no atomics, bit-reproducible. */
int ucd_conv_f32(const float* a, int lda, const float* w, int ldw, float* y, int ldy, int M, int N, int K, int taps, int H, int W,
                 int dilation, int accumulate, ucd_stream_t stream);
size_t ucd_conv_f32_wgrad_workspace_bytes(int M, int N, int K, int taps);
int ucd_conv_f32_wgrad(const float* dz, int ld_dz, const float* x, int ld_x, int M, int N, int K, int taps, int H, int W,
                       int dilation, float* dw, void* workspace, size_t workspace_bytes, ucd_stream_t stream);

/* ---- optimiser step -------------------------------------------------------------------------------------------------
 * Replaces `optim.step()` (train.py:147) of the reference's torch.optim.SGD(params, lr, momentum=0.9, nesterov=True) with
 * per-group weight decay (run.py:175-186) by ONE launch over every parameter tensor; the bf16 working copy of a
 * convolution weight (apex AMP O1's per-call cast, run.py:199-200) is written in the same pass.
 *   g' = g + wd p;  m' = mu m + g';  d = g' + mu m' (nesterov) | m';  p' = p - lr d;  w16 = bf16(p')
 * (double intermediates like torch's fused kernel; dampening 0; a zero-initialised m makes the first step torch's
 * "momentum buffer = clone of the gradient").  table [n] (device): one entry per tensor - p, g, m fp32 with identical
 * dense layouts of n elements, m NULL for momentum 0, w16 NULL or the bf16 copy of the same layout, group = index into
 * the hyper-parameter arrays.  blocks [n_blocks][2] (device, int32) = {table entry, chunk of ucd_sgd_chunk() elements}. */
#define UCD_SGD_MAX_GROUPS 8
typedef struct ucd_sgd_tensor {
  float* p;  const float* g;  float* m;  void* w16;
  long long n;
  int group;  int pad;
} ucd_sgd_tensor;
typedef struct ucd_sgd_hyper {
  double lr[UCD_SGD_MAX_GROUPS], momentum[UCD_SGD_MAX_GROUPS], weight_decay[UCD_SGD_MAX_GROUPS];
  int nesterov[UCD_SGD_MAX_GROUPS];
} ucd_sgd_hyper;
int ucd_sgd_chunk(void);
int ucd_sgd_step(const ucd_sgd_tensor* table, const int* blocks, int n_blocks, const ucd_sgd_hyper* hyper, ucd_stream_t stream);
/* The same step with the hyper-parameters in DEVICE memory (device_hyper): the form a captured hipGraph of the whole training
 * iteration (train.py:95-151) replays while PolyLR changes the learning rate every iteration (train.py:150-151) - a by-value
 * kernel argument would be frozen into the graph.  ucd_sgd_hyper_store writes host values into that device struct in stream
 * order (the values travel as a kernel argument: no pinned staging buffer that a later step could overwrite early). */
int ucd_sgd_hyper_store(ucd_sgd_hyper* device_hyper, const ucd_sgd_hyper* hyper, ucd_stream_t stream);
int ucd_sgd_step_dev(const ucd_sgd_tensor* table, const int* blocks, int n_blocks, const ucd_sgd_hyper* device_hyper,
                     ucd_stream_t stream);

/* ---- EWC / PI / RW regulariser ----------------------------------------------------------------------------------------
 * The weight-space penalty of the reference's other baselines (utils/regularizer.py, train.py:139-145) as ONE pass over every
 * trainable tensor, run between the gradient all-reduce and the optimiser step.  Per element, with g the data gradient:
 *   EWC:  F = a g^2 + b F
 *   PI:   if counter > 0: delta += g (temp - p);  temp = p
 *   RW:   if counter % iterations == 0 { if counter > 0: score += g (temp - p) / (0.5 F (p - temp)^2 + 1e-8);  temp = p }
 *         F = a g^2 + b F
 *   then, where `penalize` is set:  sum += omega (p - p_old)^2;  g += (lambda omega) (2 (p - p_old))
 * (fp32, one rounding per operation, IEEE division: the reference's torch ops bit for bit; a = float(alpha),
 * b = float(1 - alpha), lambda = float(reg_importance)).  Entry `score` holds PI's delta or RW's score.  State pointers a
 * method does not use may be NULL; p_old and omega may be NULL where penalize == 0.  All arrays of an entry share one dense
 * layout of n elements.  blocks [n_blocks][2] (device, int32) = {table entry, chunk of ucd_reg_chunk() elements}.
 * The hyper-parameters and the update counter live in device memory (written once by ucd_reg_hyper_store); the second launch
 * of ucd_reg_step adds the per-block fp64 partials (device, n_blocks doubles) in a fixed order, writes
 * penalty[0] = float(reg_importance * sum) and increments the counter, so a captured step graph advances it on every replay.
 * No allocation, no host synchronisation.  UCD_EINVAL: n_blocks < 0, NULL table / blocks / hyper / partials / penalty with
 * n_blocks > 0, unknown method.  n_blocks == 0: no-op. */
#define UCD_REG_EWC 0
#define UCD_REG_PI 1
#define UCD_REG_RW 2
typedef struct ucd_reg_tensor {
  float* p;  float* g;  const float* p_old;  const float* omega;
  float* fisher;  float* score;  float* temp;
  long long n;
  int penalize;  int pad;
} ucd_reg_tensor;
typedef struct ucd_reg_hyper {
  double reg_importance;
  float alpha, one_minus_alpha, lambda_f;
  int iterations;
  int counter;
  int pad;
} ucd_reg_hyper;
int ucd_reg_chunk(void);
int ucd_reg_hyper_store(ucd_reg_hyper* device_hyper, const ucd_reg_hyper* hyper, ucd_stream_t stream);
int ucd_reg_step(const ucd_reg_tensor* table, const int* blocks, int n_blocks, int method, ucd_reg_hyper* device_hyper,
                 double* partials, float* penalty, ucd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* UCD_HIP_H */
