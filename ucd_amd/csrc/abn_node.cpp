// Autograd node of the training-mode ABN layer in C++ (PyTorch extension, host code only).
//
// The kernels live behind the C ABI (include/ucd_hip.h); what this file replaces is the Python wrapper around them on
// the student's 106 training-mode layers: a Python autograd.Function costs ~38 us forward and ~33 us backward of host
// time per layer (tools/host_profile.py), which is what bounds the step once a GPU holds 3-6 images (4-8 GPU runs).
// Here the forward is one pybind call (~8 us) and the backward never enters Python.  It mirrors
// ucd_amd/abn.py::_ABNFunction for the case it is used for - batch statistics, dense channels-last input, optional
// fused residual, optional SyncBN through the library-owned RCCL communicator - and the Python class stays the
// reference implementation for everything else (eval mode, plane bias, slice outputs, torch.distributed fallback).
//
// The reference reaches the same work through inplace_abn's autograd Functions (segmentation_module.py:15-20).
#include <torch/extension.h>
#include <torch/csrc/autograd/engine.h>
#include <torch/csrc/autograd/graph_task.h>
#include <torch/csrc/autograd/utils/grad_layout_contract.h>

#include <array>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <tuple>

#include "../../include/ucd_hip.h"

namespace {

using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

void check(int rc, const char* what) {
  TORCH_CHECK(rc == 0, what, " failed (code ", rc, "): ", ucd_last_error());
}

// grow-only scratch per (device, stream); calls on one stream are ordered
std::mutex g_mu;
std::map<std::pair<int, int64_t>, at::Tensor> g_ws;

// Tensors that kernels on the library's SIDE stream (weight gradients, include/ucd_hip.h ucd_conv_wgrad_ex flags & 2) still read or
// write, by the caller's stream: the caching allocator knows nothing of the side stream, so the operands stay referenced here until
// a join of that stream succeeded (wgrad_side_release) - a block freed on the compute stream before that could be handed to a later
// kernel of that stream while the side stream is still reading it.
std::map<int64_t, std::vector<at::Tensor>> g_side_hold;
constexpr int kWsTags = 8;     // tags 0 / 1 scratch of the nodes, 2 / 3 slab workspaces in turn, 4 / 5 the same for side-stream calls

void* workspace(const at::Tensor& like, size_t bytes, int64_t stream, int tag = 0) {
  std::lock_guard<std::mutex> lock(g_mu);
  auto key = std::make_pair((int)like.get_device() * kWsTags + tag, stream);
  auto it = g_ws.find(key);
  if (it == g_ws.end() || (size_t)it->second.numel() < bytes) {
    size_t n = bytes < ((size_t)1 << 20) ? ((size_t)1 << 20) : bytes;
    if (it != g_ws.end() && tag >= 4) g_side_hold[stream].push_back(it->second);     // the side stream may still be in the old buffer
    g_ws[key] = at::empty({(int64_t)n}, like.options().dtype(at::kByte));
    it = g_ws.find(key);
  }
  return it->second.data_ptr();
}

// the operands held for the side work of `stream` (every stream: nullopt) - call only behind a join that succeeded
void wgrad_side_release(c10::optional<int64_t> stream) {
  std::map<int64_t, std::vector<at::Tensor>> gone;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    if (!stream) gone.swap(g_side_hold);
    else if (auto it = g_side_hold.find(*stream); it != g_side_hold.end()) gone.insert(g_side_hold.extract(it));
  }
}   // the tensors are released outside the lock

int64_t g_pass_flushes = 0;                      // test hook: end-of-pass flushes run so far
int64_t g_wgrad_calls[2] = {0, 0};               // test hook: own weight-gradient calls of the nodes, those of them issued with flags
std::map<int, std::set<int64_t>> g_pass_streams;  // under g_mu: by autograd graph task, the streams its deferring calls ran on

// A weight-gradient call that may be deferred / moved to the side stream is final only behind ucd_conv_wgrad_flush.  The
// gradient-bucket wrapper flushes in front of its copies - but a pass it does not see to its end (torch.autograd.grad under the
// wrapper: no AccumulateGrad, no hook) would hand out gradients whose last slab sum never ran.  So the first such call of a backward
// pass queues the flush as an engine callback: it runs when the pass ends, whoever started it, in stream order before the caller
// gets its gradients, and flushes every stream the pass's calls ran on (a second flush by the wrapper is a no-op).  A pass that dies
// never runs its callback (its entry stays behind, a few bytes); the next pass is another graph task and queues its own.
void queue_end_of_pass_flush(int64_t stream) {
  const int task = torch::autograd::get_current_graph_task_id();
  {
    std::lock_guard<std::mutex> lock(g_mu);
    auto [it, first] = g_pass_streams.try_emplace(task);
    it->second.insert(stream);
    if (!first) return;
  }
  torch::autograd::Engine::get_default_engine().queue_callback([task]() {
    ++g_pass_flushes;
    std::set<int64_t> streams;
    {
      std::lock_guard<std::mutex> lock(g_mu);
      streams = std::move(g_pass_streams.at(task));
      g_pass_streams.erase(task);
    }
    std::string err;
    for (int64_t s : streams) {
      const int rc = ucd_conv_wgrad_flush((ucd_stream_t)s);
      if (rc == 0) wgrad_side_release(s);
      else if (err.empty()) err = "code " + std::to_string(rc) + ": " + ucd_last_error();
    }
    TORCH_CHECK(err.empty(), "ucd_conv_wgrad_flush failed at the end of the backward pass (", err, ")");
  });
}

// test hook (tests/diag/poison_step_diag.py): fill every cached scratch buffer with a byte pattern - a kernel that reads scratch it has
// not written shows up as a changed (or NaN) result
void poison_workspaces(int64_t byte, int64_t tag) {
  std::lock_guard<std::mutex> lock(g_mu);
  for (auto& kv : g_ws)
    if (tag < 0 || kv.first.first % kWsTags == tag) kv.second.fill_(byte);
}

// ---- statistics arena (round 5) ----------------------------------------------------------------------------------------------------
// The per-layer [2 C] accumulators that the GEMM epilogues add their column sums to with fp32 atomics (ucd_conv1x1 stat_acc) live in
// ONE zero-filled buffer per device: a slot is handed out per layer and direction during the forward, and stat_arena_reset - called
// once per training step (ucd_amd/train.py, ucd_amd/ddp.py) - zeroes the used range with ONE fill and starts over.  Correctness never
// depends on the caller: every slot carries the arena's generation, a reset invalidates the slots of older generations (their
// consumers fall back to the reduction kernels), and a full arena resets itself.
struct StatArena {
  at::Tensor buf;
  int64_t off = 0, gen = 1;
  int64_t high = 0;            // high-water mark of `off` over all generations: what a reset zeroes
};
std::map<int, StatArena> g_arena;
constexpr int64_t kArenaFloats = 16 << 20;     // 64 MiB: about four steps' worth at the benchmark's shapes (replicated slots, ~15 MB per step)

int64_t arena_gen(int dev) {
  std::lock_guard<std::mutex> lock(g_mu);
  return g_arena[dev].gen;
}

void stat_arena_reset(int64_t dev, int64_t stream) {
  std::lock_guard<std::mutex> lock(g_mu);
  auto it = g_arena.find((int)dev);
  if (it == g_arena.end() || !it->second.buf.defined()) return;
  StatArena& a = it->second;
  // one fill in stream order (a memset node in a captured step).  A raw memset, not Tensor::zero_(): slots handed out earlier are
  // views of this buffer saved by autograd nodes, and an in-place ATen op would move their shared version counter - a backward that
  // follows a reset must reach the generation check (and fall back), not autograd's "modified by an inplace operation"
  // up to the HIGH-WATER mark, not the last step's footprint: a captured step graph freezes this range into its memset
  // node - had the eager step in front of the capture used fewer floats than the captured one (another batch shape: the replica
  // count of a slot depends on M), the slots beyond would never be zeroed on replay and their atomic sums would grow across replays
  if (a.off > a.high) a.high = a.off;
  if (a.high > 0) check(ucd_fill_zero(a.buf.data_ptr(), (size_t)a.high * sizeof(float), (ucd_stream_t)stream), "ucd_fill_zero");
  a.off = 0;
  a.gen += 1;
}

// n floats (rounded to 64) of zeros, or an undefined tensor (arena switched off by the caller / request larger than the arena)
at::Tensor arena_alloc(const at::Tensor& like, int64_t n, int64_t* gen, int64_t stream) {
  const int dev = (int)like.get_device();
  n = (n + 63) / 64 * 64;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    StatArena& a = g_arena[dev];
    if (!a.buf.defined()) a.buf = at::zeros({kArenaFloats}, like.options().dtype(at::kFloat));
    if (n > kArenaFloats) return at::Tensor();
    if (a.off + n <= kArenaFloats) {
      at::Tensor t = a.buf.narrow(0, a.off, n);
      a.off += n;
      *gen = a.gen;
      return t;
    }
  }
  stat_arena_reset(dev, stream);               // full (nobody resets per step): zero it, invalidate the outstanding slots
  std::lock_guard<std::mutex> lock(g_mu);
  StatArena& a = g_arena[dev];
  at::Tensor t = a.buf.narrow(0, 0, n);
  a.off = n;
  *gen = a.gen;
  return t;
}

bool dense_channels_last(const at::Tensor& x) {
  if (x.dim() != 4) return false;
  const auto B = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  (void)B;
  return H > 1 && W > 1 && x.stride(1) == 1 && x.stride(3) == C && x.stride(2) == W * C && x.stride(0) == H * W * C &&
         (reinterpret_cast<uintptr_t>(x.data_ptr()) & 15) == 0 && ((C * x.element_size()) & 15) == 0;
}

int dtype_code(const at::Tensor& x) {
  if (x.scalar_type() == at::kBFloat16) return UCD_BF16;
  TORCH_CHECK(x.scalar_type() == at::kFloat, "ucd abn node: bf16 or fp32 activations only");
  return UCD_F32;
}

const float* fptr(const at::Tensor& t) { return t.defined() ? t.data_ptr<float>() : nullptr; }

// Slab workspace of a weight-gradient call.  The calls of the autograd nodes allow the library to DEFER their slab sum into the next
// weight-gradient launch of the stream (ucd_conv_wgrad_ex, flags bit 0: the gradient goes to AccumulateGrad and is first read by the
// bucket copies, in front of which ucd_amd/ddp.py flushes) - so a call's slabs must outlive the NEXT call: two scratch buffers, taken
// in turn.
void* wgrad_workspace(const at::Tensor& like, size_t bytes, int64_t stream, bool side) {
  static std::map<std::pair<int, int64_t>, int> turn;   // per (device, stream, side): the pending sum is per stream too
  int tag;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    tag = (side ? 4 : 2) + (turn[std::make_pair((int)like.get_device() * 2 + (side ? 1 : 0), stream)] ^= 1);
  }
  return workspace(like, bytes, stream, tag);
}

// flags of a node's weight-gradient call (ucd_conv_wgrad_ex): bit 0 the slab sum may wait, bit 1 the call may leave the compute
// stream - both only for a gradient nothing reads before the wrapper's flush (sum_may_wait below); with bit 1 in force the operands
// are held until that flush.  dw: the tensor the node returns as the weight's gradient.
int sum_may_wait(const at::Tensor& w4, const at::Tensor& dw);
int wgrad_flags(const at::Tensor& w4, const at::Tensor& dw, bool* side) {
  *side = false;
  if (!sum_may_wait(w4, dw)) return 0;
  *side = (ucd_conv_wgrad_mode() & 2) != 0;
  return *side ? 3 : 1;
}
void count_wgrad_call(int flags) {
  std::lock_guard<std::mutex> lock(g_mu);
  ++g_wgrad_calls[0];
  if (flags & 3) ++g_wgrad_calls[1];
}
void hold_for_side(int64_t stream, std::initializer_list<at::Tensor> ts) {
  std::lock_guard<std::mutex> lock(g_mu);
  auto& held = g_side_hold[stream];
  held.insert(held.end(), ts);
}

// bf16 working copies of ucd_amd.master.Bf16Weights (by tensor; a weak reference keeps the address from being reused): their one
// post-accumulate-grad hook is the gradient-bucket wrapper's (ucd_amd/ddp.py _on_grad), which reads no gradient values - the code
// that consumes them (_complete / finish) flushes first
std::map<const c10::TensorImpl*, c10::weak_intrusive_ptr<c10::TensorImpl>> g_working;   // under g_mu

void wgrad_register_working(const std::vector<at::Tensor>& ts) {
  std::lock_guard<std::mutex> lock(g_mu);
  for (auto it = g_working.begin(); it != g_working.end();) it = it->second.expired() ? g_working.erase(it) : std::next(it);
  for (const auto& t : ts) g_working.insert_or_assign(t.unsafeGetTensorImpl(), c10::weak_intrusive_ptr<c10::TensorImpl>(t.getIntrusivePtr()));
}

bool registered_working(const at::Tensor& w) {
  std::lock_guard<std::mutex> lock(g_mu);
  auto it = g_working.find(w.unsafeGetTensorImpl());
  return it != g_working.end() && !it->second.expired();
}

// May the slab sum of this weight gradient wait for the next weight-gradient launch (and the product leave the compute stream)?
// Only when AccumulateGrad will adopt the returned tensor untouched and nothing reads it before the wrapper's / the end-of-pass
// flush (torch/csrc/autograd/functions/accumulate_grad.h, case 1.1):
//  - the weight is a leaf that requires its gradient (the output of autocast's per-call cast has a ToCopyBackward node behind it
//    that reads the gradient at once);
//  - it has no .grad yet (otherwise AccumulateGrad adds into it: the gradient-bucket views of ucd_amd/ddp.py are such a .grad);
//  - grad mode is off (backward(create_graph=True): AccumulateGrad clones);
//  - dw obeys the gradient layout contract with the weight (otherwise AccumulateGrad re-strides it into a copy);
//  - no tensor hook (it receives dw before AccumulateGrad) and no post-accumulate-grad hook (it reads .grad before the flush),
//    except the wrapper's own on a registered working copy.
// Everywhere else the call runs exactly as with deferral off.  Not seen here: a weight used by two nodes of one graph, whose two
// gradients the engine adds before AccumulateGrad - no model of this project shares a convolution weight.
int sum_may_wait(const at::Tensor& w4, const at::Tensor& dw) {
  if (!(w4.defined() && w4.is_leaf() && w4.requires_grad())) return 0;
  if (w4.grad().defined() || at::GradMode::is_enabled()) return 0;
  if (!torch::autograd::utils::obeys_layout_contract(dw, w4)) return 0;
  if (!torch::autograd::impl::hooks(w4).empty()) return 0;
  if (torch::autograd::impl::post_acc_grad_hooks(w4) && !registered_working(w4)) return 0;
  return 1;
}

// ---- weight gradients of the convolution nodes -------------------------------------------------------------------------------------
// Route of a layer's weight gradient (the same values as ucd_amd/blocks.py WGRAD_*): the batched split-M library products (stride-1
// 1x1 layers only: any other layer takes the library instead), MIOpen's weight-gradient solver, or the own kernel (ucd_conv_wgrad,
// csrc/wgrad.hip) where the layer is one it takes, else the caller's fallback route.
enum WgradRoute : int64_t { kWgradSplit = 0, kWgradLibrary = 1, kWgradOwn = 2 };

// Number of K-chunks of the split products over M rows: the weight gradient of a long M is eight batched K-chunks + a sum (41 us
// against 96 for the best single-kernel candidate at M = 26136).
int64_t wgrad_split(int64_t M) {
  if (M >= 8192)
    for (int64_t S : {8, 4, 12, 6, 3, 2})
      if (M % S == 0) return S;
  return 1;
}

// Does the own kernel take this layer?  Row form (x 2-D, a 1x1 layer): dz [M, N] and x [M, K] contiguous 16-byte aligned bf16.  Map
// form: dz [B, N, OH, OW] (the smaller output map of a strided layer) and x [B, K, H, W] dense channels-last bf16, a 1x1 weight or a
// 3x3 weight in channels-last order - every 3x3 layer (tools/wgrad_probe2.py, profiles/r03_wgrad_probe.txt: 64-256 channel layers
// 50-58 vs 80-100 us for MIOpen's solver, 512 -> 512 213 vs 215, the ASPP branches 392 vs 372 - plus the ~35 us of zero-fill / cast
// kernels MIOpen wraps around its solver on the step) - and 128-aligned channels when strided.  Both: 64-aligned channels, M < 2^22.
bool own_wgrad_ok(const at::Tensor& dz, const at::Tensor& x, const at::Tensor& w4, int64_t stride) {
  if (x.dim() == 2)
    return dz.dim() == 2 && dz.is_contiguous() && x.is_contiguous() && dz.scalar_type() == at::kBFloat16 &&
           x.scalar_type() == at::kBFloat16 && dz.size(1) % 64 == 0 && x.size(1) % 64 == 0 && dz.size(0) < (1 << 22) &&
           (reinterpret_cast<uintptr_t>(dz.data_ptr()) & 15) == 0 && (reinterpret_cast<uintptr_t>(x.data_ptr()) & 15) == 0;
  const int64_t N = w4.size(0), K = w4.size(1);
  return dz.defined() && dense_channels_last(dz) && dense_channels_last(x) && dz.scalar_type() == at::kBFloat16 &&
         x.scalar_type() == at::kBFloat16 && N % 64 == 0 && K % 64 == 0 && dz.size(1) == N && x.size(1) == K &&
         x.size(0) * x.size(2) * x.size(3) < (1 << 22) &&
         ((w4.size(2) == 1 && w4.size(3) == 1) ||
          (w4.size(2) == 3 && w4.size(3) == 3 && w4.is_contiguous(at::MemoryFormat::ChannelsLast))) &&
         (stride == 1 || (N % 128 == 0 && K % 128 == 0));
}

// The weight gradient of a convolution node by `route`: dz the gradient of the output, x the input (both maps, or the row matrices of
// a 1x1 layer), w4 the weight [N, K, k, k]; dilation and stride those of the convolution (padding dilation * (k / 2)).  Returns what
// the node hands AccumulateGrad: the weight's sizes, in the weight's own memory order on the own and split routes.
at::Tensor conv_wgrad(const at::Tensor& dz, const at::Tensor& x, const at::Tensor& w4, int64_t dilation, int64_t stride, int64_t route,
                      WgradRoute fallback, int64_t stream) {
  const bool rows = x.dim() == 2;
  const int64_t N = w4.size(0), K = w4.size(1), k = w4.size(2);
  if (route == kWgradOwn) {
    // a bf16 map in another memory order is made dense channels-last for the own kernel (the other routes take it as it is)
    const at::Tensor dzo = !rows && dz.scalar_type() == at::kBFloat16 && !dense_channels_last(dz)
                               ? dz.contiguous(at::MemoryFormat::ChannelsLast) : dz;
    if (own_wgrad_ok(dzo, x, w4, stride)) {
      const int64_t M = rows ? x.size(0) : x.size(0) * dzo.size(2) * dzo.size(3);
      at::Tensor dw = rows ? at::empty({N, K}, x.options()) : at::empty({N, k, k, K}, x.options());
      // the tensor returned: [N, K, kh, kw] with channels-last strides (row form: the weight's strides) - the weight's own memory
      // order; the side-stream hold keeps the base dw, so that AccumulateGrad may still adopt the view
      at::Tensor ret = rows ? dw.as_strided(w4.sizes(), w4.strides()) : dw.permute({0, 3, 1, 2});
      const size_t wsb = ucd_conv_wgrad_workspace_bytes((int)M, (int)N, (int)K, (int)(k * k));
      bool side;
      const int flags = wgrad_flags(w4, ret, &side);
      count_wgrad_call(flags);
      if (side) hold_for_side(stream, {dzo, x, dw});
      if (flags && ucd_conv_wgrad_mode()) queue_end_of_pass_flush(stream);
      check(ucd_conv_wgrad_ex(dzo.data_ptr(), (int)N, x.data_ptr(), (int)K, (int)M, (int)N, (int)K, (int)(k * k),
                              rows ? 0 : (int)x.size(2), rows ? 0 : (int)x.size(3), (int)(k == 3 ? dilation : 1), (int)stride,
                              dw.data_ptr(), nullptr, 0, wgrad_workspace(x, wsb, stream, side), wsb, flags, (ucd_stream_t)stream),
            "ucd_conv_wgrad");
      return ret;
    }
    route = fallback;
  }
  if (route == kWgradSplit && k == 1 && stride == 1) {
    const int64_t M = rows ? x.size(0) : x.size(0) * x.size(2) * x.size(3);
    const at::Tensor dz2 = rows ? dz : dz.permute({0, 2, 3, 1}).reshape({M, N}), x2 = rows ? x : x.permute({0, 2, 3, 1}).reshape({M, K});
    const int64_t S = wgrad_split(M);
    at::Tensor dw;
    if (S > 1) {
      dw = at::bmm(dz2.view({S, M / S, N}).transpose(1, 2), x2.view({S, M / S, K})).sum(0);
    } else {
      dw = at::empty({N, K}, x.options());
      const size_t wsb = ucd_gemm_workspace_bytes();
      check(ucd_gemm_bf16(2, (int)N, (int)K, (int)M, dz2.data_ptr(), (int)N, x2.data_ptr(), (int)K, dw.data_ptr(), (int)K,
                          workspace(x, wsb, stream, 1), wsb, 1, (ucd_stream_t)stream),
            "ucd_gemm_bf16");
    }
    return dw.as_strided(w4.sizes(), w4.strides());   // [N, K, 1, 1] is one memory order in either format
  }
  const int64_t pad = dilation * (k / 2);
  return std::get<1>(at::convolution_backward(dz, x, w4, c10::nullopt, {stride, stride}, {pad, pad}, {dilation, dilation}, false,
                                              {0, 0}, 1, {false, true, false}));
}

// ---- what the nodes share ----------------------------------------------------------------------------------------------------------
// The state a node keeps for its backward is ONE struct S: tensors() points at its tensor members in the order they are saved,
// scalars() ties the rest.  forward hands it to keep(), backward gets it back from kept() - no index and no key is written twice.
template <class... A> std::tuple<A...> values(const std::tuple<A&...>& refs) { return refs; }

template <class S> void keep(AutogradContext* ctx, S& s) {
  variable_list v;
  for (at::Tensor* t : s.tensors()) v.push_back(*t);
  ctx->save_for_backward(std::move(v));
  ctx->saved_data["scalars"] = values(s.scalars());
}

template <class S> S kept(AutogradContext* ctx) {
  S s;
  const variable_list saved = ctx->get_saved_variables();
  size_t i = 0;
  for (at::Tensor* t : s.tensors()) *t = saved[i++];
  auto refs = s.scalars();
  refs = ctx->saved_data["scalars"].to<decltype(values(refs))>();
  return s;
}

// what a backward returns: one gradient per argument of the node's forward, undefined until set
template <class R, class... A> variable_list no_grads(R (*)(AutogradContext*, A...)) { return variable_list(sizeof...(A)); }

at::Tensor or_undefined(const c10::optional<at::Tensor>& t) { return t.has_value() ? *t : at::Tensor(); }

// Training-mode ABN forward, y = act(BN_batch(in) [+ residual]) with the statistics left in buf (comm != 0: SyncBN through the
// library's communicator): ABNTrainNode.
void abn_batch_forward(int64_t comm, int64_t world, const at::Tensor& in, const at::Tensor& y, const at::Tensor& residual, int64_t M,
                       int64_t C, int64_t HW, const at::Tensor& weight, const at::Tensor& bias, const at::Tensor& running_mean,
                       const at::Tensor& running_var, double momentum, double eps, float* buf, int64_t act, double slope, void* ws,
                       size_t ws_bytes, int64_t stream) {
  const void* res = residual.defined() ? residual.data_ptr() : nullptr;
  const int ldr = res ? (int)C : 0, dt = dtype_code(in);
  if (comm != 0) {
    check(ucd_abn_sync_forward_comm((ucd_comm_t)comm, (int)world, in.data_ptr(), (int)C, y.data_ptr(), (int)C, res, ldr, dt, (int)M,
                                    (int)C, nullptr, (int)HW, fptr(weight), fptr(bias), running_mean.data_ptr<float>(),
                                    running_var.data_ptr<float>(), (float)momentum, (float)eps, buf, (int)act, (float)slope, ws,
                                    ws_bytes, (ucd_stream_t)stream),
          "ucd_abn_sync_forward_comm");
  } else {
    check(ucd_abn_forward(in.data_ptr(), (int)C, y.data_ptr(), (int)C, res, ldr, dt, (int)M, (int)C, nullptr, (int)HW, fptr(weight),
                          fptr(bias), running_mean.data_ptr<float>(), running_var.data_ptr<float>(), (float)momentum, (float)eps, 1,
                          buf, nullptr, (int)act, (float)slope, ws, ws_bytes, (ucd_stream_t)stream),
          "ucd_abn_forward");
  }
}

// Where the two backward sums of an ABN layer live.  `local` receives this rank's [d bias | d weight]: the layer's slice of the
// gradient bucket when the caller gave one (param_grad; the node then reports no parameter gradients), else a fresh tensor whose
// halves are dbias / dweight.  `global` is what the apply pass reads: the same place in a single process; under SyncBN the sums
// over all ranks, in front of the local ones ([global 2 N | local 2 N], or [global 2 N] alone with param_grad).
struct Sums {
  at::Tensor store, dbias, dweight;
  float *global = nullptr, *local = nullptr;
  Sums(bool sync, float* param_grad, int64_t N, const at::Tensor& like) {
    if (sync || !param_grad) store = at::empty({(sync && !param_grad ? 4 : 2) * N}, like.options().dtype(at::kFloat));
    const int64_t off = sync ? 2 * N : 0;
    local = param_grad ? param_grad : store.data_ptr<float>() + off;
    global = sync ? store.data_ptr<float>() : local;
    if (!param_grad) {
      dbias = store.narrow(0, off, N);
      dweight = store.narrow(0, off + N, N);
    }
  }
};

// Training-mode ABN backward (reduction + apply; comm != 0: SyncBN): din = d in, dres = d residual where the layer has one (else
// undefined), y the saved output where the activation's sign needs it (else undefined), b the forward's statistics buffer.
void abn_batch_backward(int64_t comm, int64_t world, const at::Tensor& in, const at::Tensor& dy, const at::Tensor& y,
                        const at::Tensor& din, const at::Tensor& dres, int64_t M, int64_t C, int64_t HW, const float* b,
                        const at::Tensor& weight, const at::Tensor& bias, const Sums& sums, int64_t act, double slope, void* ws,
                        size_t ws_bytes, int64_t stream) {
  const float *mean = b + 3 * C, *invstd = b + 4 * C, *scale = b + 5 * C;
  const void* yp = y.defined() ? y.data_ptr() : nullptr;
  void* dresp = dres.defined() ? dres.data_ptr() : nullptr;
  const int ldy = yp ? (int)C : 0, ldres = dresp ? (int)C : 0, dt = dtype_code(in);
  if (comm != 0) {
    check(ucd_abn_sync_backward_comm((ucd_comm_t)comm, (int)world, in.data_ptr(), (int)C, dy.data_ptr(), (int)C, yp, ldy, din.data_ptr(),
                                     (int)C, dresp, ldres, dt, (int)M, (int)C, nullptr, (int)HW, mean, invstd, scale, fptr(bias),
                                     fptr(weight), sums.global, sums.local, (int)act, (float)slope, ws, ws_bytes, (ucd_stream_t)stream),
          "ucd_abn_sync_backward_comm");
  } else {
    check(ucd_abn_backward(in.data_ptr(), (int)C, dy.data_ptr(), (int)C, yp, ldy, din.data_ptr(), (int)C, dresp, ldres, dt, (int)M,
                           (int)C, nullptr, (int)HW, mean, invstd, scale, fptr(bias), fptr(weight), sums.local, (float)M, 1, 1, (int)act,
                           (float)slope, ws, ws_bytes, (ucd_stream_t)stream),
          "ucd_abn_backward");
  }
}

// d x = dy . w through the tuned library product (x: rows [M, Ci], or a dense channels-last map of M rows; w4 [Co, Ci, 1, 1]) with
// the gradient of a shortcut that left x next to the convolution: folded into the product where it is bf16 (beta = 1, in place on
// dskip), else added afterwards.  dy or dskip may be undefined.
at::Tensor library_dgrad(const at::Tensor& dy, const at::Tensor& w4, const at::Tensor& x, at::Tensor dskip, int64_t M, void* ws,
                         size_t wsb, int64_t stream) {
  const int Ci = (int)w4.size(1), Co = (int)w4.size(0);
  auto product = [&](const at::Tensor& out) {
    check(ucd_gemm_bf16(1, (int)M, Ci, Co, dy.data_ptr(), Co, w4.data_ptr(), Ci, out.data_ptr(), Ci, ws, wsb, 1, (ucd_stream_t)stream),
          "ucd_gemm_bf16");
  };
  if (dskip.defined() && dy.defined() && dskip.scalar_type() == at::kBFloat16) {
    if (x.dim() != 4) dskip = dskip.contiguous();
    else if (!dense_channels_last(dskip)) dskip = dskip.contiguous(at::MemoryFormat::ChannelsLast);
    if (!ucd_gemm_has_plan(1, (int)M, Ci, Co, Co, Ci, Ci)) product(at::empty_like(x));   // tune once, into scratch
    check(ucd_gemm_bf16_acc(1, (int)M, Ci, Co, dy.data_ptr(), Co, w4.data_ptr(), Ci, dskip.data_ptr(), Ci, ws, wsb, (ucd_stream_t)stream),
          "ucd_gemm_bf16_acc");
    return dskip;
  }
  if (!dy.defined()) return dskip;
  at::Tensor dx = at::empty_like(x);
  product(dx);
  return dskip.defined() ? dx + dskip : dx;
}

// The plain fields of a product of the own kernel, y[M, N] = a[M, K] . w[N, taps K]^T, all dense: a 1x1 layer, or with dilation > 0
// the 3x3 layer (padding = dilation) over H x W maps as an implicit GEMM.  The callers add their epilogue.
ucd_conv1x1_desc conv_desc(const at::Tensor& a, const at::Tensor& w, const at::Tensor& y, int64_t M, int64_t N, int64_t K,
                           int64_t H = 0, int64_t W = 0, int64_t dilation = 0) {
  ucd_conv1x1_desc d;
  memset(&d, 0, sizeof(d));
  d.a = a.data_ptr(); d.lda = (int)K; d.w = w.data_ptr(); d.ldw = (int)(dilation > 0 ? 9 * K : K); d.y = y.data_ptr(); d.ldy = (int)N;
  d.M = (int)M; d.N = (int)N; d.K = (int)K; d.out_mode = 0;
  if (dilation > 0) { d.taps = 9; d.H = (int)H; d.W = (int)W; d.dilation = (int)dilation; }
  return d;
}

class ABNTrainNode : public torch::autograd::Function<ABNTrainNode> {
  struct Kept {
    at::Tensor x, y, weight, bias, buf;
    int64_t act = 0, comm = 0, world = 0, stream = 0, param_grad = 0;
    double slope = 0;
    bool has_res = false;
    std::array<at::Tensor*, 5> tensors() { return {&x, &y, &weight, &bias, &buf}; }
    auto scalars() { return std::tie(act, comm, world, stream, param_grad, slope, has_res); }
  };

 public:
  static at::Tensor forward(AutogradContext* ctx, at::Tensor x, at::Tensor weight, at::Tensor bias,
                            c10::optional<at::Tensor> residual_, at::Tensor running_mean, at::Tensor running_var,
                            double momentum, double eps, int64_t act, double slope, int64_t comm, int64_t world,
                            int64_t stream, int64_t param_grad) {
    // param_grad != 0: address of this layer's [d bias | d weight] storage (2*C floats, the parameters' .grad views laid
    // out back to back by ucd_amd.ddp); the backward kernels then write the parameter gradients there themselves and the
    // node reports none - no gradient tensors, no AccumulateGrad adds (212 tiny launches per step)
    TORCH_CHECK(dense_channels_last(x), "ucd abn node: input must be a dense channels-last tensor");
    at::Tensor residual = or_undefined(residual_);
    const bool has_res = residual.defined();
    if (has_res) TORCH_CHECK(dense_channels_last(residual) && residual.sizes() == x.sizes() && residual.scalar_type() == x.scalar_type(),
                             "ucd abn node: residual must match the input");
    const int64_t C = x.size(1), HW = x.size(2) * x.size(3), M = x.size(0) * HW;
    at::Tensor y = at::empty_like(x);   // preserves channels-last
    at::Tensor buf = at::empty({(comm != 0 ? 8 + 2 * world : 6) * C}, x.options().dtype(at::kFloat));
    const size_t ws_bytes = ucd_abn_workspace_bytes((int)M, (int)C);
    abn_batch_forward(comm, world, x, y, residual, M, C, HW, weight, bias, running_mean, running_var, momentum, eps,
                      buf.data_ptr<float>(), act, slope, workspace(x, ws_bytes, stream), ws_bytes, stream);
    const bool needs_y = has_res && (act & UCD_ACT_MASK) != UCD_ACT_IDENTITY;  // the sign of z is not recoverable from x alone
    Kept k{x, needs_y ? y : at::Tensor(), weight, bias, buf, act, comm, world, stream, param_grad, slope, has_res};
    keep(ctx, k);
    return y;
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    Kept k = kept<Kept>(ctx);
    const at::Tensor& x = k.x;
    const int64_t C = x.size(1), HW = x.size(2) * x.size(3), M = x.size(0) * HW;
    at::Tensor dy = grads[0];
    if (dy.scalar_type() != x.scalar_type()) dy = dy.to(x.scalar_type());
    if (!dense_channels_last(dy)) dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
    at::Tensor dx = at::empty_like(x);
    at::Tensor dres = k.has_res ? at::empty_like(x) : at::Tensor();
    const Sums sums(k.comm != 0, reinterpret_cast<float*>(k.param_grad), C, x);
    const size_t ws_bytes = ucd_abn_workspace_bytes((int)M, (int)C);
    abn_batch_backward(k.comm, k.world, x, dy, k.y, dx, dres, M, C, HW, k.buf.data_ptr<float>(), k.weight, k.bias, sums, k.act, k.slope,
                       workspace(x, ws_bytes, k.stream), ws_bytes, k.stream);
    variable_list out = no_grads(&forward);
    out[0] = dx; out[1] = sums.dweight; out[2] = sums.dbias; out[3] = dres;
    return out;
  }
};

// ---- wide 1x1 convolution as a row-matrix GEMM (ucd_amd/blocks.py::_Gemm1x1 is the Python twin) ------------------
// y[M, Co] = rows[M, Ci] . w[Co, Ci]^T through ucd_gemm_bf16 (hipBLASLt, tuned once per shape)
at::Tensor gemm1x1_forward(AutogradContext* ctx, const at::Tensor& rows, const at::Tensor& w4, int64_t stream, bool own_wg,
                           const char* who) {
  TORCH_CHECK(rows.dim() == 2 && rows.is_contiguous() && rows.scalar_type() == at::kBFloat16 && w4.dim() == 4 &&
                  w4.scalar_type() == at::kBFloat16 && w4.size(1) == rows.size(1) && w4.size(2) == 1 && w4.size(3) == 1,
              "ucd ", who, ": rows [M, Ci] bf16 contiguous and weight [Co, Ci, 1, 1] bf16 expected");
  ctx->saved_data["own_wgrad"] = own_wg;
  const int64_t M = rows.size(0), Ci = rows.size(1), Co = w4.size(0);
  at::Tensor y = at::empty({M, Co}, rows.options());
  const size_t wsb = ucd_gemm_workspace_bytes();
  check(ucd_gemm_bf16(0, (int)M, (int)Co, (int)Ci, rows.data_ptr(), (int)Ci, w4.data_ptr(), (int)Ci, y.data_ptr(), (int)Co,
                      workspace(rows, wsb, stream, 1), wsb, 1, (ucd_stream_t)stream),
        "ucd_gemm_bf16");
  ctx->save_for_backward({rows, w4});
  ctx->saved_data["stream"] = stream;
  return y;
}

// (d rows, d w, none, none); dskip: the gradient of the shortcut that Gemm1x1SkipNode hands out, undefined for Gemm1x1Node
variable_list gemm1x1_backward(AutogradContext* ctx, at::Tensor dy, const at::Tensor& dskip) {
  const auto saved = ctx->get_saved_variables();
  const at::Tensor &rows = saved[0], &w4 = saved[1];
  const int64_t stream = ctx->saved_data["stream"].toInt();
  const size_t wsb = ucd_gemm_workspace_bytes();
  void* ws = workspace(rows, wsb, stream, 1);
  at::Tensor dx, dw;
  if (dy.defined()) {
    dy = dy.contiguous();
    if (dy.scalar_type() != at::kBFloat16) dy = dy.to(at::kBFloat16);
  }
  if (ctx->needs_input_grad(0)) dx = library_dgrad(dy, w4, rows, dskip, rows.size(0), ws, wsb, stream);
  if (ctx->needs_input_grad(1) && dy.defined())
    dw = conv_wgrad(dy, rows, w4, 1, 1, ctx->saved_data["own_wgrad"].toBool() ? kWgradOwn : kWgradSplit, kWgradSplit, stream);
  return {dx, dw, at::Tensor(), at::Tensor()};
}

class Gemm1x1Node : public torch::autograd::Function<Gemm1x1Node> {
 public:
  static at::Tensor forward(AutogradContext* ctx, at::Tensor rows, at::Tensor w4, int64_t stream, bool own_wg) {
    return gemm1x1_forward(ctx, rows, w4, stream, own_wg, "gemm1x1 node");
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) { return gemm1x1_backward(ctx, grads[0], at::Tensor()); }
};

at::Tensor gemm1x1(at::Tensor rows, at::Tensor w4, int64_t stream, bool own_wg) { return Gemm1x1Node::apply(rows, w4, stream, own_wg); }

// First 1x1 convolution of an identity-shortcut bottleneck block, together with the shortcut itself: returns (y, rows) so
// that the block input has ONE consumer.  The backward then receives the shortcut's gradient next to dy and folds it
// into the input-gradient GEMM, dx = dskip + dy . w (beta = 1, in place on dskip), instead of autograd adding two
// [M, Ci] tensors afterwards (one 3-pass elementwise kernel per block, 24 blocks).
class Gemm1x1SkipNode : public torch::autograd::Function<Gemm1x1SkipNode> {
 public:
  static variable_list forward(AutogradContext* ctx, at::Tensor rows, at::Tensor w4, int64_t stream, bool own_wg) {
    at::Tensor y = gemm1x1_forward(ctx, rows, w4, stream, own_wg, "gemm1x1 skip node");
    return {y, rows};          // an input returned as an output: autograd hands out an alias with this node as grad_fn
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) { return gemm1x1_backward(ctx, grads[0], grads[1]); }
};

std::vector<at::Tensor> gemm1x1_skip(at::Tensor rows, at::Tensor w4, int64_t stream, bool own_wg) {
  return Gemm1x1SkipNode::apply(rows, w4, stream, own_wg);
}

// ---- stride-1 convolution (3x3 with padding = dilation, or 1x1) whose input gradient runs on the FORWARD solver --------
// dx = conv2d(dy, w.flip(2,3).transpose(0,1), padding, dilation): MIOpen's backward-data solvers are 1.3-2x slower than its
// forward solvers on these problems (tools/dgrad_probe.py, tools/dgrad1x1_probe.py).  ucd_amd/blocks.py::_StrideOneConvFn is
// the Python twin.
class StrideOneConvNode : public torch::autograd::Function<StrideOneConvNode> {
 public:
  // own_fwd / own_dgrad (3x3 only, dense channels-last bf16, 64-aligned channels): the implicit-GEMM kernel
  // (ucd_conv1x1, taps = 9) instead of MIOpen where it is the faster one (the ASPP branches: 303-315 vs 382-390 us)
  static at::Tensor own3x3(const at::Tensor& a, const at::Tensor& w, int64_t d, int64_t stream) {
    const int64_t B = a.size(0), K = a.size(1), H = a.size(2), W = a.size(3), N = w.size(0);
    at::Tensor y = at::empty({B, N, H, W}, a.options().memory_format(at::MemoryFormat::ChannelsLast));
    ucd_conv1x1_desc dsc;
    memset(&dsc, 0, sizeof(dsc));
    dsc.a = a.data_ptr(); dsc.lda = (int)K; dsc.w = w.data_ptr(); dsc.ldw = (int)(9 * K); dsc.y = y.data_ptr(); dsc.ldy = (int)N;
    dsc.M = (int)(B * H * W); dsc.N = (int)N; dsc.K = (int)K; dsc.out_mode = 0;
    dsc.taps = 9; dsc.H = (int)H; dsc.W = (int)W; dsc.dilation = (int)d;
    check(ucd_conv1x1(&dsc, (ucd_stream_t)stream), "ucd_conv1x1");
    return y;
  }

  static at::Tensor forward(AutogradContext* ctx, at::Tensor x, at::Tensor w, int64_t d, c10::optional<at::Tensor> wt_,
                            bool own_fwd, bool own_dgrad, int64_t stream, bool own_wg) {
    const int64_t pad = d * (w.size(2) / 2);
    // wt = w.flip(2, 3).transpose(0, 1) in channels-last order when the caller keeps it cached (ucd_amd/master.py: one
    // batched kernel per optimiser step instead of a flip + copy per layer and step)
    ctx->save_for_backward({x, w, wt_.has_value() ? *wt_ : at::Tensor()});
    ctx->saved_data["d"] = d;
    ctx->saved_data["own_dgrad"] = own_dgrad;
    ctx->saved_data["own_wgrad"] = own_wg;
    ctx->saved_data["stream"] = stream;
    if (own_fwd) return own3x3(x, w, d, stream);
    return at::conv2d(x, w, {}, {1, 1}, {pad, pad}, {d, d}, 1);
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    at::Tensor x = saved[0], w = saved[1], wt = saved[2], dy = grads[0];
    const int64_t d = ctx->saved_data["d"].toInt(), pad = d * (w.size(2) / 2);
    at::Tensor dx, dw;
    if (ctx->needs_input_grad(0)) {
      if (!wt.defined())
        wt = (w.size(2) == 1 ? w.transpose(0, 1) : w.flip({2, 3}).transpose(0, 1)).contiguous(at::MemoryFormat::ChannelsLast);
      if (ctx->saved_data["own_dgrad"].toBool() && dy.scalar_type() == at::kBFloat16) {
        if (!dense_channels_last(dy)) dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
        dx = own3x3(dy, wt, d, ctx->saved_data["stream"].toInt());
      } else {
        dx = at::conv2d(dy, wt, {}, {1, 1}, {pad, pad}, {d, d}, 1);
      }
    }
    if (ctx->needs_input_grad(1))
      dw = conv_wgrad(dy, x, w, d, 1, ctx->saved_data["own_wgrad"].toBool() ? kWgradOwn : kWgradLibrary, kWgradLibrary,
                      ctx->saved_data["stream"].toInt());
    return {dx, dw, at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor()};
  }
};

at::Tensor conv_stride1(at::Tensor x, at::Tensor w, int64_t d, c10::optional<at::Tensor> wt, bool own_fwd, bool own_dgrad,
                        int64_t stream, bool own_wg) {
  return StrideOneConvNode::apply(x, w, d, wt, own_fwd, own_dgrad, stream, own_wg);
}

// ---- 1x1 convolution + training-mode ABN as ONE node ------------------------------------------------------
// forward   z = x . w^T with the statistics of z accumulated in the GEMM's epilogue (ucd_conv1x1 out_mode 2: no statistics
//           pass over z) -> finalize (or the SyncBN exchange) -> y = act(norm(z) [+ residual]); every layer the node takes runs
//           this way (the library products + a statistics pass it once chose between: DESIGN.md section 10)
// backward  ABN backward (d z, d residual, parameter gradients) -> d x = d z . w (+ the shortcut's gradient, beta = 1)
//           -> d w = d z^T . x as batched split-M products
// with_skip: x is also the block's identity shortcut; the node returns (y, alias of x) so that x has one consumer and the
// shortcut's gradient is folded into the input-gradient product (Gemm1x1SkipNode's trick).
// Reference: conv1 -> bn1, conv3 -> bn3 (+ shortcut, activation), proj_conv -> proj_bn of modules/residual.py:57-97.
//
// Backward link between two nodes  A (producer) -> B (consumer)  where A's output feeds B only: B's input-gradient product applies
// A's activation derivative and accumulates A's two backward sums in its epilogue, so A's backward skips its reduction pass
// (ucd_abn_bwd_reduce: two reads of the map).  The protocol is three operations on the link's flag, a 6-word int64 CPU tensor that
// A's forward returns and B receives with the rest of the link:
//   offer (A forward)   a fresh flag and the `partial` the sums will go to: per-tile rows [row tiles][2][N], or - atomic link, round
//                       5 - a zeroed arena slot [replicas][2 N] (SyncBN: twice that, to-be-reduced | local) with its generation;
//   serve (B backward)  B's product takes the epilogue; the flag gets served, the address and version of the dx it writes, and an
//                       atomic slot goes empty -> filled;
//   claim (A backward)  dy must be that very dx, untouched; served is cleared, an atomic slot goes filled -> read.
class LinkFlag {
 public:
  enum State : int64_t { kEmpty = 0, kFilled = 1, kRead = 2 };      // of an atomic link's arena slot
  enum Claim { kNotLinked, kTileRows, kAtomic };

  explicit LinkFlag(const at::Tensor& t) : f_(t.defined() ? t.data_ptr<int64_t>() : nullptr) {
    TORCH_CHECK(!f_ || t.numel() == kWords, "ucd conv+abn node: a backward link's flag has ", (int)kWords, " words");
  }
  explicit operator bool() const { return f_ != nullptr; }
  bool atomic() const { return f_ && f_[kGeneration] != 0; }
  int64_t replicas() const { return f_[kReplicas]; }      // the producer sized the slot: [R][2 C], SyncBN twice

  // (partial, flag) for the output [M, N] of a producer on `stream`
  static std::pair<at::Tensor, at::Tensor> offer(const at::Tensor& x, int64_t M, int64_t N, bool sync, bool stat_atomic, int64_t stream) {
    at::Tensor flag = at::zeros({(int64_t)kWords}, at::TensorOptions().dtype(at::kLong)), partial;
    int64_t gen = 0;
    const int64_t R = ucd_conv1x1_stat_replicas((int)M), floats = (sync ? 2 : 1) * R * 2 * N;
    if (stat_atomic && N % 8 == 0) partial = arena_alloc(x, floats, &gen, stream);
    if (partial.defined()) {
      partial = partial.narrow(0, 0, floats);
      int64_t* f = flag.data_ptr<int64_t>();
      f[kGeneration] = gen;
      f[kReplicas] = R;
    } else {
      partial = at::empty({(int64_t)ucd_conv1x1_row_tiles((int)M), 2, N}, x.options().dtype(at::kFloat));
    }
    return {partial, flag};
  }

  // may a consumer on device `dev` serve the link?  (tile rows: always; atomic: the slot must be of the current generation and empty)
  bool servable(int dev) const {
    if (!atomic()) return true;
    TORCH_CHECK(f_[kState] != kFilled, "ucd conv+abn node: a backward link's accumulator was filled twice (retain_graph replay of the consumer) - "
                                       "run with UCD_STAT_ATOMIC=0");
    return f_[kState] == kEmpty && f_[kGeneration] == arena_gen(dev);
  }

  // The product d, which writes dx [M, C], leaves the two sums in `partial`.  served: the producer's backward may skip its reduction
  // pass - but ONLY for the gradient this product writes.  The address of that tensor is recorded so the producer can tell "dy is
  // exactly the consumer's dx" from "autograd summed several contributions" (a second consumer of the producer's output: the
  // derivative would be applied to a part of dy only), and its version counter because the engine's input buffer may
  // later add a second consumer's gradient INTO that tensor in place - same address - which bumps it.
  void serve(ucd_conv1x1_desc& d, const at::Tensor& partial, const at::Tensor& dx) {
    const int64_t C = d.N;
    d.partial = partial.data_ptr<float>();
    if (atomic()) {
      const int64_t R = replicas();
      d.stat_acc = partial.data_ptr<float>();
      d.stat_rep = (int)R;
      d.stat_acc2 = partial.numel() >= 2 * R * 2 * C ? d.stat_acc + R * 2 * C : nullptr;
      f_[kState] = kFilled;
    }
    f_[kServed] = 1;
    f_[kAddress] = address(dx);
    f_[kVersion] = (int64_t)dx._version();
  }

  // The link's promise (one consumer of y) is checked, not trusted: the incoming gradient must be the very tensor the consumer's
  // input-gradient product wrote.  Anything else (a sum made by the engine, a hook's copy, a stale flag from a backward pass that
  // stopped short of this node) carries a derivative on part of dy only - wrong gradients, silently.
  Claim claim(const at::Tensor& dy, int dev) {
    if (!f_ || f_[kServed] != 1) return kNotLinked;
    const bool same = dy.defined() && address(dy) == f_[kAddress] && (int64_t)dy._version() == f_[kVersion];
    f_[kServed] = 0;
    TORCH_CHECK(same, "ucd conv+abn node: the backward link was served but the gradient that arrived is not the consumer's "
                      "input gradient, or was added to in place since - the linked map has a second consumer (hook, "
                      "ret_intermediate tap, retain_graph replay).  Run with UCD_BWD_LINK=0.");
    if (!atomic()) return kTileRows;
    TORCH_CHECK(f_[kState] == kFilled && f_[kGeneration] == arena_gen(dev),
                "ucd conv+abn node: the statistics arena was reset between a link's consumer and its producer (a training forward "
                "inside a backward pass?) - run with UCD_STAT_ATOMIC=0");
    f_[kState] = kRead;
    return kAtomic;
  }

 private:
  enum Field { kServed, kAddress, kVersion, kGeneration /* of the arena slot; 0: tile rows */, kState, kReplicas, kWords };
  static int64_t address(const at::Tensor& t) { return (int64_t)reinterpret_cast<intptr_t>(t.data_ptr()); }
  int64_t* f_;
};

// The link a node consumes: its producer's z, statistics buffer, bias, partial, flag, activation.
// kChain: A (conv + ABN) -> B (conv + ABN); B's product runs out_mode 3 against A's statistics.
// kBlock: A is the LAST node of a residual block, out = act(norm(z) + shortcut), and B the first convolution of the next,
// identity-shortcut block (with_skip), whose input-gradient product has the shortcut's gradient folded in (accumulate): what it
// computes is d out, so its epilogue (out_mode 4) applies the block activation's derivative (sign of out = B's own input x) and
// accumulates the two sums against x-hat(z).  A then runs reduce-partials + apply on d pre and hands d pre on as the shortcut's
// gradient (no second tensor).  bias and act are unused.
struct Link {
  enum Kind : int64_t { kNone = 0, kChain = 1, kBlock = 3 };
  at::Tensor z, buf, bias, partial, flag;
  int64_t act = 0;
  double slope = 0;
  int64_t kind = kNone;

  // complete, and of a form this consumer (K input channels) can serve?
  bool consumable(bool with_skip, int64_t K) const {
    return z.defined() && buf.defined() && (bias.defined() || kind == kBlock) && partial.defined() && flag.defined() &&
           (kind != kBlock || with_skip) && (!LinkFlag(flag).atomic() || K % 8 == 0);
  }

  // serve: give the input-gradient product d, which writes dx (d out of the producer = the gradient of this node's input `out`),
  // the producer's backward reduction as its epilogue.  alone: no shortcut gradient arrives next to dx; fold: one does and is this
  // product's accumulate operand - a chain link needs the first, a block link either.  False: not served, the producer reduces for
  // itself (also an atomic link whose arena slot is stale).
  bool serve(ucd_conv1x1_desc& d, const at::Tensor& dx, const at::Tensor& out, bool alone, bool fold) const {
    LinkFlag f(flag);
    if (!f || !f.servable((int)out.get_device())) return false;
    if (!(alone || (kind == kBlock && fold))) return false;
    const int64_t C = d.N;
    const float* b = buf.data_ptr<float>();
    d.out_mean = b + 3 * C; d.out_invstd = b + 4 * C;
    d.ldr = (int)C;
    d.out_slope = (float)slope;
    if (kind == kBlock) {
      d.out_mode = 4;
      d.residual = out.data_ptr();
      d.side2 = z.data_ptr(); d.ld2 = (int)C;
      d.out_act = UCD_ACT_LEAKY_RELU;
    } else {
      d.out_mode = 3;
      d.out_scale = b + 5 * C;
      d.out_shift = bias.data_ptr<float>();
      d.residual = z.data_ptr();
      d.out_act = (int)(act & UCD_ACT_MASK);
    }
    f.serve(d, partial, dx);
    return true;
  }
};

class ConvABNTrainNode : public torch::autograd::Function<ConvABNTrainNode> {
  struct Kept {
    at::Tensor x, w4, z, y, weight, bias, buf, wflip;
    Link link;                                // the link consumed (undefined tensors: none)
    at::Tensor my_partial, my_flag;           // the link offered
    int64_t act = 0, comm = 0, world = 0, stream = 0, param_grad = 0, dilation = 0, stride = 1, wgrad_conv = 0;
    double slope = 0;
    bool has_res = false, with_skip = false, own_dgrad = false;
    std::array<at::Tensor*, 15> tensors() {
      return {&x, &w4, &z, &y, &weight, &bias, &buf, &wflip, &link.z, &link.buf, &link.bias, &link.partial, &link.flag, &my_partial,
              &my_flag};
    }
    auto scalars() {
      return std::tie(link.act, link.slope, link.kind, act, comm, world, stream, param_grad, dilation, stride, wgrad_conv, slope, has_res,
                      with_skip, own_dgrad);
    }
  };

 public:
  static variable_list forward(AutogradContext* ctx, at::Tensor x, at::Tensor w4, at::Tensor weight, at::Tensor bias,
                               c10::optional<at::Tensor> residual_, at::Tensor running_mean, at::Tensor running_var,
                               double momentum, double eps, int64_t act, double slope, int64_t comm, int64_t world,
                               int64_t stream, int64_t param_grad, bool with_skip, int64_t dilation,
                               c10::optional<at::Tensor> wflip_, bool own_dgrad, int64_t wgrad_conv, bool make_link,
                               c10::optional<at::Tensor> lk_z_, c10::optional<at::Tensor> lk_buf_,
                               c10::optional<at::Tensor> lk_bias_, c10::optional<at::Tensor> lk_partial_,
                               c10::optional<at::Tensor> lk_flag_, int64_t lk_act, double lk_slope, int64_t lk_kind,
                               int64_t stride, bool stat_atomic) {
    // stat_atomic (round 5): statistics and link sums through fp32 atomics into arena slots, finalised in the prologue of the apply
    // passes (no tile_stats_reduce / reduce_bands launches); off: the deterministic per-tile rows + second-stage kernels
    // stride > 1: the strided layers of the first block of a stage (conv2 3x3 stride 2 with padding = dilation, proj_conv 1x1
    // stride 2): forward and weight gradient on the own kernels (the strided row gather / implicit GEMM, the strided weight-gradient
    // form), input gradient through the library's backward-data solver; no shortcut fold, no link consumed (it may still MAKE one).
    // make_link: offer a backward link (LinkFlag above) - also return (z, buf, partial, flag).  lk_*: the Link consumed; under
    // SyncBN its producer all-reduces the sums.
    // dilation = 0: 1x1 convolution; dilation >= 1: 3x3, stride 1, padding = dilation (implicit GEMM, taps = 9), weight in
    // channels-last memory order; wflip = w.flip(2, 3).transpose(0, 1) (channels-last; for a 1x1 layer the transposed
    // weight [Ci, Co]) for the input gradient through the own kernel (own_dgrad); wgrad_conv: the WgradRoute of the weight gradient
    // (conv_wgrad; a layer the own kernel does not take falls back to the split products, which a 3x3 / strided layer takes on MIOpen)
    Link link{or_undefined(lk_z_), or_undefined(lk_buf_), or_undefined(lk_bias_), or_undefined(lk_partial_), or_undefined(lk_flag_),
              lk_act, lk_slope, lk_kind};
    TORCH_CHECK(dense_channels_last(x) && x.scalar_type() == at::kBFloat16, "ucd conv+abn node: x must be dense channels-last bf16");
    const bool conv3 = dilation > 0;
    TORCH_CHECK(w4.dim() == 4 && w4.scalar_type() == at::kBFloat16 && w4.size(1) == x.size(1) &&
                    (conv3 ? (w4.size(2) == 3 && w4.size(3) == 3 && w4.is_contiguous(at::MemoryFormat::ChannelsLast))
                           : (w4.size(2) == 1 && w4.size(3) == 1 && w4.is_contiguous())),
                "ucd conv+abn node: weight [Co, Ci, 1, 1] (contiguous) or [Co, Ci, 3, 3] (channels-last) bf16 expected");
    TORCH_CHECK(!(conv3 && with_skip), "ucd conv+abn node: the shortcut fold belongs to the 1x1 layers");
    at::Tensor residual = or_undefined(residual_);
    const bool has_res = residual.defined();
    const int64_t B = x.size(0), K = x.size(1), H = x.size(2), W = x.size(3), N = w4.size(0);
    if (stride < 1) stride = 1;
    TORCH_CHECK(stride == 1 || (!with_skip && !lk_z_.has_value()), "ucd conv+abn node: a strided layer takes no shortcut fold / link");
    const int64_t OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
    const int64_t HW = OH * OW, M = B * HW;                     // rows of the OUTPUT map
    if (has_res)
      TORCH_CHECK(dense_channels_last(residual) && residual.size(1) == N && residual.size(0) == B && residual.size(2) == OH &&
                      residual.size(3) == OW && residual.scalar_type() == at::kBFloat16,
                  "ucd conv+abn node: residual must match the output");
    const bool sync = comm != 0;
    auto opts = x.options().memory_format(at::MemoryFormat::ChannelsLast);
    at::Tensor z = at::empty({B, N, OH, OW}, opts), y = at::empty({B, N, OH, OW}, opts);
    at::Tensor buf = at::empty({(sync ? 8 + 2 * world : 6) * N}, x.options().dtype(at::kFloat));
    float* b = buf.data_ptr<float>();
    const size_t ws_bytes = ucd_abn_workspace_bytes((int)M, (int)N);
    const void* resp = has_res ? residual.data_ptr() : nullptr;
    size_t need = ucd_conv1x1_stats_partial_bytes((int)M, (int)N);
    float* partial = (float*)workspace(x, need > ws_bytes ? need : ws_bytes, stream);
    ucd_conv1x1_desc d = conv_desc(x, w4, z, M, N, K, H, W, dilation);
    d.out_mode = 2; d.partial = partial;
    if (stride > 1) { d.H = (int)H; d.W = (int)W; d.stride = (int)stride; }
    int64_t gen = 0;
    const int64_t R = ucd_conv1x1_stat_replicas((int)M);
    at::Tensor acc = (stat_atomic && N % 8 == 0) ? arena_alloc(x, R * 2 * N, &gen, stream) : at::Tensor();
    if (acc.defined()) {
      // sums about the running mean (equal on every rank), straight into the layer's accumulator; SyncBN: one all-reduce of the
      // 2 N raw sums (they are additive about a common shift) instead of gather + Chan combination
      d.stat_acc = acc.data_ptr<float>();
      d.stat_rep = (int)R;
      d.stat_shift = running_mean.data_ptr<float>();
      d.partial = b + 2 * N;                                   // the snapshot of the shift
      check(ucd_conv1x1(&d, (ucd_stream_t)stream), "ucd_conv1x1");
      if (sync) check(ucd_comm_all_reduce_sum((ucd_comm_t)comm, d.stat_acc, (size_t)(R * 2 * N), (ucd_stream_t)stream), "ucd_comm_all_reduce_sum");
      check(ucd_abn_apply_stats(z.data_ptr(), (int)N, y.data_ptr(), (int)N, resp, has_res ? (int)N : 0, (int)M, (int)N, d.stat_acc,
                                (int)R, b + 2 * N, (float)M * (sync ? (float)world : 1.f), fptr(weight), fptr(bias),
                                running_mean.data_ptr<float>(), running_var.data_ptr<float>(), (float)momentum, (float)eps, b + 3 * N,
                                b + 4 * N, b + 5 * N, (int)act, (float)slope, (ucd_stream_t)stream),
            "ucd_abn_apply_stats");
    } else {
      check(ucd_conv1x1(&d, (ucd_stream_t)stream), "ucd_conv1x1");
      if (!sync) {
        check(ucd_conv1x1_stats_finalize(partial, (int)M, (int)N, fptr(weight), running_mean.data_ptr<float>(),
                                         running_var.data_ptr<float>(), (float)momentum, (float)eps, b, nullptr, (int)act,
                                         (ucd_stream_t)stream),
              "ucd_conv1x1_stats_finalize");
        check(ucd_abn_apply(z.data_ptr(), (int)N, y.data_ptr(), (int)N, resp, has_res ? (int)N : 0, UCD_BF16, (int)M, (int)N, nullptr,
                            (int)HW, b + 3 * N, b + 5 * N, fptr(bias), (int)act, (float)slope, (ucd_stream_t)stream),
              "ucd_abn_apply");
      } else {
        float *pack = b + 6 * N, *gathered = b + 8 * N;
        check(ucd_conv1x1_stats_finalize(partial, (int)M, (int)N, nullptr, nullptr, nullptr, (float)momentum, (float)eps, b, pack, 0,
                                         (ucd_stream_t)stream),
              "ucd_conv1x1_stats_finalize");
        check(ucd_comm_all_gather((ucd_comm_t)comm, pack, gathered, (size_t)2 * N, (ucd_stream_t)stream), "ucd_comm_all_gather");
        check(ucd_abn_sync_forward(z.data_ptr(), (int)N, y.data_ptr(), (int)N, resp, has_res ? (int)N : 0, UCD_BF16, (int)M, (int)N,
                                   nullptr, (int)HW, gathered, (int)world, fptr(weight), fptr(bias), running_mean.data_ptr<float>(),
                                   running_var.data_ptr<float>(), (float)momentum, (float)eps, b, (int)act, (float)slope,
                                   (ucd_stream_t)stream),
              "ucd_abn_sync_forward");
      }
    }
    const bool needs_y = has_res && (act & UCD_ACT_MASK) != UCD_ACT_IDENTITY;
    if (!link.consumable(with_skip, K)) link = Link();
    // a link needs leaky_relu / identity (the fused epilogues' activations); with a residual it is the block link, whose
    // consumer reads the sign from y - so y must be among the saved tensors (needs_y: leaky_relu with a residual)
    make_link = make_link && bias.defined() && (act & UCD_ACT_MASK) != UCD_ACT_ELU && (!has_res || needs_y);
    at::Tensor my_partial, my_flag;
    if (make_link) std::tie(my_partial, my_flag) = LinkFlag::offer(x, M, N, sync, stat_atomic, stream);
    Kept k{x, w4, z, needs_y ? y : at::Tensor(), weight, bias, buf, or_undefined(wflip_), link, my_partial, my_flag, act, comm, world,
           stream, param_grad, dilation, stride, wgrad_conv, slope, has_res, with_skip, own_dgrad};
    keep(ctx, k);
    variable_list out = {y};
    if (with_skip) out.push_back(x);
    if (make_link) {   // outputs: y, [x], z, buf, partial, flag
      // no zero-filled stand-ins for the gradients of the link tensors (the engine would launch a fill per output and step)
      ctx->set_materialize_grads(false);
      ctx->mark_non_differentiable({z, buf, my_partial, my_flag});
      out.insert(out.end(), {z, buf, my_partial, my_flag});
    }
    return out;
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    Kept k = kept<Kept>(ctx);
    const at::Tensor &x = k.x, &w4 = k.w4, &z = k.z;
    const int64_t dilation = k.dilation, stride = k.stride, stream = k.stream;
    const bool conv3 = dilation > 0, sync = k.comm != 0;
    float* param_grad = reinterpret_cast<float*>(k.param_grad);
    const int64_t B = x.size(0), K = x.size(1), H = x.size(2), W = x.size(3), N = w4.size(0);
    const int64_t HW = z.size(2) * z.size(3), M = B * HW;       // rows of the output map (smaller than x's when strided)
    at::Tensor dy = grads[0];
    at::Tensor dskip = k.with_skip ? grads[1] : at::Tensor();
    at::Tensor dx, dw, dweight, dbias, dres;
    at::Tensor dz;   // gradient w.r.t. the convolution output z
    LinkFlag my_flag(k.my_flag);
    const LinkFlag::Claim claim = my_flag.claim(dy, (int)x.get_device());
    if (dy.defined()) {
      if (dy.scalar_type() != at::kBFloat16) dy = dy.to(at::kBFloat16);
      if (!dense_channels_last(dy)) dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
      dz = at::empty_like(z);
      if (k.has_res && claim == LinkFlag::kNotLinked) dres = at::empty_like(z);
      Sums sums(sync, param_grad, N, x);
      const float* b = k.buf.data_ptr<float>();
      const float *mean = b + 3 * N, *invstd = b + 4 * N, *scale = b + 5 * N;
      const size_t ws_bytes = ucd_abn_workspace_bytes((int)M, (int)N);
      void* ws = workspace(x, ws_bytes, stream);
      const float count = (float)M * (sync ? (float)k.world : 1.f);
      const int norm_only = (int)(UCD_ACT_IDENTITY | (k.act & UCD_NORM_ABS_GAMMA));   // a served link: the activation is done
      if (claim == LinkFlag::kAtomic) {
        // atomic link: the consumer's product added the two sums into this layer's arena slot; the apply pass finalises them in its
        // prologue and writes the parameter gradients (SyncBN: the first half is all-reduced, the second stays this rank's)
        const int64_t R = my_flag.replicas();
        float* global = k.my_partial.data_ptr<float>();
        float* local = sync ? global + R * 2 * N : global;
        if (sync) check(ucd_comm_all_reduce_sum((ucd_comm_t)k.comm, global, (size_t)(R * 2 * N), (ucd_stream_t)stream), "ucd_comm_all_reduce_sum");
        sums = Sums(false, param_grad, N, x);      // only the parameter gradients need a home
        check(ucd_abn_bwd_apply_raw(z.data_ptr(), (int)N, dy.data_ptr(), (int)N, nullptr, 0, dz.data_ptr(), (int)N, nullptr, 0, (int)M,
                                    (int)N, mean, invstd, scale, fptr(k.bias), fptr(k.weight), global, local, (int)R, sums.local, count,
                                    norm_only, 0.f, (ucd_stream_t)stream),
              "ucd_abn_bwd_apply_raw");
      } else if (claim == LinkFlag::kTileRows) {
        // the consumer's input-gradient product already applied this layer's activation derivative and left the two sums
        // as per-tile partials: combine them (fixed order) and go straight to the apply pass
        // single process: the sums are the parameter gradients and the constants of the apply pass.  SyncBN: the apply
        // pass needs the sums over all ranks (all-reduce, like ucd_abn_sync_backward_comm), the parameter gradients stay
        // this rank's (the DDP wrapper averages them).
        check(ucd_abn_reduce_partials(k.my_partial.data_ptr<float>(), ucd_conv1x1_row_tiles((int)M), (int)N, sums.global,
                                      sync ? sums.local : nullptr, fptr(k.weight), (int)(k.act & UCD_NORM_ABS_GAMMA), (ucd_stream_t)stream),
              "ucd_abn_reduce_partials");
        if (sync) check(ucd_comm_all_reduce_sum((ucd_comm_t)k.comm, sums.global, (size_t)2 * N, (ucd_stream_t)stream), "ucd_comm_all_reduce_sum");
        check(ucd_abn_bwd_apply(z.data_ptr(), (int)N, dy.data_ptr(), (int)N, nullptr, 0, dz.data_ptr(), (int)N, nullptr, 0, UCD_BF16,
                                (int)M, (int)N, nullptr, (int)HW, mean, invstd, scale, fptr(k.bias), fptr(k.weight), sums.global, count, 0,
                                norm_only, 0.f, (ucd_stream_t)stream),
              "ucd_abn_bwd_apply");
      } else {
        abn_batch_backward(k.comm, k.world, z, dy, k.y, dz, dres, M, N, HW, b, k.weight, k.bias, sums, k.act, k.slope, ws, ws_bytes, stream);
      }
      // block link: dy already IS d pre = d out * act'(out); the shortcut's gradient is that same tensor (no copy, no write)
      if (k.has_res && claim != LinkFlag::kNotLinked) dres = dy;
      dbias = sums.dbias;
      dweight = sums.dweight;
    }
    if (stride > 1) {
      const int64_t pad = conv3 ? dilation : 0, dil = conv3 ? dilation : 1;
      if (ctx->needs_input_grad(0) && dz.defined())
        dx = std::get<0>(at::convolution_backward(dz, x, w4, c10::nullopt, {stride, stride}, {pad, pad}, {dil, dil}, false, {0, 0}, 1,
                                                  {true, false, false}));
    } else if (conv3) {
      // 3x3: input gradient = the same convolution on the flipped + transposed weight (own implicit GEMM, or MIOpen's
      // FORWARD solver when the cached weight is missing / the map is too small to fill the chip)
      if (ctx->needs_input_grad(0) && dz.defined()) {
        at::Tensor wflip = k.wflip.defined() ? k.wflip : w4.flip({2, 3}).transpose(0, 1).contiguous(at::MemoryFormat::ChannelsLast);
        if (k.own_dgrad) {
          dx = at::empty_like(x);
          ucd_conv1x1_desc d = conv_desc(dz, wflip, dx, M, K, N, H, W, dilation);
          k.link.serve(d, dx, x, true, false);
          check(ucd_conv1x1(&d, (ucd_stream_t)stream), "ucd_conv1x1");
        } else {
          dx = at::conv2d(dz, wflip, {}, {1, 1}, {dilation, dilation}, {dilation, dilation}, 1);
        }
      }
    } else if (ctx->needs_input_grad(0)) {
      const size_t wsb = ucd_gemm_workspace_bytes();
      void* gws = workspace(x, wsb, stream, 1);
      if (k.own_dgrad && dz.defined() && k.wflip.defined()) {
        // narrow / short-K layers: d x = d z . w through the own kernel on the cached transposed weight [Ci, Co]; the
        // shortcut's gradient is the accumulate operand (no separate add)
        const bool fold = dskip.defined() && dskip.scalar_type() == at::kBFloat16;
        if (fold && !dense_channels_last(dskip)) dskip = dskip.contiguous(at::MemoryFormat::ChannelsLast);
        dx = fold ? dskip : at::empty_like(x);
        ucd_conv1x1_desc d = conv_desc(dz, k.wflip, dx, M, K, N);
        d.accumulate = fold ? 1 : 0;
        k.link.serve(d, dx, x, !dskip.defined(), fold);
        check(ucd_conv1x1(&d, (ucd_stream_t)stream), "ucd_conv1x1");
        if (!fold && dskip.defined()) dx = dx + dskip;
      } else {
        dx = library_dgrad(dz, w4, x, dskip, M, gws, wsb, stream);
      }
    }
    if (ctx->needs_input_grad(1) && dz.defined())
      dw = conv_wgrad(dz, x, w4, conv3 ? dilation : 1, stride, k.wgrad_conv, kWgradSplit, stream);
    variable_list out = no_grads(&forward);
    out[0] = dx; out[1] = dw; out[2] = dweight; out[3] = dbias; out[4] = dres;
    return out;
  }
};

// the link as Python hands it over (ucd_amd/blocks.py Link): the fields of Link above in their order, bias None on a block link
using PyLink = std::tuple<at::Tensor, at::Tensor, c10::optional<at::Tensor>, at::Tensor, at::Tensor, int64_t, double, int64_t>;

std::vector<at::Tensor> conv_abn_train(at::Tensor x, at::Tensor w4, at::Tensor weight, at::Tensor bias,
                                       c10::optional<at::Tensor> residual, at::Tensor running_mean, at::Tensor running_var,
                                       double momentum, double eps, int64_t act, double slope, int64_t comm, int64_t world,
                                       int64_t stream, int64_t param_grad, bool with_skip, int64_t dilation,
                                       c10::optional<at::Tensor> wflip, bool own_dgrad, int64_t wgrad_conv, bool make_link,
                                       c10::optional<PyLink> link, int64_t stride, bool stat_atomic) {
  // the link's tensors stay arguments of the node (they keep their edges in the graph, the producer's bias among them)
  c10::optional<at::Tensor> lk_z, lk_buf, lk_bias, lk_partial, lk_flag;
  int64_t lk_act = 0, lk_kind = Link::kNone;
  double lk_slope = 0.0;
  if (link) std::tie(lk_z, lk_buf, lk_bias, lk_partial, lk_flag, lk_act, lk_slope, lk_kind) = *link;
  return ConvABNTrainNode::apply(x, w4, weight, bias, residual, running_mean, running_var, momentum, eps, act, slope, comm, world,
                                 stream, param_grad, with_skip, dilation, wflip, own_dgrad, wgrad_conv, make_link, lk_z,
                                 lk_buf, lk_bias, lk_partial, lk_flag, lk_act, lk_slope, lk_kind, stride, stat_atomic);
}

at::Tensor abn_train(at::Tensor x, at::Tensor weight, at::Tensor bias, c10::optional<at::Tensor> residual,
                     at::Tensor running_mean, at::Tensor running_var, double momentum, double eps, int64_t act, double slope,
                     int64_t comm, int64_t world, int64_t stream, int64_t param_grad) {
  return ABNTrainNode::apply(x, weight, bias, residual, running_mean, running_var, momentum, eps, act, slope, comm, world, stream,
                             param_grad);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "C++ autograd node of the training-mode ABN layer over libucd_hip.so";
  m.def("poison_workspaces", &poison_workspaces);
  m.def("pass_flushes", []() { return g_pass_flushes; }, "number of end-of-pass flushes the nodes' engine callbacks have run (test hook)");
  m.def("wgrad_calls", []() {
    std::lock_guard<std::mutex> lock(g_mu);
    return std::make_pair(g_wgrad_calls[0], g_wgrad_calls[1]);
  }, "(own weight-gradient calls of the nodes, those issued deferred / for the side stream) so far (test hook)");
  m.def("wgrad_register_working", &wgrad_register_working,
        "weights whose only post-accumulate-grad hook is the gradient-bucket wrapper's (ucd_amd.master.Bf16Weights working copies)");
  m.def("wgrad_side_release", &wgrad_side_release, py::arg("stream") = py::none(),
        "drop the operands held for the side work of a stream (None: every stream) - only after its join succeeded");
  m.def("stat_arena_reset", &stat_arena_reset, "zero the used part of the statistics arena of a device and start a new generation");
  m.def("abn_train", &abn_train, "y = act(BN_batch(x) [+ residual]) with autograd in C++");
  m.def("dense_channels_last", &dense_channels_last);
  m.def("conv_stride1", &conv_stride1, "stride-1 conv (3x3 pad=dilation, or 1x1) with the input gradient on the forward solver");
  m.def("gemm1x1_skip", &gemm1x1_skip, "(rows x w^T, rows): first 1x1 conv of an identity-shortcut block with the shortcut");
  m.def("gemm1x1", &gemm1x1, "rows[M, Ci] x w[Co, Ci, 1, 1]^T with autograd in C++ (call ucd_gemm_load first)");
  m.def("conv_abn_train", &conv_abn_train, "1x1 convolution + training-mode ABN (+ residual) as one node, statistics in the GEMM epilogue");
}
