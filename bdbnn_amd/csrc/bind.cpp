// Python bindings for the bdbnn_amd gfx950 kernels (pack / xnor conv /
// kurtosis / weight-KD / fused optimizers).  Pure HIP underneath — no CUDA
// compatibility layer; this file only marshals ATen tensors.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <atomic>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "api.h"

namespace {

hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

bool is_bf16(const at::Tensor& t) { return t.scalar_type() == at::kBFloat16; }

// Argument check of the elementwise kernels that pick `bf16 ? bf16 : float`
// from the tensor: any other dtype would be read as float, past the end
// of an fp16 buffer.  vec8_c: the tensor is also indexed by chan_map8
// (csrc/vec8.h), one thread per 8 channels, which needs a 4-D tensor with
// C a power of two in [8, 1024] (C < 8 divides by zero threads per row).
void check_vec8(const at::Tensor& t, bool vec8_c, const char* name,
                const char* who) {
  TORCH_CHECK(t.is_cuda() && (t.scalar_type() == at::kBFloat16 ||
                              t.scalar_type() == at::kFloat),
              who, ": ", name, " must be a bf16 or fp32 CUDA tensor");
  if (vec8_c) {
    TORCH_CHECK(t.dim() == 4, who, ": ", name, " must be 4-D (N,C,H,W)");
    int64_t C = t.size(1);
    TORCH_CHECK(C >= 8 && C <= 1024 && (C & (C - 1)) == 0, who,
                ": C must be a power of two, 8 <= C <= 1024");
  }
}

// Build the multi-tensor block schedule (block -> tensor, offset) on the
// device; callers pass BDBNN_CHUNK_ELEMS, what one block covers.
struct Schedule {
  at::Tensor bt, bo;   // int32 / int64 device tensors
  int n_blocks;
};

Schedule build_schedule_uncached(const std::vector<at::Tensor>& ts,
                                 int64_t chunk_elems, const at::Device& dev) {
  std::vector<int> bt;
  std::vector<int64_t> bo;
  for (size_t l = 0; l < ts.size(); ++l) {
    int64_t n = ts[l].numel();
    for (int64_t off = 0; off < n; off += chunk_elems) {
      bt.push_back((int)l);
      bo.push_back(off);
    }
  }
  Schedule s;
  s.n_blocks = (int)bt.size();
  s.bt = at::from_blob(bt.data(), {(int64_t)bt.size()},
                       at::TensorOptions().dtype(at::kInt))
             .to(dev, /*non_blocking=*/false);
  s.bo = at::from_blob(bo.data(), {(int64_t)bo.size()},
                       at::TensorOptions().dtype(at::kLong))
             .to(dev, /*non_blocking=*/false);
  return s;
}

// The tensor sets of the fused calls are stable across steps (the same
// parameters every iteration): cache the device-side schedules keyed by
// the size list + chunking so the per-step host->device copies go away.
Schedule build_schedule(const std::vector<at::Tensor>& ts,
                        int64_t chunk_elems, const at::Device& dev) {
  static std::unordered_map<std::string, Schedule> cache;
  std::string key;
  key.reserve(ts.size() * 9 + 16);
  key += std::to_string(chunk_elems);
  key += '/';
  key += std::to_string(dev.index());
  for (auto& t : ts) {
    key += ':';
    key += std::to_string(t.numel());
  }
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  if (cache.size() > 256) cache.clear();  // bound memory; rebuilt on demand
  auto s = build_schedule_uncached(ts, chunk_elems, dev);
  cache.emplace(std::move(key), s);
  return s;
}

TensorListArg make_meta(const std::vector<at::Tensor>& ts) {
  TORCH_CHECK((int)ts.size() <= BDBNN_MAX_TENSORS,
              "too many tensors for one fused call");
  TensorListArg a;
  a.n = (int)ts.size();
  for (size_t i = 0; i < ts.size(); ++i) {
    // dense layout in ANY memory format: the kernels are elementwise /
    // permutation-invariant over physical memory
    TORCH_CHECK((ts[i].is_contiguous() ||
                 ts[i].is_contiguous(at::MemoryFormat::ChannelsLast)) &&
                    ts[i].scalar_type() == at::kFloat,
                "fused multi-tensor ops need dense fp32");
    a.ptr[i] = ts[i].data_ptr<float>();
    a.numel[i] = ts[i].numel();
  }
  return a;
}

// Two dense tensors whose element i in physical memory is the same logical
// element: equal strides, or both dense in the same memory format (size-1
// dimensions leave the strides themselves ambiguous).
bool same_layout(const at::Tensor& a, const at::Tensor& b) {
  if (a.strides() == b.strides()) return true;
  if (a.is_contiguous() && b.is_contiguous()) return true;
  return a.is_contiguous(at::MemoryFormat::ChannelsLast) &&
         b.is_contiguous(at::MemoryFormat::ChannelsLast);
}

// A further list of a fused call.  The kernels index it by the leading
// list's tensor number and element count and pair the elements over
// physical memory, so it must pair up with `lead_ts` (the leading list,
// whose make_meta is `lead`) one to one, in size and in layout.
PtrList make_ptrs(const std::vector<at::Tensor>& ts,
                  const TensorListArg& lead,
                  const std::vector<at::Tensor>& lead_ts) {
  TORCH_CHECK((int)ts.size() == lead.n && (int)lead_ts.size() == lead.n,
              "fused multi-tensor ops need lists of equal length");
  PtrList p;
  for (size_t i = 0; i < ts.size(); ++i) {
    TORCH_CHECK(ts[i].is_cuda() && ts[i].scalar_type() == at::kFloat &&
                    (ts[i].is_contiguous() ||
                     ts[i].is_contiguous(at::MemoryFormat::ChannelsLast)) &&
                    ts[i].numel() == lead.numel[i],
                "fused multi-tensor ops need dense fp32 CUDA tensors sized "
                "like the leading list's");
    TORCH_CHECK(same_layout(ts[i], lead_ts[i]),
                "fused multi-tensor ops pair elements over physical memory: "
                "tensor ", i, " has strides ", ts[i].strides(),
                " against the leading list's ", lead_ts[i].strides());
    p.ptr[i] = ts[i].data_ptr<float>();
  }
  return p;
}

// the logit dtypes loss.hip has kernels for; anything else would be read
// as fp32 (ops/losses.py routes other dtypes to the torch formulas)
void check_logits(const at::Tensor& s, const char* who) {
  TORCH_CHECK(s.is_cuda() && s.dim() == 2 &&
                  (s.scalar_type() == at::kFloat ||
                   s.scalar_type() == at::kBFloat16),
              who, ": logits must be a (B,C) fp32 or bf16 CUDA tensor");
}

// fp32 contiguous copy of a per-channel tensor (a no-op for fp32 [C])
at::Tensor chan_f32(const at::Tensor& t) {
  return t.contiguous().to(at::kFloat);
}

// Optional per-channel tensor as the kernels take it: `hold` keeps the
// fp32 copy alive until the launch is queued; nullptr when absent.
const float* opt_chan_ptr(const c10::optional<at::Tensor>& t,
                          at::Tensor& hold) {
  if (!t.has_value()) return nullptr;
  hold = chan_f32(*t);
  return hold.data_ptr<float>();
}

// Optional skip tensor in xc's dtype, channels_last; same holder rule.
const void* opt_skip_ptr(const c10::optional<at::Tensor>& skip,
                         const at::Tensor& xc, at::Tensor& hold) {
  if (!skip.has_value()) return nullptr;
  hold = skip->to(xc.scalar_type())
             .contiguous(at::MemoryFormat::ChannelsLast);
  return hold.data_ptr();
}

// a per-channel tensor the kernels read or write through float* as it is
bool is_f32_chan(const at::Tensor& t, int64_t C) {
  return t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous() &&
         t.numel() == C;
}

// Training statistics of the fused BN entry points: {mean, invstd} of xc
// (channels_last, C channels) from the pre-accumulated sums (possibly
// [nslice][C] partials of a producing conv's epilogue; finalize folds
// them) or from a bn_stats pass; updates the running stats when given.
std::pair<at::Tensor, at::Tensor> bn_train_stats(
    const at::Tensor& xc, int C, const c10::optional<at::Tensor>& pre_s1,
    const c10::optional<at::Tensor>& pre_s2,
    const c10::optional<at::Tensor>& running_mean,
    const c10::optional<at::Tensor>& running_var, double momentum,
    double eps, const char* who) {
  TORCH_CHECK(pre_s1.has_value() == pre_s2.has_value(), who,
              ": pre_s1 and pre_s2 go together");
  TORCH_CHECK(running_mean.has_value() == running_var.has_value(), who,
              ": running_mean and running_var go together");
  TORCH_CHECK(!running_mean.has_value() ||
                  (is_f32_chan(*running_mean, C) &&
                   is_f32_chan(*running_var, C)),
              who, ": running stats must be contiguous fp32 [C]");
  int64_t n = xc.numel();
  auto fopt = xc.options().dtype(at::kFloat);
  at::Tensor s1, s2;
  int nslice = 32;
  if (pre_s1.has_value()) {
    s1 = pre_s1->contiguous();
    s2 = pre_s2->contiguous();
    TORCH_CHECK(s1.is_cuda() && s2.is_cuda() &&
                    s1.scalar_type() == at::kFloat &&
                    s2.scalar_type() == at::kFloat &&
                    s1.numel() == s2.numel(),
                who, ": stats must be matching fp32 CUDA tensors");
    nslice = (int)(s1.numel() / C);
    TORCH_CHECK(nslice >= 1 && (int64_t)nslice * C == s1.numel(), who,
                ": stats shape mismatch");
  } else {
    s1 = at::empty({32, C}, fopt);   // sliced partials (finalize folds)
    s2 = at::empty({32, C}, fopt);
    bdbnn_bn_stats(xc.data_ptr(), s1.data_ptr<float>(),
                   s2.data_ptr<float>(), n, C, is_bf16(xc), cur_stream());
  }
  auto mean = at::empty({C}, fopt);
  auto invstd = at::empty({C}, fopt);
  bool run = running_mean.has_value();
  bdbnn_bn_finalize(s1.data_ptr<float>(), s2.data_ptr<float>(),
                    mean.data_ptr<float>(), invstd.data_ptr<float>(),
                    run ? running_mean->data_ptr<float>() : nullptr,
                    run ? running_var->data_ptr<float>() : nullptr, C,
                    (float)(n / C), (float)momentum, (float)eps, nslice,
                    cur_stream());
  return {mean, invstd};
}

}  // namespace

// ---------------- pack / quantizer ----------------

at::Tensor sign_pack_nhwc(const at::Tensor& x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4, "sign_pack: 4-D CUDA tensor");
  check_vec8(x, false, "x", "sign_pack");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "sign_pack: channels_last input required");
  int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  int CW = (int)((C + 31) / 32);
  auto out = at::empty({N, H, W, CW},
                       x.options().dtype(at::kInt));
  bdbnn_sign_pack(x.data_ptr(), (uint32_t*)out.data_ptr<int>(),
                  N * H * W, (int)C, CW, is_bf16(x), cur_stream());
  return out;
}

std::vector<at::Tensor> weight_pack(const at::Tensor& w) {
  TORCH_CHECK(w.is_cuda() && w.dim() == 4, "weight_pack: 4-D CUDA tensor");
  auto wf = w.contiguous().to(at::kFloat);
  int K = (int)wf.size(0), C = (int)wf.size(1);
  int KH = (int)wf.size(2), KW = (int)wf.size(3);
  int CW = (C + 31) / 32;
  auto wp = at::empty({K, KH, KW, CW}, wf.options().dtype(at::kInt));
  auto alpha = at::empty({K}, wf.options());
  auto stab = at::empty({K, KH * KW}, wf.options());
  bdbnn_weight_pack(wf.data_ptr<float>(), (uint32_t*)wp.data_ptr<int>(),
                    alpha.data_ptr<float>(), stab.data_ptr<float>(), K, C,
                    KH, KW, CW, cur_stream());
  return {wp, alpha, stab};
}

at::Tensor binsign_decode(const at::Tensor& x, bool out_bf16) {
  check_vec8(x, false, "x", "binsign_decode");
  TORCH_CHECK(x.numel() % 8 == 0, "binsign_decode: numel % 8 == 0");
  auto fmt = x.dim() == 4 ? at::MemoryFormat::ChannelsLast
                          : at::MemoryFormat::Contiguous;
  auto xc = x.contiguous(fmt);
  auto out = at::empty_like(xc, xc.options().dtype(
      out_bf16 ? at::kBFloat16 : at::kFloat), fmt);
  bdbnn_binsign_decode(xc.data_ptr(), out.data_ptr(), xc.numel(),
                       is_bf16(xc), out_bf16, cur_stream());
  return out;
}

at::Tensor ste_mask_mul(const at::Tensor& g, const at::Tensor& x, int mode,
                        double t, double k) {
  TORCH_CHECK(g.is_cuda() && x.is_cuda() && g.numel() == x.numel(),
              "ste_mask_mul: matching CUDA tensors");
  check_vec8(g, false, "g", "ste_mask_mul");
  check_vec8(x, false, "x", "ste_mask_mul");
  TORCH_CHECK(x.numel() % 8 == 0, "ste_mask_mul: numel % 8 == 0");
  auto fmt = x.dim() == 4 ? at::MemoryFormat::ChannelsLast
                          : at::MemoryFormat::Contiguous;
  auto xc = x.contiguous(fmt);
  auto gc = g.contiguous(fmt);
  auto out = at::empty_like(xc, xc.options(), fmt);
  bdbnn_ste_mask_mul(gc.data_ptr(), xc.data_ptr(), out.data_ptr(),
                     xc.numel(), is_bf16(gc), is_bf16(xc), mode, (float)t,
                     (float)k, cur_stream());
  return out;
}

// ---------------- packed-bit fast path ----------------

std::vector<at::Tensor> sign_mask_pack_nhwc(const at::Tensor& x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4, "sign_mask_pack: 4-D CUDA tensor");
  check_vec8(x, false, "x", "sign_mask_pack");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "sign_mask_pack: channels_last input required");
  int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  int CW = (int)((C + 31) / 32);
  auto sp = at::empty({N, H, W, CW}, x.options().dtype(at::kInt));
  auto mp = at::empty({N, H, W, CW}, x.options().dtype(at::kInt));
  bdbnn_sign_mask_pack(x.data_ptr(), (uint32_t*)sp.data_ptr<int>(),
                       (uint32_t*)mp.data_ptr<int>(), N * H * W, (int)C, CW,
                       is_bf16(x), cur_stream());
  return {sp, mp};
}

at::Tensor decode_packed(const at::Tensor& sp, int64_t C, bool out_bf16) {
  TORCH_CHECK(sp.is_cuda() && sp.dim() == 4 && sp.scalar_type() == at::kInt,
              "decode_packed: int32 [N,H,W,CW]");
  int64_t N = sp.size(0), H = sp.size(1), W = sp.size(2);
  int CW = (int)sp.size(3);
  auto out = at::empty({N, C, H, W},
                       sp.options().dtype(out_bf16 ? at::kBFloat16
                                                   : at::kFloat),
                       at::MemoryFormat::ChannelsLast);
  bdbnn_decode_packed((const uint32_t*)sp.data_ptr<int>(), out.data_ptr(),
                      N * H * W, (int)C, CW, out_bf16, cur_stream());
  return out;
}

at::Tensor mask_mul_packed(const at::Tensor& g, const at::Tensor& mp,
                           int64_t C, bool out_bf16) {
  TORCH_CHECK(g.is_cuda() && mp.is_cuda(), "mask_mul_packed: CUDA tensors");
  check_vec8(g, false, "g", "mask_mul_packed");
  auto gc = g.contiguous(at::MemoryFormat::ChannelsLast);
  int64_t N = mp.size(0), H = mp.size(1), W = mp.size(2);
  int CW = (int)mp.size(3);
  TORCH_CHECK(gc.numel() == N * H * W * C, "mask_mul_packed: shape mismatch");
  auto out = at::empty({N, C, H, W},
                       g.options().dtype(out_bf16 ? at::kBFloat16
                                                  : at::kFloat),
                       at::MemoryFormat::ChannelsLast);
  bdbnn_mask_mul_packed(gc.data_ptr(), (const uint32_t*)mp.data_ptr<int>(),
                        out.data_ptr(), N * H * W, (int)C, CW, is_bf16(gc),
                        out_bf16, cur_stream());
  return out;
}

at::Tensor weight_decode(const at::Tensor& wp, const at::Tensor& alpha,
                         int64_t C, bool out_bf16) {
  TORCH_CHECK(wp.is_cuda() && wp.dim() == 4 && wp.scalar_type() == at::kInt,
              "weight_decode: int32 [K,KH,KW,CW]");
  int K = (int)wp.size(0), KH = (int)wp.size(1), KW = (int)wp.size(2);
  int CW = (int)wp.size(3);
  auto out = at::empty({K, C, KH, KW},
                       wp.options().dtype(out_bf16 ? at::kBFloat16
                                                   : at::kFloat));
  bdbnn_weight_decode((const uint32_t*)wp.data_ptr<int>(),
                      alpha.data_ptr<float>(), out.data_ptr(), K, (int)C,
                      KH * KW, CW, out_bf16, cur_stream());
  return out;
}

// ---------------- xnor conv ----------------

// which kernel a forward conv call runs: by the routing table of
// xnor_conv_mfma.hip (kAuto), or forced for tests and benchmarks
enum XnorRoute { kAuto, kMfma, kValu };

// calls since load that took {MFMA, VALU}: the routing tests read them
static std::atomic<int64_t> g_xnor_route_calls[2];

std::vector<at::Tensor> xnor_conv_route(
    const at::Tensor& xp, const at::Tensor& wp, const at::Tensor& alpha,
    const at::Tensor& stab, int64_t C, int64_t stride, int64_t pad,
    bool out_bf16, bool want_stats, XnorRoute route) {
  TORCH_CHECK(xp.is_cuda() && xp.dim() == 4 && xp.scalar_type() == at::kInt,
              "xnor_conv: packed activations int32 [N,H,W,CW]");
  TORCH_CHECK(wp.dim() == 4, "xnor_conv: packed weights [K,KH,KW,CW]");
  int N = (int)xp.size(0), H = (int)xp.size(1), W = (int)xp.size(2);
  int K = (int)wp.size(0), KH = (int)wp.size(1), KW = (int)wp.size(2);
  TORCH_CHECK(KH * KW * wp.size(3) <= 160,
              "xnor_conv: KH*KW*ceil(C/32) must be <= 160 "
              "(kernel address-table size; C <= 512 at 3x3)");
  TORCH_CHECK(KH * KW <= 32,
              "xnor_conv: at most 32 taps (invalid-tap bitmask width)");
  int Ho = (int)((H + 2 * pad - KH) / stride + 1);
  int Wo = (int)((W + 2 * pad - KW) / stride + 1);
  auto out = at::empty({N, K, Ho, Wo},
                       xp.options().dtype(out_bf16 ? at::kBFloat16
                                                   : at::kFloat),
                       at::MemoryFormat::ChannelsLast);
  at::Tensor s1, s2;
  float *s1p = nullptr, *s2p = nullptr;
  if (want_stats) {
    auto fopt = xp.options().dtype(at::kFloat);
    s1 = at::empty({32, K}, fopt);   // 32-way sliced partial sums
    s2 = at::empty({32, K}, fopt);
    s1p = s1.data_ptr<float>();
    s2p = s2.data_ptr<float>();
  }
  bool mfma = route == kMfma;
  if (route == kAuto)
    mfma = !want_stats && bdbnn_xnor_mfma_routed((int)C, K, KH, KW,
                                                 (int)stride, (int)pad);
  if (mfma) {
    TORCH_CHECK(!want_stats, "xnor_conv_mfma: no BN statistics epilogue");
    TORCH_CHECK(wp.size(3) * 32 == C && xp.size(3) == wp.size(3),
                "xnor_conv_mfma: C must equal 32 * CW of both operands");
    int rc = bdbnn_xnor_conv_mfma_fwd(
        (const uint32_t*)xp.data_ptr<int>(),
        (const uint32_t*)wp.data_ptr<int>(), alpha.data_ptr<float>(),
        out.data_ptr(), out_bf16, N, H, W, (int)C, K, KH, KW, (int)stride,
        (int)pad, Ho, Wo, cur_stream());
    TORCH_CHECK(rc == 0, "xnor_conv_mfma: ",
                rc == -1 ? "unsupported shape" : "tensor too large");
    ++g_xnor_route_calls[0];
    return {out};
  }
  bdbnn_xnor_conv_fwd((const uint32_t*)xp.data_ptr<int>(),
                      (const uint32_t*)wp.data_ptr<int>(),
                      alpha.data_ptr<float>(), stab.data_ptr<float>(),
                      out.data_ptr(), s1p, s2p, out_bf16, N, H, W, (int)C,
                      K, KH, KW, (int)stride, (int)pad, Ho, Wo,
                      cur_stream());
  ++g_xnor_route_calls[1];
  if (want_stats) return {out, s1, s2};
  return {out};
}

std::vector<at::Tensor> xnor_conv_fwd(
    const at::Tensor& xp, const at::Tensor& wp, const at::Tensor& alpha,
    const at::Tensor& stab, int64_t C, int64_t stride, int64_t pad,
    bool out_bf16, bool want_stats) {
  return xnor_conv_route(xp, wp, alpha, stab, C, stride, pad, out_bf16,
                         want_stats, kAuto);
}

// the two kernels by name, whatever the routing table says
at::Tensor xnor_conv_mfma_fwd(const at::Tensor& xp, const at::Tensor& wp,
                              const at::Tensor& alpha, int64_t C,
                              int64_t stride, int64_t pad, bool out_bf16) {
  TORCH_CHECK(wp.dim() == 4 &&
                  bdbnn_xnor_mfma_supported((int)C, (int)wp.size(0),
                                            (int)wp.size(1), (int)wp.size(2),
                                            (int)stride, (int)pad),
              "xnor_conv_mfma_fwd: shape not supported by the MFMA kernel");
  return xnor_conv_route(xp, wp, alpha, alpha, C, stride, pad, out_bf16,
                         false, kMfma)[0];
}

std::vector<at::Tensor> xnor_conv_valu_fwd(
    const at::Tensor& xp, const at::Tensor& wp, const at::Tensor& alpha,
    const at::Tensor& stab, int64_t C, int64_t stride, int64_t pad,
    bool out_bf16, bool want_stats) {
  return xnor_conv_route(xp, wp, alpha, stab, C, stride, pad, out_bf16,
                         want_stats, kValu);
}

bool xnor_mfma_supported(int64_t C, int64_t K, int64_t KH, int64_t KW,
                         int64_t stride, int64_t pad) {
  return bdbnn_xnor_mfma_supported((int)C, (int)K, (int)KH, (int)KW,
                                   (int)stride, (int)pad) != 0;
}

// (calls on the MFMA kernel, calls on the VALU kernel) since load
std::vector<int64_t> xnor_route_calls() {
  return {g_xnor_route_calls[0].load(), g_xnor_route_calls[1].load()};
}

// ---- inference: conv + folded eval BN (+ skip) + act (+ sign plane) ----

// launches of the fused inference conv since load (the engine tests read it)
static std::atomic<int64_t> g_xnor_fused_calls;

int64_t xnor_fused_calls() { return g_xnor_fused_calls.load(); }

// (sc, sh) of an eval-mode BN as bn_act_eval_kernel computes them for
// itself, by the same device function; b1 (RPReLU) is added to sh
std::vector<at::Tensor> bn_fold(const at::Tensor& gamma,
                                const at::Tensor& beta, const at::Tensor& rm,
                                const at::Tensor& rv, double eps,
                                const c10::optional<at::Tensor>& b1) {
  TORCH_CHECK(gamma.is_cuda() && gamma.numel() > 0,
              "bn_fold: gamma must be a non-empty CUDA tensor");
  int64_t C = gamma.numel();
  TORCH_CHECK(beta.numel() == C && rm.numel() == C && rv.numel() == C &&
                  (!b1.has_value() || b1->numel() == C),
              "bn_fold: per-channel tensors must have C elements");
  auto gf = chan_f32(gamma);
  auto bf = chan_f32(beta);
  auto rmf = chan_f32(rm);
  auto rvf = chan_f32(rv);
  at::Tensor b1f;
  const float* b1_ptr = opt_chan_ptr(b1, b1f);
  auto sc = at::empty({C}, gf.options());
  auto sh = at::empty({C}, gf.options());
  bdbnn_bn_fold(gf.data_ptr<float>(), bf.data_ptr<float>(),
                rmf.data_ptr<float>(), rvf.data_ptr<float>(), b1_ptr,
                sc.data_ptr<float>(), sh.data_ptr<float>(), (int)C,
                (float)eps, cur_stream());
  return {sc, sh};
}

py::list xnor_conv_bn_act_fwd(
    const at::Tensor& xp, const at::Tensor& wp, const at::Tensor& alpha,
    const at::Tensor& sc, const at::Tensor& sh,
    const c10::optional<at::Tensor>& a, const c10::optional<at::Tensor>& b2,
    const c10::optional<at::Tensor>& skip, int64_t C, int64_t stride,
    int64_t pad, int64_t act_kind, bool out_bf16, bool want_pack) {
  const char* who = "xnor_conv_bn_act_fwd: ";
  TORCH_CHECK(xp.is_cuda() && xp.dim() == 4 && xp.scalar_type() == at::kInt &&
                  xp.is_contiguous(),
              who, "packed activations int32 [N,H,W,CW]");
  TORCH_CHECK(wp.is_cuda() && wp.dim() == 4 && wp.scalar_type() == at::kInt &&
                  wp.is_contiguous(),
              who, "packed weights int32 [K,KH,KW,CW]");
  int N = (int)xp.size(0), H = (int)xp.size(1), W = (int)xp.size(2);
  int K = (int)wp.size(0), KH = (int)wp.size(1), KW = (int)wp.size(2);
  TORCH_CHECK(bdbnn_xnor_mfma_supported((int)C, K, KH, KW, (int)stride,
                                        (int)pad),
              who, "shape not supported by the MFMA kernel");
  TORCH_CHECK(wp.size(3) * 32 == C && xp.size(3) == wp.size(3),
              who, "C must equal 32 * CW of both operands");
  TORCH_CHECK(act_kind >= 0 && act_kind <= 3, who, "act_kind must be 0..3");
  // the kernel reads the per-channel operands as float4 through float*
  auto chan_ok = [&](const at::Tensor& t) {
    return is_f32_chan(t, K) && (uintptr_t)t.data_ptr() % 16 == 0;
  };
  TORCH_CHECK(chan_ok(alpha) && chan_ok(sc) && chan_ok(sh),
              who, "alpha, sc, sh must be contiguous fp32 CUDA [K]");
  const bool need_a = act_kind == 1 || act_kind == 3;
  TORCH_CHECK(!need_a || a.has_value(), who, "PReLU needs its slopes a");
  TORCH_CHECK(act_kind != 3 || b2.has_value(), who, "RPReLU needs b2");
  TORCH_CHECK((!need_a || chan_ok(*a)) && (act_kind != 3 || chan_ok(*b2)),
              who, "a, b2 must be contiguous fp32 CUDA [K]");
  int Ho = (int)((H + 2 * pad - KH) / stride + 1);
  int Wo = (int)((W + 2 * pad - KW) / stride + 1);
  auto out = at::empty({N, K, Ho, Wo},
                       xp.options().dtype(out_bf16 ? at::kBFloat16
                                                   : at::kFloat),
                       at::MemoryFormat::ChannelsLast);
  const void* skip_ptr = nullptr;
  if (skip.has_value()) {
    TORCH_CHECK(skip->is_cuda() && skip->sizes() == out.sizes() &&
                    skip->scalar_type() == out.scalar_type() &&
                    skip->is_contiguous(at::MemoryFormat::ChannelsLast) &&
                    (uintptr_t)skip->data_ptr() % 16 == 0,
                who, "skip must have out's shape, dtype and channels_last "
                     "layout");
    skip_ptr = skip->data_ptr();
  }
  at::Tensor plane;
  uint32_t* plane_ptr = nullptr;
  if (want_pack) {
    plane = at::empty({N, Ho, Wo, K / 32}, xp.options());
    plane_ptr = (uint32_t*)plane.data_ptr<int>();
  }
  int rc = bdbnn_xnor_conv_bn_act_fwd(
      (const uint32_t*)xp.data_ptr<int>(),
      (const uint32_t*)wp.data_ptr<int>(), alpha.data_ptr<float>(),
      sc.data_ptr<float>(), sh.data_ptr<float>(),
      need_a ? a->data_ptr<float>() : nullptr,
      act_kind == 3 ? b2->data_ptr<float>() : nullptr, skip_ptr,
      out.data_ptr(), plane_ptr, (int)act_kind, out_bf16, N, H, W, (int)C, K,
      KH, KW, (int)stride, (int)pad, Ho, Wo, cur_stream());
  TORCH_CHECK(rc == 0, who,
              rc == -1 ? "unsupported shape"
                       : rc == -2 ? "tensor too large" : "bad act operands");
  ++g_xnor_fused_calls;
  py::list res;
  res.append(out);
  if (want_pack) res.append(plane);
  else res.append(py::none());
  return res;
}


// ---------------- stem conv (7x7/2, C=3 -> 64) ----------------

std::vector<at::Tensor> stem_conv_fwd(const at::Tensor& x,
                                      const at::Tensor& w) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && x.size(1) == 3,
              "stem: (N,3,H,W) input");
  TORCH_CHECK(w.dim() == 4 && w.size(0) == 64 && w.size(1) == 3 &&
                  w.size(2) == 7 && w.size(3) == 7,
              "stem: (64,3,7,7) weights");
  int N = (int)x.size(0), H = (int)x.size(2), W = (int)x.size(3);
  TORCH_CHECK(H % 2 == 0 && W % 2 == 0, "stem: even H,W");
  auto xc = x.contiguous(at::MemoryFormat::ChannelsLast);
  bool bf16 = is_bf16(xc);
  auto bopt = xc.options().dtype(at::kBFloat16);
  auto x4 = at::empty({N, H, W, 4}, bopt);
  bdbnn_stem_pack_x4(xc.data_ptr(), x4.data_ptr(), (int64_t)N * H * W,
                     bf16, cur_stream());
  auto wf = w.contiguous().to(at::kFloat);
  auto w4T = at::empty({64, 224}, bopt);
  bdbnn_stem_pack_w4(wf.data_ptr<float>(), w4T.data_ptr(), cur_stream());
  auto out = at::empty({N, 64, H / 2, W / 2}, bopt,
                       at::MemoryFormat::ChannelsLast);
  bdbnn_stem_fwd(x4.data_ptr(), w4T.data_ptr(), out.data_ptr(), N, H, W,
                 cur_stream());
  return {out, x4};
}

at::Tensor stem_conv_wrw(const at::Tensor& x4, const at::Tensor& gy) {
  TORCH_CHECK(x4.is_cuda() && x4.dim() == 4 && x4.size(3) == 4 &&
                  x4.scalar_type() == at::kBFloat16,
              "stem wrw: packed x4 (N,H,W,4) bf16");
  int N = (int)x4.size(0), H = (int)x4.size(1), W = (int)x4.size(2);
  auto gc = gy.to(at::kBFloat16).contiguous(at::MemoryFormat::ChannelsLast);
  TORCH_CHECK(gc.size(1) == 64 && gc.size(2) == H / 2 &&
                  gc.size(3) == W / 2, "stem wrw: grad shape");
  int nslab = bdbnn_stem_wrw_nslab(N, H, W);
  auto fopt = x4.options().dtype(at::kFloat);
  auto slabs = at::empty({nslab, 64, 224}, fopt);
  bdbnn_stem_wrw(x4.data_ptr(), gc.data_ptr(), slabs.data_ptr<float>(),
                 N, H, W, cur_stream());
  auto dw = at::empty({64, 3, 7, 7}, fopt);
  bdbnn_stem_fold_dw4(slabs.data_ptr<float>(), dw.data_ptr<float>(),
                      nslab, cur_stream());
  return dw;
}

// ---------------- fused classification losses ----------------

std::vector<at::Tensor> kd_logit_fwd(const at::Tensor& s,
                                     const at::Tensor& t) {
  check_logits(s, "kd_logit_fwd");
  TORCH_CHECK(t.is_cuda() && s.sizes() == t.sizes(),
              "kd_logit_fwd: teacher logits must be a CUDA tensor of the "
              "student's shape");
  auto sc = s.contiguous();
  auto tc = t.to(s.scalar_type()).contiguous();
  int B = (int)s.size(0), C = (int)s.size(1);
  auto fopt = sc.options().dtype(at::kFloat);
  auto stats = at::empty({B, 4}, fopt);
  auto out = at::empty({}, fopt);
  bdbnn_kd_logit_fwd(sc.data_ptr(), tc.data_ptr(), stats.data_ptr<float>(),
                     out.data_ptr<float>(), B, C, is_bf16(sc),
                     cur_stream());
  return {out, stats, tc};
}

at::Tensor kd_logit_bwd(const at::Tensor& s, const at::Tensor& t,
                        const at::Tensor& stats, double gscale) {
  check_logits(s, "kd_logit_bwd");
  // t and stats are what kd_logit_fwd returned: read as they are
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == s.scalar_type() &&
                  t.sizes() == s.sizes() && t.is_contiguous(),
              "kd_logit_bwd: t must be contiguous, of s's dtype and shape");
  TORCH_CHECK(stats.is_cuda() && stats.scalar_type() == at::kFloat &&
                  stats.is_contiguous() && stats.numel() == 4 * s.size(0),
              "kd_logit_bwd: stats must be contiguous fp32 [B,4]");
  auto sc = s.contiguous();
  int B = (int)s.size(0), C = (int)s.size(1);
  auto ds = at::empty_like(sc);
  bdbnn_kd_logit_bwd(sc.data_ptr(), t.data_ptr(), stats.data_ptr<float>(),
                     ds.data_ptr(), (float)(gscale / B), B, C, is_bf16(sc),
                     cur_stream());
  return ds;
}

std::vector<at::Tensor> ce_fwd(const at::Tensor& s, const at::Tensor& y) {
  check_logits(s, "ce_fwd");
  TORCH_CHECK(y.is_cuda() && y.scalar_type() == at::kLong && y.dim() == 1 &&
                  y.size(0) == s.size(0),
              "ce_fwd: targets must be an int64 CUDA tensor [B]");
  auto sc = s.contiguous();
  auto yc = y.contiguous();
  int B = (int)s.size(0), C = (int)s.size(1);
  auto fopt = sc.options().dtype(at::kFloat);
  auto stats = at::empty({B}, fopt);
  auto out = at::empty({}, fopt);
  bdbnn_ce_fwd(sc.data_ptr(), yc.data_ptr<int64_t>(),
               stats.data_ptr<float>(), out.data_ptr<float>(), B, C,
               is_bf16(sc), cur_stream());
  return {out, stats};
}

at::Tensor ce_bwd(const at::Tensor& s, const at::Tensor& y,
                  const at::Tensor& stats, double gscale) {
  check_logits(s, "ce_bwd");
  TORCH_CHECK(y.is_cuda() && y.scalar_type() == at::kLong && y.dim() == 1 &&
                  y.size(0) == s.size(0),
              "ce_bwd: targets must be an int64 CUDA tensor [B]");
  TORCH_CHECK(stats.is_cuda() && stats.scalar_type() == at::kFloat &&
                  stats.is_contiguous() && stats.numel() == s.size(0),
              "ce_bwd: stats must be contiguous fp32 [B]");
  auto sc = s.contiguous();
  auto yc = y.contiguous();   // the kernel indexes y[b] with unit stride
  int B = (int)s.size(0), C = (int)s.size(1);
  auto ds = at::empty_like(sc);
  bdbnn_ce_bwd(sc.data_ptr(), yc.data_ptr<int64_t>(),
               stats.data_ptr<float>(), ds.data_ptr(),
               (float)(gscale / B), B, C, is_bf16(sc), cur_stream());
  return ds;
}

// ---------------- maxpool ----------------

std::vector<at::Tensor> maxpool_fwd(const at::Tensor& x, int64_t ks,
                                    int64_t stride, int64_t pad) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4, "maxpool_fwd: 4-D CUDA tensor");
  check_vec8(x, false, "x", "maxpool_fwd");
  auto xc = x.contiguous(at::MemoryFormat::ChannelsLast);
  int N = (int)x.size(0), C = (int)x.size(1);
  int H = (int)x.size(2), W = (int)x.size(3);
  int Ho = (int)((H + 2 * pad - ks) / stride + 1);
  int Wo = (int)((W + 2 * pad - ks) / stride + 1);
  auto out = at::empty({N, C, Ho, Wo}, xc.options(),
                       at::MemoryFormat::ChannelsLast);
  auto idx = at::empty({N, Ho, Wo, C}, xc.options().dtype(at::kByte));
  bdbnn_maxpool_fwd(xc.data_ptr(), out.data_ptr(),
                    idx.data_ptr<unsigned char>(), N, C, H, W, Ho, Wo,
                    (int)ks, (int)stride, (int)pad, is_bf16(xc),
                    cur_stream());
  return {out, idx};
}

at::Tensor maxpool_bwd(const at::Tensor& dy, const at::Tensor& idx,
                       int64_t H, int64_t W, int64_t ks, int64_t stride,
                       int64_t pad) {
  TORCH_CHECK(dy.dim() == 4, "maxpool_bwd: 4-D CUDA tensor");
  check_vec8(dy, false, "dy", "maxpool_bwd");
  auto dyc = dy.contiguous(at::MemoryFormat::ChannelsLast);
  int N = (int)dy.size(0), C = (int)dy.size(1);
  int Ho = (int)dy.size(2), Wo = (int)dy.size(3);
  auto dx = at::empty({N, C, H, W}, dyc.options(),
                      at::MemoryFormat::ChannelsLast);
  bdbnn_maxpool_bwd(dyc.data_ptr(), idx.data_ptr<unsigned char>(),
                    dx.data_ptr(), N, C, (int)H, (int)W, Ho, Wo, (int)ks,
                    (int)stride, (int)pad, is_bf16(dyc), cur_stream());
  return dx;
}

// ---------------- prelu ----------------

at::Tensor prelu_fwd(const at::Tensor& x, const at::Tensor& a) {
  check_vec8(x, true, "x", "prelu_fwd");
  int C = (int)x.size(1);
  TORCH_CHECK(a.is_cuda() && a.numel() == C,
              "prelu_fwd: a must be a CUDA tensor of C elements");
  auto xc = x.contiguous(at::MemoryFormat::ChannelsLast);
  auto af = chan_f32(a);
  auto y = at::empty_like(xc, xc.options(), at::MemoryFormat::ChannelsLast);
  bdbnn_prelu_fwd(xc.data_ptr(), af.data_ptr<float>(), y.data_ptr(),
                  xc.numel(), C, xc.scalar_type() == at::kBFloat16,
                  cur_stream());
  return y;
}

std::vector<at::Tensor> prelu_bwd(const at::Tensor& g, const at::Tensor& x,
                                  const at::Tensor& a) {
  check_vec8(x, true, "x", "prelu_bwd");
  check_vec8(g, true, "g", "prelu_bwd");
  TORCH_CHECK(g.scalar_type() == x.scalar_type() && g.sizes() == x.sizes(),
              "prelu_bwd: grad dtype and shape must match input");
  int C = (int)x.size(1);
  TORCH_CHECK(a.is_cuda() && a.numel() == C,
              "prelu_bwd: a must be a CUDA tensor of C elements");
  auto xc = x.contiguous(at::MemoryFormat::ChannelsLast);
  auto gc = g.contiguous(at::MemoryFormat::ChannelsLast);
  auto af = chan_f32(a);
  auto dx = at::empty_like(xc, xc.options(), at::MemoryFormat::ChannelsLast);
  auto da = at::empty({C}, xc.options().dtype(at::kFloat));
  bdbnn_prelu_bwd(xc.data_ptr(), gc.data_ptr(), af.data_ptr<float>(),
                  dx.data_ptr(), da.data_ptr<float>(), xc.numel(), C,
                  xc.scalar_type() == at::kBFloat16, cur_stream());
  return {dx, da};
}

// ---------------- fused BN (+add) (+act) ----------------

// RPReLU (act_kind 3) reads a, b1 and b2 per channel: all three present,
// on the device, C elements each.  The other kinds take no shifts.
static void check_rprelu_args(int64_t act_kind, int64_t C,
                              const c10::optional<at::Tensor>& a,
                              const c10::optional<at::Tensor>& b1,
                              const c10::optional<at::Tensor>& b2,
                              const char* who) {
  if (act_kind != 3) return;
  const c10::optional<at::Tensor>* ts[3] = {&a, &b1, &b2};
  const char* names[3] = {"a", "b1", "b2"};
  for (int i = 0; i < 3; ++i) {
    TORCH_CHECK(ts[i]->has_value(), who, ": RPReLU needs ", names[i]);
    TORCH_CHECK((*ts[i])->is_cuda() && (*ts[i])->numel() == C, who, ": ",
                names[i], " must be a CUDA tensor of C elements");
  }
}

std::vector<at::Tensor> bn_act_fwd_train(
    const at::Tensor& x, const c10::optional<at::Tensor>& skip,
    const at::Tensor& gamma, const at::Tensor& beta,
    const c10::optional<at::Tensor>& a,
    c10::optional<at::Tensor> running_mean,
    c10::optional<at::Tensor> running_var, double momentum, double eps,
    int64_t act_kind, const c10::optional<at::Tensor>& pre_s1,
    const c10::optional<at::Tensor>& pre_s2, bool want_pack,
    const c10::optional<at::Tensor>& b1,
    const c10::optional<at::Tensor>& b2) {
  check_vec8(x, true, "x", "bn_act_fwd_train");
  auto xc = x.contiguous(at::MemoryFormat::ChannelsLast);
  int C = (int)x.size(1);
  check_rprelu_args(act_kind, C, a, b1, b2, "bn_act_fwd_train");
  TORCH_CHECK(gamma.numel() == C && beta.numel() == C &&
                  (!a.has_value() || a->numel() == C),
              "bn_act_fwd_train: gamma, beta and a must have C elements");
  TORCH_CHECK(act_kind != 1 || a.has_value(),
              "bn_act_fwd_train: PReLU needs its slopes a");
  int64_t n = xc.numel();
  bool bf16 = is_bf16(xc);
  auto [mean, invstd] =
      bn_train_stats(xc, C, pre_s1, pre_s2, running_mean, running_var,
                     momentum, eps, "bn_act_fwd_train");
  auto out = at::empty_like(xc, xc.options(), at::MemoryFormat::ChannelsLast);
  // PReLU backward needs the true pre-activation z (RPReLU: the shifted
  // u = z + b1, which is what the kernel stores for it); ReLU only needs
  // its sign (recoverable from out) and identity ignores it — skip the
  // write.
  at::Tensor z;
  void* zptr = nullptr;
  if (act_kind == 1 || act_kind == 3) {
    z = at::empty_like(xc, xc.options(), at::MemoryFormat::ChannelsLast);
    zptr = z.data_ptr();
  } else {
    z = out;
  }
  at::Tensor skipc;
  const void* skip_ptr = opt_skip_ptr(skip, xc, skipc);
  auto gf = chan_f32(gamma);
  auto bf = chan_f32(beta);
  at::Tensor af;
  const float* a_ptr = opt_chan_ptr(a, af);
  at::Tensor b1f, b2f;
  const float* b1_ptr = act_kind == 3 ? opt_chan_ptr(b1, b1f) : nullptr;
  const float* b2_ptr = act_kind == 3 ? opt_chan_ptr(b2, b2f) : nullptr;
  // consumer-conv sign/mask pack fused into the epilogue (the next
  // binary conv then skips its own pack read pass; csrc/bn_act.hip)
  at::Tensor xpk, mpk;
  uint32_t *xpk_p = nullptr, *mpk_p = nullptr;
  if (want_pack) {
    TORCH_CHECK(C % 32 == 0, "bn pack fusion needs C % 32 == 0");
    int CW = C / 32;
    auto iopt = xc.options().dtype(at::kInt);
    xpk = at::empty({x.size(0), x.size(2), x.size(3), CW}, iopt);
    mpk = at::empty({x.size(0), x.size(2), x.size(3), CW}, iopt);
    xpk_p = (uint32_t*)xpk.data_ptr<int>();
    mpk_p = (uint32_t*)mpk.data_ptr<int>();
  }
  bdbnn_bn_act_fwd(xc.data_ptr(), skip_ptr, mean.data_ptr<float>(),
                   invstd.data_ptr<float>(), gf.data_ptr<float>(),
                   bf.data_ptr<float>(), a_ptr, b1_ptr, b2_ptr,
                   out.data_ptr(), zptr, n, C, (int)act_kind, xpk_p, mpk_p,
                   bf16, cur_stream());
  if (want_pack) return {out, z, mean, invstd, xpk, mpk};
  return {out, z, mean, invstd};
}

std::vector<at::Tensor> bn_act_bwd(
    const at::Tensor& dy, const at::Tensor& z, const at::Tensor& x,
    const at::Tensor& mean, const at::Tensor& invstd,
    const at::Tensor& gamma, const c10::optional<at::Tensor>& a,
    int64_t act_kind, bool need_dskip) {
  check_vec8(x, true, "x", "bn_act_bwd");
  check_vec8(dy, true, "dy", "bn_act_bwd");
  TORCH_CHECK(dy.sizes() == x.sizes(), "bn_act_bwd: dy shape must match x");
  // identity never reads z; the other kinds read it with x's type and index
  TORCH_CHECK(act_kind == 0 || (z.is_cuda() && z.sizes() == x.sizes() &&
                                z.scalar_type() == x.scalar_type()),
              "bn_act_bwd: z must match x in shape and dtype");
  TORCH_CHECK(mean.numel() == x.size(1) && invstd.numel() == x.size(1) &&
                  gamma.numel() == x.size(1) &&
                  (!a.has_value() || a->numel() == x.size(1)),
              "bn_act_bwd: mean, invstd, gamma and a must have C elements");
  // RPReLU's backward reads a alone: the shifts are in the saved plane
  TORCH_CHECK((act_kind != 1 && act_kind != 3) || a.has_value(),
              "bn_act_bwd: PReLU and RPReLU need their slopes a");
  auto xc = x.contiguous(at::MemoryFormat::ChannelsLast);
  auto zc = z.contiguous(at::MemoryFormat::ChannelsLast);
  auto dyc = dy.to(xc.scalar_type()).contiguous(at::MemoryFormat::ChannelsLast);
  int C = (int)x.size(1);
  int64_t n = xc.numel();
  bool bf16 = is_bf16(xc);
  auto fopt = xc.options().dtype(at::kFloat);
  const int NR = bdbnn_bn_sum_rows((int)act_kind);
  auto sums32 = at::empty({32, C, NR}, fopt);  // sliced partials
  auto sums = at::empty({C, NR}, fopt);
  at::Tensor af;
  const float* a_ptr = opt_chan_ptr(a, af);
  bdbnn_bn_act_bwd_reduce(dyc.data_ptr(), zc.data_ptr(), xc.data_ptr(),
                          mean.data_ptr<float>(), invstd.data_ptr<float>(),
                          a_ptr, sums32.data_ptr<float>(),
                          sums.data_ptr<float>(), n, C, (int)act_kind,
                          bf16, cur_stream());
  auto gf = chan_f32(gamma);
  auto dx = at::empty_like(xc, xc.options(), at::MemoryFormat::ChannelsLast);
  at::Tensor dskip;
  void* dskip_ptr = nullptr;
  if (need_dskip) {
    dskip = at::empty_like(xc, xc.options(), at::MemoryFormat::ChannelsLast);
    dskip_ptr = dskip.data_ptr();
  } else {
    dskip = at::empty({0}, xc.options());
  }
  bdbnn_bn_act_bwd_apply(dyc.data_ptr(), zc.data_ptr(), xc.data_ptr(),
                         mean.data_ptr<float>(), invstd.data_ptr<float>(),
                         gf.data_ptr<float>(), a_ptr, sums.data_ptr<float>(),
                         dx.data_ptr(), dskip_ptr, n, C, (int)act_kind,
                         (float)(1.0 / (double)(n / C)), bf16, cur_stream());
  auto dbeta = sums.select(1, 0).clone();
  auto dgamma = sums.select(1, 1).clone();
  auto da = sums.select(1, 2).clone();
  if (act_kind == 3) {
    // db1 = sum dz, the number dbeta is; db2 = sum dy
    return {dx, dskip, dgamma, dbeta, da, dbeta.clone(),
            sums.select(1, 3).clone()};
  }
  return {dx, dskip, dgamma, dbeta, da};
}

at::Tensor bn_act_eval(const at::Tensor& x,
                       const c10::optional<at::Tensor>& skip,
                       const at::Tensor& gamma, const at::Tensor& beta,
                       const c10::optional<at::Tensor>& a,
                       const at::Tensor& rm, const at::Tensor& rv,
                       double eps, int64_t act_kind,
                       const c10::optional<at::Tensor>& b1,
                       const c10::optional<at::Tensor>& b2) {
  check_vec8(x, true, "x", "bn_act_eval");
  check_rprelu_args(act_kind, x.size(1), a, b1, b2, "bn_act_eval");
  TORCH_CHECK(gamma.numel() == x.size(1) && beta.numel() == x.size(1) &&
                  rm.numel() == x.size(1) && rv.numel() == x.size(1) &&
                  (!a.has_value() || a->numel() == x.size(1)),
              "bn_act_eval: per-channel tensors must have C elements");
  TORCH_CHECK(act_kind != 1 || a.has_value(),
              "bn_act_eval: PReLU needs its slopes a");
  auto xc = x.contiguous(at::MemoryFormat::ChannelsLast);
  int C = (int)x.size(1);
  int64_t n = xc.numel();
  bool bf16 = is_bf16(xc);
  auto out = at::empty_like(xc, xc.options(), at::MemoryFormat::ChannelsLast);
  at::Tensor skipc;
  const void* skip_ptr = opt_skip_ptr(skip, xc, skipc);
  auto gf = chan_f32(gamma);
  auto bf = chan_f32(beta);
  auto rmf = chan_f32(rm);
  auto rvf = chan_f32(rv);
  at::Tensor af;
  const float* a_ptr = opt_chan_ptr(a, af);
  at::Tensor b1f, b2f;
  const float* b1_ptr = act_kind == 3 ? opt_chan_ptr(b1, b1f) : nullptr;
  const float* b2_ptr = act_kind == 3 ? opt_chan_ptr(b2, b2f) : nullptr;
  bdbnn_bn_act_eval(xc.data_ptr(), skip_ptr, rmf.data_ptr<float>(),
                    rvf.data_ptr<float>(), gf.data_ptr<float>(),
                    bf.data_ptr<float>(), a_ptr, b1_ptr, b2_ptr,
                    out.data_ptr(), n, C, (int)act_kind, (float)eps, bf16,
                    cur_stream());
  return out;
}

// ---------------- fused stem tail: BN + ReLU + maxpool (csrc/bn_pool.hip) --

// window and channel checks shared by the two entry points; sets Ho, Wo
static void check_bn_pool_geom(const at::Tensor& x, int64_t ks,
                               int64_t stride, int64_t pad, int64_t& Ho,
                               int64_t& Wo, const char* who) {
  check_vec8(x, true, "x", who);
  TORCH_CHECK(ks >= 1 && ks <= 15 && stride >= 1 && pad >= 0 &&
                  2 * pad <= ks,
              who, ": need 1 <= ks <= 15 (u8 tap index), stride >= 1, "
              "0 <= pad <= ks/2");
  Ho = (x.size(2) + 2 * pad - ks) / stride + 1;
  Wo = (x.size(3) + 2 * pad - ks) / stride + 1;
  TORCH_CHECK(x.size(2) + 2 * pad >= ks && x.size(3) + 2 * pad >= ks &&
                  Ho >= 1 && Wo >= 1,
              who, ": window larger than the padded input");
  TORCH_CHECK(x.size(0) * x.size(2) * x.size(3) < (int64_t(1) << 31), who,
              ": N*H*W must be < 2^31");
}

static void check_chan_f32(const at::Tensor& t, int64_t C, const char* name,
                           const char* who) {
  TORCH_CHECK(t.is_cuda() && t.numel() == C, who, ": ", name,
              " must be a CUDA tensor of C elements");
}

std::vector<at::Tensor> bn_relu_maxpool_fwd_train(
    const at::Tensor& x, const at::Tensor& gamma, const at::Tensor& beta,
    c10::optional<at::Tensor> running_mean,
    c10::optional<at::Tensor> running_var, double momentum, double eps,
    int64_t ks, int64_t stride, int64_t pad,
    const c10::optional<at::Tensor>& pre_s1,
    const c10::optional<at::Tensor>& pre_s2, bool want_pack) {
  const char* who = "bn_relu_maxpool_fwd_train";
  int64_t Ho, Wo;
  check_bn_pool_geom(x, ks, stride, pad, Ho, Wo, who);
  auto xc = x.contiguous(at::MemoryFormat::ChannelsLast);
  int N = (int)x.size(0), C = (int)x.size(1);
  int H = (int)x.size(2), W = (int)x.size(3);
  check_chan_f32(gamma, C, "gamma", who);
  check_chan_f32(beta, C, "beta", who);
  bool bf16 = is_bf16(xc);
  auto [mean, invstd] = bn_train_stats(
      xc, C, pre_s1, pre_s2, running_mean, running_var, momentum, eps, who);
  auto gf = chan_f32(gamma);
  auto bf = chan_f32(beta);
  auto out = at::empty({N, C, Ho, Wo}, xc.options(),
                       at::MemoryFormat::ChannelsLast);
  auto idx = at::empty({N, Ho, Wo, C}, xc.options().dtype(at::kByte));
  at::Tensor xpk, mpk;
  uint32_t *xpk_p = nullptr, *mpk_p = nullptr;
  if (want_pack) {
    TORCH_CHECK(C % 32 == 0, who, ": pack fusion needs C % 32 == 0");
    auto iopt = xc.options().dtype(at::kInt);
    xpk = at::empty({N, Ho, Wo, C / 32}, iopt);
    mpk = at::empty({N, Ho, Wo, C / 32}, iopt);
    xpk_p = (uint32_t*)xpk.data_ptr<int>();
    mpk_p = (uint32_t*)mpk.data_ptr<int>();
  }
  bdbnn_bn_relu_maxpool_fwd(xc.data_ptr(), mean.data_ptr<float>(),
                            invstd.data_ptr<float>(), gf.data_ptr<float>(),
                            bf.data_ptr<float>(), out.data_ptr(),
                            idx.data_ptr<unsigned char>(), xpk_p, mpk_p, N,
                            C, H, W, (int)Ho, (int)Wo, (int)ks, (int)stride,
                            (int)pad, bf16, cur_stream());
  if (want_pack) return {out, idx, mean, invstd, xpk, mpk};
  return {out, idx, mean, invstd};
}

std::vector<at::Tensor> bn_relu_maxpool_bwd(
    const at::Tensor& dy, const at::Tensor& idx, const at::Tensor& x,
    const at::Tensor& mean, const at::Tensor& invstd,
    const at::Tensor& gamma, const at::Tensor& beta, int64_t ks,
    int64_t stride, int64_t pad) {
  const char* who = "bn_relu_maxpool_bwd";
  int64_t Ho, Wo;
  check_bn_pool_geom(x, ks, stride, pad, Ho, Wo, who);
  auto xc = x.contiguous(at::MemoryFormat::ChannelsLast);
  int N = (int)x.size(0), C = (int)x.size(1);
  int H = (int)x.size(2), W = (int)x.size(3);
  TORCH_CHECK(dy.is_cuda() && dy.dim() == 4 && dy.size(0) == N &&
                  dy.size(1) == C && dy.size(2) == Ho && dy.size(3) == Wo,
              who, ": dy must be the pooled shape (N,C,Ho,Wo)");
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == at::kByte &&
                  idx.is_contiguous() && idx.dim() == 4 &&
                  idx.size(0) == N && idx.size(1) == Ho &&
                  idx.size(2) == Wo && idx.size(3) == C,
              who, ": idx must be contiguous u8 [N][Ho][Wo][C]");
  check_chan_f32(gamma, C, "gamma", who);
  check_chan_f32(beta, C, "beta", who);
  TORCH_CHECK(is_f32_chan(mean, C) && is_f32_chan(invstd, C), who,
              ": mean and invstd must be contiguous fp32 [C]");
  auto dyc =
      dy.to(xc.scalar_type()).contiguous(at::MemoryFormat::ChannelsLast);
  bool bf16 = is_bf16(xc);
  auto fopt = xc.options().dtype(at::kFloat);
  auto gf = chan_f32(gamma);
  auto bf = chan_f32(beta);
  auto sums32 = at::empty({32, C, 2}, fopt);  // sliced partials
  auto sums = at::empty({C, 2}, fopt);
  bdbnn_bn_relu_maxpool_bwd_reduce(
      dyc.data_ptr(), idx.data_ptr<unsigned char>(), xc.data_ptr(),
      mean.data_ptr<float>(), invstd.data_ptr<float>(),
      gf.data_ptr<float>(), bf.data_ptr<float>(), sums32.data_ptr<float>(),
      sums.data_ptr<float>(), N, C, H, W, (int)Ho, (int)Wo, (int)ks,
      (int)stride, (int)pad, bf16, cur_stream());
  auto dx = at::empty_like(xc, xc.options(), at::MemoryFormat::ChannelsLast);
  bdbnn_bn_relu_maxpool_bwd_apply(
      dyc.data_ptr(), idx.data_ptr<unsigned char>(), xc.data_ptr(),
      mean.data_ptr<float>(), invstd.data_ptr<float>(),
      gf.data_ptr<float>(), bf.data_ptr<float>(), sums.data_ptr<float>(),
      dx.data_ptr(), N, C, H, W, (int)Ho, (int)Wo, (int)ks, (int)stride,
      (int)pad, bf16, cur_stream());
  auto dbeta = sums.select(1, 0).clone();
  auto dgamma = sums.select(1, 1).clone();
  return {dx, dgamma, dbeta};
}

// ---------------- MFMA backward (csrc/conv_bwd.hip, conv_bwd_s2.hip) -----
// Argument handling shared by the stride-1 and stride-2 entry points;
// `who` is the python-visible name, for the message.

static void check_grad_bf16_cl(const at::Tensor& g, const char* who) {
  TORCH_CHECK(g.is_cuda() && g.dim() == 4 &&
                  g.scalar_type() == at::kBFloat16,
              who, ": g must be a 4-D bf16 CUDA tensor");
  TORCH_CHECK(g.is_contiguous(at::MemoryFormat::ChannelsLast), who,
              ": g must be channels_last");
}

// the saved activation of the value-mask modes, read at dx's address
static void check_act_bf16_cl(const at::Tensor& x, int64_t N, int64_t C,
                              int64_t H, int64_t W, const char* who) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 &&
                  x.scalar_type() == at::kBFloat16,
              who, ": x must be a 4-D bf16 CUDA tensor");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast), who,
              ": x must be channels_last");
  TORCH_CHECK(x.size(0) == N && x.size(1) == C && x.size(2) == H &&
                  x.size(3) == W,
              who, ": x shape must match dx (N,C,H,W)");
}

// the deferred skip gradient as the kernels read it (bf16 channels_last,
// dx's shape); undefined when there is none.  The caller holds the
// returned tensor until its launch is queued.
static at::Tensor acc_as_bf16_cl(const c10::optional<at::Tensor>& acc,
                                 int64_t N, int64_t C, int64_t H, int64_t W,
                                 const char* who) {
  if (!acc.has_value()) return at::Tensor();
  at::Tensor ac =
      acc->scalar_type() == at::kBFloat16
          ? acc->contiguous(at::MemoryFormat::ChannelsLast)
          : acc->to(at::kBFloat16).contiguous(at::MemoryFormat::ChannelsLast);
  TORCH_CHECK(ac.is_cuda() && ac.dim() == 4 && ac.size(0) == N &&
                  ac.size(1) == C && ac.size(2) == H && ac.size(3) == W,
              who, ": acc shape must match dx (N,C,H,W)");
  return ac;
}

static at::Tensor empty_dx(const at::Tensor& g, int64_t N, int64_t C,
                           int64_t H, int64_t W) {
  return at::empty({N, C, H, W}, g.options(),
                   at::MemoryFormat::ChannelsLast);
}

// packed bits -> mirrored transposed +-alpha bf16 [ks*ks][C][K]
static at::Tensor dgrad_wdec_impl(const at::Tensor& wp,
                                  const at::Tensor& alpha, int64_t C,
                                  int64_t ks, const char* who) {
  TORCH_CHECK(wp.is_cuda() && wp.dim() == 4 && wp.size(1) == ks &&
                  wp.size(2) == ks && wp.scalar_type() == at::kInt,
              who, ": wp must be packed ", ks, "x", ks,
              " weights [K][ks][ks][CW] int32");
  int K = (int)wp.size(0);
  TORCH_CHECK(K % 8 == 0 && (C % 32 == 0 || C == 16) &&
                  wp.size(3) == (C + 31) / 32,
              who, ": C must match wp (K%8, C%32 or C = 16)");
  TORCH_CHECK(alpha.is_cuda() && alpha.scalar_type() == at::kFloat &&
                  alpha.numel() == K,
              who, ": alpha must be fp32 [K]");
  auto wd = at::empty({ks * ks, C, K}, wp.options().dtype(at::kBFloat16));
  auto al = alpha.contiguous();
  auto wpc = wp.contiguous();
  bdbnn_dgrad_wdec((const uint32_t*)wpc.data_ptr<int>(),
                   al.data_ptr<float>(), wd.data_ptr(), (int)C, K,
                   (int)(ks * ks), cur_stream());
  return wd;
}

at::Tensor dgrad_weight_decode(const at::Tensor& wp, const at::Tensor& alpha,
                               int64_t C) {
  return dgrad_wdec_impl(wp, alpha, C, 3, "dgrad_weight_decode");
}

at::Tensor dgrad_weight_decode_1x1(const at::Tensor& wp,
                                   const at::Tensor& alpha, int64_t C) {
  return dgrad_wdec_impl(wp, alpha, C, 1, "dgrad_weight_decode_1x1");
}

// activation sign bits -> per-channel u64 row planes [C][N*H]; parity:
// columns split even (low word) / odd (high word) for the stride-2 wgrad
static at::Tensor repack_cplane_impl(const at::Tensor& xp, int64_t C,
                                     c10::optional<int64_t> H, int64_t W,
                                     bool parity, const char* who) {
  TORCH_CHECK(xp.is_cuda() && xp.dim() == 4 &&
                  xp.scalar_type() == at::kInt && xp.is_contiguous(),
              who, ": xp must be contiguous int32 [N][H][W][CW]");
  TORCH_CHECK(xp.size(3) == (C + 31) / 32, who,
              ": C does not match xp's word count");
  TORCH_CHECK((!H.has_value() || xp.size(1) == *H) && xp.size(2) == W, who,
              ": H, W do not match xp");
  TORCH_CHECK(W >= 1 && W <= 64, who, ": W must be <= 64");
  int NH = (int)(xp.size(0) * xp.size(1));
  auto planes = at::empty({C, NH}, xp.options().dtype(at::kLong));
  bdbnn_repack_cplane((const uint32_t*)xp.data_ptr<int>(),
                      (uint64_t*)planes.data_ptr<int64_t>(), NH, (int)W,
                      (int)C, (int)xp.size(3), parity, cur_stream());
  return planes;
}

at::Tensor repack_cplane(const at::Tensor& xp, int64_t C, int64_t W) {
  return repack_cplane_impl(xp, C, c10::nullopt, W, false, "repack_cplane");
}

at::Tensor repack_cplane_s2(const at::Tensor& xp, int64_t C, int64_t H,
                            int64_t W) {
  return repack_cplane_impl(xp, C, H, W, true, "repack_cplane_s2");
}

// dw[K][C][ks][ks] = sum of the wgrad slabs, transposed, |w|<=1 STE mask
static at::Tensor wgrad_finish_impl(const at::Tensor& dwT,
                                    const at::Tensor& w, bool allow_1x1,
                                    const char* who) {
  TORCH_CHECK(w.is_cuda() && w.dim() == 4 && w.size(2) == w.size(3) &&
                  (w.size(2) == 3 || (allow_1x1 && w.size(2) == 1)) &&
                  w.scalar_type() == at::kFloat,
              who, ": w must be fp32 [K][C][ks][ks], ks ",
              allow_1x1 ? "in {1,3}" : "= 3");
  int K = (int)w.size(0), C = (int)w.size(1);
  int T = (int)(w.size(2) * w.size(3));
  TORCH_CHECK(dwT.is_cuda() && dwT.dim() == 4 && dwT.size(1) == T &&
                  dwT.size(2) == C && dwT.size(3) == K &&
                  dwT.scalar_type() == at::kFloat,
              who, ": dwT must be fp32 [nslab][ks*ks][C][K]");
  auto wc = w.contiguous();
  auto dw = at::empty_like(wc);
  bdbnn_wgrad_finish(dwT.contiguous().data_ptr<float>(),
                     wc.data_ptr<float>(), dw.data_ptr<float>(), C, K, T,
                     (int)dwT.size(0), cur_stream());
  return dw;
}

at::Tensor wgrad_finish(const at::Tensor& dwT, const at::Tensor& w) {
  return wgrad_finish_impl(dwT, w, false, "wgrad_finish");
}

at::Tensor wgrad_finish_s2(const at::Tensor& dwT, const at::Tensor& w) {
  return wgrad_finish_impl(dwT, w, true, "wgrad_finish_s2");
}

// ---------------- stride 1 (3x3/s1/p1) ----------------

// dx with the mask in the epilogue: mode 0 reads the clip-STE bitplane
// mp, modes 1 (ReAct polynomial) / 2 (EDE) evaluate the value mask of
// the saved bf16 activation x
static at::Tensor conv_dgrad2_impl(const at::Tensor& g, const at::Tensor& wd,
                                   const at::Tensor* mp, const at::Tensor* x,
                                   int64_t C, int64_t mode, double t,
                                   double k,
                                   const c10::optional<at::Tensor>& acc,
                                   const char* who) {
  check_grad_bf16_cl(g, who);
  int N = (int)g.size(0), K = (int)g.size(1);
  int H = (int)g.size(2), W = (int)g.size(3);
  TORCH_CHECK(wd.is_cuda() && wd.dim() == 3 && wd.size(0) == 9 &&
                  wd.size(1) == C && wd.size(2) == K &&
                  wd.scalar_type() == at::kBFloat16 && wd.is_contiguous(),
              who, ": decoded weights [9][C][K] bf16");
  if (mp) {
    TORCH_CHECK(mp->size(-1) == C / 32 &&
                    mp->numel() == (int64_t)N * H * W * (C / 32),
                who, ": mask bitplane [...P...][C/32]");
  } else {
    check_act_bf16_cl(*x, N, C, H, W, who);
  }
  TORCH_CHECK(bdbnn_dgrad2_supported(H, W, (int)C, K) != 0, who,
              ": unsupported shape");
  at::Tensor ac = acc_as_bf16_cl(acc, N, C, H, W, who);
  auto dx = empty_dx(g, N, C, H, W);
  int rc = bdbnn_conv_dgrad2(
      g.data_ptr(), wd.data_ptr(),
      mp ? (const uint32_t*)mp->data_ptr<int>() : nullptr,
      x ? x->data_ptr() : nullptr, dx.data_ptr(),
      ac.defined() ? ac.data_ptr() : nullptr, (int)mode, (float)t, (float)k,
      N, H, W, (int)C, K, cur_stream());
  TORCH_CHECK(rc == 0, who, ": launch rejected the shape");
  return dx;
}

at::Tensor conv_dgrad2(const at::Tensor& g, const at::Tensor& wd,
                       const at::Tensor& mp, int64_t C,
                       const c10::optional<at::Tensor>& acc) {
  return conv_dgrad2_impl(g, wd, &mp, nullptr, C, 0, 0.0, 0.0, acc,
                          "conv_dgrad2");
}

at::Tensor conv_dgrad2_x(const at::Tensor& g, const at::Tensor& wd,
                         const at::Tensor& x, int64_t C, int64_t mode,
                         double t, double k,
                         const c10::optional<at::Tensor>& acc) {
  TORCH_CHECK(mode == 1 || mode == 2,
              "conv_dgrad2_x: mode must be 1 (approx) or 2 (EDE)");
  return conv_dgrad2_impl(g, wd, nullptr, &x, C, mode, t, k, acc,
                          "conv_dgrad2_x");
}

at::Tensor conv_wgrad2(const at::Tensor& g, const at::Tensor& xcp,
                       int64_t C) {
  check_grad_bf16_cl(g, "conv_wgrad2");
  int N = (int)g.size(0), K = (int)g.size(1);
  int H = (int)g.size(2), W = (int)g.size(3);
  TORCH_CHECK(xcp.dim() == 2 && xcp.size(0) == C &&
                  xcp.size(1) == (int64_t)N * H,
              "conv_wgrad2: c-plane bitplanes [C][N*H]");
  TORCH_CHECK(C % 64 == 0 && K % 64 == 0 && W <= 64,
              "conv_wgrad2: unsupported shape");
  int nslab = bdbnn_wgrad2_nslab(N, H, W, (int)C, K);
  TORCH_CHECK(nslab > 0, "conv_wgrad2: unsupported shape");
  // per-m-split-block partial slabs; every word is written (no memset)
  auto dwT = at::empty({nslab, 9, C, K}, g.options().dtype(at::kFloat));
  int rc = bdbnn_conv_wgrad2(g.data_ptr(),
                             (const uint64_t*)xcp.data_ptr<int64_t>(),
                             dwT.data_ptr<float>(), N, H, W, (int)C, K,
                             cur_stream());
  TORCH_CHECK(rc == 0, "conv_wgrad2: launch rejected the shape");
  return dwT;
}

// the same weight gradient straight from the NHWC sign plane xp
// [N][H][W][C/32] (csrc/conv_wgrad3.hip); slabs as conv_wgrad2's
at::Tensor conv_wgrad3(const at::Tensor& g, const at::Tensor& xp,
                       int64_t C) {
  check_grad_bf16_cl(g, "conv_wgrad3");
  int N = (int)g.size(0), K = (int)g.size(1);
  int H = (int)g.size(2), W = (int)g.size(3);
  TORCH_CHECK(C >= 64 && C % 64 == 0 && K % 64 == 0 && W <= 64,
              "conv_wgrad3: unsupported shape");
  TORCH_CHECK(xp.is_cuda() && xp.dim() == 4 &&
                  xp.scalar_type() == at::kInt && xp.is_contiguous() &&
                  xp.size(0) == N && xp.size(1) == H && xp.size(2) == W &&
                  xp.size(3) == C / 32,
              "conv_wgrad3: xp must be contiguous int32 [N][H][W][C/32]");
  int nslab = bdbnn_wgrad3_nslab(N, H, W, (int)C, K);
  TORCH_CHECK(nslab > 0, "conv_wgrad3: unsupported shape");
  // per-m-split-block partial slabs; every word is written (no memset)
  auto dwT = at::empty({nslab, 9, C, K}, g.options().dtype(at::kFloat));
  int rc = bdbnn_conv_wgrad3(g.data_ptr(),
                             (const uint32_t*)xp.data_ptr<int>(),
                             dwT.data_ptr<float>(), N, H, W, (int)C, K,
                             cur_stream());
  TORCH_CHECK(rc == 0, "conv_wgrad3: launch rejected the shape");
  return dwT;
}

// ---------------- stride 1, C and K in {16, 32} (conv_bwd_small.hip) -----

// conv_dgrad2's dx for the 16/32-channel convs: mode 0 masks with the
// bitplane mp ([N][H][W][1], bits c < C), modes 1/2 with the value mask of
// the saved activation x
at::Tensor conv_dgrad_small(const at::Tensor& g, const at::Tensor& wd,
                            int64_t C, int64_t mode,
                            const c10::optional<at::Tensor>& mp,
                            const c10::optional<at::Tensor>& x, double t,
                            double k, const c10::optional<at::Tensor>& acc) {
  const char* who = "conv_dgrad_small";
  check_grad_bf16_cl(g, who);
  int64_t N = g.size(0), K = g.size(1), H = g.size(2), W = g.size(3);
  TORCH_CHECK((C == 16 || C == 32) && (K == 16 || K == 32) && W <= 64 &&
                  H <= (1 << 20) && N * H * W < (int64_t(1) << 31),
              who, ": unsupported shape (C, K in {16, 32}, W <= 64)");
  TORCH_CHECK(wd.is_cuda() && wd.dim() == 3 && wd.size(0) == 9 &&
                  wd.size(1) == C && wd.size(2) == K &&
                  wd.scalar_type() == at::kBFloat16 && wd.is_contiguous(),
              who, ": decoded weights [9][C][K] bf16");
  TORCH_CHECK(mode >= 0 && mode <= 2, who,
              ": mode must be 0 (clip-STE), 1 (approx) or 2 (EDE)");
  const uint32_t* mp_ptr = nullptr;
  const void* x_ptr = nullptr;
  if (mode == 0) {
    TORCH_CHECK(mp.has_value() && !x.has_value(), who,
                ": mode 0 needs mp and x=None");
    TORCH_CHECK(mp->is_cuda() && mp->scalar_type() == at::kInt &&
                    mp->is_contiguous() && mp->size(-1) == 1 &&
                    mp->numel() == N * H * W,
                who, ": mp must be the int32 mask bitplane [N,H,W,1]");
    mp_ptr = (const uint32_t*)mp->data_ptr<int>();
  } else {
    TORCH_CHECK(x.has_value() && !mp.has_value(), who,
                ": modes 1/2 need x and mp=None");
    check_act_bf16_cl(*x, N, C, H, W, who);
    x_ptr = x->data_ptr();
  }
  at::Tensor ac = acc_as_bf16_cl(acc, N, C, H, W, who);
  auto dx = empty_dx(g, N, C, H, W);
  int rc = bdbnn_conv_dgrad_small(
      g.data_ptr(), wd.data_ptr(), mp_ptr, x_ptr, dx.data_ptr(),
      ac.defined() ? ac.data_ptr() : nullptr, (int)mode, (float)t, (float)k,
      (int)N, (int)H, (int)W, (int)C, (int)K, cur_stream());
  TORCH_CHECK(rc == 0, who, ": launch rejected the shape");
  return dx;
}

// conv_wgrad3's slabs for the 16/32-channel convs, from the NHWC sign
// plane xp [N][H][W][1].  fold: more than 8 block slabs are summed into one
// by a slab-parallel pass before they are returned (wgrad_finish walks the
// slabs serially); fold = false returns the block slabs as written.
at::Tensor conv_wgrad_small(const at::Tensor& g, const at::Tensor& xp,
                            int64_t C, bool fold) {
  const char* who = "conv_wgrad_small";
  check_grad_bf16_cl(g, who);
  int64_t N = g.size(0), K = g.size(1), H = g.size(2), W = g.size(3);
  TORCH_CHECK((C == 16 || C == 32) && (K == 16 || K == 32) && W <= 64 &&
                  H <= (1 << 20) && N * H * W < (int64_t(1) << 31),
              who, ": unsupported shape (C, K in {16, 32}, W <= 64)");
  TORCH_CHECK(xp.is_cuda() && xp.dim() == 4 &&
                  xp.scalar_type() == at::kInt && xp.is_contiguous() &&
                  xp.size(0) == N && xp.size(1) == H && xp.size(2) == W &&
                  xp.size(3) == 1,
              who, ": xp must be contiguous int32 [N][H][W][1]");
  int nslab = bdbnn_wgrad_small_nslab((int)N, (int)H, (int)W, (int)C, (int)K);
  TORCH_CHECK(nslab > 0, who, ": unsupported shape");
  // per-block partial slabs; every word is written (no memset)
  auto dwT = at::empty({nslab, 9, C, K}, g.options().dtype(at::kFloat));
  int rc = bdbnn_conv_wgrad_small(g.data_ptr(),
                                  (const uint32_t*)xp.data_ptr<int>(),
                                  dwT.data_ptr<float>(), (int)N, (int)H,
                                  (int)W, (int)C, (int)K, cur_stream());
  TORCH_CHECK(rc == 0, who, ": launch rejected the shape");
  if (!fold || nslab <= 8) return dwT;
  auto one = at::empty({1, 9, C, K}, dwT.options());
  bdbnn_wgrad_small_fold(dwT.data_ptr<float>(), one.data_ptr<float>(), nslab,
                         (int)C, (int)K, cur_stream());
  return one;
}

// ---------------- stride 2 (3x3/s2/p1, 1x1/s2/p0) ----------------

// shape predicates of the stride-2 path; H, W are the INPUT (dx) size,
// ks the kernel size (3 -> pad 1, 1 -> pad 0).  dgrad2_s2_ok: what the
// kernels can run (argument check of the entry points);
// dgrad2_s2_routed: the routing predicate exposed to python, which also
// excludes the shapes measured slower than the fallback
static bool s2_dims_sane(int64_t H, int64_t W, int64_t C, int64_t K) {
  return H >= 1 && W >= 1 && H <= (1 << 20) && C <= (1 << 20) &&
         K <= (1 << 20);
}
static bool dgrad2_s2_ok(int64_t H, int64_t W, int64_t C, int64_t K,
                         int64_t ks) {
  return s2_dims_sane(H, W, C, K) &&
         bdbnn_s2_kernels_can_run((int)H, (int)W, (int)C, (int)K,
                                  (int)ks) != 0;
}
static bool dgrad2_s2_routed(int64_t H, int64_t W, int64_t C, int64_t K,
                             int64_t ks) {
  return s2_dims_sane(H, W, C, K) &&
         bdbnn_dgrad2_s2_supported((int)H, (int)W, (int)C, (int)K,
                                   (int)ks) != 0;
}

// dx of a 3x3/s2/p1 (wd [9][C][K]) or 1x1/s2/p0 (wd [1][C][K]) conv at
// input size (H, W); mode 0 masks with the bitplane mp, modes 1/2 with
// the value mask of the saved activation x
at::Tensor conv_dgrad2_s2(const at::Tensor& g, const at::Tensor& wd,
                          int64_t H, int64_t W, int64_t C, int64_t mode,
                          const c10::optional<at::Tensor>& mp,
                          const c10::optional<at::Tensor>& x, double t,
                          double k, const c10::optional<at::Tensor>& acc) {
  const char* who = "conv_dgrad2_s2";
  check_grad_bf16_cl(g, who);
  int N = (int)g.size(0), K = (int)g.size(1);
  TORCH_CHECK(wd.is_cuda() && wd.dim() == 3 &&
                  wd.scalar_type() == at::kBFloat16 && wd.is_contiguous(),
              "conv_dgrad2_s2: wd must be contiguous bf16 [ks*ks][C][K]");
  TORCH_CHECK(wd.size(0) == 9 || wd.size(0) == 1,
              "conv_dgrad2_s2: wd.size(0) must be 9 (3x3) or 1 (1x1)");
  int ks = wd.size(0) == 9 ? 3 : 1;
  TORCH_CHECK(wd.size(1) == C && wd.size(2) == K,
              "conv_dgrad2_s2: wd must be [ks*ks][C][K] for this g and C");
  TORCH_CHECK(dgrad2_s2_ok(H, W, C, K, ks),
              "conv_dgrad2_s2: unsupported shape (H, W, C, K, ks)");
  int64_t Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  TORCH_CHECK(g.size(2) == Ho && g.size(3) == Wo,
              "conv_dgrad2_s2: g spatial size must be the (Ho, Wo) implied "
              "by (H, W, ks)");
  TORCH_CHECK(mode >= 0 && mode <= 2,
              "conv_dgrad2_s2: mode must be 0 (clip-STE), 1 (approx) or 2 "
              "(EDE)");
  const uint32_t* mp_ptr = nullptr;
  const void* x_ptr = nullptr;
  if (mode == 0) {
    TORCH_CHECK(mp.has_value() && !x.has_value(),
                "conv_dgrad2_s2: mode 0 needs mp and x=None");
    TORCH_CHECK(mp->is_cuda() && mp->scalar_type() == at::kInt &&
                    mp->is_contiguous() && mp->size(-1) == C / 32 &&
                    mp->numel() == (int64_t)N * H * W * (C / 32),
                "conv_dgrad2_s2: mp must be the int32 mask bitplane "
                "[N,H,W,C/32] at input resolution");
    mp_ptr = (const uint32_t*)mp->data_ptr<int>();
  } else {
    TORCH_CHECK(x.has_value() && !mp.has_value(),
                "conv_dgrad2_s2: modes 1/2 need x and mp=None");
    check_act_bf16_cl(*x, N, C, H, W, who);
    x_ptr = x->data_ptr();
  }
  at::Tensor ac = acc_as_bf16_cl(acc, N, C, H, W, who);
  auto dx = empty_dx(g, N, C, H, W);
  int rc = bdbnn_conv_dgrad2_s2(g.data_ptr(), wd.data_ptr(), mp_ptr, x_ptr,
                                dx.data_ptr(),
                                ac.defined() ? ac.data_ptr() : nullptr, ks,
                                (int)mode, (float)t, (float)k, N, (int)H,
                                (int)W, (int)C, K, cur_stream());
  TORCH_CHECK(rc == 0, "conv_dgrad2_s2: launch rejected the shape");
  return dx;
}

at::Tensor conv_wgrad2_s2(const at::Tensor& g, const at::Tensor& planes,
                          int64_t C, int64_t H, int64_t W, int64_t ks) {
  check_grad_bf16_cl(g, "conv_wgrad2_s2");
  int N = (int)g.size(0), K = (int)g.size(1);
  TORCH_CHECK(dgrad2_s2_ok(H, W, C, K, ks),
              "conv_wgrad2_s2: unsupported shape (H, W, C, K, ks)");
  TORCH_CHECK(g.size(2) == (H + 1) / 2 && g.size(3) == (W + 1) / 2,
              "conv_wgrad2_s2: g spatial size must be the (Ho, Wo) implied "
              "by (H, W, ks)");
  TORCH_CHECK(planes.is_cuda() && planes.dim() == 2 &&
                  planes.scalar_type() == at::kLong &&
                  planes.is_contiguous() && planes.size(0) == C &&
                  planes.size(1) == (int64_t)N * H,
              "conv_wgrad2_s2: planes must be int64 [C][N*H] "
              "(repack_cplane_s2)");
  int nslab = bdbnn_wgrad2_s2_nslab(N, (int)H, (int)W, (int)C, K, (int)ks);
  TORCH_CHECK(nslab > 0, "conv_wgrad2_s2: unsupported shape");
  // per-m-split-block partial slabs; every word is written (no memset)
  auto dwT = at::empty({nslab, ks * ks, C, K},
                       g.options().dtype(at::kFloat));
  int rc = bdbnn_conv_wgrad2_s2(g.data_ptr(),
                                (const uint64_t*)planes.data_ptr<int64_t>(),
                                dwT.data_ptr<float>(), (int)ks, N, (int)H,
                                (int)W, (int)C, K, cur_stream());
  TORCH_CHECK(rc == 0, "conv_wgrad2_s2: launch rejected the shape");
  return dwT;
}

// ---------------- kurtosis ----------------

std::vector<at::Tensor> kurtosis_fwd(const std::vector<at::Tensor>& ws,
                                     const at::Tensor& targets) {
  auto meta = make_meta(ws);
  auto dev = ws[0].device();
  auto sched = build_schedule(ws, BDBNN_CHUNK_ELEMS, dev);
  int L = (int)ws.size();
  auto opts = ws[0].options();
  auto mom = at::zeros({L, 4}, opts.dtype(at::kDouble));
  auto stats = at::empty({L, 4}, opts);
  auto losses = at::empty({L}, opts);
  auto kurts = at::empty({L}, opts);
  auto tgt = targets.to(dev, at::kFloat).contiguous();
  bdbnn_kurtosis_fwd(&meta, sched.bt.data_ptr<int>(),
                     sched.bo.data_ptr<int64_t>(), sched.n_blocks,
                     mom.data_ptr<double>(), tgt.data_ptr<float>(),
                     stats.data_ptr<float>(), losses.data_ptr<float>(),
                     kurts.data_ptr<float>(), cur_stream());
  return {losses, kurts, stats};
}

std::vector<at::Tensor> kurtosis_bwd(const std::vector<at::Tensor>& ws,
                                     const at::Tensor& stats,
                                     const at::Tensor& targets,
                                     const at::Tensor& gscale) {
  auto meta = make_meta(ws);
  auto dev = ws[0].device();
  auto sched = build_schedule(ws, BDBNN_CHUNK_ELEMS, dev);
  std::vector<at::Tensor> grads;
  for (auto& w : ws)  // preserve_format: grad layout == weight layout
    grads.push_back(at::empty_like(w, w.options(),
                                   at::MemoryFormat::Preserve));
  auto gp = make_ptrs(grads, meta, ws);
  auto tgt = targets.to(dev, at::kFloat).contiguous();
  auto st = stats.contiguous();
  // gscale is a 0-dim DEVICE tensor: no host sync in the backward
  auto gs = gscale.to(dev, at::kFloat).contiguous();
  bdbnn_kurtosis_bwd(&meta, &gp, sched.bt.data_ptr<int>(),
                     sched.bo.data_ptr<int64_t>(), sched.n_blocks,
                     st.data_ptr<float>(), tgt.data_ptr<float>(),
                     gs.data_ptr<float>(), cur_stream());
  return grads;
}

// ---------------- weight KD ----------------

at::Tensor weight_kd_fwd(const std::vector<at::Tensor>& ws,
                         const std::vector<at::Tensor>& wt) {
  auto meta = make_meta(ws);
  auto sched = build_schedule(ws, BDBNN_CHUNK_ELEMS, ws[0].device());
  auto s_ptr = make_ptrs(ws, meta, ws);
  // the teacher as given: ops/kd.py aligns its layout to the student's,
  // and make_ptrs rejects a pair whose layouts differ
  auto t_ptr = make_ptrs(wt, meta, ws);
  auto out = at::zeros({}, ws[0].options().dtype(at::kDouble));
  bdbnn_weight_kd_fwd(&meta, &s_ptr, &t_ptr, sched.bt.data_ptr<int>(),
                      sched.bo.data_ptr<int64_t>(), sched.n_blocks,
                      out.data_ptr<double>(), cur_stream());
  return out.to(at::kFloat);
}

std::vector<at::Tensor> weight_kd_bwd(const std::vector<at::Tensor>& wt,
                                      const at::Tensor& gscale) {
  auto meta = make_meta(wt);
  auto sched = build_schedule(wt, BDBNN_CHUNK_ELEMS, wt[0].device());
  auto t_ptr = make_ptrs(wt, meta, wt);
  std::vector<at::Tensor> grads;
  for (auto& t : wt)
    grads.push_back(at::empty_like(t, t.options(),
                                   at::MemoryFormat::Preserve));
  auto gp = make_ptrs(grads, meta, wt);
  auto gs = gscale.to(wt[0].device(), at::kFloat).contiguous();
  bdbnn_weight_kd_bwd(&meta, &t_ptr, &gp, sched.bt.data_ptr<int>(),
                      sched.bo.data_ptr<int64_t>(), sched.n_blocks,
                      gs.data_ptr<float>(), cur_stream());
  return grads;
}

// ---------------- fused optimizers ----------------

void fused_sgd(const std::vector<at::Tensor>& p,
               const std::vector<at::Tensor>& g,
               const std::vector<at::Tensor>& buf, double lr, double momentum,
               double wd) {
  auto meta = make_meta(p);
  auto sched = build_schedule(p, BDBNN_CHUNK_ELEMS, p[0].device());
  auto pp = make_ptrs(p, meta, p);
  auto gg = make_ptrs(g, meta, p);  // python aligns grad layout to the param's
  auto bb = make_ptrs(buf, meta, p);
  bdbnn_fused_sgd(&meta, &pp, &gg, &bb, sched.bt.data_ptr<int>(),
                  sched.bo.data_ptr<int64_t>(), sched.n_blocks, (float)lr,
                  (float)momentum, (float)wd, cur_stream());
}

void fused_adam(const std::vector<at::Tensor>& p,
                const std::vector<at::Tensor>& g,
                const std::vector<at::Tensor>& m1,
                const std::vector<at::Tensor>& m2, double lr, double beta1,
                double beta2, double eps, double wd, double bc1, double bc2) {
  auto meta = make_meta(p);
  auto sched = build_schedule(p, BDBNN_CHUNK_ELEMS, p[0].device());
  auto pp = make_ptrs(p, meta, p);
  auto gg = make_ptrs(g, meta, p);  // python aligns grad layout to the param's
  auto mm1 = make_ptrs(m1, meta, p);
  auto mm2 = make_ptrs(m2, meta, p);
  bdbnn_fused_adam(&meta, &pp, &gg, &mm1, &mm2, sched.bt.data_ptr<int>(),
                   sched.bo.data_ptr<int64_t>(), sched.n_blocks, (float)lr,
                   (float)beta1, (float)beta2, (float)eps, (float)wd,
                   (float)bc1, (float)bc2, cur_stream());
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("sign_pack_nhwc", &sign_pack_nhwc, "sign+bitpack NHWC activations");
  m.def("weight_pack", &weight_pack,
        "pack conv weights -> (bits, alpha, pad-correction table)");
  m.def("binsign_decode", &binsign_decode, "elementwise +-1 decode");
  m.def("ste_mask_mul", &ste_mask_mul, "quantizer backward mask multiply");
  m.def("sign_mask_pack_nhwc", &sign_mask_pack_nhwc,
        "pack sign + clip-STE mask bitplanes in one pass");
  m.def("decode_packed", &decode_packed, "packed signs -> +-1 NHWC tensor");
  m.def("mask_mul_packed", &mask_mul_packed, "dx = mask_bit ? g : 0");
  m.def("weight_decode", &weight_decode, "packed weights -> alpha*(+-1)");
  m.def("xnor_conv_fwd", &xnor_conv_fwd,
        "binary conv forward (i8 MFMA or XNOR+popcount, by the routing "
        "table)");
  m.def("xnor_mfma_supported", &xnor_mfma_supported,
        "(C, K, KH, KW, stride, pad): can the i8 MFMA forward run it");
  m.def("xnor_conv_mfma_fwd", &xnor_conv_mfma_fwd,
        "binary conv forward, i8 MFMA kernel forced");
  m.def("xnor_conv_valu_fwd", &xnor_conv_valu_fwd,
        "binary conv forward, XNOR+popcount kernel forced");
  m.def("xnor_route_calls", &xnor_route_calls,
        "(MFMA, VALU) forward conv calls since load");
  m.def("bn_fold", &bn_fold,
        "eval BN folded as bn_act_eval does it -> (sc, sh) fp32 [C]; b1 "
        "(RPReLU) is added to sh",
        py::arg("gamma"), py::arg("beta"), py::arg("rm"), py::arg("rv"),
        py::arg("eps"), py::arg("b1") = py::none());
  m.def("xnor_conv_bn_act_fwd", &xnor_conv_bn_act_fwd,
        "inference: i8 MFMA binary conv + folded BN (+ skip) + act in one "
        "kernel -> [out, sign plane of out | None]",
        py::arg("xp"), py::arg("wp"), py::arg("alpha"), py::arg("sc"),
        py::arg("sh"), py::arg("a"), py::arg("b2"), py::arg("skip"),
        py::arg("C"), py::arg("stride"), py::arg("pad"), py::arg("act_kind"),
        py::arg("out_bf16"), py::arg("want_pack"));
  m.def("xnor_fused_calls", &xnor_fused_calls,
        "launches of xnor_conv_bn_act_fwd since load");
  m.def("stem_conv_fwd", &stem_conv_fwd,
        "MFMA 7x7/2 stem conv fwd (returns out, packed x4)");
  m.def("stem_conv_wrw", &stem_conv_wrw, "MFMA stem conv weight grad");
  m.def("kd_logit_fwd", &kd_logit_fwd, "fused logit-KD fwd");
  m.def("kd_logit_bwd", &kd_logit_bwd, "fused logit-KD bwd");
  m.def("ce_fwd", &ce_fwd, "fused cross-entropy fwd");
  m.def("ce_bwd", &ce_bwd, "fused cross-entropy bwd");
  m.def("maxpool_fwd", &maxpool_fwd, "fused NHWC maxpool fwd (+u8 idx)");
  m.def("maxpool_bwd", &maxpool_bwd, "gather-based NHWC maxpool bwd");
  m.def("prelu_fwd", &prelu_fwd, "fused NHWC per-channel PReLU fwd");
  m.def("prelu_bwd", &prelu_bwd, "fused NHWC per-channel PReLU bwd");
  m.def("bn_act_fwd_train", &bn_act_fwd_train,
        "fused BN(+add)(+act) training forward -> [out, z, mean, invstd(, "
        "xpk, mpk)]; act_kind 3 (RPReLU) takes b1, b2 and stores u = z + b1 "
        "as z",
        py::arg("x"), py::arg("skip"), py::arg("gamma"), py::arg("beta"),
        py::arg("a"), py::arg("running_mean"), py::arg("running_var"),
        py::arg("momentum"), py::arg("eps"), py::arg("act_kind"),
        py::arg("pre_s1"), py::arg("pre_s2"), py::arg("want_pack"),
        py::arg("b1") = py::none(), py::arg("b2") = py::none());
  m.def("bn_act_bwd", &bn_act_bwd,
        "fused BN(+add)(+act) backward -> [dx, dskip, dgamma, dbeta, da]; "
        "act_kind 3 appends db1, db2");
  m.def("bn_act_eval", &bn_act_eval, "fused BN(+add)(+act) eval forward",
        py::arg("x"), py::arg("skip"), py::arg("gamma"), py::arg("beta"),
        py::arg("a"), py::arg("rm"), py::arg("rv"), py::arg("eps"),
        py::arg("act_kind"), py::arg("b1") = py::none(),
        py::arg("b2") = py::none());
  m.def("bn_relu_maxpool_fwd_train", &bn_relu_maxpool_fwd_train,
        "fused BN + ReLU + maxpool training forward -> [out, idx, mean, "
        "invstd(, xpk, mpk)]",
        py::arg("x"), py::arg("gamma"), py::arg("beta"),
        py::arg("running_mean"), py::arg("running_var"),
        py::arg("momentum"), py::arg("eps"), py::arg("ks"),
        py::arg("stride"), py::arg("pad"), py::arg("pre_s1") = py::none(),
        py::arg("pre_s2") = py::none(), py::arg("want_pack") = false);
  m.def("bn_relu_maxpool_bwd", &bn_relu_maxpool_bwd,
        "fused BN + ReLU + maxpool backward -> [dx, dgamma, dbeta]");
  m.def("conv_dgrad2", &conv_dgrad2,
        "MFMA bf16 dgrad v2: halo-staged 9-tap implicit GEMM with fused "
        "clip-STE mask (3x3/s1/p1); optional acc adds a same-shape "
        "skip-gradient tensor in the epilogue",
        py::arg("g"), py::arg("wd"), py::arg("mp"), py::arg("C"),
        py::arg("acc") = py::none());
  m.def("conv_dgrad2_x", &conv_dgrad2_x,
        "conv_dgrad2 with a value mask of the saved bf16 activation x in "
        "the epilogue: mode 1 = ReAct polynomial, 2 = EDE(t, k)",
        py::arg("g"), py::arg("wd"), py::arg("x"), py::arg("C"),
        py::arg("mode"), py::arg("t"), py::arg("k"),
        py::arg("acc") = py::none());
  m.def("dgrad_weight_decode", &dgrad_weight_decode,
        "packed bits -> mirrored transposed +-alpha bf16 [9][C][K]");
  m.def("dgrad2_supported",
        [](int64_t H, int64_t W, int64_t C, int64_t K) {
          return bdbnn_dgrad2_supported((int)H, (int)W, (int)C, (int)K) !=
                 0;
        },
        "shape support predicate for conv_dgrad2");
  m.def("conv_wgrad2", &conv_wgrad2,
        "MFMA bf16 wgrad v2: all-9-tap block GEMM from sign BITS "
        "(3x3/s1/p1) -> fp32 [9][C][K]");
  m.def("conv_wgrad3", &conv_wgrad3,
        "MFMA bf16 wgrad v3: pipelined all-9-tap block GEMM from the NHWC "
        "sign plane, transposed LDS reads (3x3/s1/p1) -> fp32 "
        "[nslab][9][C][K]");
  m.def("wgrad3_supported",
        [](int64_t H, int64_t W, int64_t C, int64_t K) {
          return bdbnn_wgrad3_supported((int)H, (int)W, (int)C, (int)K) !=
                 0;
        },
        "shape predicate of the conv_wgrad3 route");
  m.def("repack_cplane", &repack_cplane,
        "activation sign bits -> padded per-channel u64 row planes");
  m.def("wgrad_finish", &wgrad_finish,
        "dwT transpose to [K][C][3][3] + |w|<=1 STE mask, one pass");
  m.def("conv_dgrad_small", &conv_dgrad_small,
        "MFMA bf16 dgrad of a 3x3/s1/p1 binary conv with C and K in "
        "{16, 32} (wd [9][C][K]); mode 0 masks with the bitplane mp, modes "
        "1/2 with the value mask of x; optional acc adds a same-shape "
        "skip-gradient tensor in the epilogue",
        py::arg("g"), py::arg("wd"), py::arg("C"), py::arg("mode"),
        py::arg("mp"), py::arg("x"), py::arg("t"), py::arg("k"),
        py::arg("acc") = py::none());
  m.def("conv_wgrad_small", &conv_wgrad_small,
        "MFMA bf16 wgrad of a 3x3/s1/p1 binary conv with C and K in "
        "{16, 32} from the NHWC sign plane -> fp32 [nslab][9][C][K]; more "
        "than 8 block slabs come back summed into one unless fold is false",
        py::arg("g"), py::arg("xp"), py::arg("C"), py::arg("fold") = true);
  m.def("bwd_small_supported",
        [](int64_t H, int64_t W, int64_t C, int64_t K) {
          return H >= 1 && W >= 1 && H <= (1 << 20) && W <= (1 << 20) &&
                 C <= (1 << 20) && K <= (1 << 20) &&
                 bdbnn_bwd_small_supported((int)H, (int)W, (int)C,
                                           (int)K) != 0;
        },
        "routing predicate of conv_dgrad_small / conv_wgrad_small: "
        "3x3/s1/p1 with C and K both in {16, 32}, W <= 64",
        py::arg("H"), py::arg("W"), py::arg("C"), py::arg("K"));
  m.def("dgrad2_s2_supported",
        [](int64_t H, int64_t W, int64_t C, int64_t K, int64_t ks) {
          return dgrad2_s2_routed(H, W, C, K, ks);
        },
        "routing predicate of the stride-2 MFMA backward; H, W are the "
        "input (dx) size, ks in {3 (pad 1), 1 (pad 0)}; false also for "
        "the shapes the kernels run but lose on (3x3 with C >= 128 and "
        "K >= 256)",
        py::arg("H"), py::arg("W"), py::arg("C"), py::arg("K"),
        py::arg("ks"));
  m.def("conv_dgrad2_s2", &conv_dgrad2_s2,
        "MFMA bf16 dgrad of a 3x3/s2/p1 (wd [9][C][K]) or 1x1/s2/p0 (wd "
        "[1][C][K]) binary conv by pixel parity; mode 0 masks with the "
        "bitplane mp, modes 1/2 with the value mask of x; optional acc "
        "adds a same-shape skip-gradient tensor in the epilogue",
        py::arg("g"), py::arg("wd"), py::arg("H"), py::arg("W"),
        py::arg("C"), py::arg("mode"), py::arg("mp"), py::arg("x"),
        py::arg("t"), py::arg("k"), py::arg("acc") = py::none());
  m.def("dgrad_weight_decode_1x1", &dgrad_weight_decode_1x1,
        "packed 1x1 bits -> transposed +-alpha bf16 [1][C][K]");
  m.def("repack_cplane_s2", &repack_cplane_s2,
        "activation sign bits -> per-channel u64 row planes split by "
        "column parity (even columns low word, odd columns high word)",
        py::arg("xp"), py::arg("C"), py::arg("H"), py::arg("W"));
  m.def("conv_wgrad2_s2", &conv_wgrad2_s2,
        "MFMA bf16 wgrad of a 3x3/s2/p1 or 1x1/s2/p0 binary conv from the "
        "parity planes -> fp32 [nslab][ks*ks][C][K]",
        py::arg("g"), py::arg("planes"), py::arg("C"), py::arg("H"),
        py::arg("W"), py::arg("ks"));
  m.def("wgrad_finish_s2", &wgrad_finish_s2,
        "dwT slab sum + transpose to [K][C][ks][ks] + |w|<=1 STE mask");
  m.def("kurtosis_fwd", &kurtosis_fwd, "fused multi-tensor kurtosis fwd");
  m.def("kurtosis_bwd", &kurtosis_bwd, "fused multi-tensor kurtosis bwd");
  m.def("weight_kd_fwd", &weight_kd_fwd, "fused weight-space KD fwd");
  m.def("weight_kd_bwd", &weight_kd_bwd, "fused weight-space KD bwd");
  m.def("fused_sgd", &fused_sgd, "fused multi-tensor SGD-momentum step");
  m.def("fused_adam", &fused_adam, "fused multi-tensor Adam step");
}
