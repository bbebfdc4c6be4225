// The native kernel ABI: every extern "C" launcher the .hip translation
// units define and csrc/bind.cpp calls, declared once.  Host-clean (no
// device code) so the host compiler can include it; the .hip files get it
// through common.h, so each definition is checked against its prototype
// and a drifted argument list is a build error instead of shifted
// arguments at run time.  A new launcher is declared here first.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// Multi-tensor descriptors: fit in kernel args (<4 KB).
constexpr int BDBNN_MAX_TENSORS = 64;

struct TensorListArg {
  const float* ptr[BDBNN_MAX_TENSORS];
  int64_t numel[BDBNN_MAX_TENSORS];
  int n;
};

struct PtrList { float* ptr[BDBNN_MAX_TENSORS]; };

// Elements one block of a multi-tensor kernel covers; the host schedule
// (block -> tensor, offset) is built with the same constant.
constexpr int64_t BDBNN_CHUNK_ELEMS = 32 * 1024;

// Rows of the fused BN backward's per-channel sums ([C][rows]; the sliced
// partials are [32][C][rows]): sum dz, sum dz*xhat, da, and for RPReLU
// (act_kind 3) sum dy.  The bn_act.hip kernels, their launchers and the
// allocations in bind.cpp all size by this.
constexpr int bdbnn_bn_sum_rows(int act_kind) {
  return act_kind == 3 ? 4 : 3;
}

extern "C" {

// ---- pack.hip ----
void bdbnn_sign_pack(const void* x, uint32_t* out, int64_t pixels, int C,
                     int CW, bool bf16, hipStream_t stream);
void bdbnn_binsign_decode(const void* x, void* y, int64_t n, bool in_bf16,
                          bool out_bf16, hipStream_t stream);
void bdbnn_ste_mask_mul(const void* g, const void* x, void* y, int64_t n,
                        bool g_bf16, bool x_bf16, int mode, float t, float k,
                        hipStream_t stream);
void bdbnn_weight_pack(const float* w, uint32_t* wp, float* alpha,
                       float* stab, int K, int C, int KH, int KW, int CW,
                       hipStream_t stream);
void bdbnn_sign_mask_pack(const void* x, uint32_t* sp, uint32_t* mp,
                          int64_t pixels, int C, int CW, bool bf16,
                          hipStream_t stream);
void bdbnn_decode_packed(const uint32_t* sp, void* y, int64_t pixels, int C,
                         int CW, bool out_bf16, hipStream_t stream);
void bdbnn_mask_mul_packed(const void* g, const uint32_t* mp, void* dx,
                           int64_t pixels, int C, int CW, bool g_bf16,
                           bool out_bf16, hipStream_t stream);
void bdbnn_weight_decode(const uint32_t* wp, const float* alpha, void* w,
                         int K, int C, int T, int CW, bool out_bf16,
                         hipStream_t stream);

// ---- xnor_conv.hip ----
void bdbnn_xnor_conv_fwd(
    const uint32_t* xp, const uint32_t* wp, const float* alpha,
    const float* stab, void* out, float* s1, float* s2, bool out_bf16,
    int N, int H, int W, int C, int K, int KH, int KW, int stride, int pad,
    int Ho, int Wo, hipStream_t stream);

// ---- xnor_conv_mfma.hip (the same conv on i8 MFMA; 3x3/p1, s1 or s2,
// C % 64 == 0, K % 64 == 0, no BN statistics) ----
int bdbnn_xnor_mfma_supported(int C, int K, int KH, int KW, int stride,
                              int pad);
// supported AND routed there by default AND BDBNN_XNOR_MFMA != 0
int bdbnn_xnor_mfma_routed(int C, int K, int KH, int KW, int stride,
                           int pad);
// 0 launched, -1 unsupported shape, -2 tensor too large for int indices
int bdbnn_xnor_conv_mfma_fwd(
    const uint32_t* xp, const uint32_t* wp, const float* alpha, void* out,
    bool out_bf16, int N, int H, int W, int C, int K, int KH, int KW,
    int stride, int pad, int Ho, int Wo, hipStream_t stream);
// The same conv with the eval-mode block tail in its epilogue (inference):
// out = act(sc_k * round(alpha_k * dot) + sh_k (+ skip)), act_kind as
// bn_act.hip's, (sc, sh) from bdbnn_bn_fold; a for kinds 1 and 3, b2 for
// kind 3, skip (out's dtype and layout) and plane ([N,Ho,Wo,K/32] sign
// plane of out) may be null.  Return codes as above, -3 bad act operands.
int bdbnn_xnor_conv_bn_act_fwd(
    const uint32_t* xp, const uint32_t* wp, const float* alpha,
    const float* sc, const float* sh, const float* a, const float* b2,
    const void* skip, void* out, uint32_t* plane, int act_kind,
    bool out_bf16, int N, int H, int W, int C, int K, int KH, int KW,
    int stride, int pad, int Ho, int Wo, hipStream_t stream);

// ---- stem_conv.hip ----
void bdbnn_stem_pack_x4(const void* x, void* x4, int64_t npix, bool bf16,
                        hipStream_t stream);
void bdbnn_stem_pack_w4(const float* w, void* w4T, hipStream_t stream);
void bdbnn_stem_fwd(const void* x4, const void* w4T, void* out, int N, int H,
                    int W, hipStream_t stream);
int bdbnn_stem_wrw_nslab(int N, int H, int W);
void bdbnn_stem_wrw(const void* x4, const void* g, float* dwslab, int N,
                    int H, int W, hipStream_t stream);
void bdbnn_stem_fold_dw4(const float* slabs, float* dw, int nslab,
                         hipStream_t stream);

// ---- loss.hip ----
void bdbnn_kd_logit_fwd(const void* s, const void* t, float* stats,
                        float* out, int B, int C, bool bf16,
                        hipStream_t stream);
void bdbnn_kd_logit_bwd(const void* s, const void* t, const float* stats,
                        void* ds, float gscale, int B, int C, bool bf16,
                        hipStream_t stream);
void bdbnn_ce_fwd(const void* s, const int64_t* y, float* stats, float* out,
                  int B, int C, bool bf16, hipStream_t stream);
void bdbnn_ce_bwd(const void* s, const int64_t* y, const float* stats,
                  void* ds, float gscale, int B, int C, bool bf16,
                  hipStream_t stream);

// ---- pool.hip ----
void bdbnn_maxpool_fwd(const void* x, void* out, unsigned char* idx, int N,
                       int C, int H, int W, int Ho, int Wo, int ks,
                       int stride, int pad, bool bf16, hipStream_t stream);
void bdbnn_maxpool_bwd(const void* dy, const unsigned char* idx, void* dx,
                       int N, int C, int H, int W, int Ho, int Wo, int ks,
                       int stride, int pad, bool bf16, hipStream_t stream);

// ---- prelu.hip ----
void bdbnn_prelu_fwd(const void* x, const float* a, void* y, int64_t n,
                     int C, bool bf16, hipStream_t stream);
void bdbnn_prelu_bwd(const void* x, const void* g, const float* a, void* dx,
                     float* da, int64_t n, int C, bool bf16,
                     hipStream_t stream);

// ---- bn_act.hip ----
// act_kind: 0 identity, 1 PReLU (a), 2 ReLU, 3 RPReLU (a, b1, b2); sums32 /
// sums hold bdbnn_bn_sum_rows(act_kind) rows per channel
void bdbnn_bn_stats(const void* x, float* s1, float* s2, int64_t n, int C,
                    bool bf16, hipStream_t stream);
void bdbnn_bn_finalize(const float* s1, const float* s2, float* mean,
                       float* invstd, float* running_mean,
                       float* running_var, int C, float n, float momentum,
                       float eps, int nslice, hipStream_t stream);
void bdbnn_bn_act_fwd(const void* x, const void* skip, const float* mean,
                      const float* invstd, const float* gamma,
                      const float* beta, const float* a, const float* b1,
                      const float* b2, void* out, void* zout, int64_t n,
                      int C, int act_kind, uint32_t* xpk, uint32_t* mpk,
                      bool bf16, hipStream_t stream);
void bdbnn_bn_act_bwd_reduce(const void* dy, const void* z, const void* x,
                             const float* mean, const float* invstd,
                             const float* a, float* sums32, float* sums,
                             int64_t n, int C, int act_kind, bool bf16,
                             hipStream_t stream);
// also called from bn_pool.hip
void bdbnn_bn_fold_sums(const float* sums32, float* sums, int n,
                        hipStream_t stream);
void bdbnn_bn_act_bwd_apply(const void* dy, const void* z, const void* x,
                            const float* mean, const float* invstd,
                            const float* gamma, const float* a,
                            const float* sums, void* dx, void* dskip,
                            int64_t n, int C, int act_kind, float inv_n,
                            bool bf16, hipStream_t stream);
void bdbnn_bn_act_eval(const void* x, const void* skip, const float* rm,
                       const float* rv, const float* gamma,
                       const float* beta, const float* a, const float* b1,
                       const float* b2, void* out, int64_t n, int C,
                       int act_kind, float eps, bool bf16,
                       hipStream_t stream);
// the eval kernel's folded constants on their own: sc = gamma * rsqrt(rv +
// eps), sh = beta - rm * sc (+ b1 when not null), fp32 [C]
void bdbnn_bn_fold(const float* gamma, const float* beta, const float* rm,
                   const float* rv, const float* b1, float* sc, float* sh,
                   int C, float eps, hipStream_t stream);

// ---- bn_pool.hip ----
void bdbnn_bn_relu_maxpool_fwd(
    const void* x, const float* mean, const float* invstd,
    const float* gamma, const float* beta, void* out, unsigned char* idx,
    uint32_t* xpk, uint32_t* mpk, int N, int C, int H, int W, int Ho, int Wo,
    int ks, int stride, int pad, bool bf16, hipStream_t stream);
void bdbnn_bn_relu_maxpool_bwd_reduce(
    const void* dy, const unsigned char* idx, const void* x,
    const float* mean, const float* invstd, const float* gamma,
    const float* beta, float* sums32, float* sums, int N, int C, int H,
    int W, int Ho, int Wo, int ks, int stride, int pad, bool bf16,
    hipStream_t stream);
void bdbnn_bn_relu_maxpool_bwd_apply(
    const void* dy, const unsigned char* idx, const void* x,
    const float* mean, const float* invstd, const float* gamma,
    const float* beta, const float* sums, void* dx, int N, int C, int H,
    int W, int Ho, int Wo, int ks, int stride, int pad, bool bf16,
    hipStream_t stream);

// ---- conv_bwd.hip (3x3/s1/p1 MFMA backward + shared pack/finish) ----
int bdbnn_dgrad2_supported(int H, int W, int C, int K);
int bdbnn_conv_dgrad2(const void* g, const void* wd, const uint32_t* mp,
                      const void* x, void* dx, const void* accp, int mode,
                      float t, float k, int N, int H, int W, int C, int K,
                      hipStream_t stream);
void bdbnn_dgrad_wdec(const uint32_t* wp, const float* alpha, void* wd,
                      int C, int K, int nt, hipStream_t stream);
int bdbnn_wgrad2_nslab(int N, int H, int W, int C, int K);
int bdbnn_conv_wgrad2(const void* g, const uint64_t* xcp, float* dwT, int N,
                      int H, int W, int C, int K, hipStream_t stream);
void bdbnn_repack_cplane(const uint32_t* xp, uint64_t* xcp, int NH, int W,
                         int C, int CW, bool parity, hipStream_t stream);
void bdbnn_wgrad_finish(const float* dwT, const float* w, float* dw, int C,
                        int K, int T, int nslab, hipStream_t stream);

// ---- conv_wgrad3.hip (3x3/s1/p1 wgrad from the NHWC sign plane xp
// [N][H][W][C/32]; slab contract and m-split of conv_wgrad2) ----
// shape can run AND its class is routed here by default
int bdbnn_wgrad3_supported(int H, int W, int C, int K);
int bdbnn_wgrad3_nslab(int N, int H, int W, int C, int K);
int bdbnn_conv_wgrad3(const void* g, const uint32_t* xp, float* dwT, int N,
                      int H, int W, int C, int K, hipStream_t stream);

// ---- conv_bwd_small.hip (3x3/s1/p1 MFMA backward, C and K in {16, 32},
// W <= 64; the contracts of conv_dgrad2 and conv_wgrad3) ----
// shape can run AND its class is routed here by default
int bdbnn_bwd_small_supported(int H, int W, int C, int K);
// 0 launched, -1 unsupported shape, -2 too large for int pixel indices,
// -3 bad mode
int bdbnn_conv_dgrad_small(const void* g, const void* wd, const uint32_t* mp,
                           const void* x, void* dx, const void* accp,
                           int mode, float t, float k, int N, int H, int W,
                           int C, int K, hipStream_t stream);
int bdbnn_wgrad_small_nslab(int N, int H, int W, int C, int K);
int bdbnn_conv_wgrad_small(const void* g, const uint32_t* xp, float* dwT,
                           int N, int H, int W, int C, int K,
                           hipStream_t stream);
// slab-parallel sum of slabs [nslab][9][C][K] into out [9][C][K]
void bdbnn_wgrad_small_fold(const float* slabs, float* out, int nslab, int C,
                            int K, hipStream_t stream);

// ---- conv_bwd_s2.hip (3x3/s2/p1 and 1x1/s2/p0 MFMA backward) ----
int bdbnn_s2_kernels_can_run(int H, int W, int C, int K, int ks);
int bdbnn_dgrad2_s2_supported(int H, int W, int C, int K, int ks);
int bdbnn_conv_dgrad2_s2(const void* g, const void* wd, const uint32_t* mp,
                         const void* x, void* dx, const void* accp, int ks,
                         int mode, float t, float k, int N, int H, int W,
                         int C, int K, hipStream_t stream);
int bdbnn_wgrad2_s2_nslab(int N, int H, int W, int C, int K, int ks);
int bdbnn_conv_wgrad2_s2(const void* g, const uint64_t* planes, float* dwT,
                         int ks, int N, int H, int W, int C, int K,
                         hipStream_t stream);

// ---- kurtosis.hip ----
void bdbnn_kurtosis_fwd(const TensorListArg* lists,
                        const int* block_tensor_dev,
                        const int64_t* block_off_dev, int n_blocks,
                        double* mom_dev, const float* targets, float* stats,
                        float* losses, float* kurts, hipStream_t stream);
void bdbnn_kurtosis_bwd(const TensorListArg* lists, const PtrList* gp,
                        const int* block_tensor_dev,
                        const int64_t* block_off_dev, int n_blocks,
                        const float* stats, const float* targets,
                        const float* gscale, hipStream_t stream);

// ---- kd.hip ----
void bdbnn_weight_kd_fwd(const TensorListArg* meta, const PtrList* ws,
                         const PtrList* wt, const int* bt, const int64_t* bo,
                         int n_blocks, double* out, hipStream_t stream);
void bdbnn_weight_kd_bwd(const TensorListArg* meta, const PtrList* wt,
                         const PtrList* grads, const int* bt,
                         const int64_t* bo, int n_blocks,
                         const float* gscale, hipStream_t stream);

// ---- optim.hip ----
void bdbnn_fused_sgd(const TensorListArg* meta, const PtrList* p,
                     const PtrList* g, const PtrList* buf, const int* bt,
                     const int64_t* bo, int n_blocks, float lr,
                     float momentum, float wd, hipStream_t stream);
void bdbnn_fused_adam(const TensorListArg* meta, const PtrList* p,
                      const PtrList* g, const PtrList* m1, const PtrList* m2,
                      const int* bt, const int64_t* bo, int n_blocks,
                      float lr, float beta1, float beta2, float eps,
                      float wd, float bc1, float bc2, hipStream_t stream);

}  // extern "C"
