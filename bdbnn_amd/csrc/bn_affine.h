// The BN affine + ReLU expression shared by bn_act.hip (which stores the
// activation) and bn_pool.hip (which recomputes it per pool tap and again
// in backward).  One definition, explicit fma: the two paths are
// bit-identical by construction and cannot drift.
#pragma once
#include "common.h"

// sc = gamma * invstd, sh = beta - mean * sc
__device__ __forceinline__ void bn_scale_shift(float gamma, float beta,
                                               float mean, float invstd,
                                               float& sc, float& sh) {
  sc = gamma * invstd;
  sh = __builtin_fmaf(-mean, sc, beta);
}

// pre-activation z = sc * x + sh
__device__ __forceinline__ float bn_affine(float sc, float x, float sh) {
  return __builtin_fmaf(sc, x, sh);
}

__device__ __forceinline__ float bn_relu(float z) { return fmaxf(z, 0.f); }

// ---- eval mode (running statistics) ----
// Shared by bn_act_eval_kernel, bn_fold_kernel (bn_act.hip) and the fused
// epilogue of xnor_conv_mfma.hip.  These keep the eval kernel's original
// plain expressions (the compiler contracts them), not the explicit fma of
// the training functions above: the eval kernel's output must not move.

// folded eval constants: sc = gamma * rsqrt(rv + eps), sh = beta - rm * sc.
// RPReLU's callers then add b1 to sh (the first shift rides in the
// affine's constant, as in bn_act_fwd_kernel).
__device__ __forceinline__ void bn_eval_scale_shift(float gamma, float beta,
                                                    float rm, float rv,
                                                    float eps, float& sc,
                                                    float& sh) {
  float is = rsqrtf(rv + eps);
  sc = gamma * is;
  sh = beta - rm * sc;
}

// out = act(sc * v + sh (+ s)); ACT as the launchers' act_kind
template <int ACT>
__device__ __forceinline__ float bn_eval_act(float sc, float v, float sh,
                                             bool has_skip, float s,
                                             float av, float b2v) {
  float zv = sc * v + sh;
  if (has_skip) zv += s;
  float o = zv;
  if (ACT == 1) o = zv > 0.f ? zv : av * zv;
  else if (ACT == 2) o = fmaxf(zv, 0.f);
  else if (ACT == 3) o = (zv > 0.f ? zv : av * zv) + b2v;
  return o;
}

// a value as the storage type T holds it (bf16: round-to-nearest-even)
template <typename T>
__device__ __forceinline__ float round_storage(float v) {
  if constexpr (sizeof(T) == 2) return bf16_to_f32(f32_to_bf16(v));
  else return v;
}

// ReLU(BN(x)) as a tensor of T stores it — what the pool compares and
// what the ReLU mask of backward tests
template <typename T>
__device__ __forceinline__ float bn_relu_stored(float sc, float x, float sh) {
  return round_storage<T>(bn_relu(bn_affine(sc, x, sh)));
}
