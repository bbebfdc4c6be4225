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
