// Shared helpers for the bdbnn_amd gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#include "api.h"  // launcher prototypes, TensorListArg, PtrList, chunk size

#define BDBNN_WAVE 64

template <typename T>
__host__ __device__ __forceinline__ T bd_min(T a, T b) {
  return a < b ? a : b;
}

__device__ __forceinline__ float bf16_to_f32(uint16_t u) {
  union { uint32_t u; float f; } v;
  v.u = uint32_t(u) << 16;
  return v.f;
}

__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
  union { float f; uint32_t u; } v;
  v.f = f;
  // round-to-nearest-even
  uint32_t rounding = 0x7fff + ((v.u >> 16) & 1);
  return uint16_t((v.u + rounding) >> 16);
}

// XCD-aware block remap (8 XCDs with private L2s): consecutive remapped
// ids run on ONE XCD, so neighbouring tiles (sharing input rows) land on
// one L2.  Bijective for any grid size.
__device__ __forceinline__ int bd_xcd_remap(int wg, int nwg) {
  int q = nwg / 8, r = nwg % 8;
  int xcd = wg % 8, idx = wg / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// Grid-stride helper
#define GRID_STRIDE(i, n)                                            \
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;   \
       i < (n); i += (int64_t)gridDim.x * blockDim.x)

// ---- host side: runtime flag -> compile-time tag, for the launchers ----
// One ladder per kind of flag instead of one per launcher; the callee is a
// generic lambda that launches the kernel instantiation the tag names.

// storage type of a bf16 / fp32 buffer:
//   with_dtype(bf16, [&](auto t) { using T = decltype(t); ... });
template <typename F>
inline void with_dtype(bool bf16, F&& f) {
  if (bf16) f(uint16_t{});
  else      f(float{});
}

// two buffers of independent dtype: f(tag_a, tag_b)
template <typename F>
inline void with_dtype2(bool a_bf16, bool b_bf16, F&& f) {
  with_dtype(a_bf16, [&](auto a) {
    with_dtype(b_bf16, [&](auto b) { f(a, b); });
  });
}

// a small closed set of ints; the LAST listed value is the kernel's
// generic case and takes every v that matches none before it:
//   with_int<3, 2, 0>(ks, [&](auto k) { constexpr int KS = decltype(k)::value; ... });
template <int V, int... Rest, typename F>
inline void with_int(int v, F&& f) {
  if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<int, V>{});
  else if (v == V) f(std::integral_constant<int, V>{});
  else with_int<Rest...>(v, f);
}

template <typename F>
inline void with_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else   f(std::false_type{});
}
