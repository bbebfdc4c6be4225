// Pieces shared by the MFMA backward kernels (conv_bwd.hip: stride 1,
// conv_bwd_s2.hip: stride 2).
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

// MODE: which activation-gradient mask the dgrad epilogue applies
//   0  clip-STE, one bit per element from the packed plane `mp`
//   1  ReAct polynomial of x  (2+2x on [-1,0), 2-2x on [0,1), else 0)
//   2  EDE  k*t*(1 - tanh^2(t*x))
// Modes 1/2 depend on the VALUE of x, so they read the saved bf16 NHWC
// activation `xin` at the very address they store dx to (`mp` unused);
// semantics are those of ste_mask_mul_kernel (csrc/pack.hip).
template <int MODE>
__device__ __forceinline__ float dgrad2_value_mask(float x, float et,
                                                   float ekt) {
  static_assert(MODE == 1 || MODE == 2, "value mask: mode 1 or 2");
  if constexpr (MODE == 1) {
    return (x >= -1.f && x < 0.f) ? 2.f + 2.f * x
         : (x >= 0.f && x < 1.f) ? 2.f - 2.f * x : 0.f;
  }
  // 1 - tanh^2(u) = 4e/(1+e)^2 with e = exp(-2|u|) in (0,1]: nothing
  // can overflow, and large |t*x| underflows cleanly to 0 (the
  // tanh-then-square form is fine too, but exp(+2u) variants are not)
  float e = __expf(-2.f * fabsf(et * x));
  float d = 1.f + e;
  return ekt * __fdividef(4.f * e, d * d);
}
