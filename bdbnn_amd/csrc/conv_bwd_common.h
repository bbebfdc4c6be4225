// Pieces shared by the MFMA backward kernels (conv_bwd.hip: stride 1,
// conv_bwd_s2.hip: stride 2).
#pragma once
#include "common.h"
#include "act_masks.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

// One padded-width class of a launch table as a type: the table calls its
// visitor with the class, so the launcher (which needs the constants as
// template arguments) and the host-side size queries read ONE table.
template <int WPV, int RBV, int GBV>
struct BwdClass {
  static constexpr int WP = WPV, RB = RBV, GB = GBV;
};

// C/D layout of mfma_f32_32x32x16: col = lane&31, row of accumulator
// register `reg` in lane half `half` (= lane>>5)
__device__ __forceinline__ int mfma32_cd_row(int reg, int half) {
  return (reg & 3) + 8 * (reg >> 2) + 4 * half;
}

// byte -> 8 x (+-1) bf16 LUT of the wgrad sign decode (bit 1 <=> x >= 0
// <=> +1), filled by a 512-thread block
__device__ __forceinline__ void wgrad2_fill_sign_lut(__bf16 (*lut)[8],
                                                     int tid) {
  for (int b = tid; b < 256; b += 512) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      lut[b][j] = (__bf16)(((b >> j) & 1) ? 1.f : -1.f);
  }
}

// End of a wgrad block: the 8 waves are 4 (c-half, k-half) quads x 2
// m-split groups; group 1 hands its partials to group 0 through `red`,
// which adds them and writes the block's slab [NT][C][K] with plain
// coalesced stores (the slabs are summed by wgrad_finish).
template <int NT>
__device__ __forceinline__ void wgrad2_combine_store(
    const f32x16 (&acc)[NT], float (*red)[32][32], float* __restrict__ slab,
    int C, int K, int c0, int k0, int wid, int lane) {
  const int quad = wid & 3, ms_grp = wid >> 2;
  const int qc = (wid >> 1) & 1, qk = wid & 1;
  const int lrow = lane & 31, lhalf = lane >> 5;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    __syncthreads();
    if (ms_grp == 1) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg)
        red[quad][mfma32_cd_row(reg, lhalf)][lrow] = acc[t][reg];
    }
    __syncthreads();
    if (ms_grp == 0) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        int row = mfma32_cd_row(reg, lhalf);
        float v = acc[t][reg] + red[quad][row][lrow];
        slab[((int64_t)t * C + c0 + qc * 32 + row) * K + k0 + qk * 32 +
             lrow] = v;
      }
    }
  }
}

// MODE: which activation-gradient mask the dgrad epilogue applies
//   0  clip-STE, one bit per element from the packed plane `mp`
//   1  ReAct polynomial of x  (2+2x on [-1,0), 2-2x on [0,1), else 0)
//   2  EDE  k*t*(1 - tanh^2(t*x))
// Modes 1/2 depend on the VALUE of x, so they read the saved bf16 NHWC
// activation `xin` at the very address they store dx to (`mp` unused);
// mode 1 is ste_mask_mul_kernel's (csrc/pack.hip) react_poly_mask.
template <int MODE>
__device__ __forceinline__ float dgrad2_value_mask(float x, float et,
                                                   float ekt) {
  static_assert(MODE == 1 || MODE == 2, "value mask: mode 1 or 2");
  if constexpr (MODE == 1) {
    return react_poly_mask(x);
  }
  // 1 - tanh^2(u) = 4e/(1+e)^2 with e = exp(-2|u|) in (0,1]: nothing
  // can overflow, and large |t*x| underflows cleanly to 0 (the
  // tanh-then-square form is fine too, but exp(+2u) variants are not)
  float e = __expf(-2.f * fabsf(et * x));
  float d = 1.f + e;
  return ekt * __fdividef(4.f * e, d * d);
}
