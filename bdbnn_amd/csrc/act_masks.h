// The activation bit and mask conventions, one definition each (as
// bn_affine.h does for the BN expression): every kernel that packs a sign
// or clip-mask bit, or applies the ReAct polynomial, calls these, so the
// standalone pack kernels, the fused PACK epilogues and the dgrad value
// mask agree by construction.
#pragma once
#include "common.h"

// activation sign bit: 1 iff v >= 0 (so -0.0 packs as +1)
__device__ __forceinline__ bool sign_bit(float v) { return v >= 0.f; }

// clip-STE mask bit: 1 iff |v| <= 1
__device__ __forceinline__ bool clip_bit(float v) { return fabsf(v) <= 1.f; }

// ReActNet's piecewise-polynomial sign gradient:
// 2+2x on [-1,0), 2-2x on [0,1), else 0
__device__ __forceinline__ float react_poly_mask(float x) {
  return (x >= -1.f && x < 0.f) ? 2.f + 2.f * x
       : (x >= 0.f && x < 1.f) ? 2.f - 2.f * x : 0.f;
}

// PACK epilogue of the 8-channels-per-thread NHWC kernels: r holds this
// thread's 8 values AS STORED (already rounded to the storage type), i.e.
// one byte of the sign plane and one of the clip-mask plane.  The 4 lanes
// of a 32-channel word are consecutive (C % 32 == 0 => threads per pixel
// row % 4 == 0) and combine with intra-wave shuffles; lane sub == 0
// (sub = threadIdx.x & 3) stores both words at index `word`.
__device__ __forceinline__ void pack_sign_mask8(const float r[8], int sub,
                                                uint32_t* __restrict__ xpk,
                                                uint32_t* __restrict__ mpk,
                                                int64_t word) {
  unsigned both = 0;   // sign byte | mask byte << 8
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    both |= unsigned(sign_bit(r[j])) << j;
    both |= unsigned(clip_bit(r[j])) << (8 + j);
  }
  unsigned b1 = __shfl_down(both, 1);
  unsigned b2 = __shfl_down(both, 2);
  unsigned b3 = __shfl_down(both, 3);
  if (sub == 0) {
    uint32_t sw = (both & 0xffu) | ((b1 & 0xffu) << 8) |
                  ((b2 & 0xffu) << 16) | ((b3 & 0xffu) << 24);
    uint32_t mw = ((both >> 8) & 0xffu) | (((b1 >> 8) & 0xffu) << 8) |
                  (((b2 >> 8) & 0xffu) << 16) |
                  (((b3 >> 8) & 0xffu) << 24);
    xpk[word] = sw;
    mpk[word] = mw;
  }
}
