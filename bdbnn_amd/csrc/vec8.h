// 8-element vector load/store helpers (bf16: one 16-B uint4; fp32: two
// float4).  Guide G13: scalar bf16 loads cost ~2-2.5x on gfx950.
#pragma once
#include "common.h"

// one element of a bf16 (T = uint16_t) / fp32 buffer, as float
template <typename T>
__device__ __forceinline__ float ld1(const T* p, int64_t i) {
  if constexpr (sizeof(T) == 2) return bf16_to_f32(((const uint16_t*)p)[i]);
  else                          return ((const float*)p)[i];
}

template <typename T>
__device__ __forceinline__ void st1(T* p, int64_t i, float v) {
  if constexpr (sizeof(T) == 2) ((uint16_t*)p)[i] = f32_to_bf16(v);
  else                          ((float*)p)[i] = v;
}

template <typename T>
__device__ __forceinline__ void load8(const T* p, int64_t i, float v[8]) {
  if constexpr (sizeof(T) == 2) {
    uint4 r = *(const uint4*)(p + i);
    const uint16_t* u = (const uint16_t*)&r;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = bf16_to_f32(u[j]);
  } else {
    float4 a = *(const float4*)((const float*)p + i);
    float4 b = *(const float4*)((const float*)p + i + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
}

template <typename T>
__device__ __forceinline__ void store8(T* p, int64_t i, const float v[8]) {
  if constexpr (sizeof(T) == 2) {
    uint4 r;
    uint16_t* u = (uint16_t*)&r;
#pragma unroll
    for (int j = 0; j < 8; ++j) u[j] = f32_to_bf16(v[j]);
    *(uint4*)(p + i) = r;
  } else {
    float4 a{v[0], v[1], v[2], v[3]}, b{v[4], v[5], v[6], v[7]};
    *(float4*)((float*)p + i) = a;
    *(float4*)((float*)p + i + 4) = b;
  }
}

// channel-group geometry for NHWC kernels: thread owns VEC=8 consecutive
// channels; C is a power of two >= 8.
struct ChanMap {
  int c0;        // first owned channel
  int64_t p0;    // first pixel
  int64_t pstep; // pixel stride
};

__device__ __forceinline__ ChanMap chan_map8(int C) {
  int tpr = C / 8;                       // threads per pixel row
  ChanMap m;
  m.c0 = (threadIdx.x % tpr) * 8;
  int rows = 256 / tpr;                  // rows covered per block iter
  m.p0 = (int64_t)blockIdx.x * rows + threadIdx.x / tpr;
  m.pstep = (int64_t)gridDim.x * rows;
  return m;
}

__host__ __device__ __forceinline__ int grid_pix8(int64_t n_pix, int C) {
  int rows = 256 / (C / 8 < 256 ? C / 8 : 256);
  if (C / 8 >= 256) rows = 1;
  int64_t g = (n_pix + rows - 1) / rows;
  return (int)(g < 2048 ? g : 2048);
}

// ---- per-channel block sums of the chan_map8 reductions ----
// NS sums per channel: every thread accumulates its 8 channels in
// registers over its pixel stripe, the block combines them in LDS rows
// [NS][C] (one LDS atomic per owned channel and sum), and one global atomic
// per non-zero row entry leaves the block.
template <int NS>
__device__ __forceinline__ void chan_sums_zero(float* lds, int C) {
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
#pragma unroll
    for (int k = 0; k < NS; ++k) lds[k * C + c] = 0.f;
  }
  __syncthreads();
}

// a[k]: this thread's 8 register sums of row k (channels c0 .. c0+7).
// An array of pointers on purpose: as a parameter pack the same helper cost
// bn_relu_maxpool_bwd_reduce_kernel<.., 2> its packed fp32 math
// (profiles/r07_elementwise_helpers_isa.md).
template <int NS>
__device__ __forceinline__ void chan_sums_add(float* lds, int C, int c0,
                                              const float* const (&a)[NS]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
#pragma unroll
    for (int k = 0; k < NS; ++k) atomicAdd(&lds[k * C + c0 + j], a[k][j]);
  }
}

// Sum k of channel c is added to out[k][c * cstride].  SLICED: into slice
// blockIdx & 31 of 32 slices of `slice` floats each, which a fold kernel
// sums afterwards — full-grid atomics onto C words serialize ~2048-deep
// otherwise.  Zero sums (channels the block never touched) are skipped.
template <int NS, bool SLICED>
__device__ __forceinline__ void chan_sums_flush(const float* lds, int C,
                                                float* const (&out)[NS],
                                                int cstride, int slice) {
  __syncthreads();
  const int off = SLICED ? (blockIdx.x & 31) * slice : 0;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      float v = lds[k * C + c];
      if (v != 0.f) atomicAdd(&out[k][off + c * cstride], v);
    }
  }
}
