// Max-pool geometry shared by pool.hip and the fused stem tail of
// bn_pool.hip.
#pragma once
#include "common.h"

struct PoolParams {
  int N, C, H, W, Ho, Wo, ks, stride, pad;
};

// Along one axis: the output windows o in [lo, hi] whose taps cover input
// coordinate i, i.e. o*stride - pad <= i < o*stride - pad + ks, clipped to
// the n_out windows there are.  At most ceil(ks/stride) of them.
__device__ __forceinline__ void pool_window_range(const PoolParams& p, int i,
                                                  int n_out, int& lo,
                                                  int& hi) {
  lo = max(0, (i + p.pad - p.ks + p.stride) / p.stride);
  hi = min(n_out - 1, (i + p.pad) / p.stride);
}
