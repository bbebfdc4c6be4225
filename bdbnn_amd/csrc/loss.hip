// K4/K6 — fused classification losses over (B, C) logits.
//
// logit KD (ref:utils/KD_loss.py:10-43):
//   loss = mean_n( -sum_c softmax(t)_c * log_softmax(s)_c )
// cross-entropy (ref:train.py:318):
//   loss = mean_n( logsumexp(s_n) - s_n[y_n] )
//
// One block per row forward (max + logsumexp + dot in registers/LDS,
// logits read once); elementwise backward from saved row stats:
//   KD: ds = g/B * (softmax(s) - softmax(t))
//   CE: ds = g/B * (softmax(s) - onehot(y))
#include "common.h"
#include "vec8.h"

__device__ __forceinline__ float block_reduce(float v, float* red, int op) {
  // op 0 = max, 1 = sum
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = blockDim.x / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o)
      red[threadIdx.x] = op == 0
          ? fmaxf(red[threadIdx.x], red[threadIdx.x + o])
          : red[threadIdx.x] + red[threadIdx.x + o];
    __syncthreads();
  }
  float r = red[0];
  __syncthreads();
  return r;
}

// stats[b] = (m_s, lseZ_s, m_t, lseZ_t); out += loss_row / B
template <typename T>
__global__ void kd_logit_fwd_kernel(const T* __restrict__ s,
                                    const T* __restrict__ t,
                                    float* __restrict__ stats,
                                    float* __restrict__ out, int B, int C) {
  __shared__ float red[256];
  int b = blockIdx.x;
  const T* sr = s + (int64_t)b * C;
  const T* tr = t + (int64_t)b * C;
  float ms = -3.4e38f, mt = -3.4e38f;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    ms = fmaxf(ms, ld1(sr, c));
    mt = fmaxf(mt, ld1(tr, c));
  }
  ms = block_reduce(ms, red, 0);
  mt = block_reduce(mt, red, 0);
  float zs = 0.f, zt = 0.f;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    zs += expf(ld1(sr, c) - ms);
    zt += expf(ld1(tr, c) - mt);
  }
  zs = block_reduce(zs, red, 1);
  zt = block_reduce(zt, red, 1);
  float lzs = logf(zs), lzt = logf(zt);
  float dot = 0.f;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float pt = expf(ld1(tr, c) - mt - lzt);
    dot += pt * (ld1(sr, c) - ms - lzs);
  }
  dot = block_reduce(dot, red, 1);
  if (threadIdx.x == 0) {
    stats[b * 4 + 0] = ms + lzs;
    stats[b * 4 + 1] = mt + lzt;
    atomicAdd(out, -dot / (float)B);
  }
}

template <typename T>
__global__ void kd_logit_bwd_kernel(const T* __restrict__ s,
                                    const T* __restrict__ t,
                                    const float* __restrict__ stats,
                                    T* __restrict__ ds, float gscale,
                                    int64_t n, int C) {
  GRID_STRIDE(i, n) {
    int b = int(i / C);
    float lse_s = stats[b * 4 + 0], lse_t = stats[b * 4 + 1];
    float ps = expf(ld1(s, i) - lse_s);
    float pt = expf(ld1(t, i) - lse_t);
    float v = gscale * (ps - pt);
    st1(ds, i, v);
  }
}

template <typename T>
__global__ void ce_fwd_kernel(const T* __restrict__ s,
                              const int64_t* __restrict__ y,
                              float* __restrict__ stats,
                              float* __restrict__ out, int B, int C) {
  __shared__ float red[256];
  int b = blockIdx.x;
  const T* sr = s + (int64_t)b * C;
  float ms = -3.4e38f;
  for (int c = threadIdx.x; c < C; c += blockDim.x)
    ms = fmaxf(ms, ld1(sr, c));
  ms = block_reduce(ms, red, 0);
  float zs = 0.f;
  for (int c = threadIdx.x; c < C; c += blockDim.x)
    zs += expf(ld1(sr, c) - ms);
  zs = block_reduce(zs, red, 1);
  if (threadIdx.x == 0) {
    float lse = ms + logf(zs);
    stats[b] = lse;
    atomicAdd(out, (lse - ld1(sr, (int)y[b])) / (float)B);
  }
}

template <typename T>
__global__ void ce_bwd_kernel(const T* __restrict__ s,
                              const int64_t* __restrict__ y,
                              const float* __restrict__ stats,
                              T* __restrict__ ds, float gscale, int64_t n,
                              int C) {
  GRID_STRIDE(i, n) {
    int b = int(i / C);
    int c = int(i % C);
    float p = expf(ld1(s, i) - stats[b]);
    float v = gscale * (p - (c == (int)y[b] ? 1.f : 0.f));
    st1(ds, i, v);
  }
}

extern "C" void bdbnn_kd_logit_fwd(const void* s, const void* t,
                                   float* stats, float* out, int B, int C,
                                   bool bf16, hipStream_t stream) {
  hipMemsetAsync(out, 0, sizeof(float), stream);
  with_dtype(bf16, [&](auto tag) {
    using T = decltype(tag);
    kd_logit_fwd_kernel<T><<<B, 256, 0, stream>>>((const T*)s, (const T*)t,
                                                  stats, out, B, C);
  });
}

extern "C" void bdbnn_kd_logit_bwd(const void* s, const void* t,
                                   const float* stats, void* ds,
                                   float gscale, int B, int C, bool bf16,
                                   hipStream_t stream) {
  int64_t n = (int64_t)B * C;
  int grid = (int)bd_min<int64_t>((n + 255) / 256, 2048);
  with_dtype(bf16, [&](auto tag) {
    using T = decltype(tag);
    kd_logit_bwd_kernel<T><<<grid, 256, 0, stream>>>(
        (const T*)s, (const T*)t, stats, (T*)ds, gscale, n, C);
  });
}

extern "C" void bdbnn_ce_fwd(const void* s, const int64_t* y, float* stats,
                             float* out, int B, int C, bool bf16,
                             hipStream_t stream) {
  hipMemsetAsync(out, 0, sizeof(float), stream);
  with_dtype(bf16, [&](auto tag) {
    using T = decltype(tag);
    ce_fwd_kernel<T><<<B, 256, 0, stream>>>((const T*)s, y, stats, out, B,
                                            C);
  });
}

extern "C" void bdbnn_ce_bwd(const void* s, const int64_t* y,
                             const float* stats, void* ds, float gscale,
                             int B, int C, bool bf16, hipStream_t stream) {
  int64_t n = (int64_t)B * C;
  int grid = (int)bd_min<int64_t>((n + 255) / 256, 2048);
  with_dtype(bf16, [&](auto tag) {
    using T = decltype(tag);
    ce_bwd_kernel<T><<<grid, 256, 0, stream>>>((const T*)s, y, stats,
                                               (T*)ds, gscale, n, C);
  });
}
