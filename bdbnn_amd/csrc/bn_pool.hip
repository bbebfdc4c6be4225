// K8c — the stem tail bn1 -> ReLU -> maxpool as ONE op, NHWC, training.
//
// The unfused pair (csrc/bn_act.hip + csrc/pool.hip) materialises three
// full-resolution tensors that the result does not need: the ReLU output
// (written, re-read by the pool, saved as the ReLU mask), the pool's
// input gradient (three-quarters zeros; written once, read twice) and
// the pooled activation's re-read for the next conv's pack.  Here
//   fwd:    the pool applies BN+ReLU to the taps it reads; writes the
//           pooled tensor, the u8 argmax plane and (PACK) the consuming
//           binary conv's sign / clip-mask bitplanes
//   reduce: every INPUT pixel gathers its dy from the pooled gradient +
//           argmax plane (as maxpool_bwd_kernel does), recomputes the
//           ReLU mask from x, and sums dz / dz*xhat
//   apply:  the same gather, writes dx
// Per tap the forward computes exactly what the pair computes — the
// shared helper of bn_affine.h, rounded through the storage type because
// the pair compares the STORED tensor — with pool.hip's strict '>'
// first-maximum rule and tap order, so out and idx are bit-identical to
// maxpool_fwd(bn_act_fwd_train(x)) for the same mean / invstd.  There is
// no "pool first, then affine" shortcut: sc can be <= 0 per channel.
//
// Thread layout as in bn_act.hip: 8 consecutive channels per thread, C a
// power of two, 8 <= C <= 1024.  Block ids go through bd_xcd_remap so
// that one XCD sweeps a contiguous run of pixels: neighbouring output
// rows share an input row (the window halo) and neighbouring input rows
// share their windows, and those re-reads should hit that XCD's L2.
#include "common.h"
#include "vec8.h"
#include "bn_affine.h"
#include "act_masks.h"
#include "pool_common.h"

// chan_map8 on the XCD-remapped block id
__device__ __forceinline__ ChanMap pool_map8(int C) {
  int tpr = C / 8;
  int rows = 256 / tpr;
  int lb = bd_xcd_remap((int)blockIdx.x, (int)gridDim.x);
  ChanMap m;
  m.c0 = (threadIdx.x % tpr) * 8;
  m.p0 = (int64_t)lb * rows + threadIdx.x / tpr;
  m.pstep = (int64_t)gridDim.x * rows;
  return m;
}

__device__ __forceinline__ void load_scale_shift(
    const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ gamma, const float* __restrict__ beta, int c0,
    float sc[8], float sh[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int cc = c0 + j;
    bn_scale_shift(gamma[cc], beta[cc], mean[cc], invstd[cc], sc[j], sh[j]);
  }
}

// ---- forward: thread owns 8 channels of one OUTPUT pixel ----
// KS > 0: compile-time window, every tap load issued up front from a
// clamped (always in-bounds) address and masked afterwards — KS*KS
// independent loads in flight per thread.  KS == 0: any window, one
// blocking load per tap.
// PACK: sign + clip-mask bitplanes of the pooled (already rounded)
// values, by pack_sign_mask8 as in bn_act_fwd_kernel<PACK>.
template <typename T, int KS, bool PACK>
__global__ void __launch_bounds__(256) bn_relu_maxpool_fwd_kernel(
    const T* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, T* __restrict__ out,
    unsigned char* __restrict__ idx, uint32_t* __restrict__ xpk,
    uint32_t* __restrict__ mpk, PoolParams p, int n_opix) {
  ChanMap m = pool_map8(p.C);
  float sc[8], sh[8];
  load_scale_shift(mean, invstd, gamma, beta, m.c0, sc, sh);
  const int ks = KS > 0 ? KS : p.ks;
  const int HoWo = p.Ho * p.Wo;
  const int sub = threadIdx.x & 3;         // byte slot within the word
  const int64_t cw = m.c0 >> 5;            // word column (lane sub == 0)
  const int CW = p.C >> 5;
  for (int64_t op = m.p0; op < n_opix; op += m.pstep) {
    int n = (int)op / HoWo;
    int rem = (int)op - n * HoWo;
    int oy = rem / p.Wo, ox = rem - oy * p.Wo;
    int iy0 = oy * p.stride - p.pad;
    int ix0 = ox * p.stride - p.pad;
    const int64_t img = (int64_t)n * p.H;
    float best[8];
    int bi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { best[j] = -3.4e38f; bi[j] = 0; }
    if constexpr (KS > 0) {
      float v[KS * KS][8];
      bool ok[KS * KS];
#pragma unroll
      for (int t = 0; t < KS * KS; ++t) {
        int iy = iy0 + t / KS, ix = ix0 + t % KS;
        ok[t] = iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
        int cy = min(max(iy, 0), p.H - 1), cx = min(max(ix, 0), p.W - 1);
        load8(x, ((img + cy) * p.W + cx) * p.C + m.c0, v[t]);
      }
#pragma unroll
      for (int t = 0; t < KS * KS; ++t) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float o = bn_relu_stored<T>(sc[j], v[t][j], sh[j]);
          if (ok[t] && o > best[j]) { best[j] = o; bi[j] = t; }
        }
      }
    } else {
      for (int t = 0; t < ks * ks; ++t) {
        int iy = iy0 + t / ks, ix = ix0 + t % ks;
        if (iy < 0 || iy >= p.H || ix < 0 || ix >= p.W) continue;
        float v[8];
        load8(x, ((img + iy) * p.W + ix) * p.C + m.c0, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float o = bn_relu_stored<T>(sc[j], v[j], sh[j]);
          if (o > best[j]) { best[j] = o; bi[j] = t; }
        }
      }
    }
    store8(out, op * p.C + m.c0, best);
    uint2 iw;
    iw.x = (unsigned)bi[0] | ((unsigned)bi[1] << 8) |
           ((unsigned)bi[2] << 16) | ((unsigned)bi[3] << 24);
    iw.y = (unsigned)bi[4] | ((unsigned)bi[5] << 8) |
           ((unsigned)bi[6] << 16) | ((unsigned)bi[7] << 24);
    *(uint2*)(idx + op * p.C + m.c0) = iw;
    if constexpr (PACK) pack_sign_mask8(best, sub, xpk, mpk, op * CW + cw);
  }
}

// tap byte j of the 8 index bytes a thread loads as one uint2
__device__ __forceinline__ int idx_byte(const uint2& q, int j) {
  return int(((j < 4 ? q.x : q.y) >> (8 * (j & 3))) & 0xffu);
}

// ---- backward: thread owns 8 channels of one INPUT pixel ----
// dy of the pixel = sum over the <= ceil(ks/stride)^2 windows whose
// argmax is this tap (maxpool_bwd_kernel's arithmetic), kept in fp32.
// W2 (ceil(ks/stride) <= 2): the four candidate windows are read
// unconditionally from clamped addresses and masked, so their 4 dy + 4
// index loads and the caller's x load are all in flight together; one
// blocking load per window leaves the wave latency-bound (the comments
// of bn_act_bwd_reduce_kernel).  Otherwise: a plain loop.
template <typename T, bool W2>
__device__ __forceinline__ void pool_gather_dy(
    const T* __restrict__ dy, const unsigned char* __restrict__ idx,
    const PoolParams& p, int n, int iy, int ix, int c0, float acc[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  // windows (oy, ox) with iy0 <= iy < iy0+ks
  int oy_lo, oy_hi, ox_lo, ox_hi;
  pool_window_range(p, iy, p.Ho, oy_lo, oy_hi);
  pool_window_range(p, ix, p.Wo, ox_lo, ox_hi);
  const int64_t img = (int64_t)n * p.Ho;
  if constexpr (W2) {
    float g[4][8];
    uint2 q[4];
    int t[4];
    bool ok[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      int oy = oy_lo + (w >> 1), ox = ox_lo + (w & 1);
      ok[w] = oy <= oy_hi && ox <= ox_hi;
      oy = min(oy, p.Ho - 1);
      ox = min(ox, p.Wo - 1);
      t[w] = (iy - (oy * p.stride - p.pad)) * p.ks +
             (ix - (ox * p.stride - p.pad));
      int64_t e = ((img + oy) * p.Wo + ox) * p.C + c0;
      load8(dy, e, g[w]);
      q[w] = *(const uint2*)(idx + e);
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (ok[w] && idx_byte(q[w], j) == t[w]) acc[j] += g[w][j];
    }
  } else {
    for (int oy = oy_lo; oy <= oy_hi; ++oy)
      for (int ox = ox_lo; ox <= ox_hi; ++ox) {
        int t = (iy - (oy * p.stride - p.pad)) * p.ks +
                (ix - (ox * p.stride - p.pad));
        int64_t e = ((img + oy) * p.Wo + ox) * p.C + c0;
        float g[8];
        load8(dy, e, g);
        uint2 q = *(const uint2*)(idx + e);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (idx_byte(q, j) == t) acc[j] += g[j];
      }
  }
}

// One sweep over the input pixels for both backward kernels: for every
// pixel, body(element index, x[8], dz[8]) with dz = the gathered dy under
// the ReLU mask recomputed from x.
// GATHER 0 / 1: thread owns one input pixel per iteration
//   (pool_gather_dy<W2 = GATHER>).
// GATHER 2, the 3x3 / stride 2 / pad 1 stem pool: thread owns the 2x2
//   input quad (2qy + a, 2qx + b).  Its four pixels draw on the same four
//   windows (qy + r, qx + c): row 2qy is tap row 1 of window row qy, row
//   2qy+1 is tap row 2 of window row qy and tap row 0 of window row qy+1
//   (columns alike), so the taps are compile-time constants.  Against
//   one pixel per iteration this loads dy and idx once per quad instead
//   of once per pixel, decodes one index instead of four, and tests 9
//   (pixel, window) pairs instead of 16: the per-pixel form was bound by
//   its vector instruction count, not by memory.  4 x + 4 dy + 4 idx
//   loads are in flight per thread.
template <typename T, int GATHER, typename F>
__device__ __forceinline__ void pool_bwd_sweep(
    const T* __restrict__ dy, const unsigned char* __restrict__ idx,
    const T* __restrict__ x, const PoolParams& p, const ChanMap& m,
    const float sc[8], const float sh[8], F body) {
  if constexpr (GATHER == 2) {
    const int Wq = p.Wo, HqWq = p.Ho * p.Wo;   // Ho = ceil(H/2) quad rows
    const int n_quad = p.N * HqWq;
    for (int64_t q = m.p0; q < n_quad; q += m.pstep) {
      int n = (int)q / HqWq;
      int rem = (int)q - n * HqWq;
      int qy = rem / Wq, qx = rem - qy * Wq;
      // second pixel row / column inside the image, second window row /
      // column inside the pooled plane; what is outside is loaded from
      // the first (in-bounds) address and masked
      const bool py1 = 2 * qy + 1 < p.H, px1 = 2 * qx + 1 < p.W;
      const bool wy1 = qy + 1 < p.Ho, wx1 = qx + 1 < p.Wo;
      const int iy[2] = {2 * qy, 2 * qy + (py1 ? 1 : 0)};
      const int ix[2] = {2 * qx, 2 * qx + (px1 ? 1 : 0)};
      const int oy[2] = {qy, qy + (wy1 ? 1 : 0)};
      const int ox[2] = {qx, qx + (wx1 ? 1 : 0)};
      float xv[4][8], g[4][8];
      uint2 iw[4];
      int64_t xi[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        xi[k] = (((int64_t)n * p.H + iy[k >> 1]) * p.W + ix[k & 1]) * p.C +
                m.c0;
        load8(x, xi[k], xv[k]);
      }
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        int64_t e = (((int64_t)n * p.Ho + oy[w >> 1]) * p.Wo + ox[w & 1]) *
                        p.C + m.c0;
        load8(dy, e, g[w]);
        iw[w] = *(const uint2*)(idx + e);
        // a window outside the plane: tap byte 255 matches nothing
        bool wok = ((w >> 1) == 0 || wy1) && ((w & 1) == 0 || wx1);
        if (!wok) { iw[w].x = ~0u; iw[w].y = ~0u; }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int a = k >> 1, b = k & 1;
        float dz[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) dz[j] = 0.f;
        // windows in maxpool_bwd_kernel's order (oy, then ox, ascending)
#pragma unroll
        for (int r = 0; r <= a; ++r) {
#pragma unroll
          for (int c = 0; c <= b; ++c) {
            const int ty = a == 0 ? 1 : (r == 0 ? 2 : 0);
            const int tx = b == 0 ? 1 : (c == 0 ? 2 : 0);
            const int t = ty * 3 + tx, w = r * 2 + c;
#pragma unroll
            for (int j = 0; j < 8; ++j)
              dz[j] += idx_byte(iw[w], j) == t ? g[w][j] : 0.f;
          }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
          dz[j] = bn_relu_stored<T>(sc[j], xv[k][j], sh[j]) > 0.f ? dz[j]
                                                                  : 0.f;
        if ((a == 0 || py1) && (b == 0 || px1)) body(xi[k], xv[k], dz);
      }
    }
  } else {
    const int HW = p.H * p.W;
    const int n_ipix = p.N * HW;
    float xv[8], dz[8];
    for (int64_t ip = m.p0; ip < n_ipix; ip += m.pstep) {
      int n = (int)ip / HW;
      int rem = (int)ip - n * HW;
      int iy = rem / p.W, ix = rem - iy * p.W;
      int64_t i = ip * p.C + m.c0;
      load8(x, i, xv);
      pool_gather_dy<T, GATHER == 1>(dy, idx, p, n, iy, ix, m.c0, dz);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        dz[j] = bn_relu_stored<T>(sc[j], xv[j], sh[j]) > 0.f ? dz[j] : 0.f;
      body(i, xv, dz);
    }
  }
}

// ---- backward pass 1: per-channel sum dz, sum dz*xhat ----
// sums layout: [32 slices][C][2] partials, folded by bn_fold_sums_kernel
// (the slicing and its reason: bn_act_bwd_reduce_kernel).
template <typename T, int GATHER>
__global__ void __launch_bounds__(256) bn_relu_maxpool_bwd_reduce_kernel(
    const T* __restrict__ dy, const unsigned char* __restrict__ idx,
    const T* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ sums,
    PoolParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* lds = (float*)smem_raw;   // [2][C]
  chan_sums_zero<2>(lds, p.C);
  ChanMap m = pool_map8(p.C);
  float sc[8], sh[8], mu[8], is[8];
  load_scale_shift(mean, invstd, gamma, beta, m.c0, sc, sh);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mu[j] = mean[m.c0 + j]; is[j] = invstd[m.c0 + j];
  }
  float s0[8] = {}, s1[8] = {};
  pool_bwd_sweep<T, GATHER>(
      dy, idx, x, p, m, sc, sh,
      [&](int64_t, const float* xv, const float* dz) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float xhat = (xv[j] - mu[j]) * is[j];
          s0[j] += dz[j];
          s1[j] += dz[j] * xhat;
        }
      });
  chan_sums_add<2>(lds, p.C, m.c0, {s0, s1});
  chan_sums_flush<2, true>(lds, p.C, {sums, sums + 1}, 2, p.C * 2);
}

// ---- backward pass 2: dx ----
// sums: folded [C][2] = (sum dz, sum dz*xhat)
template <typename T, int GATHER>
__global__ void __launch_bounds__(256) bn_relu_maxpool_bwd_apply_kernel(
    const T* __restrict__ dy, const unsigned char* __restrict__ idx,
    const T* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ sums,
    T* __restrict__ dx, PoolParams p, float inv_n) {
  ChanMap m = pool_map8(p.C);
  float sc[8], sh[8], mu[8], is[8], sdz_n[8], sdzx_n[8];
  load_scale_shift(mean, invstd, gamma, beta, m.c0, sc, sh);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int cc = m.c0 + j;
    mu[j] = mean[cc]; is[j] = invstd[cc];
    sdz_n[j] = sums[cc * 2 + 0] * inv_n;
    sdzx_n[j] = sums[cc * 2 + 1] * inv_n;
  }
  pool_bwd_sweep<T, GATHER>(
      dy, idx, x, p, m, sc, sh,
      [&](int64_t i, const float* xv, const float* dz) {
        float dxv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float xhat = (xv[j] - mu[j]) * is[j];
          // sc = gamma * invstd
          dxv[j] = sc[j] * (dz[j] - sdz_n[j] - xhat * sdzx_n[j]);
        }
        store8(dx, i, dxv);
      });
}

// how the backward sweeps: 2 = quads of the 3/2/1 pool, 1 = per pixel
// with the four candidate windows unrolled, 0 = per pixel, any window
static int pool_gather_mode(int ks, int stride, int pad) {
  if (ks == 3 && stride == 2 && pad == 1) return 2;
  return (ks + stride - 1) / stride <= 2 ? 1 : 0;
}

// ---------------- launchers ----------------

extern "C" void bdbnn_bn_relu_maxpool_fwd(
    const void* x, const float* mean, const float* invstd,
    const float* gamma, const float* beta, void* out, unsigned char* idx,
    uint32_t* xpk, uint32_t* mpk, int N, int C, int H, int W, int Ho, int Wo,
    int ks, int stride, int pad, bool bf16, hipStream_t stream) {
  PoolParams p{N, C, H, W, Ho, Wo, ks, stride, pad};
  int n_opix = N * Ho * Wo;
  int grid = grid_pix8(n_opix, C);
  with_dtype(bf16, [&](auto t) {
    with_int<3, 2, 0>(ks, [&](auto k) {
      with_bool(xpk != nullptr, [&](auto pack) {
        using T = decltype(t);
        bn_relu_maxpool_fwd_kernel<T, decltype(k)::value,
                                   decltype(pack)::value>
            <<<grid, 256, 0, stream>>>((const T*)x, mean, invstd, gamma,
                                       beta, (T*)out, idx, xpk, mpk, p,
                                       n_opix);
      });
    });
  });
}

// sums32: [32][C][2] scratch, sums: [C][2] result
extern "C" void bdbnn_bn_relu_maxpool_bwd_reduce(
    const void* dy, const unsigned char* idx, const void* x,
    const float* mean, const float* invstd, const float* gamma,
    const float* beta, float* sums32, float* sums, int N, int C, int H,
    int W, int Ho, int Wo, int ks, int stride, int pad, bool bf16,
    hipStream_t stream) {
  (void)hipMemsetAsync(sums32, 0, sizeof(float) * 32 * C * 2, stream);
  PoolParams p{N, C, H, W, Ho, Wo, ks, stride, pad};
  int mode = pool_gather_mode(ks, stride, pad);
  int grid = grid_pix8(mode == 2 ? N * Ho * Wo : N * H * W, C);
  size_t lds = 2 * sizeof(float) * C;
  with_dtype(bf16, [&](auto t) {
    with_int<2, 1, 0>(mode, [&](auto g) {
      using T = decltype(t);
      bn_relu_maxpool_bwd_reduce_kernel<T, decltype(g)::value>
          <<<grid, 256, lds, stream>>>((const T*)dy, idx, (const T*)x, mean,
                                       invstd, gamma, beta, sums32, p);
    });
  });
  bdbnn_bn_fold_sums(sums32, sums, C * 2, stream);
}

extern "C" void bdbnn_bn_relu_maxpool_bwd_apply(
    const void* dy, const unsigned char* idx, const void* x,
    const float* mean, const float* invstd, const float* gamma,
    const float* beta, const float* sums, void* dx, int N, int C, int H,
    int W, int Ho, int Wo, int ks, int stride, int pad, bool bf16,
    hipStream_t stream) {
  PoolParams p{N, C, H, W, Ho, Wo, ks, stride, pad};
  int mode = pool_gather_mode(ks, stride, pad);
  int grid = grid_pix8(mode == 2 ? N * Ho * Wo : N * H * W, C);
  float inv_n = (float)(1.0 / ((double)N * H * W));
  with_dtype(bf16, [&](auto t) {
    with_int<2, 1, 0>(mode, [&](auto g) {
      using T = decltype(t);
      bn_relu_maxpool_bwd_apply_kernel<T, decltype(g)::value>
          <<<grid, 256, 0, stream>>>((const T*)dy, idx, (const T*)x, mean,
                                     invstd, gamma, beta, sums, (T*)dx, p,
                                     inv_n);
    });
  });
}
