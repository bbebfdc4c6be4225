// K8 — fused BatchNorm (+ residual add) (+ PReLU/ReLU) for NHWC, training
// and eval.  Replaces the MIOpen BN pipeline + separate add + activation
// (6+ kernel launches and ~8 tensor passes per block position) with:
//   fwd: stats pass (one read) + normalize/add/act pass (reads x,skip;
//        writes out and the pre-activation z needed by backward)
//   bwd: reduce pass (reads dy,z,x -> per-channel sums + da) +
//        apply pass (reads dy,z,x -> writes dx and dskip)
//
// Memory layout: every thread owns 8 consecutive channels (16-B vector
// loads, guide G13), accumulates channel sums in registers over its pixel
// stripe, and lands one LDS add + one global atomic per owned channel.
// C must be a power of two, 8 <= C <= 1024 (python guards; fallback is
// the composition path).
//
// BN semantics match nn.BatchNorm2d: biased batch var for normalization,
// unbiased var into running_var, momentum update in the finalize step.
// act_kind: 0 = identity, 1 = per-channel PReLU, 2 = ReLU,
// 3 = RPReLU (ReActNet): u = z + b1, out = PReLU_a(u) + b2, with the two
// per-channel fp32 shifts b1 / b2.  The plane saved for backward holds u
// (rounded to the storage type), never z: backward needs the branch u > 0
// and, for da, the value of u, and rounding keeps the sign of u, so both
// directions take the same branch.  u recomputed from a rounded z + b1
// would not.
#include "common.h"
#include "vec8.h"
#include "bn_affine.h"
#include "act_masks.h"

// ---- pass 1: per-channel sum / sumsq ----
template <typename T>
__global__ void bn_stats_kernel(const T* __restrict__ x,
                                float* __restrict__ s1,
                                float* __restrict__ s2,
                                int64_t n_pix, int C) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* lds = (float*)smem_raw;   // [2][C]
  chan_sums_zero<2>(lds, C);
  ChanMap m = chan_map8(C);
  float a1[8] = {}, a2[8] = {};
  // 4 independent pixel loads in flight per wave: one blocking load per
  // iteration leaves the wave latency-bound at ~0.6 B/cyc/CU (34 VGPR,
  // plenty of headroom for the extra 48 registers)
  float v0[8], v1[8], v2[8], v3[8];
  int64_t p = m.p0;
  for (; p + 3 * m.pstep < n_pix; p += 4 * m.pstep) {
    load8(x, p * C + m.c0, v0);
    load8(x, (p + m.pstep) * C + m.c0, v1);
    load8(x, (p + 2 * m.pstep) * C + m.c0, v2);
    load8(x, (p + 3 * m.pstep) * C + m.c0, v3);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a1[j] += v0[j] + v1[j] + v2[j] + v3[j];
      a2[j] += v0[j] * v0[j] + v1[j] * v1[j] + v2[j] * v2[j] +
               v3[j] * v3[j];
    }
  }
  for (; p < n_pix; p += m.pstep) {
    load8(x, p * C + m.c0, v0);
#pragma unroll
    for (int j = 0; j < 8; ++j) { a1[j] += v0[j]; a2[j] += v0[j] * v0[j]; }
  }
  chan_sums_add<2>(lds, C, m.c0, {a1, a2});
  // 32-way sliced output (s1, s2: [32][C] each, folded by bn_finalize)
  chan_sums_flush<2, true>(lds, C, {s1, s2}, 1, C);
}

// ---- finalize: mean/invstd + running-stat update ----
// nslice > 1: s1/s2 are [nslice][C] partial sums (the conv epilogue's
// 32-way sliced accumulators) — summed here, where it costs nothing.
__global__ void bn_finalize_kernel(const float* __restrict__ s1,
                                   const float* __restrict__ s2,
                                   float* __restrict__ mean,
                                   float* __restrict__ invstd,
                                   float* __restrict__ running_mean,
                                   float* __restrict__ running_var,
                                   int C, float n, float momentum, float eps,
                                   int nslice) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float a1 = 0.f, a2 = 0.f;
  for (int j = 0; j < nslice; ++j) {
    a1 += s1[j * C + c];
    a2 += s2[j * C + c];
  }
  float m = a1 / n;
  float var = fmaxf(a2 / n - m * m, 0.f);
  mean[c] = m;
  invstd[c] = rsqrtf(var + eps);
  if (running_mean != nullptr) {
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * m;
    float var_unb = var * n / fmaxf(n - 1.f, 1.f);
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * var_unb;
  }
}

// ---- pass 2: normalize + add + act (+ next conv's sign/mask pack) ----
// PACK: the consuming binary conv's sign + clip-STE-mask bitplanes are
// assembled in the epilogue from the ROUNDED stored values (bit-exact
// with csrc/pack.hip sign_mask_pack_kernel on the written tensor), so
// that conv never re-reads the activation to pack it.  Each thread owns
// 8 consecutive channels -> one byte of each plane, combined across the 4
// lanes of a word by pack_sign_mask8 (act_masks.h).
template <typename T, int ACT, bool PACK>
__global__ void bn_act_fwd_kernel(const T* __restrict__ x,
                                  const T* __restrict__ skip,
                                  const float* __restrict__ mean,
                                  const float* __restrict__ invstd,
                                  const float* __restrict__ gamma,
                                  const float* __restrict__ beta,
                                  const float* __restrict__ a,
                                  const float* __restrict__ b1,
                                  const float* __restrict__ b2,
                                  T* __restrict__ out, T* __restrict__ zout,
                                  int64_t n_pix, int C,
                                  uint32_t* __restrict__ xpk,
                                  uint32_t* __restrict__ mpk) {
  ChanMap m = chan_map8(C);
  float sc[8], sh[8], av[8], b2v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int cc = m.c0 + j;
    bn_scale_shift(gamma[cc], beta[cc], mean[cc], invstd[cc], sc[j], sh[j]);
    av[j] = (ACT == 1 || ACT == 3) ? a[cc] : 0.f;
    // RPReLU: the first shift rides in the affine's constant, so z below
    // is u = BN(x) + b1 (+ skip) at no register or instruction cost
    if (ACT == 3) sh[j] += b1[cc];
    b2v[j] = (ACT == 3) ? b2[cc] : 0.f;
  }
  const int sub = threadIdx.x & 3;       // byte slot within the word
  const int64_t cw = m.c0 >> 5;            // word column (lane sub == 0)
  const int CW = C >> 5;
  float v[8], s[8], z[8], o[8];
  for (int64_t p = m.p0; p < n_pix; p += m.pstep) {
    int64_t i = p * C + m.c0;
    load8(x, i, v);
    if (skip != nullptr) load8(skip, i, s);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      z[j] = bn_affine(sc[j], v[j], sh[j]);
      if (skip != nullptr) z[j] += s[j];
      o[j] = z[j];
      if (ACT == 1) o[j] = z[j] > 0.f ? z[j] : av[j] * z[j];
      else if (ACT == 2) o[j] = bn_relu(z[j]);
      else if (ACT == 3) o[j] = (z[j] > 0.f ? z[j] : av[j] * z[j]) + b2v[j];
    }
    store8(out, i, o);
    if (zout != nullptr) store8(zout, i, z);
    if constexpr (PACK) {
      float r[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = round_storage<T>(o[j]);
      pack_sign_mask8(r, sub, xpk, mpk, p * CW + cw);
    }
  }
}

// ---- backward pass 1: per-channel reductions ----
// sums layout: [32 slices][C][NR] = (sum dz, sum dz*xhat, da) partials,
// NR = bdbnn_bn_sum_rows(ACT) (api.h): RPReLU adds a fourth row, sum dy
// (= db2; db1 is sum dz, the same number as dbeta).  32-way sliced so the
// end-of-kernel global atomics see 1/32 of the per-word contention (2048
// blocks onto 3C words measured as a >20 us serial tail);
// bn_fold_sums_kernel folds the slices.
template <typename T, int ACT>
__global__ void bn_act_bwd_reduce_kernel(
    const T* __restrict__ dy, const T* __restrict__ z,
    const T* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ a,
    float* __restrict__ sums, int64_t n_pix, int C) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  constexpr int NR = bdbnn_bn_sum_rows(ACT);
  float* lds = (float*)smem_raw;   // [NR][C]
  chan_sums_zero<NR>(lds, C);
  ChanMap m = chan_map8(C);
  float mu[8], is[8], av[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int cc = m.c0 + j;
    mu[j] = mean[cc]; is[j] = invstd[cc];
    av[j] = (ACT == 1 || ACT == 3) ? a[cc] : 0.f;
  }
  float s0[8] = {}, s1[8] = {}, s2[8] = {}, s3[8] = {};
  // 2 pixel iterations in flight (6 independent loads): one blocking
  // triple per iteration leaves the wave latency-bound.  (The r1
  // attempt unrolled with a COMBINED body and regressed on register
  // pressure; issuing the loads up front then reducing keeps liveness
  // to the 6 vector buffers.)
  float dyv[8], zv[8], xv[8], dyw[8], zw[8], xw[8];
#define BN_RED_BODY(DYV, ZV, XV)                                          \
  {                                                                       \
    _Pragma("unroll")                                                     \
    for (int j = 0; j < 8; ++j) {                                         \
      float dz = DYV[j];                                                  \
      if (ACT == 1 || ACT == 3) {                                         \
        dz = ZV[j] > 0.f ? DYV[j] : av[j] * DYV[j];                       \
        if (ZV[j] <= 0.f) s2[j] += DYV[j] * ZV[j];                        \
        if (ACT == 3) s3[j] += DYV[j];                                    \
      } else if (ACT == 2) {                                              \
        dz = ZV[j] > 0.f ? DYV[j] : 0.f;                                  \
      }                                                                   \
      float xhat = (XV[j] - mu[j]) * is[j];                               \
      s0[j] += dz;                                                        \
      s1[j] += dz * xhat;                                                 \
    }                                                                     \
  }
  int64_t p = m.p0;
  for (; p + m.pstep < n_pix; p += 2 * m.pstep) {
    int64_t i = p * C + m.c0;
    int64_t i2 = (p + m.pstep) * C + m.c0;
    load8(dy, i, dyv);
    load8(x, i, xv);
    if (ACT != 0) load8(z, i, zv);
    load8(dy, i2, dyw);
    load8(x, i2, xw);
    if (ACT != 0) load8(z, i2, zw);
    BN_RED_BODY(dyv, zv, xv)
    BN_RED_BODY(dyw, zw, xw)
  }
  for (; p < n_pix; p += m.pstep) {
    int64_t i = p * C + m.c0;
    load8(dy, i, dyv);
    load8(x, i, xv);
    if (ACT != 0) load8(z, i, zv);
    BN_RED_BODY(dyv, zv, xv)
  }
#undef BN_RED_BODY
  // da (row 2) is PReLU's and RPReLU's only; the row stays zero and is
  // skipped otherwise.  Row 3 (sum dy) exists for RPReLU alone.
  if constexpr (ACT == 3) {
    chan_sums_add<4>(lds, C, m.c0, {s0, s1, s2, s3});
    chan_sums_flush<4, true>(lds, C, {sums, sums + 1, sums + 2, sums + 3},
                             NR, C * NR);
  } else {
    if (ACT == 1) chan_sums_add<3>(lds, C, m.c0, {s0, s1, s2});
    else          chan_sums_add<2>(lds, C, m.c0, {s0, s1});
    chan_sums_flush<3, true>(lds, C, {sums, sums + 1, sums + 2}, NR, C * NR);
  }
}

// fold the 32 slices -> [C][NR] (tiny; launched right after the reduce)
__global__ void bn_fold_sums_kernel(const float* __restrict__ sums32,
                                    float* __restrict__ out, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v = 0.f;
#pragma unroll
  for (int s = 0; s < 32; ++s) v += sums32[s * n + i];
  out[i] = v;
}

// ---- backward pass 2: dx (+ dskip) ----
template <typename T, int ACT>
__global__ void bn_act_bwd_apply_kernel(
    const T* __restrict__ dy, const T* __restrict__ z,
    const T* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ gamma,
    const float* __restrict__ a, const float* __restrict__ sums,
    T* __restrict__ dx, T* __restrict__ dskip, int64_t n_pix, int C,
    float inv_n) {
  constexpr int NR = bdbnn_bn_sum_rows(ACT);
  ChanMap m = chan_map8(C);
  float mu[8], is[8], gis[8], av[8], sdz_n[8], sdzx_n[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int cc = m.c0 + j;
    mu[j] = mean[cc]; is[j] = invstd[cc];
    gis[j] = gamma[cc] * is[j];
    av[j] = (ACT == 1 || ACT == 3) ? a[cc] : 0.f;
    sdz_n[j] = sums[cc * NR + 0] * inv_n;
    sdzx_n[j] = sums[cc * NR + 1] * inv_n;
  }
  // 2 pixel iterations in flight (up to 6 independent loads): one
  // blocking triple per iteration leaves the wave latency-bound
  float dyv[8], zv[8], xv[8], dxv[8], dzv[8];
  float dyw[8], zw[8], xw[8];
#define BN_APPLY_BODY(DYV, ZV, XV, I)                                     \
  {                                                                       \
    _Pragma("unroll")                                                     \
    for (int j = 0; j < 8; ++j) {                                         \
      float dz = DYV[j];                                                  \
      if (ACT == 1 || ACT == 3)                                           \
        dz = ZV[j] > 0.f ? DYV[j] : av[j] * DYV[j];                       \
      else if (ACT == 2) dz = ZV[j] > 0.f ? DYV[j] : 0.f;                 \
      float xhat = (XV[j] - mu[j]) * is[j];                               \
      dxv[j] = gis[j] * (dz - sdz_n[j] - xhat * sdzx_n[j]);               \
      dzv[j] = dz;                                                        \
    }                                                                     \
    store8(dx, I, dxv);                                                   \
    if (dskip != nullptr) store8(dskip, I, dzv);                          \
  }
  int64_t p = m.p0;
  for (; p + m.pstep < n_pix; p += 2 * m.pstep) {
    int64_t i = p * C + m.c0;
    int64_t i2 = (p + m.pstep) * C + m.c0;
    load8(dy, i, dyv);
    load8(x, i, xv);
    if (ACT != 0) load8(z, i, zv);
    load8(dy, i2, dyw);
    load8(x, i2, xw);
    if (ACT != 0) load8(z, i2, zw);
    BN_APPLY_BODY(dyv, zv, xv, i)
    BN_APPLY_BODY(dyw, zw, xw, i2)
  }
  for (; p < n_pix; p += m.pstep) {
    int64_t i = p * C + m.c0;
    load8(dy, i, dyv);
    load8(x, i, xv);
    if (ACT != 0) load8(z, i, zv);
    BN_APPLY_BODY(dyv, zv, xv, i)
  }
#undef BN_APPLY_BODY
}

// ---- eval-mode fused normalize(+add)(+act) using running stats ----
template <typename T, int ACT>
__global__ void bn_act_eval_kernel(const T* __restrict__ x,
                                   const T* __restrict__ skip,
                                   const float* __restrict__ rm,
                                   const float* __restrict__ rv,
                                   const float* __restrict__ gamma,
                                   const float* __restrict__ beta,
                                   const float* __restrict__ a,
                                   const float* __restrict__ b1,
                                   const float* __restrict__ b2,
                                   T* __restrict__ out, int64_t n_pix, int C,
                                   float eps) {
  ChanMap m = chan_map8(C);
  float sc[8], sh[8], av[8], b2v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int cc = m.c0 + j;
    bn_eval_scale_shift(gamma[cc], beta[cc], rm[cc], rv[cc], eps, sc[j],
                        sh[j]);
    av[j] = (ACT == 1 || ACT == 3) ? a[cc] : 0.f;
    if (ACT == 3) sh[j] += b1[cc];   // as in bn_act_fwd_kernel
    b2v[j] = (ACT == 3) ? b2[cc] : 0.f;
  }
  float v[8], s[8], o[8];
  for (int64_t p = m.p0; p < n_pix; p += m.pstep) {
    int64_t i = p * C + m.c0;
    load8(x, i, v);
    if (skip != nullptr) load8(skip, i, s);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      o[j] = bn_eval_act<ACT>(sc[j], v[j], sh[j], skip != nullptr, s[j],
                              av[j], b2v[j]);
    store8(out, i, o);
  }
}

// the eval kernel's folded (sc, sh) on their own, computed on the device by
// the same function: what the inference engine folds once per BN and hands
// to the fused conv epilogue (xnor_conv_mfma.hip) equals, bit for bit, what
// bn_act_eval_kernel computes for itself on every launch
__global__ void bn_fold_kernel(const float* __restrict__ gamma,
                               const float* __restrict__ beta,
                               const float* __restrict__ rm,
                               const float* __restrict__ rv,
                               const float* __restrict__ b1,
                               float* __restrict__ sc, float* __restrict__ sh,
                               int C, float eps) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s, h;
  bn_eval_scale_shift(gamma[c], beta[c], rm[c], rv[c], eps, s, h);
  if (b1 != nullptr) h += b1[c];   // RPReLU
  sc[c] = s;
  sh[c] = h;
}

// ---------------- launchers ----------------

extern "C" void bdbnn_bn_stats(const void* x, float* s1, float* s2,
                               int64_t n, int C, bool bf16,
                               hipStream_t stream) {
  hipMemsetAsync(s1, 0, sizeof(float) * 32 * C, stream);
  hipMemsetAsync(s2, 0, sizeof(float) * 32 * C, stream);
  int64_t n_pix = n / C;
  int grid = grid_pix8(n_pix, C);
  size_t lds = 2 * sizeof(float) * C;
  with_dtype(bf16, [&](auto t) {
    using T = decltype(t);
    bn_stats_kernel<T><<<grid, 256, lds, stream>>>((const T*)x, s1, s2,
                                                   n_pix, C);
  });
}

extern "C" void bdbnn_bn_finalize(const float* s1, const float* s2,
                                  float* mean, float* invstd,
                                  float* running_mean, float* running_var,
                                  int C, float n, float momentum, float eps,
                                  int nslice, hipStream_t stream) {
  bn_finalize_kernel<<<(C + 255) / 256, 256, 0, stream>>>(
      s1, s2, mean, invstd, running_mean, running_var, C, n, momentum, eps,
      nslice);
}

extern "C" void bdbnn_bn_act_fwd(const void* x, const void* skip,
                                 const float* mean, const float* invstd,
                                 const float* gamma, const float* beta,
                                 const float* a, const float* b1,
                                 const float* b2, void* out, void* zout,
                                 int64_t n, int C, int act_kind,
                                 uint32_t* xpk, uint32_t* mpk, bool bf16,
                                 hipStream_t stream) {
  int64_t n_pix = n / C;
  int grid = grid_pix8(n_pix, C);
  with_dtype(bf16, [&](auto t) {
    with_int<1, 2, 3, 0>(act_kind, [&](auto act) {
      with_bool(xpk != nullptr, [&](auto pack) {
        using T = decltype(t);
        bn_act_fwd_kernel<T, decltype(act)::value, decltype(pack)::value>
            <<<grid, 256, 0, stream>>>((const T*)x, (const T*)skip, mean,
                                       invstd, gamma, beta, a, b1, b2,
                                       (T*)out, (T*)zout, n_pix, C, xpk,
                                       mpk);
      });
    });
  });
}

extern "C" void bdbnn_bn_act_bwd_reduce(const void* dy, const void* z,
                                        const void* x, const float* mean,
                                        const float* invstd, const float* a,
                                        float* sums32, float* sums,
                                        int64_t n, int C, int act_kind,
                                        bool bf16, hipStream_t stream) {
  const int NR = bdbnn_bn_sum_rows(act_kind);
  hipMemsetAsync(sums32, 0, sizeof(float) * 32 * C * NR, stream);
  int64_t n_pix = n / C;
  int grid = grid_pix8(n_pix, C);
  size_t lds = NR * sizeof(float) * C;
  with_dtype(bf16, [&](auto t) {
    with_int<1, 2, 3, 0>(act_kind, [&](auto act) {
      using T = decltype(t);
      bn_act_bwd_reduce_kernel<T, decltype(act)::value>
          <<<grid, 256, lds, stream>>>((const T*)dy, (const T*)z,
                                       (const T*)x, mean, invstd, a, sums32,
                                       n_pix, C);
    });
  });
  bn_fold_sums_kernel<<<(C * NR + 255) / 256, 256, 0, stream>>>(
      sums32, sums, C * NR);
}

// the slice fold on its own, for csrc/bn_pool.hip's reduce
extern "C" void bdbnn_bn_fold_sums(const float* sums32, float* sums, int n,
                                   hipStream_t stream) {
  bn_fold_sums_kernel<<<(n + 255) / 256, 256, 0, stream>>>(sums32, sums, n);
}

extern "C" void bdbnn_bn_act_bwd_apply(const void* dy, const void* z,
                                       const void* x, const float* mean,
                                       const float* invstd,
                                       const float* gamma, const float* a,
                                       const float* sums, void* dx,
                                       void* dskip, int64_t n, int C,
                                       int act_kind, float inv_n, bool bf16,
                                       hipStream_t stream) {
  int64_t n_pix = n / C;
  int grid = grid_pix8(n_pix, C);
  with_dtype(bf16, [&](auto t) {
    with_int<1, 2, 3, 0>(act_kind, [&](auto act) {
      using T = decltype(t);
      bn_act_bwd_apply_kernel<T, decltype(act)::value>
          <<<grid, 256, 0, stream>>>((const T*)dy, (const T*)z, (const T*)x,
                                     mean, invstd, gamma, a, sums, (T*)dx,
                                     (T*)dskip, n_pix, C, inv_n);
    });
  });
}

extern "C" void bdbnn_bn_act_eval(const void* x, const void* skip,
                                  const float* rm, const float* rv,
                                  const float* gamma, const float* beta,
                                  const float* a, const float* b1,
                                  const float* b2, void* out, int64_t n,
                                  int C, int act_kind, float eps, bool bf16,
                                  hipStream_t stream) {
  int64_t n_pix = n / C;
  int grid = grid_pix8(n_pix, C);
  with_dtype(bf16, [&](auto t) {
    with_int<1, 2, 3, 0>(act_kind, [&](auto act) {
      using T = decltype(t);
      bn_act_eval_kernel<T, decltype(act)::value><<<grid, 256, 0, stream>>>(
          (const T*)x, (const T*)skip, rm, rv, gamma, beta, a, b1, b2,
          (T*)out, n_pix, C, eps);
    });
  });
}

extern "C" void bdbnn_bn_fold(const float* gamma, const float* beta,
                              const float* rm, const float* rv,
                              const float* b1, float* sc, float* sh, int C,
                              float eps, hipStream_t stream) {
  bn_fold_kernel<<<(C + 255) / 256, 256, 0, stream>>>(gamma, beta, rm, rv, b1,
                                                      sc, sh, C, eps);
}
