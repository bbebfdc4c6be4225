// Stride-1 3x3 weight gradient, v3: the wgrad2 GEMM (conv_bwd.hip)
//
//   dwT[t][c][k] = sum_m xb[pix(m) + Delta_t][c] * g[pix(m)][k]
//
// with both operands staged PIXEL-MAJOR in LDS — one 128-byte row of 64
// channels per pixel — and read through gfx950's transposing
// ds_read_b64_tr_b16, which hands each lane 4 consecutive pixels of one
// channel: the m-contiguous fragment both MFMA operands want.
//
//   g image  [2 stages][128 m][64 k]: the coalesced global rows, stored
//            as they arrive (ds_write_b128, no transpose).
//   X image  [plane][x = -1 .. WP][64 c]: sign(x) decoded ONCE per pixel
//            straight from the NHWC sign plane xp of the forward (a word
//            of 32 bits -> 64 bytes through the byte LUT).  A tap is a
//            pixel offset (dy planes, dx pixels), aligned by construction,
//            so wgrad2's three shifted copies and its channel-major
//            repack (repack_cplane) are not needed.  Pad rows, the two
//            halo columns and the dummy columns x >= W are zeros.
//
// The planes are a ring with room for two windows: while chunk i is
// multiplied, the loads of chunk i+1 are in flight and are decoded into
// the free planes / the other g stage right after the wave's MFMAs, so a
// chunk costs ONE barrier.
//
// Class geometry (WP, RB, GB), chunking, m-split, wave decomposition and
// the slab output contract are wgrad2's (conv_bwd_common.h).
#include "conv_bwd_common.h"

typedef __attribute__((ext_vector_type(4))) short wg3_s16x4;
typedef __attribute__((ext_vector_type(8))) short wg3_s16x8;

// Byte offset of byte cb (0..127) of pixel row pix.  The 64-byte halves
// swap on every second pixel PAIR: a 32-lane half of a transposed read
// takes 4 consecutive pixels x 64 contiguous bytes, and with this swap
// those land on 4 distinct quarters of the 256-byte bank row for ANY
// first pixel (taps shift it by arbitrary amounts): (pix & 1) picks bit
// 5 of the bank, (pix & 2) ^ half bit 4.
__device__ __forceinline__ int wg3_off(int pix, int cb) {
  return pix * 128 + (cb ^ ((pix & 2) << 5));
}

// ds_read_b64_tr_b16: EXEC must be all ones here (no divergence around
// any call), every lane passes an in-bounds 8-byte-aligned address
__device__ __forceinline__ wg3_s16x4 wg3_tr_read(const char* base, int off) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) wg3_s16x4*)(base + off));
}

__device__ __forceinline__ bf16x8 wg3_frag(wg3_s16x4 lo, wg3_s16x4 hi) {
  wg3_s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

// The 36 MFMAs of one wave on one chunk: its 64-m half in 4 steps of 16,
// all 9 taps each.  pb = plane of the chunk's window row 0.
template <int WP, int RB, int GB>
__device__ __forceinline__ void wg3_chunk_mfma(
    f32x16 (&acc)[9], const char* X, const char* Gs, int pb, int ms_grp,
    int lhalf, int tq, int a_cb, int b_cb) {
  constexpr int WR = RB + 2, XW = WP + 2;
  constexpr int XPL = GB == 1 ? 2 * RB + 4 : 2 * GB * WR;
  constexpr int LGWP = WP == 8 ? 3 : WP == 16 ? 4 : WP == 32 ? 5 : 6;
#pragma unroll
  for (int msl = 0; msl < 4; ++msl) {
    // this lane's 8 m: two runs of 4 pixels, the second 4 pixels on
    // (same row: WP >= 8; same swizzle: +4 keeps pix & 2)
    const int mrun = ms_grp * 64 + msl * 16 + lhalf * 8;
    const int boff = wg3_off(mrun + tq, b_cb);
    bf16x8 bfrag = wg3_frag(wg3_tr_read(Gs, boff),
                            wg3_tr_read(Gs, boff + 4 * 128));
    const int rl = mrun >> LGWP;
    const int band = rl / RB, rloc = rl - band * RB;
    // window column of pixel (x + tq) at dx = 0 (x = -1 is column 0)
    const int xq = (mrun & (WP - 1)) + tq;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      int plane = pb + band * WR + rloc + dy;
      if (plane >= XPL) plane -= XPL;
      const int pix0 = plane * XW + xq;
#pragma unroll
      for (int dxs = 0; dxs < 3; ++dxs) {
        const int aoff = wg3_off(pix0 + dxs, a_cb);
        bf16x8 afrag = wg3_frag(wg3_tr_read(X, aoff),
                                wg3_tr_read(X, aoff + 4 * 128));
        acc[dy * 3 + dxs] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            afrag, bfrag, acc[dy * 3 + dxs], 0, 0, 0);
      }
    }
  }
}

template <int WP, int RB, int GB>
__global__ __launch_bounds__(512, 2) void conv_wgrad3_kernel(
    const __bf16* __restrict__ g, const uint32_t* __restrict__ xp32,
    float* __restrict__ dwT, Wgrad2Params p, int grid_ck) {
  constexpr int WR = RB + 2;              // window rows of a band (halo)
  constexpr int XW = WP + 2;              // pixels of a plane (x = -1..WP)
  constexpr bool RING = (GB == 1);        // GB>1: bands are whole images
  // RING: a continuation chunk adds RB planes, a fresh window WR; either
  // must fit beside the WR planes being read.  !RING: two whole stages.
  constexpr int XPL = RING ? 2 * RB + 4 : 2 * GB * WR;
  constexpr int LGWP = WP == 8 ? 3 : WP == 16 ? 4 : WP == 32 ? 5 : 6;
  constexpr int XITEMS = GB * WR * XW * 2;    // 64-byte decode targets
  constexpr int XIT = (XITEMS + 511) / 512;

  const int tid = threadIdx.x;
  const int wg = bd_xcd_remap(blockIdx.x, gridDim.x);
  const int ck = wg % grid_ck;            // (c,k) tile
  const int split_id = wg / grid_ck;
  const int c_blk = ck % (p.C / WG2_BC);
  const int k_blk = ck / (p.C / WG2_BC);
  const int c0 = c_blk * WG2_BC, k0 = k_blk * WG2_BK;

  __shared__ __align__(16) char X[XPL * XW * 128];
  __shared__ __align__(16) char G[2][WG2_CHUNK * 128];
  __shared__ __align__(16) __bf16 lut[256][8];
  __shared__ float red[4][32][32];        // m-split combine scratch

  wgrad2_fill_sign_lut(lut, tid);

  // ---- wave decomposition: quad (c-half, k-half) x m-split ----
  const int wid = tid >> 6, lane = tid & 63;
  const int qc = (wid >> 1) & 1, qk = wid & 1, ms_grp = wid >> 2;
  const int lhalf = lane >> 5;
  // transposed-read role of the lane inside its 16-lane group: it passes
  // the address of pixel +tq, channels 4*tp .. 4*tp+3 of the group's 16,
  // and receives channel (lane & 15) of the group's 4 pixels
  const int tq = (lane & 15) >> 2, tp = lane & 3, tgrp = (lane >> 4) & 1;
  const int a_cb = (qc * 32 + tgrp * 16 + tp * 4) * 2;   // byte in X row
  const int b_cb = (qk * 32 + tgrp * 16 + tp * 4) * 2;   // byte in g row

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

  // contiguous chunk range of this split block
  const int cpb = (p.total_chunks + p.split - 1) / p.split;
  const int ch_lo = split_id * cpb;
  const int ch_hi = bd_min(ch_lo + cpb, p.total_chunks);
  const int n_chunks = ch_hi - ch_lo;   // may be 0: slab still written
  int ch = ch_lo;

  // g staging: a thread owns 16 k of ONE pixel (4 lanes = one 128-byte
  // row, coalesced) and stores them as two 16-byte pieces of that row.
  // Loads run one chunk ahead of the MFMAs (two chunks ahead, with a
  // second register set, measured no faster).
  const int sg_m = tid >> 2;              // 0..127
  const int sg_k16 = (tid & 3) * 16;
  uint4 gregA[2];

  // block-uniform per-band facts of a chunk
  int u_n[GB], u_y0[GB];
  bool u_vs[GB];
#define CHUNK_INFO(chunk)                                                 \
  {                                                                       \
    _Pragma("unroll")                                                     \
    for (int b = 0; b < GB; ++b) {                                        \
      int slot = (chunk)*GB + b;                                          \
      u_vs[b] = slot < p.total_slots;                                     \
      int n = slot / p.bands_per_image;                                   \
      u_n[b] = n;                                                         \
      u_y0[b] = (slot - n * p.bands_per_image) * RB;                      \
    }                                                                     \
  }

// (uses the CHUNK_INFO of the same chunk — call order guarantees it)
#define G_LOAD(greg)                                                      \
  {                                                                       \
    int band = sg_m / (RB * WP);                                          \
    int rem = sg_m - band * (RB * WP);                                    \
    int x = rem & (WP - 1);                                               \
    uint4 z{0, 0, 0, 0};                                                  \
    greg[0] = z; greg[1] = z;                                             \
    if (u_vs[band] && x < p.W) {                                          \
      int y = u_y0[band] + (rem >> LGWP);                                 \
      if (y < p.H) {                                                      \
        const __bf16* src =                                               \
            g + ((int64_t)(u_n[band] * p.H + y) * p.W + x) * p.K + k0 +   \
            sg_k16;                                                       \
        greg[0] = *(const uint4*)src;                                     \
        greg[1] = *(const uint4*)(src + 8);                               \
      }                                                                   \
    }                                                                     \
  }
#define G_WRITE(buf, greg)                                                \
  {                                                                       \
    char* dst = G[buf] + wg3_off(sg_m, sg_k16 * 2);                       \
    *(uint4*)dst = greg[0];                                               \
    *(uint4*)(dst + 16) = greg[1];                                        \
  }

  // ---- sign bits of the window rows [r0, r0+NR) of every band: one
  // 32-channel WORD (half a pixel row) per decode target, loaded into a
  // register next to the target's LDS offset: -1 nothing to write, bit 0
  // clear = zeros (pad rows, halo and dummy columns), bit 0 set = the 4
  // bytes through the LUT.  pbase is the plane of window row 0 of band 0.
  int xwA[XIT], xoA[XIT];
  const int cw = p.C / 32;
#define XB_LOAD(r0, NR, pbase, xw, xo)                                    \
  {                                                                       \
    _Pragma("unroll")                                                     \
    for (int it = 0; it < XIT; ++it) {                                    \
      int i = tid + it * 512;                                             \
      int v = 0, o = -1;                                                  \
      if (i < GB * (NR) * XW * 2) {                                       \
        int h = i & 1, px = i >> 1;                                       \
        int col = px % XW;                                                \
        int rem = px / XW;                                                \
        int w = (r0) + rem % (NR);                                        \
        int band = rem / (NR);                                            \
        int x = col - 1, y = u_y0[band] + w - 1;                          \
        int plane = (pbase) + band * WR + w;                              \
        if (plane >= XPL) plane -= XPL;                                   \
        o = wg3_off(plane * XW + col, h * 64);                            \
        if (u_vs[band] && x >= 0 && x < p.W && y >= 0 && y < p.H) {       \
          v = xp32[((int64_t)(u_n[band] * p.H + y) * p.W + x) * cw +      \
                   (c0 >> 5) + h];                                        \
          o |= 1;                                                         \
        }                                                                 \
      }                                                                   \
      xw[it] = v;                                                         \
      xo[it] = o;                                                         \
    }                                                                     \
  }
#define XB_WRITE(xw, xo)                                                  \
  {                                                                       \
    _Pragma("unroll")                                                     \
    for (int it = 0; it < XIT; ++it) {                                    \
      if (xo[it] >= 0) {                                                  \
        char* dst = X + (xo[it] & ~1);                                    \
        const bool on = xo[it] & 1;                                       \
        _Pragma("unroll")                                                 \
        for (int jj = 0; jj < 4; ++jj) {                                  \
          uint4 vv{0, 0, 0, 0};                                           \
          if (on)                                                         \
            vv = *(const uint4*)&lut[((unsigned)xw[it] >> (8 * jj)) &     \
                                     255u][0];                            \
          *(uint4*)(dst + jj * 16) = vv;                                  \
        }                                                                 \
      }                                                                   \
    }                                                                     \
  }

  // continuation = same image's next band (GB==1 ranges walk bands in
  // order; a new image or the range start decodes the full window)
#define IS_CONT(chunk) \
  (RING && (chunk) > ch_lo && ((chunk) % p.bands_per_image) != 0)
// plane of window row 0 of `chunk`, from its predecessor's
#define PB_NEXT(pbprev, chunk)                                            \
  (((pbprev) + (IS_CONT(chunk) ? RB : GB * WR)) % XPL)
// all global loads of `chunk` whose window starts at plane pbase
#define LOADS(chunk, pbase, greg, xw, xo)                                 \
  {                                                                       \
    CHUNK_INFO(chunk);                                                    \
    if (IS_CONT(chunk)) XB_LOAD(2, RB, pbase, xw, xo)                     \
    else XB_LOAD(0, WR, pbase, xw, xo)                                    \
    G_LOAD(greg);                                                         \
  }

  // planes of window row 0 of chunk ci and ci+1
  int pb0 = 0, pb1 = 0;
  if (n_chunks > 0) {
    LOADS(ch, 0, gregA, xwA, xoA);
    __syncthreads();                      // lut filled
    XB_WRITE(xwA, xoA);
    G_WRITE(0, gregA);
  }
  int gb = 0;

  for (int ci = 0; ci < n_chunks; ++ci) {
    // chunk ci's images are visible; everyone is done reading chunk
    // ci-1's, which are the planes / g stage written below
    __syncthreads();
    if (ci + 1 < n_chunks) {
      pb1 = PB_NEXT(pb0, ch + 1);
      LOADS(ch + 1, pb1, gregA, xwA, xoA);  // land during the MFMAs
    }
    wg3_chunk_mfma<WP, RB, GB>(acc, X, G[gb], pb0, ms_grp, lhalf, tq, a_cb,
                               b_cb);
    if (ci + 1 < n_chunks) {
      XB_WRITE(xwA, xoA);
      G_WRITE(gb ^ 1, gregA);
    }
    gb ^= 1;
    pb0 = pb1;
    ++ch;
  }

  // ---- m-split combine + plain coalesced slab store ----
  wgrad2_combine_store<9>(acc, red, dwT + (int64_t)split_id * 9 * p.C * p.K,
                          p.C, p.K, c0, k0, wid, lane);
}

// Classes routed to this kernel by default: those whose whole measured
// range lies below repack_cplane + conv_wgrad2's at batch 2048
// (benchmarks/RESULTS.md); the others keep wgrad2.  The kernel itself
// runs every class (bdbnn_conv_wgrad3 takes any wgrad2 shape).
static bool wgrad3_class_routed(int WP) {
  return WP == 64 || WP == 32 || WP == 16 || WP == 8;
}

extern "C" int bdbnn_wgrad3_supported(int H, int W, int C, int K) {
  if (H < 1 || W < 1 || C < 64 || K < 64 || !wgrad2_shape_ok(W, C, K))
    return 0;
  return wgrad2_class(H, W, [&](auto cls) {
    return (int)wgrad3_class_routed(decltype(cls)::WP);
  });
}

// slab count for the host-side dwT allocation (wgrad2's m-split)
extern "C" int bdbnn_wgrad3_nslab(int N, int H, int W, int C, int K) {
  if (!wgrad2_shape_ok(W, C, K)) return -1;
  return wgrad2_class(H, W, [&](auto cls) {
    return wgrad2_params(cls, N, H, W, C, K).split;
  });
}

// xp: the NHWC sign plane [N][H][W][C/32] (bit c of a word = x >= 0)
extern "C" int bdbnn_conv_wgrad3(const void* g, const uint32_t* xp,
                                 float* dwT, int N, int H, int W, int C,
                                 int K, hipStream_t stream) {
  if (!wgrad2_shape_ok(W, C, K)) return -1;
  return wgrad2_class(H, W, [&](auto cls) {
    using G = decltype(cls);
    Wgrad2Params p = wgrad2_params(cls, N, H, W, C, K);
    int grid_ck = (C / WG2_BC) * (K / WG2_BK);
    dim3 grid(grid_ck * p.split);
    conv_wgrad3_kernel<G::WP, G::RB, G::GB><<<grid, 512, 0, stream>>>(
        (const __bf16*)g, xp, dwT, p, grid_ck);
    return 0;
  });
}
