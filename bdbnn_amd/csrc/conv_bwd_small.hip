// MFMA bf16 backward of the 3x3/stride-1/pad-1 binary convolutions with 16
// or 32 channels on either side (the first two stages of CIFAR ResNet-20):
//
//   conv_dgrad_small   dx[n,y,x,c] = mask * sum_{t,k} g[n,y+dy-1,x+dx-1,k]
//                                    * wd[t][c][k]  (+ skip gradient)
//   conv_wgrad_small   dwT[t][c][k] = sum_m xb[pix(m)+Delta_t][c] * g[pix(m)][k]
//
// the contracts of conv_dgrad2 (conv_bwd.hip) and conv_wgrad3
// (conv_wgrad3.hip), whose tiles want multiples of 64 channels.  C and K
// are template parameters in {16, 32}; g, dx, the saved activation and the
// skip gradient are bf16 NHWC, W <= 64.
//
// Both kernels are a few MB of traffic and well under a microsecond of
// MFMA time per layer at batch 256, so they are built to be resident many
// blocks per CU (256 threads, 13-50 KB of LDS) rather than to pipeline
// deeply inside one block, and both use v_mfma_f32_16x16x32_bf16.
//
// Geometry (one table, bwd_small_geom): a TILE is a band of RB rows of one
// image in padded x-coordinates, WP = W rounded up to 8 and RB * WP <= 128.
// Pad rows, halo columns and dummy columns (x >= W) are zeros in LDS;
// dummy pixels are not stored.
#include "conv_bwd_common.h"

typedef __attribute__((ext_vector_type(4))) float bs_f32x4;
typedef __attribute__((ext_vector_type(4))) short bs_s16x4;
typedef __attribute__((ext_vector_type(8))) short bs_s16x8;

#define BS_THREADS 256
#define BS_TILE 128       // padded pixels of a tile at most
#define BS_NHE 264        // (RB + 2) * (WP + 2) at most (WP = 64, RB = 2)
#define BS_MAX_BLOCKS 2048  // dgrad grid cap: 8 blocks on each of 256 CUs

struct BwdSmallGeom {
  int WP, RB;
  int bands;              // ceil(H / RB): tiles per image
};

// THE tile table of both kernels, launchers and predicates: H >= 1,
// 1 <= W <= 64.  RB <= 16 (WP = 8), so (RB + 2) * (WP + 2) peaks at
// WP = 64 with BS_NHE.
static inline BwdSmallGeom bwd_small_geom(int H, int W) {
  BwdSmallGeom q;
  q.WP = (W + 7) & ~7;
  q.RB = bd_min(BS_TILE / q.WP, H);
  q.bands = (H + q.RB - 1) / q.RB;
  return q;
}

struct BwdSmallParams {
  int N, H, W;
  int WP, RB, bands;
  int total;              // N * bands tiles
  int per_block;          // contiguous tiles per block
};

// what the kernels can run (argument check of the launchers)
static inline bool bwd_small_can_run(int H, int W, int C, int K) {
  return (C == 16 || C == 32) && (K == 16 || K == 32) && H >= 1 && W >= 1 &&
         W <= 64 && H <= (1 << 20);
}

// Classes routed to these kernels by default: those whose whole measured
// range lies below the fallback's in both mask modes at batch 256
// (benchmarks/RESULTS.md).  The kernels run every class.
static inline bool bwd_small_class_routed(int C, int K) {
  (void)C; (void)K;
  return true;
}

extern "C" int bdbnn_bwd_small_supported(int H, int W, int C, int K) {
  return bwd_small_can_run(H, W, C, K) && bwd_small_class_routed(C, K);
}

static inline bool bwd_small_fill(BwdSmallParams& p, int N, int H, int W) {
  if (N < 1 || (int64_t)N * H * W >= (int64_t(1) << 31)) return false;
  BwdSmallGeom q = bwd_small_geom(H, W);
  p.N = N; p.H = H; p.W = W;
  p.WP = q.WP; p.RB = q.RB; p.bands = q.bands;
  p.total = N * q.bands;
  p.per_block = 1;
  return true;
}

// byte offset of 16-byte piece `piece` of row `row` of an LDS image with
// ROWB-byte rows, XOR-swizzled so that the consecutive rows a ds_read_b128
// touches spread over the banks (64-byte rows: xnor_conv_mfma.hip's xm_slot)
template <int ROWB>
__device__ __forceinline__ int bs_off(int row, int piece) {
  if constexpr (ROWB == 64)
    return row * 64 + ((piece ^ ((row >> 1) & 3)) << 4);
  else
    return row * 32 + ((piece ^ ((row >> 2) & 1)) << 4);
}

// ======================= dgrad =======================
//
// Weights are the MFMA's A operand (rows = dx channels), pixels its B
// operand, so a lane ends with 4 CONSECUTIVE channels of one pixel: the
// store, the saved-x load and the skip-gradient load are 8 bytes and the
// four clip-STE bits come from one word.
//
// The whole wd (4.5-18 KB) is staged once per block; its fragments are
// tile-invariant and are lifted into registers before the tile loop.  At
// K = 32 one MFMA is one tap; at K = 16 two taps fill the 32-deep
// reduction (lane quarters 0,1 read tap 2j, quarters 2,3 tap 2j+1) and the
// tenth tap is a zero block of wd in LDS against a zero halo entry.
template <int C, int K, bool ACC, int MODE>
__global__ __launch_bounds__(BS_THREADS) void conv_dgrad_small_kernel(
    const __bf16* __restrict__ g, const __bf16* __restrict__ wd,
    const uint32_t* __restrict__ mp, __bf16* __restrict__ dx,
    const __bf16* __restrict__ accp, const __bf16* __restrict__ xin,
    float et, float ek, BwdSmallParams p) {
  constexpr int CT = C / 16;              // 16-channel tiles of dx
  constexpr int NJ = K == 32 ? 9 : 5;     // MFMAs per (pixel group, c tile)
  constexpr int ROWB = K * 2;             // bytes of a halo pixel / wd row
  constexpr int PP = ROWB / 16;           // 16-byte pieces per row
  constexpr int WROWS = (K == 32 ? 9 : 10) * C;   // K = 16: + the zero tap

  __shared__ __align__(16) char wl[WROWS * ROWB];
  // entry BS_NHE is the zero pixel of the tenth tap
  __shared__ __align__(16) char halo[(BS_NHE + 1) * ROWB];

  const int tid = threadIdx.x;
  const int wid = tid >> 6, lane = tid & 63;
  const int l15 = lane & 15, q = lane >> 4;
  const int wg = bd_xcd_remap(blockIdx.x, gridDim.x);
  const int tile0 = wg * p.per_block;
  const int tile_end = bd_min(tile0 + p.per_block, p.total);

  for (int i = tid; i < WROWS * PP; i += BS_THREADS) {
    int row = i / PP, piece = i - row * PP;
    uint4 v{0, 0, 0, 0};
    if (row < 9 * C) v = *(const uint4*)(wd + row * K + piece * 8);
    *(uint4*)(wl + bs_off<ROWB>(row, piece)) = v;
  }
  if (tid < PP) {
    uint4 z{0, 0, 0, 0};
    *(uint4*)(halo + bs_off<ROWB>(BS_NHE, tid)) = z;
  }
  __syncthreads();

  // this lane's piece of a row and its tap per MFMA step
  const int piece = K == 32 ? q : (q & 1);
  const int WH = p.W + 2;                 // halo row width
  bf16x8 afr[NJ][CT];
  int tapoff[NJ];                         // halo entry offset of the tap
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int t = K == 32 ? j : 2 * j + (q >> 1);   // t == 9: the zero tap
    tapoff[j] = t < 9 ? (t / 3) * WH + (t % 3) : -1;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
      afr[j][ct] = *(const bf16x8*)(
          wl + bs_off<ROWB>(t * C + ct * 16 + l15, piece));
  }

  const float ekt = ek * et;
  const int nhe = (p.RB + 2) * WH;
  const int ngroups = (p.RB * p.WP + 15) >> 4;

  for (int tile = tile0; tile < tile_end; ++tile) {
    const int n = tile / p.bands;
    const int y0 = (tile - n * p.bands) * p.RB;

    // halo: rows y0-1 .. y0+RB, columns -1 .. W, zeros outside the image
    for (int i = tid; i < nhe * PP; i += BS_THREADS) {
      int he = i / PP, pc = i - he * PP;
      int hr = he / WH, hx = he - hr * WH;
      int y = y0 - 1 + hr, x = hx - 1;
      uint4 v{0, 0, 0, 0};
      if (y >= 0 && y < p.H && x >= 0 && x < p.W)
        v = *(const uint4*)(g + ((int64_t)(n * p.H + y) * p.W + x) * K +
                            pc * 8);
      *(uint4*)(halo + bs_off<ROWB>(he, pc)) = v;
    }
    __syncthreads();

    // a wave takes 16-pixel groups (wave-uniform loop: full EXEC at the
    // MFMAs); the lane's pixel is the MFMA column lane & 15
    for (int grp = wid; grp < ngroups; grp += BS_THREADS / 64) {
      const int m = grp * 16 + l15;
      const int r = m / p.WP, x = m - r * p.WP;
      const bool valid = r < p.RB && y0 + r < p.H && x < p.W;
      const int he00 = valid ? r * WH + x : 0;

      bs_f32x4 acc[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[ct] = bs_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int he = tapoff[j] < 0 ? BS_NHE : he00 + tapoff[j];
        bf16x8 b = *(const bf16x8*)(halo + bs_off<ROWB>(he, piece));
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
          acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afr[j][ct], b, acc[ct], 0, 0, 0);
      }

      // epilogue: accumulator register i of tile ct is channel
      // ct*16 + 4*q + i of the lane's pixel
      if (valid) {
        const int64_t pix = (int64_t)(n * p.H + y0 + r) * p.W + x;
        uint32_t mw = 0;
        if constexpr (MODE == 0) mw = mp[pix];      // one word per pixel
        uint2 xv[CT], av[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const int64_t o = pix * C + ct * 16 + q * 4;
          if constexpr (MODE != 0) xv[ct] = *(const uint2*)(xin + o);
          if constexpr (ACC) av[ct] = *(const uint2*)(accp + o);
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const int c4 = ct * 16 + q * 4;
          uint16_t h[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float v = acc[ct][i];
            if constexpr (MODE == 0) {
              v = (mw >> (c4 + i)) & 1 ? v : 0.f;
            } else {
              uint32_t w = i < 2 ? xv[ct].x : xv[ct].y;
              uint16_t xb = uint16_t(w >> (16 * (i & 1)));
              v *= dgrad2_value_mask<MODE>(bf16_to_f32(xb), et, ekt);
            }
            if constexpr (ACC) {
              uint32_t w = i < 2 ? av[ct].x : av[ct].y;
              v += bf16_to_f32(uint16_t(w >> (16 * (i & 1))));
            }
            h[i] = f32_to_bf16(v);
          }
          uint2 o2;
          o2.x = uint32_t(h[0]) | (uint32_t(h[1]) << 16);
          o2.y = uint32_t(h[2]) | (uint32_t(h[3]) << 16);
          *(uint2*)(dx + pix * C + c4) = o2;
        }
      }
    }
    __syncthreads();      // the next tile overwrites the halo
  }
}

template <int C, int K, int MODE>
static int dgrad_small_launch(const void* g, const void* wd,
                              const uint32_t* mp, void* dx, const void* accp,
                              const void* xin, float et, float ek, int N,
                              int H, int W, hipStream_t stream) {
  BwdSmallParams p;
  if (!bwd_small_fill(p, N, H, W)) return -2;
  int nb = bd_min(p.total, BS_MAX_BLOCKS);
  p.per_block = (p.total + nb - 1) / nb;
  nb = (p.total + p.per_block - 1) / p.per_block;
  with_bool(accp != nullptr, [&](auto acc) {
    conv_dgrad_small_kernel<C, K, decltype(acc)::value, MODE>
        <<<nb, BS_THREADS, 0, stream>>>(
            (const __bf16*)g, (const __bf16*)wd, mp, (__bf16*)dx,
            (const __bf16*)accp, (const __bf16*)xin, et, ek, p);
  });
  return 0;
}

template <int C, int K>
static int dgrad_small_mode(const void* g, const void* wd,
                            const uint32_t* mp, const void* x, void* dx,
                            const void* accp, int mode, float t, float k,
                            int N, int H, int W, hipStream_t stream) {
  if (mode == 0)
    return dgrad_small_launch<C, K, 0>(g, wd, mp, dx, accp, nullptr, 0.f,
                                       0.f, N, H, W, stream);
  if (mode == 1)
    return dgrad_small_launch<C, K, 1>(g, wd, nullptr, dx, accp, x, 0.f, 0.f,
                                       N, H, W, stream);
  if (mode == 2)
    return dgrad_small_launch<C, K, 2>(g, wd, nullptr, dx, accp, x, t, k, N,
                                       H, W, stream);
  return -3;
}

// mode 0: mp = clip-STE bitplane [N][H][W][1], x unused; mode 1 (ReAct
// polynomial) / 2 (EDE(t, k)): x = saved bf16 NHWC activation, mp unused.
// 0 launched, -1 unsupported shape, -2 too large for int pixel indices,
// -3 bad mode
extern "C" int bdbnn_conv_dgrad_small(const void* g, const void* wd,
                                      const uint32_t* mp, const void* x,
                                      void* dx, const void* accp, int mode,
                                      float t, float k, int N, int H, int W,
                                      int C, int K, hipStream_t stream) {
  if (!bwd_small_can_run(H, W, C, K)) return -1;
  if (C == 16 && K == 16)
    return dgrad_small_mode<16, 16>(g, wd, mp, x, dx, accp, mode, t, k, N, H,
                                    W, stream);
  if (C == 16)
    return dgrad_small_mode<16, 32>(g, wd, mp, x, dx, accp, mode, t, k, N, H,
                                    W, stream);
  if (K == 16)
    return dgrad_small_mode<32, 16>(g, wd, mp, x, dx, accp, mode, t, k, N, H,
                                    W, stream);
  return dgrad_small_mode<32, 32>(g, wd, mp, x, dx, accp, mode, t, k, N, H,
                                  W, stream);
}

// ======================= wgrad =======================
//
// D[c][k] per tap with the reduction over pixels: both operands want 8
// consecutive m of one channel per lane, so g and the decoded sign(x) are
// staged PIXEL-MAJOR (one 32- or 64-byte row per pixel) and read through
// ds_read_b64_tr_b16, as conv_wgrad3 does.
//
//   G image  [128 m][K]: the tile's g rows as they arrive; dummy pixels
//            (x >= W, y >= H, m >= RB * WP) are zero rows, so whatever X
//            holds there adds nothing.
//   X image  [RB + 2][x = -1 .. WP][C]: sign(x) as +-1 bf16 decoded from
//            the NHWC sign plane (one word per pixel: CW = 1, bits c < C),
//            zeros outside the image.  A tap is a pixel offset.
//
// Two stages of both images: the loads of chunk i+1 are in flight during
// chunk i's MFMAs and are written behind them, ONE barrier per chunk.
// There is a single (c, k) tile, so all parallelism is the m-split: a
// block owns a contiguous chunk range, its 4 waves take the 32-m steps of
// a chunk in turn and add their accumulators through LDS (over the dead
// stages) into the block's slab; wgrad_finish sums the slabs.

__device__ __forceinline__ bs_s16x4 bs_tr_read(const char* base, int off) {
  // EXEC all ones, 8-byte-aligned in-bounds address in every lane
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) bs_s16x4*)(base + off));
}

__device__ __forceinline__ bf16x8 bs_frag(bs_s16x4 lo, bs_s16x4 hi) {
  bs_s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

// 8 sign bits (bit 1 <=> x >= 0 <=> +1) -> 8 bf16 +-1
__device__ __forceinline__ uint4 bs_decode8(uint32_t b) {
  uint32_t v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    v[j] = 0xBF80BF80u ^ (((b >> (2 * j)) & 1u) << 15) ^
           (((b >> (2 * j + 1)) & 1u) << 31);
  return uint4{v[0], v[1], v[2], v[3]};
}

template <int C, int K>
__global__ __launch_bounds__(BS_THREADS) void conv_wgrad_small_kernel(
    const __bf16* __restrict__ g, const uint32_t* __restrict__ xp,
    float* __restrict__ dwT, BwdSmallParams p) {
  constexpr int CT = C / 16, KT = K / 16;
  constexpr int XROW = C * 2, GROW = K * 2;     // bytes per pixel row
  constexpr int XP = XROW / 16, GP = GROW / 16; // 16-byte pieces per row
  constexpr int XBYTES = BS_NHE * XROW, GBYTES = BS_TILE * GROW;
  constexpr int STAGE = XBYTES + GBYTES;
  constexpr int RED = 9 * C * K * 4;
  constexpr int SMEM = 2 * STAGE > RED ? 2 * STAGE : RED;
  constexpr int GPT = BS_TILE * GP / BS_THREADS;          // 1 or 2
  constexpr int XPT = (BS_NHE + BS_THREADS - 1) / BS_THREADS;  // 2

  __shared__ __align__(16) char smem[SMEM];

  const int tid = threadIdx.x;
  const int wid = tid >> 6, lane = tid & 63;
  const int l15 = lane & 15, q = lane >> 4;
  // transposed-read role inside the 16-lane group: the lane passes the
  // address of pixel +tq, channels 4*tp .. 4*tp+3, and receives channel
  // (lane & 15) of the group's 4 pixels
  const int tq = l15 >> 2, tp = l15 & 3;
  const int split_id = bd_xcd_remap(blockIdx.x, gridDim.x);
  const int ch_lo = split_id * p.per_block;
  const int ch_hi = bd_min(ch_lo + p.per_block, p.total);
  const int n_chunks = ch_hi - ch_lo;     // >= 1 by the host's split

  const int XW = p.WP + 2;
  const int nxe = (p.RB + 2) * XW;
  const int nruns = (p.RB * p.WP) >> 3;   // 8-pixel runs of a chunk
  const int nsteps = (nruns + 3) >> 2;    // 32-m MFMA steps

  bs_f32x4 acc[9][CT][KT];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int kt = 0; kt < KT; ++kt)
        acc[t][ct][kt] = bs_f32x4{0.f, 0.f, 0.f, 0.f};

  uint4 greg[GPT];
  uint32_t xw[XPT];
  bool xon[XPT];

#define BS_LOADS(chunk)                                                   \
  {                                                                       \
    const int n_ = (chunk) / p.bands;                                     \
    const int y0_ = ((chunk) - n_ * p.bands) * p.RB;                      \
    _Pragma("unroll")                                                     \
    for (int it = 0; it < GPT; ++it) {                                    \
      int i = tid + it * BS_THREADS;                                      \
      int m = i / GP, pc = i - m * GP;                                    \
      int r = m / p.WP, x = m - r * p.WP;                                 \
      uint4 v{0, 0, 0, 0};                                                \
      if (r < p.RB && y0_ + r < p.H && x < p.W)                           \
        v = *(const uint4*)(g + ((int64_t)(n_ * p.H + y0_ + r) * p.W +    \
                                 x) * K + pc * 8);                        \
      greg[it] = v;                                                       \
    }                                                                     \
    _Pragma("unroll")                                                     \
    for (int it = 0; it < XPT; ++it) {                                    \
      int e = tid + it * BS_THREADS;                                      \
      int hr = e / XW, col = e - hr * XW;                                 \
      int y = y0_ - 1 + hr, x = col - 1;                                  \
      uint32_t w = 0;                                                     \
      bool on = false;                                                    \
      if (e < nxe && y >= 0 && y < p.H && x >= 0 && x < p.W) {            \
        w = xp[(int64_t)(n_ * p.H + y) * p.W + x];                        \
        on = true;                                                        \
      }                                                                   \
      xw[it] = w;                                                         \
      xon[it] = on;                                                       \
    }                                                                     \
  }

#define BS_WRITES(stage)                                                  \
  {                                                                       \
    char* Xs = smem + (stage) * STAGE;                                    \
    char* Gs = Xs + XBYTES;                                               \
    _Pragma("unroll")                                                     \
    for (int it = 0; it < GPT; ++it) {                                    \
      int i = tid + it * BS_THREADS;                                      \
      *(uint4*)(Gs + i * 16) = greg[it];                                  \
    }                                                                     \
    _Pragma("unroll")                                                     \
    for (int it = 0; it < XPT; ++it) {                                    \
      int e = tid + it * BS_THREADS;                                      \
      if (e < nxe) {                                                      \
        _Pragma("unroll")                                                 \
        for (int pc = 0; pc < XP; ++pc) {                                 \
          uint4 v{0, 0, 0, 0};                                            \
          if (xon[it]) v = bs_decode8(xw[it] >> (8 * pc));                \
          *(uint4*)(Xs + e * XROW + pc * 16) = v;                         \
        }                                                                 \
      }                                                                   \
    }                                                                     \
  }

  BS_LOADS(ch_lo);
  BS_WRITES(0);
  int st = 0;
  for (int ci = 0; ci < n_chunks; ++ci) {
    // stage st is visible; everyone is done reading stage st^1
    __syncthreads();
    const bool more = ci + 1 < n_chunks;
    if (more) BS_LOADS(ch_lo + ci + 1);   // land during the MFMAs

    const char* Xs = smem + st * STAGE;
    const char* Gs = Xs + XBYTES;
    // wave-uniform loop: full EXEC at the transposed reads
    for (int step = wid; step < nsteps; step += BS_THREADS / 64) {
      // lane quarter q takes the 8-pixel run 4*step + q: m = 8q .. 8q+7
      // of the MFMA's reduction.  A run past the chunk reads g's zero rows
      // and, for X, run 0 (finite values against zeros).
      const int run = step * 4 + q;
      const int mrun = run * 8;
      const int mx = run < nruns ? mrun : 0;
      const int rl = mx / p.WP;
      const int xq = mx - rl * p.WP + tq;   // window column at dx = 0
      bf16x8 bfr[KT];
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        const int boff = (mrun + tq) * GROW + (kt * 16 + tp * 4) * 2;
        bfr[kt] = bs_frag(bs_tr_read(Gs, boff),
                          bs_tr_read(Gs, boff + 4 * GROW));
      }
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
        for (int dxs = 0; dxs < 3; ++dxs) {
          const int pix0 = (rl + dy) * XW + xq + dxs;
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            const int aoff = pix0 * XROW + (ct * 16 + tp * 4) * 2;
            bf16x8 afr = bs_frag(bs_tr_read(Xs, aoff),
                                 bs_tr_read(Xs, aoff + 4 * XROW));
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
              acc[dy * 3 + dxs][ct][kt] =
                  __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                      afr, bfr[kt], acc[dy * 3 + dxs][ct][kt], 0, 0, 0);
          }
        }
      }
    }
    if (more) BS_WRITES(st ^ 1);
    st ^= 1;
  }
#undef BS_LOADS
#undef BS_WRITES

  // ---- the 4 waves' partials, added in wave order over the dead stages;
  // accumulator register i is row c = 4*q + i, column k = lane & 15 ----
  float* red = (float*)smem;
  for (int w = 0; w < BS_THREADS / 64; ++w) {
    __syncthreads();
    if (wid == w) {
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int idx =
                  (t * C + ct * 16 + q * 4 + i) * K + kt * 16 + l15;
              float v = acc[t][ct][kt][i];
              red[idx] = w == 0 ? v : red[idx] + v;
            }
    }
  }
  __syncthreads();
  float4* slab = (float4*)(dwT + (int64_t)split_id * 9 * C * K);
  for (int i = tid; i < 9 * C * K / 4; i += BS_THREADS)
    slab[i] = ((const float4*)red)[i];
}

// THE m-split of conv_wgrad_small: the launcher and bdbnn_wgrad_small_nslab
// both take it from here, so the kernel writes exactly the slabs the caller
// allocated.  A slab is 36*C*K bytes and g is 2*N*H*W*K bytes, so at most
// N*H*W / (18*C) slabs keep the slab traffic below the g read; the count
// is then rounded so that no block's chunk range is empty.
static inline void wgrad_small_split(BwdSmallParams& p, int C) {
  int64_t cap = (int64_t)p.N * p.H * p.W / (18 * C);
  int split = (int)bd_min<int64_t>(bd_min<int64_t>(p.total, cap), 1024);
  if (split < 1) split = 1;
  p.per_block = (p.total + split - 1) / split;
}

static inline int wgrad_small_nslab(const BwdSmallParams& p) {
  return (p.total + p.per_block - 1) / p.per_block;
}

// ---- slab fold ----
// wgrad_finish sums the slabs with one thread per weight, serially over
// the slabs: fine for the few slabs of the 64-channel kernels, but here
// there are 9*C*K = 2304..9216 weights and up to 1024 slabs (measured at
// C = K = 16, batch 256: 683 slabs, 0.2 ms in wgrad_finish against 10 us in
// the wgrad kernel).  This pass sums them slab-parallel into ONE slab in a
// fixed order: a block owns 8 float4 columns, its 32 thread groups take the
// slabs s = grp, grp + 32, .. and group 0 adds the 32 partials in order.
#define BS_FOLD_COLS 8
#define BS_FOLD_GROUPS (BS_THREADS / BS_FOLD_COLS)

__global__ __launch_bounds__(BS_THREADS) void wgrad_small_fold_kernel(
    const float4* __restrict__ in, float4* __restrict__ out, int e4,
    int nslab) {
  __shared__ float4 red[BS_FOLD_GROUPS][BS_FOLD_COLS];
  const int cl = threadIdx.x % BS_FOLD_COLS, grp = threadIdx.x / BS_FOLD_COLS;
  const int col = blockIdx.x * BS_FOLD_COLS + cl;   // e4 % BS_FOLD_COLS == 0
  float4 a{0.f, 0.f, 0.f, 0.f};
  for (int s = grp; s < nslab; s += BS_FOLD_GROUPS) {
    float4 v = in[(int64_t)s * e4 + col];
    a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
  }
  red[grp][cl] = a;
  __syncthreads();
  if (grp == 0) {
    for (int i = 1; i < BS_FOLD_GROUPS; ++i) {
      float4 v = red[i][cl];
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    out[col] = a;
  }
}

// slabs [nslab][9][C][K] -> out [9][C][K], C and K in {16, 32}
extern "C" void bdbnn_wgrad_small_fold(const float* slabs, float* out,
                                       int nslab, int C, int K,
                                       hipStream_t stream) {
  const int e4 = 9 * C * K / 4;
  wgrad_small_fold_kernel<<<e4 / BS_FOLD_COLS, BS_THREADS, 0, stream>>>(
      (const float4*)slabs, (float4*)out, e4, nslab);
}

// slab count for the host-side dwT allocation, -1 unsupported
extern "C" int bdbnn_wgrad_small_nslab(int N, int H, int W, int C, int K) {
  BwdSmallParams p;
  if (!bwd_small_can_run(H, W, C, K) || !bwd_small_fill(p, N, H, W))
    return -1;
  wgrad_small_split(p, C);
  return wgrad_small_nslab(p);
}

// xp: the NHWC sign plane [N][H][W][1] (bit c of the word = x >= 0);
// dwT: [nslab][9][C][K] fp32, every word written
extern "C" int bdbnn_conv_wgrad_small(const void* g, const uint32_t* xp,
                                      float* dwT, int N, int H, int W, int C,
                                      int K, hipStream_t stream) {
  BwdSmallParams p;
  if (!bwd_small_can_run(H, W, C, K)) return -1;
  if (!bwd_small_fill(p, N, H, W)) return -2;
  wgrad_small_split(p, C);
  const int nb = wgrad_small_nslab(p);
  auto launch = [&](auto c, auto k) {
    conv_wgrad_small_kernel<decltype(c)::value, decltype(k)::value>
        <<<nb, BS_THREADS, 0, stream>>>((const __bf16*)g, xp, dwT, p);
  };
  with_int<16, 32>(C, [&](auto c) {
    with_int<16, 32>(K, [&](auto k) { launch(c, k); });
  });
  return 0;
}
