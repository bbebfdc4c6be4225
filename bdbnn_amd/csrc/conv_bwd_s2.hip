// MFMA bf16 backward for the STRIDE-2 binary convolutions — the 3x3/s2/p1
// conv1 and the 1x1/s2/p0 downsample conv of every downsampling block.
// Sibling of csrc/conv_bwd.hip (stride 1); same operands, same epilogue.
//
// dgrad.  No zero-insertion: dx is decomposed by pixel PARITY.  With
// q = y>>1, r = x>>1 a dx pixel (y, x) receives tap (ky, kx) only when
// y+p-ky and x+p-kx are even, from g pixel ((y+p-ky)/2, (x+p-kx)/2):
//
//   3x3/p1   coordinate even: tap k=1 from g index q
//            coordinate odd : tap k=2 from q, tap k=0 from q+1
//            -> phases (y&1, x&1) carry 1, 2, 2, 4 taps (9 in all: the
//            conv's MAC count, nothing wasted on inserted zeros)
//   1x1/p0   phase (0,0): the single tap from (q, r); the other three
//            phases have no tap and are stored as 0 (or the skip grad)
//
// So one block tile is 128 g pixels (q, r) in padded coordinates (Wo
// rounded up to 4/8/16/32) and produces the 2x2 dx pixels of each, one
// f32x16 accumulator set per phase.  Every A read lies in
// g[q..q+1][r..r+1]: the g tile is staged in LDS once per 64-channel K
// chunk with a one-entry bottom/right halo (index Ho / Wo is reached
// only for even H / W and is an explicit zero), XOR-swizzled, and the
// nine (tap, phase) steps read shifted windows of it while the B tile
// wd[8 - (3ky+kx)] (dgrad_weight_decode's mirrored layout) streams per
// tap, one barrier per tap, double buffered.  Blocks walk a contiguous
// tile range (tables, halo and B prefetched across tiles) behind the
// XCD remap.  The epilogue is conv_dgrad2's — clip-STE bit from the
// packed plane at INPUT resolution (MODE 0) or the value mask of the
// saved activation (MODE 1/2), optional unmasked skip grad — applied at
// the dx address of each phase.
//
// wgrad.  For tap (ky, kx), a = ky-p, b = kx-p:
//   dw[k,c,ky,kx] = sum g[n,oy,ox,k] * xb[n, 2oy+a, 2ox+b, c]
// A stride-2 repack of the sign plane (repack_cplane_s2: one u64 per
// (c, n, input row), even-column bits in the low word, odd-column bits
// in the high word) turns this into conv_wgrad2's scheme at OUTPUT
// resolution: the three column-shifted X copies are (odd << 1, even,
// odd), the three row offsets are input rows (2oy-1, 2oy, 2oy+1);
// positions outside the input are explicit zeros.  1x1/p0 is the single
// even/even tap.  Byte -> 8 x bf16 LUT decode, g staged transposed,
// per-block slabs summed by wgrad_finish_s2 — no decoded activation
// tensor, no full-grid atomics.
//
// Constraints (python keeps the aten/MIOpen path otherwise):
//   3x3/s2/p1 or 1x1/s2/p0, C % 64 == 0, K % 64 == 0, input W <= 64
//   (any H, odd sizes and H != W included), g bf16 NHWC, dx bf16 NHWC.
#include "conv_bwd_common.h"

#define DS2_BM 128       // g pixels (M rows) per block
#define DS2_BN 64        // dx channels per block
#define DS2_BK 64        // g channels per K-chunk

struct Dgrad2S2Params {
  int N, H, W, Ho, Wo, C, K;
  int bands_per_image;   // ceil(Ho / RB)
  int total_slots;       // N * bands_per_image
  int CW;                // C/32 (mask words per pixel)
};

// One instantiation per padded-Wo class.
//   WP: padded g row width; RB: g rows per band; GB: bands per block.
//   GB*RB*WP == 128.
// KS: 3 (3x3/p1) or 1 (1x1/p0).  MODE: see conv_bwd_common.h.
template <int WP, int RB, int GB, int KS, int MODE>
__global__ __launch_bounds__(512, 2) void conv_dgrad2_s2_kernel(
    const __bf16* __restrict__ g, const __bf16* __restrict__ wd,
    const uint32_t* __restrict__ mp, __bf16* __restrict__ dx,
    const __bf16* __restrict__ accp, const __bf16* __restrict__ xin,
    float et, float ek,
    Dgrad2S2Params p, int grid_m, int nb_m, int tiles_per_block) {
  static_assert(GB * RB * WP == DS2_BM, "tile is 128 g pixels");
  constexpr int NT = KS * KS;                 // taps
  constexpr int WH = WP + 1;                  // halo row width
  constexpr int NHE = GB * (RB + 1) * WH;     // halo entries (128 B each)
  constexpr int PIECES = NHE * 8;             // 16-B staging pieces
  constexpr int PPT = (PIECES + 511) / 512;   // pieces per thread

  const int wg = bd_xcd_remap(blockIdx.x, gridDim.x);
  const int rb_m = wg % nb_m;               // which m-tile RANGE
  const int c_blk = wg / nb_m;
  const int c0 = c_blk * DS2_BN;
  const int tile0 = rb_m * tiles_per_block;
  const int tile_end = bd_min(tile0 + tiles_per_block, grid_m);
  const int my_tiles = tile_end - tile0;
  if (my_tiles <= 0) return;
  const int tid = threadIdx.x;
  const bool has_acc = accp != nullptr;

  __shared__ __align__(16) __bf16 halo[2][NHE * DS2_BK];
  __shared__ __align__(16) __bf16 blds[2][DS2_BN * DS2_BK];
  __shared__ int he_base[2][NHE];     // g pixel index of halo entry, or -1
  __shared__ int tab_he[2][DS2_BM];   // halo entry of g pixel (q, r)
  __shared__ int tab_out[2][DS2_BM];  // dx pixel index of (2q, 2r), or -1
  // bit 0: column 2r+1 exists, bit 1: row 2q+1 exists
  __shared__ unsigned char tab_fl[2][DS2_BM];

#define BUILD_TABLES(tile, tb)                                            \
  {                                                                       \
    const int slot0 = (tile)*GB;                                          \
    for (int he = tid; he < NHE; he += 512) {                             \
      int band = he / ((RB + 1) * WH);                                    \
      int rem = he - band * ((RB + 1) * WH);                              \
      int hr = rem / WH, hx = rem - hr * WH;                              \
      int slot = slot0 + band;                                            \
      int base = -1;                                                      \
      if (slot < p.total_slots) {                                         \
        int n = slot / p.bands_per_image;                                 \
        int y = (slot - n * p.bands_per_image) * RB + hr;                 \
        if (y < p.Ho && hx < p.Wo) base = (n * p.Ho + y) * p.Wo + hx;     \
      }                                                                   \
      he_base[tb][he] = base;                                             \
    }                                                                     \
    for (int m = tid; m < DS2_BM; m += 512) {                             \
      int band = m / (RB * WP);                                           \
      int rem = m - band * (RB * WP);                                     \
      int rloc = rem / WP, x = rem - rloc * WP;                           \
      int slot = slot0 + band;                                            \
      tab_he[tb][m] = band * (RB + 1) * WH + rloc * WH + x;               \
      int out = -1, fl = 0;                                               \
      if (slot < p.total_slots) {                                         \
        int n = slot / p.bands_per_image;                                 \
        int q = (slot - n * p.bands_per_image) * RB + rloc;               \
        if (q < p.Ho && x < p.Wo) {                                       \
          out = (n * p.H + 2 * q) * p.W + 2 * x;                          \
          fl = (2 * x + 1 < p.W ? 1 : 0) | (2 * q + 1 < p.H ? 2 : 0);     \
        }                                                                 \
      }                                                                   \
      tab_out[tb][m] = out;                                               \
      tab_fl[tb][m] = (unsigned char)fl;                                  \
    }                                                                     \
  }

  // ---- wave decomposition: 8 waves as 4(M) x 2(N) ----
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int wm0 = (wid >> 1) * 32;       // wave's M offset (32 g pixels)
  const int wc = (wid & 1) * 32;         // wave's c offset (32 cols)
  const int lrow = lane & 31;
  const int lk8 = lane >> 5;             // which 8-element k-half

  const int mA = wm0 + lrow;
  const int cB = wc + lrow;
  int heA;                               // reloaded at each tile switch

  // one accumulator set per phase ph = 2*(y&1) + (x&1)
  f32x16 acc[4];
#pragma unroll
  for (int ph = 0; ph < 4; ++ph)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[ph][i] = 0.f;

  uint4 hreg[PPT];
  uint4 breg;

#define HALO_LOAD(tb, k0)                                                 \
  {                                                                       \
    _Pragma("unroll")                                                     \
    for (int it = 0; it < PPT; ++it) {                                    \
      int i = tid + it * 512;                                             \
      uint4 v{0, 0, 0, 0};                                                \
      if (i < PIECES) {                                                   \
        int he = i >> 3, k8 = i & 7;                                      \
        int base = he_base[tb][he];                                       \
        if (base >= 0)                                                    \
          v = *(const uint4*)(g + (int64_t)base * p.K + (k0) + k8 * 8);   \
      }                                                                   \
      hreg[it] = v;                                                       \
    }                                                                     \
  }

  // swizzle key = halo entry index & 7: the 8 consecutive entries a
  // lane group reads land on 8 different 16-B slots
#define HALO_WRITE(buf)                                                   \
  {                                                                       \
    _Pragma("unroll")                                                     \
    for (int it = 0; it < PPT; ++it) {                                    \
      int i = tid + it * 512;                                             \
      if (i < PIECES) {                                                   \
        int he = i >> 3, k8 = i & 7;                                      \
        *(uint4*)&halo[buf][he * DS2_BK + ((k8 ^ (he & 7)) << 3)] =       \
            hreg[it];                                                     \
      }                                                                   \
    }                                                                     \
  }

  const int b_c = tid >> 3;        // 0..63
  const int b_k8 = tid & 7;        // 0..7
  // step t of a K chunk is tap (ky, kx) = (t/3, t%3); its weights sit at
  // the mirrored index NT-1-t of wd
#define B_LOAD(t, k0)                                                     \
  breg = *(const uint4*)(wd +                                             \
                         (((NT - 1 - (t)) * p.C + c0 + b_c) *             \
                          (int64_t)p.K) + (k0) + b_k8 * 8);
#define B_WRITE(buf)                                                      \
  *(uint4*)&blds[buf][b_c * DS2_BK + ((b_k8 ^ (b_c & 7)) << 3)] = breg;

  // epilogue: mask + (optional) skip grad, bf16 store, once per phase.
  // C/D layout: col = lane&31, row = mfma32_cd_row(reg, lane>>5).
  const int ccol = c0 + wc + lrow;
  const int cw_word = ccol >> 5;
  const int cbit = ccol & 31;
  const float ekt = ek * et;
#define EPILOGUE(tb)                                                      \
  {                                                                       \
    _Pragma("unroll")                                                     \
    for (int ph = 0; ph < 4; ++ph) {                                      \
      const int py = ph >> 1, px = ph & 1;                                \
      /* 1x1: phases 1..3 have no tap -> plain 0 (or skip grad) */        \
      const bool live = (KS == 3) || ph == 0;                             \
      int pixr[16];                                                       \
      uint32_t mpw[16];                                                   \
      uint16_t xv[16];                                                    \
      uint16_t av[16];                                                    \
      _Pragma("unroll")                                                   \
      for (int reg = 0; reg < 16; ++reg) {                                \
        int m = wm0 + mfma32_cd_row(reg, lk8);                            \
        int base = tab_out[tb][m];                                        \
        int fl = tab_fl[tb][m];                                           \
        bool ok = base >= 0 && (!px || (fl & 1)) && (!py || (fl & 2));    \
        pixr[reg] = ok ? base + py * p.W + px : -1;                       \
      }                                                                   \
      /* batch-issue the mask/skip-grad loads; pix<0 lanes read a safe */ \
      /* dummy address and are masked below                            */ \
      _Pragma("unroll")                                                   \
      for (int reg = 0; reg < 16; ++reg) {                                \
        int64_t pz = pixr[reg] < 0 ? 0 : (int64_t)pixr[reg];              \
        if (live) {                                                       \
          if constexpr (MODE == 0) mpw[reg] = mp[pz * p.CW + cw_word];    \
          else xv[reg] = *(const uint16_t*)(xin + pz * p.C + ccol);       \
        }                                                                 \
        if (has_acc)                                                      \
          av[reg] = *(const uint16_t*)(accp + pz * p.C + ccol);           \
      }                                                                   \
      _Pragma("unroll")                                                   \
      for (int reg = 0; reg < 16; ++reg) {                                \
        int pix = pixr[reg];                                              \
        if (pix < 0) continue;                                            \
        float v = 0.f;                                                    \
        if (live) {                                                       \
          if constexpr (MODE == 0)                                        \
            v = (mpw[reg] >> cbit) & 1 ? acc[ph][reg] : 0.f;              \
          else                                                            \
            v = acc[ph][reg] *                                            \
                dgrad2_value_mask<MODE>(bf16_to_f32(xv[reg]), et, ekt);   \
        }                                                                 \
        if (has_acc) v += bf16_to_f32(av[reg]);                           \
        uint16_t h = f32_to_bf16(v);                                      \
        *(uint16_t*)(dx + (int64_t)pix * p.C + ccol) = h;                 \
      }                                                                   \
    }                                                                     \
  }

  // ---- (tile, k-chunk) stream with cross-tile prefetch ----
  const int n_k0 = p.K / DS2_BK;
  const int S = my_tiles * n_k0;

  BUILD_TABLES(tile0, 0);
  __syncthreads();
  heA = tab_he[0][mA];
  HALO_LOAD(0, 0);
  HALO_WRITE(0);
  B_LOAD(0, 0);
  B_WRITE(0);
  __syncthreads();

  int hb = 0, bb = 0, tb = 0;
  for (int s = 0; s < S; ++s) {
    const int ki = s % n_k0;
    const int k0 = ki * DS2_BK;
    const bool more = s + 1 < S;
    const bool tile_switch = (ki == n_k0 - 1);  // next s starts a new tile
    const int nki = tile_switch ? 0 : ki + 1;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      // tap (ky, kx): an odd coordinate takes k=2 from q and k=0 from
      // q+1, an even one k=1 from q
      const int ky = KS == 3 ? t / 3 : 1, kx = KS == 3 ? t - ky * 3 : 1;
      const int ph = (ky != 1 ? 2 : 0) + (kx != 1 ? 1 : 0);
      const int sy = ky == 0 ? 1 : 0, sx = kx == 0 ? 1 : 0;
      if (t < NT - 1) {
        B_LOAD(t + 1, k0);
      } else if (more) {
        B_LOAD(0, nki * DS2_BK);
      }
      if (t == 0 && more && tile_switch) {
        // build the NEXT tile's tables into the other buffer (free: the
        // barrier after the previous tile's epilogue retired its
        // readers); a barrier publishes them before HALO_LOAD reads
        BUILD_TABLES(tile0 + (s + 1) / n_k0, tb ^ 1);
        if (NT == 1) __syncthreads();
      }
      if (t == (NT == 1 ? 0 : 1) && more) {
        HALO_LOAD(tile_switch ? tb ^ 1 : tb, nki * DS2_BK);
      }
      const int heT = heA + sy * WH + sx;
      const int keyA = (heT & 7) ^ lk8;
      const int keyB = (cB & 7) ^ lk8;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        bf16x8 a = *(const bf16x8*)&halo[hb][heT * DS2_BK +
                                             (((kk << 1) ^ keyA) << 3)];
        bf16x8 b = *(const bf16x8*)&blds[bb][cB * DS2_BK +
                                             (((kk << 1) ^ keyB) << 3)];
        acc[ph] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[ph], 0,
                                                          0, 0);
      }
      if (t == NT - 1 && more) HALO_WRITE(hb ^ 1);
      if (t < NT - 1 || more) {
        B_WRITE(bb ^ 1);
        __syncthreads();
        bb ^= 1;
      }
    }
    hb ^= 1;
    if (tile_switch) {
      EPILOGUE(tb);
#pragma unroll
      for (int ph = 0; ph < 4; ++ph)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[ph][i] = 0.f;
      tb ^= 1;
      heA = tab_he[tb][mA];
      // the epilogue's table reads must retire before the next step
      // rebuilds that buffer
      __syncthreads();
    }
  }
#undef BUILD_TABLES
#undef HALO_LOAD
#undef HALO_WRITE
#undef B_LOAD
#undef B_WRITE
#undef EPILOGUE
}

// ---------------- host side ----------------

static bool s2_shape_ok(int H, int W, int C, int K, int ks) {
  if (ks != 1 && ks != 3) return false;
  if (H < 1 || W < 1 || W > 64) return false;
  if (C < 64 || K < 64 || C % 64 || K % 64) return false;
  return true;
}

// what the kernels can run (the entry points' argument check)
extern "C" int bdbnn_s2_kernels_can_run(int H, int W, int C, int K,
                                        int ks) {
  return s2_shape_ok(H, W, C, K, ks) ? 1 : 0;
}

// what python ROUTES here: the kernels' shapes minus the ones measured
// slower than the MIOpen pipeline they would replace
// (benchmarks/RESULTS.md: the 3x3 at 128->256 and 256->512 lose 10-35%
// per backward at batch 256, the 3x3 at 64->128 and every 1x1 win), so
// the deep 3x3 convs keep the fallback until the kernels are tuned
extern "C" int bdbnn_dgrad2_s2_supported(int H, int W, int C, int K,
                                         int ks) {
  if (!s2_shape_ok(H, W, C, K, ks)) return 0;
  if (ks == 3 && C >= 128 && K >= 256) return 0;
  return 1;
}

template <int KS, int MODE>
static int dgrad2_s2_launch(const void* g, const void* wd,
                            const uint32_t* mp, void* dx, const void* accp,
                            const void* xin, float et, float ek, int N,
                            int H, int W, int C, int K,
                            hipStream_t stream) {
  if (!s2_shape_ok(H, W, C, K, KS)) return -1;
  Dgrad2S2Params p;
  p.N = N; p.H = H; p.W = W; p.C = C; p.K = K;
  p.Ho = (H + 1) / 2; p.Wo = (W + 1) / 2;   // both kernel sizes
  p.CW = C / 32;
#define LAUNCH(WPV, RBV, GBV)                                             \
  {                                                                       \
    p.bands_per_image = (p.Ho + (RBV)-1) / (RBV);                         \
    p.total_slots = N * p.bands_per_image;                                \
    int grid_m = (p.total_slots + (GBV)-1) / (GBV);                       \
    int n_ctile = C / DS2_BN;                                             \
    /* two blocks fit a CU: ~2 contiguous tile ranges per resident slot */ \
    int nb_m = bd_min(grid_m, 1024 / n_ctile);                            \
    if (nb_m < 1) nb_m = 1;                                               \
    int tpb = (grid_m + nb_m - 1) / nb_m;                                 \
    nb_m = (grid_m + tpb - 1) / tpb;                                      \
    dim3 grid(nb_m * n_ctile);                                            \
    conv_dgrad2_s2_kernel<WPV, RBV, GBV, KS, MODE>                        \
        <<<grid, 512, 0, stream>>>(                                       \
            (const __bf16*)g, (const __bf16*)wd, mp, (__bf16*)dx,         \
            (const __bf16*)accp, (const __bf16*)xin, et, ek, p, grid_m,   \
            nb_m, tpb);                                                   \
    return 0;                                                             \
  }
  if (p.Wo <= 4) {
    LAUNCH(4, 4, 8);
  } else if (p.Wo <= 8) {
    LAUNCH(8, 4, 4);
  } else if (p.Wo <= 16) {
    LAUNCH(16, 8, 1);
  } else {
    LAUNCH(32, 4, 1);
  }
#undef LAUNCH
}

// mode 0: mp = clip-STE bitplane [N,H,W,C/32], x unused;
// mode 1/2: x = saved bf16 NHWC activation, mp unused.  ks in {1, 3}.
extern "C" int bdbnn_conv_dgrad2_s2(const void* g, const void* wd,
                                    const uint32_t* mp, const void* x,
                                    void* dx, const void* accp, int ks,
                                    int mode, float t, float k, int N,
                                    int H, int W, int C, int K,
                                    hipStream_t stream) {
#define DISPATCH(KSV)                                                     \
  {                                                                       \
    if (mode == 0)                                                        \
      return dgrad2_s2_launch<KSV, 0>(g, wd, mp, dx, accp, nullptr, 0.f,  \
                                      0.f, N, H, W, C, K, stream);        \
    if (mode == 1)                                                        \
      return dgrad2_s2_launch<KSV, 1>(g, wd, nullptr, dx, accp, x, 0.f,   \
                                      0.f, N, H, W, C, K, stream);        \
    if (mode == 2)                                                        \
      return dgrad2_s2_launch<KSV, 2>(g, wd, nullptr, dx, accp, x, t, k,  \
                                      N, H, W, C, K, stream);             \
    return -2;                                                            \
  }
  if (ks == 3) DISPATCH(3)
  if (ks == 1) DISPATCH(1)
#undef DISPATCH
  return -1;
}

// ======================= wgrad, stride 2 =======================
//
//   dwT[t][c][k] = sum_m X_t[c][m] * g[m][k],   m = (n, oy, ox)
//   X_t[c][m]    = xb[n, 2oy+ky-p, 2ox+kx-p, c]  (0 outside the input)
//
// conv_wgrad2's scheme at OUTPUT resolution.  A chunk is GB bands of RB
// g rows (GB*RB*WP == 128, WP = Wo padded to 8/16/32).  Per band the X
// image holds XR input rows per column copy: for 3x3, slot j is input
// row 2*oy0-1+j (j = 0..2RB), and tap ky of local g row rl reads slot
// 2rl+ky; for 1x1, slot j is input row 2(oy0+j).  Column copies:
// kx=0 -> odd bits << 1 (zero at ox=0), kx=1 -> even bits, kx=2 -> odd
// bits (zero at ox=Wo-1 when W is odd).  Dummy columns ox >= Wo decode
// to garbage +-1 but meet g = 0 there.

#define WS2_CHUNK 128       // m entries per chunk
#define WS2_BC 64           // c tile
#define WS2_BK 64           // k tile

struct Wgrad2S2Params {
  int N, H, W, Ho, Wo, C, K;
  int bands_per_image;      // ceil(Ho / RB)
  int total_slots;          // N * bands_per_image
  int total_chunks;         // ceil(total_slots / GB)
  int split;                // blocks per (c,k) tile
  int nh_rows;              // N * H  (plane row count)
};

template <int WP, int RB, int GB, int KS>
__global__ __launch_bounds__(512, 2) void conv_wgrad2_s2_kernel(
    const __bf16* __restrict__ g, const uint64_t* __restrict__ planes,
    float* __restrict__ dwT, Wgrad2S2Params p, int grid_ck) {
  static_assert(GB * RB * WP == WS2_CHUNK, "chunk is 128 g pixels");
  constexpr int NT = KS * KS;             // taps
  constexpr int NV = KS;                  // column copies of X
  constexpr int XR = KS == 3 ? 2 * RB + 1 : RB;  // input rows per band
  constexpr int XSTRIDE = GB * XR * WP + 8;  // +16 B pad: conflict-free
  constexpr int GSTRIDE = WS2_CHUNK + 8;  // gT row stride (elements)
  constexpr int LGWP = WP == 8 ? 3 : WP == 16 ? 4 : 5;
  static_assert(NV * WS2_BC * XSTRIDE * 2 >= 4 * 32 * 32 * 4,
                "combine scratch aliases X");

  const int tid = threadIdx.x;
  int wg = blockIdx.x;
  const int ck = wg % grid_ck;            // (c,k) tile
  const int split_id = wg / grid_ck;
  const int c_blk = ck % (p.C / WS2_BC);
  const int k_blk = ck / (p.C / WS2_BC);
  const int c0 = c_blk * WS2_BC, k0 = k_blk * WS2_BK;

  // X: [NV copies][64 c] rows of GB*XR*WP (+pad) elements
  __shared__ __align__(16) __bf16 X[NV * WS2_BC * XSTRIDE];
  __shared__ __align__(16) __bf16 gT[2][WS2_BK * GSTRIDE];
  __shared__ __align__(16) __bf16 lut[256][8];
  // raw plane bits: the global u64 loads prefetch into registers during
  // the previous chunk's MFMA phase and land here at the chunk boundary
  // (Wo <= 16 leaves each parity half 16 bits: kept as one u32)
  constexpr int NBITS = WS2_BC * GB * XR;
  constexpr bool B32 = WP <= 16;
  __shared__ uint64_t xbits64[B32 ? 1 : NBITS];
  __shared__ uint32_t xbits32[B32 ? NBITS : 1];

  wgrad2_fill_sign_lut(lut, tid);

  // ---- wave decomposition: quad (c-half, k-half) x m-split ----
  const int wid = tid >> 6, lane = tid & 63;
  const int qc = (wid >> 1) & 1, qk = wid & 1, ms_grp = wid >> 2;
  const int lrow = lane & 31, lhalf = lane >> 5;

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

  // contiguous chunk range of this split block
  const int cpb = (p.total_chunks + p.split - 1) / p.split;
  const int ch_lo = split_id * cpb;
  const int ch_hi = bd_min(ch_lo + cpb, p.total_chunks);
  const int n_chunks = ch_hi - ch_lo;   // may be <= 0: slab still written
  int ch = ch_lo;

  // gT staging: thread loads 16 k-elements of ONE g pixel (a 4-lane
  // group covers one pixel's 64-ch row) and scatter-writes transposed
  const int sg_m = tid >> 2;              // 0..127
  const int sg_k16 = (tid & 3) * 16;      // k offset of its 16 elements
  uint4 greg0, greg1;

  // block-uniform per-band facts of a chunk
  int u_n[GB], u_y0[GB];
  bool u_vs[GB];
  // (select, not a runtime index: keeps the arrays in registers)
#define BSEL(arr, band) (GB == 1 ? arr[0] : ((band) ? arr[GB - 1] : arr[0]))
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
#define G_LOAD()                                                          \
  {                                                                       \
    int band = sg_m / (RB * WP);                                          \
    int rem = sg_m - band * (RB * WP);                                    \
    int x = rem & (WP - 1);                                               \
    uint4 z{0, 0, 0, 0};                                                  \
    greg0 = z; greg1 = z;                                               \
    if (BSEL(u_vs, band) && x < p.Wo) {                                         \
      int y = BSEL(u_y0, band) + (rem >> LGWP);                                 \
      if (y < p.Ho) {                                                     \
        const __bf16* src =                                               \
            g + ((int64_t)(BSEL(u_n, band) * p.Ho + y) * p.Wo + x) * p.K + k0 + \
            sg_k16;                                                       \
        greg0 = *(const uint4*)src;                                       \
        greg1 = *(const uint4*)(src + 8);                               \
      }                                                                   \
    }                                                                     \
  }

#define G_PAIR(j, w)                                                      \
  dst[(2 * (j)) * GSTRIDE] = (uint16_t)((w) & 0xffffu);                   \
  dst[(2 * (j) + 1) * GSTRIDE] = (uint16_t)((w) >> 16);
#define G_WRITE(buf)                                                      \
  {                                                                       \
    uint16_t* dst = (uint16_t*)&gT[buf][sg_k16 * GSTRIDE + sg_m];         \
    G_PAIR(0, greg0.x) G_PAIR(1, greg0.y)                             \
    G_PAIR(2, greg0.z) G_PAIR(3, greg0.w)                             \
    G_PAIR(4, greg1.x) G_PAIR(5, greg1.y)                             \
    G_PAIR(6, greg1.z) G_PAIR(7, greg1.w)                             \
  }

  constexpr int BPT = (NBITS + 511) / 512;
  uint64_t bits_reg[BPT];
#define BITS_LOAD()                                                       \
  {                                                                       \
    _Pragma("unroll")                                                     \
    for (int it = 0; it < BPT; ++it) {                                    \
      int i = tid + it * 512;                                             \
      uint64_t b = 0;                                                     \
      if (i < NBITS) {                                                    \
        int j = i % XR;                                                   \
        int rem = i / XR;                                                 \
        int band = rem % GB;                                              \
        int c = rem / GB;                                                 \
        if (BSEL(u_vs, band)) {                                                 \
          int y = KS == 3 ? 2 * BSEL(u_y0, band) - 1 + j                        \
                          : 2 * (BSEL(u_y0, band) + j);                         \
          if (y >= 0 && y < p.H)                                          \
            b = planes[(int64_t)(c0 + c) * p.nh_rows + BSEL(u_n, band) * p.H +  \
                       y];                                                \
        }                                                                 \
      }                                                                   \
      bits_reg[it] = b;                                                   \
    }                                                                     \
  }
  // xbits index (c*GB + band)*XR + j == i: the load order IS the layout
#define BITS_WRITE()                                                      \
  {                                                                       \
    _Pragma("unroll")                                                     \
    for (int it = 0; it < BPT; ++it) {                                    \
      int i = tid + it * 512;                                             \
      if (i < NBITS) {                                                    \
        uint64_t b = bits_reg[it];                                        \
        if constexpr (B32)                                                \
          xbits32[i] = ((uint32_t)b & 0xffffu) | ((uint32_t)(b >> 32) << 16); \
        else                                                              \
          xbits64[i] = b;                                                 \
      }                                                                   \
    }                                                                     \
  }

  // ---- X decode for one chunk from the LDS-resident bits; the column
  // pad zeros are folded into the target write ----
  const bool w_odd = p.W & 1;
  const int eb8 = (p.Wo - 1) >> 3, eel = (p.Wo - 1) & 7;
  constexpr int XTGT = NV * WS2_BC * GB * XR * (WP / 8);
#define X_DECODE()                                                        \
  {                                                                       \
    _Pragma("unroll 2")                                                   \
    for (int it = 0; it < (XTGT + 511) / 512; ++it) {                     \
      int i = tid + it * 512;                                             \
      if (i < XTGT) {                                                     \
        int xb8 = i % (WP / 8);                                           \
        int rem = i / (WP / 8);                                           \
        int bi = rem % (WS2_BC * GB * XR);   /* (c*GB + band)*XR + j */   \
        int v = rem / (WS2_BC * GB * XR);    /* column copy */            \
        int c = bi / (GB * XR);                                           \
        int bj = bi - c * (GB * XR);         /* band*XR + j */            \
        int band = bj / XR, j = bj - band * XR;                           \
        /* input row of slot j; rows outside the image decode to 0 */     \
        int y0b = BSEL(u_y0, band);                                       \
        int y = KS == 3 ? 2 * y0b - 1 + j : 2 * (y0b + j);                \
        bool valid = BSEL(u_vs, band) && y >= 0 && y < p.H;                     \
        uint32_t ev, od;                                                  \
        if constexpr (B32) {                                              \
          uint32_t b = xbits32[bi];                                       \
          ev = b & 0xffffu; od = b >> 16;                                 \
        } else {                                                          \
          uint64_t b = xbits64[bi];                                       \
          ev = (uint32_t)b; od = (uint32_t)(b >> 32);                     \
        }                                                                 \
        const int kx = KS == 3 ? v : 1;                                   \
        uint32_t sh = kx == 0 ? (od << 1) : kx == 1 ? ev : od;            \
        unsigned byte = (sh >> (8 * xb8)) & 0xffu;                        \
        uint4 vv{0, 0, 0, 0};                                             \
        if (valid) {                                                       \
          vv = *(const uint4*)&lut[byte][0];                              \
          if (kx == 0 && xb8 == 0) vv.x &= 0xffff0000u;                   \
          if (kx == 2 && w_odd && xb8 == eb8) {                           \
            /* zero bf16 element eel (component select, not an index: */  \
            /* an indexed uint4 would leave the registers)            */  \
            uint32_t zm = ~(0xffffu << ((eel & 1) * 16));                 \
            int d = eel >> 1;                                             \
            vv.x &= d == 0 ? zm : ~0u;                                    \
            vv.y &= d == 1 ? zm : ~0u;                                    \
            vv.z &= d == 2 ? zm : ~0u;                                    \
            vv.w &= d == 3 ? zm : ~0u;                                    \
          }                                                               \
        }                                                                 \
        *(uint4*)&X[(v * WS2_BC + c) * XSTRIDE + bj * WP + xb8 * 8] = vv; \
      }                                                                   \
    }                                                                     \
  }

  if (n_chunks > 0) {
    CHUNK_INFO(ch);
    BITS_LOAD();
    G_LOAD();
    BITS_WRITE();
    G_WRITE(0);
  }
  int gb = 0;

  // per-lane fragment bases
  const int a_c = qc * 32 + lrow;         // A (X): lane row c
  const int b_k = qk * 32 + lrow;         // B (gT): lane row k

  for (int ci = 0; ci < n_chunks; ++ci) {
    const bool more = ci + 1 < n_chunks;
    __syncthreads();                  // xbits + gT + lut visible; X free
    X_DECODE();
    if (more) {
      CHUNK_INFO(ch + 1);
      BITS_LOAD();
      G_LOAD();                       // lands during the MFMA phase
    }
    __syncthreads();                  // X ready for all waves

#pragma unroll
    for (int msl = 0; msl < 4; ++msl) {   // 4 x 16-m steps = its 64-m half
      const int m16 = ms_grp * 64 + msl * 16;
      // B-frag: 8 m at fixed k from gT
      bf16x8 bfrag =
          *(const bf16x8*)&gT[gb][b_k * GSTRIDE + m16 + lhalf * 8];
      const int mstart = m16 + lhalf * 8;
      const int rl = mstart >> LGWP;
      const int band = rl / RB, rloc = rl - band * RB;
      const int xs = mstart & (WP - 1);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int ky = KS == 3 ? t / 3 : 0, kx = KS == 3 ? t - ky * 3 : 0;
        const int slot = KS == 3 ? 2 * rloc + ky : rloc;
        bf16x8 afrag = *(const bf16x8*)&X[(kx * WS2_BC + a_c) * XSTRIDE +
                                          (band * XR + slot) * WP + xs];
        acc[t] =
            __builtin_amdgcn_mfma_f32_32x32x16_bf16(afrag, bfrag, acc[t],
                                                    0, 0, 0);
      }
    }
    __syncthreads();                  // all reads of X/gT[gb] done
    if (more) {
      BITS_WRITE();
      G_WRITE(gb ^ 1);
    }
    gb ^= 1;
    ++ch;
  }

  // ---- m-split combine + plain coalesced slab store ----
  // (the scratch aliases X: every X read retired at the barrier above)
  wgrad2_combine_store<NT>(acc, (float(*)[32][32])X,
                           dwT + (int64_t)split_id * NT * p.C * p.K, p.C,
                           p.K, c0, k0, wid, lane);
#undef CHUNK_INFO
#undef G_LOAD
#undef G_WRITE
#undef G_PAIR
#undef BSEL
#undef BITS_LOAD
#undef BITS_WRITE
#undef X_DECODE
}

// THE (WP, RB, GB) table of conv_wgrad2_s2_kernel: calls f(BwdClass) for
// the padded-width class of a Wo-wide output.
template <class F>
static int wgrad2_s2_class(int Wo, F f) {
  if (Wo <= 8) return f(BwdClass<8, 8, 2>{});
  if (Wo <= 16) return f(BwdClass<16, 8, 1>{});
  return f(BwdClass<32, 4, 1>{});
}

// chunking and m-split of a shape in class G.  The launcher and the
// host-side slab count both take p.split from HERE: the kernel writes
// exactly the slabs the caller allocated.
template <class G>
static Wgrad2S2Params wgrad2_s2_params(G, int N, int H, int W, int C,
                                       int K) {
  Wgrad2S2Params p;
  p.N = N; p.H = H; p.W = W; p.C = C; p.K = K;
  p.Ho = (H + 1) / 2; p.Wo = (W + 1) / 2;
  p.nh_rows = N * H;
  p.bands_per_image = (p.Ho + G::RB - 1) / G::RB;
  p.total_slots = N * p.bands_per_image;
  p.total_chunks = (p.total_slots + G::GB - 1) / G::GB;
  // LDS admits ONE 512-thread block per CU: m-split so the grid is about
  // one block per CU
  int grid_ck = (C / WS2_BC) * (K / WS2_BK);
  p.split = bd_min((256 + grid_ck - 1) / grid_ck, p.total_chunks);
  return p;
}

// slab count (= split) for the host-side dwT allocation
extern "C" int bdbnn_wgrad2_s2_nslab(int N, int H, int W, int C, int K,
                                     int ks) {
  if (!s2_shape_ok(H, W, C, K, ks)) return -1;
  return wgrad2_s2_class((W + 1) / 2, [&](auto cls) {
    return wgrad2_s2_params(cls, N, H, W, C, K).split;
  });
}

extern "C" int bdbnn_conv_wgrad2_s2(const void* g, const uint64_t* planes,
                                    float* dwT, int ks, int N, int H, int W,
                                    int C, int K, hipStream_t stream) {
  if (!s2_shape_ok(H, W, C, K, ks)) return -1;
  return wgrad2_s2_class((W + 1) / 2, [&](auto cls) {
    using G = decltype(cls);
    Wgrad2S2Params p = wgrad2_s2_params(cls, N, H, W, C, K);
    int grid_ck = (C / WS2_BC) * (K / WS2_BK);
    dim3 grid(grid_ck * p.split);
    if (ks == 3)
      conv_wgrad2_s2_kernel<G::WP, G::RB, G::GB, 3>
          <<<grid, 512, 0, stream>>>((const __bf16*)g, planes, dwT, p,
                                     grid_ck);
    else
      conv_wgrad2_s2_kernel<G::WP, G::RB, G::GB, 1>
          <<<grid, 512, 0, stream>>>((const __bf16*)g, planes, dwT, p,
                                     grid_ck);
    return 0;
  });
}
