// Pieces shared by the MFMA backward kernels (conv_bwd.hip: stride 1,
// conv_bwd_s2.hip: stride 2, conv_wgrad3.hip: stride-1 wgrad from the
// NHWC sign plane, conv_bwd_small.hip: stride 1 at 16/32 channels).
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

// ---- geometry of the stride-1 wgrad kernels (conv_bwd.hip: wgrad2,
// conv_wgrad3.hip: wgrad3), one table for both ----
#define WG2_CHUNK 128       // m entries per chunk
#define WG2_BC 64           // c tile
#define WG2_BK 64           // k tile

struct Wgrad2Params {
  int N, H, W, C, K;
  int bands_per_image;      // ceil(H / RB)
  int total_slots;          // N * bands_per_image
  int total_chunks;         // ceil(total_slots / GB)
  int split;                // chunk stride (== blocks per (c,k) tile)
  int nh_rows;              // N * H  (xcp row count)
};

// THE (WP, RB, GB) table of conv_wgrad2_kernel: calls f(BwdClass) for the
// padded-width class of an (H, W) image.
template <class F>
static int wgrad2_class(int H, int W, F f) {
  if (W <= 8 && H <= 8) return f(BwdClass<8, 8, 2>{});
  if (W <= 16) return f(BwdClass<16, 8, 1>{});
  if (W <= 32) return f(BwdClass<32, 4, 1>{});
  return f(BwdClass<64, 2, 1>{});
}

static inline bool wgrad2_shape_ok(int W, int C, int K) {
  return !(C % 64 || K % 64 || W > 64);
}

// chunking and m-split of a shape in class G.  The launcher and the
// host-side slab count both take p.split from HERE: the kernel writes
// exactly the slabs the caller allocated.
template <class G>
static Wgrad2Params wgrad2_params(G, int N, int H, int W, int C, int K) {
  Wgrad2Params p;
  p.N = N; p.H = H; p.W = W; p.C = C; p.K = K;
  p.nh_rows = N * H;
  p.bands_per_image = (H + G::RB - 1) / G::RB;
  p.total_slots = N * p.bands_per_image;
  p.total_chunks = (p.total_slots + G::GB - 1) / G::GB;
  // LDS (wgrad2 ~140-159 KB, wgrad3 ~99-121 KB per block) admits ONE
  // 512-thread block per CU: round
  // the m-split so the grid is a whole multiple of 256 CUs (384 blocks
  // = 1.5 dispatch rounds would idle half the chip for half the time)
  int grid_ck = (C / WG2_BC) * (K / WG2_BK);
  p.split = bd_min((256 + grid_ck - 1) / grid_ck, p.total_chunks);
  return p;
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
