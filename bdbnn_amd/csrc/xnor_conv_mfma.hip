// K1, MFMA route — the binary convolution forward on the int8 matrix cores.
//
//   out[n,oy,ox,k] = alpha_k * dot( sign(x[patch]), sign(w[k]) )
//
// Same inputs and the same output as xnor_conv.hip: the activation sign
// plane xp [N,H,W,CW] (bit 1 <=> x >= 0), the packed weights wp
// [K,3,3,CW] (INVERTED bits, bit 1 <=> w < 0) and alpha[K].  Operands stay
// 1-bit in global memory and are expanded to +-1 BYTES on chip; the dot
// product then runs on v_mfma_i32_32x32x32_i8 and is exact in i32, so
// alpha_k * float(dot) is bit for bit what the VALU kernel stores.
//
// Geometry is conv_dgrad2's (conv_bwd.hip): the 256 output pixels of a
// block are image-row BANDS in padded x-coordinates (WP = 8/16/32/64
// columns, RB rows, GB bands, GB*RB*WP == 256).  Per 64-channel chunk the
// block stages the bands' input halo ONCE — (RB-1)*S+3 rows of (WP-1)*S+3
// pixels, 64 bytes each — and all 9 taps read shifted windows of it, so a
// staged pixel is expanded once, not once per tap.  Out-of-image halo
// pixels are staged as byte 0: the accumulator is the zero-padded dot
// product directly, and neither the stab table nor the invalid-tap
// correction of the VALU kernel is needed.  Dummy columns / rows (x >= Wo,
// y >= Ho) produce accumulator columns that are simply not stored.  Rows
// wider than 64 outputs are cut into 64-column segments.
//
// The weights are the MFMA's A operand (rows = output channels) and the
// pixels its B operand, so a lane ends up with 4 CONSECUTIVE channels of
// one pixel in accumulator registers 4g..4g+3: the store is 8 B (bf16) or
// 16 B (fp32) along K.
//
// Covers 3x3 / pad 1 / stride 1 or 2 with C % 64 == 0 and K % 64 == 0
// (every 3x3 conv of ResNet-18/34); everything else stays on xnor_conv.hip.
#include "conv_bwd_common.h"
#include <cstdlib>

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(16))) int i32x16;

#define XM_BM 256      // output pixels (padded) per block
#define XM_BN 64       // output channels per block
#define XM_BK 64       // input channels per chunk (= bytes per LDS row)

struct XnorMfmaParams {
  int N, H, W, Ho, Wo, K, CW;
  int segs;              // 64-column segments per output row (1 if Wo <= 64)
  int bands_per_image;   // ceil(Ho / RB)
  int total_slots;       // N * bands_per_image * segs
};

// 4 bits -> 4 bytes holding the bit (0/1): the four shifted copies of the
// nibble occupy disjoint bit ranges, so the multiply carries nothing
__device__ __forceinline__ uint32_t xm_spread4(uint32_t nib) {
  return (nib * 0x00204081u) & 0x01010101u;
}

// 16 sign bits -> 16 bytes.  INV false (activations): bit 1 -> +1, bit 0
// -> -1;  INV true (weights, inverted bits): bit 1 -> -1, bit 0 -> +1.
template <bool INV>
__device__ __forceinline__ uint4 xm_expand16(uint32_t bits) {
  uint32_t v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t m = xm_spread4((bits >> (4 * i)) & 0xfu) * 0xfeu;  // 0xfe / 0
    v[i] = INV ? (m ^ 0x01010101u) : ~m;
  }
  return uint4{v[0], v[1], v[2], v[3]};
}

// byte offset of 16-B slot q of 64-B LDS row `row`, XOR-swizzled so the
// 32 consecutive rows a ds_read_b128 touches spread over all banks
__device__ __forceinline__ int xm_slot(int row, int q) {
  return row * XM_BK + ((q ^ ((row >> 1) & 3)) << 4);
}

// S: stride;  WP/RB/GB: padded-width class (see above)
template <typename TO, int S, int WP, int RB, int GB>
__global__ __launch_bounds__(512, 2) void xnor_conv_mfma_kernel(
    const uint32_t* __restrict__ xp, const uint32_t* __restrict__ wp,
    const float* __restrict__ alpha, TO* __restrict__ out, XnorMfmaParams p,
    int grid_m) {
  constexpr int HR = (RB - 1) * S + 3;        // halo rows per band
  constexpr int WH = (WP - 1) * S + 3;        // halo row width
  constexpr int NHE = GB * HR * WH;           // halo entries (64 B each)
  constexpr int AW = NHE * 2;                 // activation words per chunk
  constexpr int APT = (AW + 511) / 512;
  constexpr int WROWS = 9 * XM_BN;            // weight rows (tap, channel)
  constexpr int WW = WROWS * 2;               // weight words per chunk
  constexpr int WPT = (WW + 511) / 512;

  const int wg = bd_xcd_remap(blockIdx.x, gridDim.x);
  const int tile = wg % grid_m;
  const int k0 = (wg / grid_m) * XM_BN;
  const int tid = threadIdx.x;

  __shared__ __align__(16) unsigned char halo[NHE * XM_BK];
  __shared__ __align__(16) unsigned char wlds[WROWS * XM_BK];
  __shared__ int he_base[NHE];      // input pixel index of halo entry, or -1
  __shared__ int tab_he[XM_BM];     // halo entry of tap (0,0) of pixel m
  __shared__ int tab_out[XM_BM];    // output pixel index, or -1

  // ---- per-block tables ----
  const int slot0 = tile * GB;
  for (int he = tid; he < NHE; he += 512) {
    int band = he / (HR * WH);
    int rem = he - band * (HR * WH);
    int hr = rem / WH, hx = rem - hr * WH;
    int slot = slot0 + band;
    int base = -1;
    if (slot < p.total_slots) {
      int n = slot / (p.bands_per_image * p.segs);
      int r2 = slot - n * (p.bands_per_image * p.segs);
      int bi = r2 / p.segs, seg = r2 - bi * p.segs;
      int iy = bi * RB * S - 1 + hr;
      int ix = seg * WP * S - 1 + hx;
      if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W)
        base = (n * p.H + iy) * p.W + ix;
    }
    he_base[he] = base;
  }
  for (int m = tid; m < XM_BM; m += 512) {
    int band = m / (RB * WP);
    int rem = m - band * (RB * WP);
    int rloc = rem / WP, x = rem - rloc * WP;
    int slot = slot0 + band;
    tab_he[m] = band * (HR * WH) + rloc * S * WH + x * S;
    int o = -1;
    if (slot < p.total_slots) {
      int n = slot / (p.bands_per_image * p.segs);
      int r2 = slot - n * (p.bands_per_image * p.segs);
      int bi = r2 / p.segs, seg = r2 - bi * p.segs;
      int oy = bi * RB + rloc, ox = seg * WP + x;
      if (oy < p.Ho && ox < p.Wo) o = (n * p.Ho + oy) * p.Wo + ox;
    }
    tab_out[m] = o;
  }
  __syncthreads();

  // ---- wave decomposition: 8 waves as 4 (pixels) x 2 (channels) ----
  const int wid = tid >> 6, lane = tid & 63;
  const int wm0 = (wid >> 1) * 64;        // wave's pixel offset (64)
  const int wc = (wid & 1) * 32;          // wave's channel offset (32)
  const int lrow = lane & 31, lh = lane >> 5;
  const int he0 = tab_he[wm0 + lrow];
  const int he1 = tab_he[wm0 + 32 + lrow];

  i32x16 acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc0[i] = 0; acc1[i] = 0; }

  // staged words of the next chunk: the global loads are issued before the
  // MFMA loop and expanded into LDS after it
  uint32_t areg[APT], wreg[WPT];
  bool aval[APT];

#define XM_LOAD(ci)                                                       \
  {                                                                       \
    _Pragma("unroll")                                                     \
    for (int it = 0; it < APT; ++it) {                                    \
      int i = tid + it * 512;                                             \
      uint32_t v = 0;                                                     \
      bool ok = false;                                                    \
      if (i < AW) {                                                       \
        int base = he_base[i >> 1];                                       \
        if (base >= 0) {                                                  \
          v = xp[(int64_t)base * p.CW + (ci) * 2 + (i & 1)];              \
          ok = true;                                                      \
        }                                                                 \
      }                                                                   \
      areg[it] = v;                                                       \
      aval[it] = ok;                                                      \
    }                                                                     \
    _Pragma("unroll")                                                     \
    for (int it = 0; it < WPT; ++it) {                                    \
      int i = tid + it * 512;                                             \
      uint32_t v = 0;                                                     \
      if (i < WW) {                                                       \
        int row = i >> 1;              /* t * 64 + kb */                  \
        int t = row >> 6, kb = row & 63;                                  \
        v = wp[((int64_t)(k0 + kb) * 9 + t) * p.CW + (ci) * 2 + (i & 1)]; \
      }                                                                   \
      wreg[it] = v;                                                       \
    }                                                                     \
  }

#define XM_WRITE()                                                        \
  {                                                                       \
    _Pragma("unroll")                                                     \
    for (int it = 0; it < APT; ++it) {                                    \
      int i = tid + it * 512;                                             \
      if (i < AW) {                                                       \
        int he = i >> 1, q = (i & 1) * 2;                                 \
        uint4 lo{0, 0, 0, 0}, hi{0, 0, 0, 0};                             \
        if (aval[it]) {                                                   \
          lo = xm_expand16<false>(areg[it] & 0xffffu);                    \
          hi = xm_expand16<false>(areg[it] >> 16);                        \
        }                                                                 \
        *(uint4*)&halo[xm_slot(he, q)] = lo;                              \
        *(uint4*)&halo[xm_slot(he, q + 1)] = hi;                          \
      }                                                                   \
    }                                                                     \
    _Pragma("unroll")                                                     \
    for (int it = 0; it < WPT; ++it) {                                    \
      int i = tid + it * 512;                                             \
      if (i < WW) {                                                       \
        int row = i >> 1, q = (i & 1) * 2;                                \
        *(uint4*)&wlds[xm_slot(row, q)] =                                 \
            xm_expand16<true>(wreg[it] & 0xffffu);                        \
        *(uint4*)&wlds[xm_slot(row, q + 1)] =                             \
            xm_expand16<true>(wreg[it] >> 16);                            \
      }                                                                   \
    }                                                                     \
  }

  const int n_chunks = p.CW / 2;
  XM_LOAD(0);
  for (int ci = 0; ci < n_chunks; ++ci) {
    const bool more = ci + 1 < n_chunks;
    XM_WRITE();
    __syncthreads();                       // chunk visible
    if (more) XM_LOAD(ci + 1);             // lands during the MFMA loop
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int dy = t / 3, dx = t - dy * 3;
      const int hA = he0 + dy * WH + dx;
      const int hB = he1 + dy * WH + dx;
      const int wr = t * XM_BN + wc + lrow;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int q = kk * 2 + lh;
        i32x4 a = *(const i32x4*)&wlds[xm_slot(wr, q)];
        i32x4 b0 = *(const i32x4*)&halo[xm_slot(hA, q)];
        i32x4 b1 = *(const i32x4*)&halo[xm_slot(hB, q)];
        acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b1, acc1, 0, 0, 0);
      }
    }
    if (more) __syncthreads();             // all reads done before rewrite
  }
#undef XM_LOAD
#undef XM_WRITE

  // ---- epilogue: D[row = channel][col = pixel]; registers 4g..4g+3 of a
  // lane are channels 8g + 4*lh + 0..3 of its pixel (mfma32_cd_row) ----
  float al[16];
#pragma unroll
  for (int g = 0; g < 4; ++g)
    *(float4*)&al[4 * g] =
        *(const float4*)&alpha[k0 + wc + mfma32_cd_row(4 * g, lh)];
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const i32x16& acc = half ? acc1 : acc0;
    const int pix = tab_out[wm0 + half * 32 + lrow];
    if (pix < 0) continue;
    TO* dst = out + (int64_t)pix * p.K + k0 + wc;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int ch = mfma32_cd_row(4 * g, lh);
      if constexpr (sizeof(TO) == 2) {
        uint16_t vals[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          vals[j] = f32_to_bf16(al[4 * g + j] * float(acc[4 * g + j]));
        *(uint2*)&dst[ch] = *(uint2*)vals;
      } else {
        float vals[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          vals[j] = al[4 * g + j] * float(acc[4 * g + j]);
        *(float4*)&dst[ch] = *(float4*)vals;
      }
    }
  }
}

// ---------------- host side ----------------

// THE (WP, RB, GB) table of xnor_conv_mfma_kernel: calls f(BwdClass) for
// the padded-width class of an output width.
template <class F>
static int xnor_mfma_class(int Wo, F f) {
  if (Wo <= 8) return f(BwdClass<8, 8, 4>{});
  if (Wo <= 16) return f(BwdClass<16, 16, 1>{});
  if (Wo <= 32) return f(BwdClass<32, 8, 1>{});
  return f(BwdClass<64, 4, 1>{});
}

// THE routing table of the forward conv: calls f(on) for the shape class
// of a conv the MFMA kernel can run, where `on` says whether the class
// ships on it by default (measured per layer, benchmarks/RESULTS.md);
// returns -1 for every shape that stays on the VALU kernel.
template <class F>
static int xnor_mfma_route_class(int C, int K, int KH, int KW, int stride,
                                 int pad, F f) {
  if (KH != 3 || KW != 3 || pad != 1) return -1;   // 1x1, 5x5, other pads
  if (C <= 0 || C % XM_BK || K <= 0 || K % XM_BN) return -1;
  if (stride == 1) return f(true);    // 3x3/s1: the 13 C=K convs
  if (stride == 2) return f(true);    // 3x3/s2: the 3 downsampling convs
  return -1;
}

extern "C" int bdbnn_xnor_mfma_supported(int C, int K, int KH, int KW,
                                         int stride, int pad) {
  return xnor_mfma_route_class(C, K, KH, KW, stride, pad,
                               [](bool) { return 0; }) == 0;
}

// 1 where xnor_conv_fwd takes the MFMA kernel: supported, its class on by
// default, and BDBNN_XNOR_MFMA (read once) not 0
extern "C" int bdbnn_xnor_mfma_routed(int C, int K, int KH, int KW,
                                      int stride, int pad) {
  static const bool knob = [] {
    const char* e = getenv("BDBNN_XNOR_MFMA");
    return e ? atoi(e) != 0 : true;
  }();
  if (!knob) return 0;
  return xnor_mfma_route_class(C, K, KH, KW, stride, pad,
                               [](bool on) { return on ? 1 : 0; }) == 1;
}

extern "C" int bdbnn_xnor_conv_mfma_fwd(
    const uint32_t* xp, const uint32_t* wp, const float* alpha, void* out,
    bool out_bf16, int N, int H, int W, int C, int K, int KH, int KW,
    int stride, int pad, int Ho, int Wo, hipStream_t stream) {
  if (!bdbnn_xnor_mfma_supported(C, K, KH, KW, stride, pad)) return -1;
  if ((int64_t)N * H * W > INT32_MAX || (int64_t)N * Ho * Wo > INT32_MAX)
    return -2;   // pixel indices are int
  return xnor_mfma_class(Wo, [&](auto cls) {
    using G = decltype(cls);
    XnorMfmaParams p;
    p.N = N; p.H = H; p.W = W; p.Ho = Ho; p.Wo = Wo; p.K = K;
    p.CW = C / 32;
    p.segs = (Wo + G::WP - 1) / G::WP;
    p.bands_per_image = (Ho + G::RB - 1) / G::RB;
    int64_t slots = (int64_t)N * p.bands_per_image * p.segs;
    int64_t blocks = (slots + G::GB - 1) / G::GB * (K / XM_BN);
    if (slots > INT32_MAX || blocks > INT32_MAX) return -2;
    p.total_slots = (int)slots;
    int grid_m = (int)((slots + G::GB - 1) / G::GB);
    dim3 grid((unsigned)blocks);
    with_dtype(out_bf16, [&](auto t) {
      using TO = decltype(t);
      if (stride == 1)
        xnor_conv_mfma_kernel<TO, 1, G::WP, G::RB, G::GB>
            <<<grid, 512, 0, stream>>>(xp, wp, alpha, (TO*)out, p, grid_m);
      else
        xnor_conv_mfma_kernel<TO, 2, G::WP, G::RB, G::GB>
            <<<grid, 512, 0, stream>>>(xp, wp, alpha, (TO*)out, p, grid_m);
    });
    return 0;
  });
}
