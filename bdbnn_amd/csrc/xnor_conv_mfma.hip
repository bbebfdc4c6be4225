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
//
// Inference epilogue (EPI >= 0, bdbnn_xnor_conv_bn_act_fwd): the block tail
// that follows the conv in eval mode runs on the accumulator registers
// instead of as bn_act_eval_kernel (+ sign_pack_nhwc for the next conv):
//   v   = round_storage<TO>(alpha_k * float(acc))   // the plain store
//   out = act(sc_k * v + sh_k (+ skip))             // bn_eval_act<EPI>
// with (sc, sh) folded once by bn_fold_kernel (bn_act.hip).  Both functions
// are bn_act_eval_kernel's own (bn_affine.h), so `out` is bit for bit the
// composition's.  Optionally the sign plane of `out` as stored is written
// for the consuming conv (act_masks.h convention; no clip-mask plane).
#include "conv_bwd_common.h"
#include "bn_affine.h"
#include "act_masks.h"
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

// Operands of the inference epilogue; unused (all null) when EPI < 0.
struct XnorEpiArgs {
  const float* sc;       // [K] folded BN scale
  const float* sh;       // [K] folded BN shift (+ b1 for kind 3)
  const float* a;        // [K] PReLU slopes (kinds 1, 3)
  const float* b2;       // [K] RPReLU output shift (kind 3)
  const void* skip;      // TO [N,Ho,Wo,K] residual, or null
  uint32_t* plane;       // [N,Ho,Wo,K/32] sign plane of out, or null
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

// S: stride;  WP/RB/GB: padded-width class (see above);  EPI: -1 stores
// alpha * dot, 0..3 the inference epilogue with that act_kind (bn_act.hip)
template <typename TO, int S, int WP, int RB, int GB, int EPI = -1>
__global__ __launch_bounds__(512, 2) void xnor_conv_mfma_kernel(
    const uint32_t* __restrict__ xp, const uint32_t* __restrict__ wp,
    const float* __restrict__ alpha, TO* __restrict__ out, XnorMfmaParams p,
    int grid_m, XnorEpiArgs e) {
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
  // inference epilogue: the block's 64 channels of alpha, sc, sh, a, b2
  constexpr int NOPS = EPI >= 0 ? 5 : 1;
  __shared__ __align__(16) float eops[NOPS][XM_BN];

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
  if constexpr (EPI >= 0) {
    // staged once per block, read back per 4-channel group in the epilogue:
    // an LDS read there instead of a global round trip per group
    for (int i = tid; i < 5 * XM_BN; i += 512) {
      const int which = i / XM_BN, kb = i - which * XM_BN;
      const float* src = which == 0 ? alpha : which == 1 ? e.sc
                       : which == 2 ? e.sh : which == 3 ? e.a : e.b2;
      eops[which][kb] = src != nullptr ? src[k0 + kb] : 0.f;
    }
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
  if constexpr (EPI >= 0) {
    // Per 4-channel group g the five per-channel operands come from LDS as
    // float4 (20 live VGPRs, not 80) and serve both pixels of the lane.
    // The skip is read at the address the output is stored to: all 8
    // loads of a lane are issued before the first use, so a block waits
    // for memory once, not once per group.  A lane sets the sign bits of
    // its 16 channels in place (bit = channel within the wave's 32); lanes
    // l and l + 32 hold the two halves of one plane word and combine them
    // with one exchange.
    using SkipVec = std::conditional_t<sizeof(TO) == 2, uint2, float4>;
    const TO* __restrict__ skip = (const TO*)e.skip;
    const int pix[2] = {tab_out[wm0 + lrow], tab_out[wm0 + 32 + lrow]};
    // element offset of the lane's channel 0 of each pixel, in out and in
    // skip; a lane without a pixel computes on pixel 0's row (in bounds),
    // stores nothing, and its sign bits are dropped below
    const int64_t row[2] = {
        (int64_t)(pix[0] < 0 ? 0 : pix[0]) * p.K + k0 + wc,
        (int64_t)(pix[1] < 0 ? 0 : pix[1]) * p.K + k0 + wc};
    // Without a skip every element adds -0.0f, the one addend that leaves
    // each float as it is (+0 + -0 = +0, -0 + -0 = -0): bit for bit the
    // eval kernel's "no add", without a select per element.
    SkipVec sk[4][2];
    if (skip != nullptr) {   // uniform; no branch per load, so one wait
#pragma unroll
      for (int half = 0; half < 2; ++half)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          sk[g][half] = *(const SkipVec*)&skip[
              row[half] + mfma32_cd_row(4 * g, lh)];
    } else {
#pragma unroll
      for (int half = 0; half < 2; ++half)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          if constexpr (sizeof(TO) == 2)
            sk[g][half] = uint2{0x80008000u, 0x80008000u};
          else
            sk[g][half] = float4{-0.f, -0.f, -0.f, -0.f};
        }
    }
    uint32_t bits[2] = {0u, 0u};
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int ch = mfma32_cd_row(4 * g, lh);
      float al[4], sc[4], sh[4], av[4] = {0.f, 0.f, 0.f, 0.f},
            b2v[4] = {0.f, 0.f, 0.f, 0.f};
      *(float4*)al = *(const float4*)&eops[0][wc + ch];
      *(float4*)sc = *(const float4*)&eops[1][wc + ch];
      *(float4*)sh = *(const float4*)&eops[2][wc + ch];
      if constexpr (EPI == 1 || EPI == 3)
        *(float4*)av = *(const float4*)&eops[3][wc + ch];
      if constexpr (EPI == 3) *(float4*)b2v = *(const float4*)&eops[4][wc + ch];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const i32x16& acc = half ? acc1 : acc0;
        float s[4], r[4];
        if constexpr (sizeof(TO) == 2) {
          const uint16_t* u = (const uint16_t*)&sk[g][half];
#pragma unroll
          for (int j = 0; j < 4; ++j) s[j] = bf16_to_f32(u[j]);
        } else {
          *(float4*)s = sk[g][half];
        }
        uint16_t vals[4];   // bf16 only: rounded once, stored and re-read
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float v = round_storage<TO>(al[j] * float(acc[4 * g + j]));
          r[j] = bn_eval_act<EPI>(sc[j], v, sh[j], true, s[j], av[j],
                                  b2v[j]);
          if constexpr (sizeof(TO) == 2) {
            vals[j] = f32_to_bf16(r[j]);
            r[j] = bf16_to_f32(vals[j]);      // = round_storage<TO>(out)
          }
          // constant shift here, the lane half's 4 * lh once at the end
          bits[half] |= uint32_t(sign_bit(r[j])) << (8 * g + j);
        }
        if (pix[half] >= 0) {
          if constexpr (sizeof(TO) == 2)
            *(uint2*)&out[row[half] + ch] = *(uint2*)vals;
          else
            *(float4*)&out[row[half] + ch] = *(float4*)r;
        }
      }
    }
    if (e.plane != nullptr) {       // uniform; every lane of the wave shuffles
      const int64_t KW32 = p.K >> 5;
      const int word = (k0 + wc) >> 5;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const uint32_t mine = bits[half] << (4 * lh);
        const uint32_t other = __shfl_xor(mine, 32);
        if (lh == 0 && pix[half] >= 0)
          e.plane[(int64_t)pix[half] * KW32 + word] = mine | other;
      }
    }
    return;
  }
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

// geometry + launch of either epilogue: EPI -1 (plain) or an act_kind
template <int EPI>
static int xnor_mfma_launch(
    const uint32_t* xp, const uint32_t* wp, const float* alpha, void* out,
    bool out_bf16, int N, int H, int W, int C, int K, int KH, int KW,
    int stride, int pad, int Ho, int Wo, XnorEpiArgs e, hipStream_t stream) {
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
        xnor_conv_mfma_kernel<TO, 1, G::WP, G::RB, G::GB, EPI>
            <<<grid, 512, 0, stream>>>(xp, wp, alpha, (TO*)out, p, grid_m,
                                       e);
      else
        xnor_conv_mfma_kernel<TO, 2, G::WP, G::RB, G::GB, EPI>
            <<<grid, 512, 0, stream>>>(xp, wp, alpha, (TO*)out, p, grid_m,
                                       e);
    });
    return 0;
  });
}

extern "C" int bdbnn_xnor_conv_mfma_fwd(
    const uint32_t* xp, const uint32_t* wp, const float* alpha, void* out,
    bool out_bf16, int N, int H, int W, int C, int K, int KH, int KW,
    int stride, int pad, int Ho, int Wo, hipStream_t stream) {
  return xnor_mfma_launch<-1>(xp, wp, alpha, out, out_bf16, N, H, W, C, K,
                              KH, KW, stride, pad, Ho, Wo, XnorEpiArgs{},
                              stream);
}

// conv + folded eval BN (+ skip) + act (+ sign plane of out) in one launch.
// -3: act_kind outside 0..3 or a per-channel operand it needs is null.
extern "C" int bdbnn_xnor_conv_bn_act_fwd(
    const uint32_t* xp, const uint32_t* wp, const float* alpha,
    const float* sc, const float* sh, const float* a, const float* b2,
    const void* skip, void* out, uint32_t* plane, int act_kind,
    bool out_bf16, int N, int H, int W, int C, int K, int KH, int KW,
    int stride, int pad, int Ho, int Wo, hipStream_t stream) {
  if (act_kind < 0 || act_kind > 3 || sc == nullptr || sh == nullptr)
    return -3;
  if ((act_kind == 1 || act_kind == 3) && a == nullptr) return -3;
  if (act_kind == 3 && b2 == nullptr) return -3;
  XnorEpiArgs e{sc, sh, a, b2, skip, plane};
  int rc = -3;
  with_int<1, 2, 3, 0>(act_kind, [&](auto act) {
    rc = xnor_mfma_launch<decltype(act)::value>(
        xp, wp, alpha, out, out_bf16, N, H, W, C, K, KH, KW, stride, pad, Ho,
        Wo, e, stream);
  });
  return rc;
}
