// The general sign-weight convolution, written once: activations x sign-weight planes as an implicit GEMM on the 32x32x16
// matrix cores of gfx950.  Instantiated by liblsq_hip.so (lsq_signw_conv2d: fp32 activations split into bf16 hi + lo,
// lsq_signw_conv.hip) and by liblsq_hip_conv_half.so (lsq_signw_conv2d_half: bf16 / fp16 activations as they are,
// conv_half/lsq_conv_half.hip).  Each library compiles its own copy (anonymous namespace); neither links the other's objects.
//
// Implicit GEMM, transposed so that stores are coalesced:  D[o][pixel] = sum_k S[o][k] * X[k][pixel], k = (tap, channel).
// A = 32 out-channels x 16 channels of +-1 (exact in bf16 and fp16), B = 16 channels x 32 pixels of activations, fp32
// accumulation.  Zero padding and channel padding are exact (x = 0 contributes 0).
//
// Two kernels.  conv_patch (any stride whose input patch fits LDS -- every ResNet layer): per 16-channel chunk the
// workgroup keeps the whole input patch its output pixels touch in LDS (already converted) together with the expanded +-1
// weights of all taps, and the taps read their fragments at precomputed addresses -- each input element is loaded and
// converted once per workgroup instead of once per tap.  conv_tiled (fall-back): im2col staging per (tap, 32-channel chunk).
// patch_plan decides between them on the host, once for both libraries.
//
// Tiles, staging roles, index math, the weight expansion's bit work, the chunk and tap loops, the epilogue's batching, the
// plan and the launch table do not depend on the activations' type, and every accumulator receives its products in one
// order -- chunk, then tap in (kh, kw) order, then plane (hi before lo) -- in every instantiation.  An instantiation is named
// by a traits struct X:
//   Args            the operand struct (SwArgs / the 16-bit library's HArgs; the geometry fields both have: fill_geom)
//   T, Raw          an element of x in memory / in a register right after its load (float, float / unsigned short, unsigned)
//   kFp32           fp32 activations: folded batch norm, clamp, bf16 hi / lo split, fused epilogue; else 16-bit words clamped
//                   in their own type and Args::store(index, value) in the epilogue
//   kFused          16-bit only (the fused library's X16F / HFArgs, conv_fused_half/): a folded batch norm in the read --
//                   fold2 on the scales and shifts of the chunk being staged, read at wave-uniform addresses, no table in
//                   LDS, so the plan does not depend on it -- and the fp32 epilogue act(out + res_pre) + res_post on 16-bit
//                   residuals before Args::store
//   kF16            the MFMA's operand type (16-bit only: fp16, else bf16)
//   kPlanes         LDS planes per patch or chunk: 2 (hi + lo) or 1;  kPerReg: activations per staged register, 1 or 2
//   Off<PATCH>      type of the epilogue's output offsets in conv_patch / conv_tiled
// The steps that differ -- the conversion of a loaded activation, the MFMA step, the constant of the weight expansion, the
// epilogue's loads and arithmetic -- stand side by side under `if constexpr (X::kFp32)` (or kPlanes == 2), written out, not
// behind functions of X: a function is simplified on its own before it is inlined, and every such helper tried (conversion
// with the validity flag as a parameter, an epilogue object, an MFMA step looping over planes) changed the schedule of the
// kernels that used it.  As written, 28 of the 30 kernels are instruction for instruction what the two files held before
// (DESIGN 4.23); the kFused branches left all 30 as they were.
#pragma once

#include "lsq_signw_conv.h"

namespace lsq {
namespace signw {
namespace {

typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

// +-1.0 of the activations' type in both halves of a dword
template <bool F16>
constexpr unsigned kOne2 = F16 ? 0x3C003C00u : 0x3F803F80u;

template <bool F16>
__device__ __forceinline__ f32x16 mfma16(const Frag& a, const Frag& b, f32x16 acc) {
  if constexpr (F16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a.u), __builtin_bit_cast(f16x8, b.u), acc, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, b.v, acc, 0, 0, 0);
}

__device__ __forceinline__ Frag lds_frag(const unsigned char* p) {
  const uint4 v = *reinterpret_cast<const uint4*>(p);
  Frag f;
  f.u[0] = v.x; f.u[1] = v.y; f.u[2] = v.z; f.u[3] = v.w;
  return f;
}

// two 16-bit activations in a dword, clamped: bf16 through fp32 (v_med3_f32 of the value shifted up; the bound is a bf16
// value, so the result is one), fp16 packed (v_pk_max_f16 / v_pk_min_f16).  Both return the non-NaN operand: under a finite
// bound a NaN activation becomes -bound (stated in lsq_hip_conv_half.h)
template <bool F16, class A>
__device__ __forceinline__ unsigned clamp2(unsigned d, const A& a) {
  if (!a.clamp) return d;              // (uniform: no min / max on the identity, which would turn a NaN into -inf)
  if constexpr (F16) {
    const f16x2 v = __builtin_bit_cast(f16x2, d), l = __builtin_bit_cast(f16x2, a.lim2);
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_elementwise_max(v, -l), l));
  } else {
    const float lo = __builtin_amdgcn_fmed3f(__builtin_bit_cast(float, d << 16), -a.lim, a.lim);
    const float hi = __builtin_amdgcn_fmed3f(__builtin_bit_cast(float, d & 0xFFFF0000u), -a.lim, a.lim);
    return (__builtin_bit_cast(unsigned, hi) & 0xFFFF0000u) | (__builtin_bit_cast(unsigned, lo) >> 16);
  }
}

// kFused: two 16-bit activations of channels with folded batch norms (s0, b0), (s1, b1) -> fl32(fl32(v * s) + b), a separate
// multiply and add, rounded to nearest even into the type (v_cvt_pk_bf16_f32 / v_cvt_f16_f32: fp16 overflow gives +-inf),
// packed as they came.  The rule of lsq_act_quant_bn_half.
template <bool F16>
__device__ __forceinline__ unsigned fold2(unsigned lo, unsigned hi, float s0, float b0, float s1, float b1) {
  if constexpr (F16) {
    const float t0 = (float)__builtin_bit_cast(_Float16, (unsigned short)lo) * s0 + b0;
    const float t1 = (float)__builtin_bit_cast(_Float16, (unsigned short)hi) * s1 + b1;
    const f16x2 h = {(_Float16)t0, (_Float16)t1};
    return __builtin_bit_cast(unsigned, h);
  } else {
    const f32x2 t = {__builtin_bit_cast(float, lo << 16) * s0 + b0, __builtin_bit_cast(float, hi << 16) * s1 + b1};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(t, bf16x2));
  }
}

// a 16-bit residual element as fp32 (kFused)
template <bool F16>
__device__ __forceinline__ float half_to_f32(unsigned short h) {
  if constexpr (F16) return (float)__builtin_bit_cast(_Float16, h);
  else return __builtin_bit_cast(float, (unsigned)h << 16);
}

// Epilogue of both kernels: lane = pixel column, registers = out-channel rows (coalesced stores: consecutive elements of a
// row per half-wave); out = base + acc * ws[o] with a separate multiply and add, base = bias[o] (or 0) at the first plane
// and the fp32 sum of the planes before it afterwards.
//   fp32:   y = relu(out + res_pre) + res_post on the last weight plane, a float store.  Off = byte offsets: unsigned when
//           the host has checked 4*N*O*Ho*Wo < 2^32 (one vector add per output address: conv_patch), else size_t.
//   16-bit: Args::store.  Off = long long element indices.  kFused: the fp32 epilogue in front of it on the last plane, the
//           residuals one 16-bit element per load at the output's own index.
template <class X, typename Off, int BM, int BN, int TM, int TN>
__device__ __forceinline__ void store_tiles(const typename X::Args& a, const f32x16 (&acc)[TM][TN], int ptile, int t, int o0,
                                            int wm, int wn, int col, int kh8) {
  const int HoWo = a.Ho * a.Wo;
  const long long total = (long long)a.N * HoWo;
  Off pbase[TN];                                       // offset of (n, out-channel o0 + 4*kh8, pixel)
  bool pok[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const long long pix = (long long)ptile * BN + (wn * TN + j) * 32 + col;
    pok[j] = pix < total;
    const int n = pok[j] ? (int)(pix / HoWo) : 0;
    const int r = pok[j] ? (int)(pix - (long long)n * HoWo) : 0;
    if constexpr (X::kFp32) pbase[j] = (Off)4 * ((Off)(n * a.O + o0 + 4 * kh8) * (Off)HoWo + (Off)r);
    else pbase[j] = ((long long)n * a.O + o0 + 4 * kh8) * HoWo + r;
  }
  [[maybe_unused]] char* yb = nullptr;
  [[maybe_unused]] const char *rpre = nullptr, *rpost = nullptr;
  [[maybe_unused]] bool want_pre = false, want_post = false;
  if constexpr (X::kFp32) {
    yb = reinterpret_cast<char*>(a.y);
    rpre = reinterpret_cast<const char*>(a.res_pre);
    rpost = reinterpret_cast<const char*>(a.res_post);
    want_pre = a.final_pass && a.res_pre, want_post = a.final_pass && a.res_post;
  }
  // kFused: the residual loads are issued unconditionally -- an absent operand reads element 0 of x, a valid address, and is
  // not added --, so that no load stands inside a branch (conv_tiled's load_chunk says why)
  [[maybe_unused]] const unsigned short *hpre = nullptr, *hpost = nullptr;
  if constexpr (X::kFused) {
    want_pre = a.final_pass && a.res_pre, want_post = a.final_pass && a.res_post;
    hpre = want_pre ? a.res_pre : a.x;
    hpost = want_post ? a.res_post : a.x;
  }
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int qh = 0; qh < 2; ++qh) {
      // batch of 8 out-channel rows x TN pixel tiles: every load of the batch (previous partial sum,
      // residuals, scale, bias) is issued before the first use -- a load consumed right after it is issued
      // costs one memory latency per output
      float ws[8], bs[8], prev[8][TN];
      [[maybe_unused]] float sl[8], r1[8][TN], r2[8][TN];                 // fp32 and kFused only
      Off yo[8][TN];
      bool ok[8][TN];
#pragma unroll
      for (int qq = 0; qq < 8; ++qq) {
        const int q = qh * 8 + qq;
        const int olu = (wm * TM + i) * 32 + (q & 3) + 8 * (q >> 2);      // wave-uniform part of the row
        const int ol = olu + 4 * kh8;                                     // C/D layout of the 32x32 MFMA
        const bool rok = t * BM + ol < a.og;
        const int o = o0 + (rok ? ol : 0);
        ws[qq] = a.wscale[o];
        if constexpr (X::kFp32) {
          bs[qq] = (!a.accumulate && a.bias) ? a.bias[o] : 0.f;
          sl[qq] = (a.final_pass && a.relu >= LSQ_ACT_PRELU) ? a.slope[a.relu == LSQ_ACT_PRELU ? 0 : o] : 0.f;
          const Off rowoff = (Off)4 * (Off)olu * (Off)HoWo;               // scalar
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            ok[qq][j] = rok && pok[j];
            yo[qq][j] = ok[qq][j] ? pbase[j] + rowoff : (Off)0;
            prev[qq][j] = a.accumulate ? *reinterpret_cast<const float*>(yb + yo[qq][j]) : 0.f;
            r1[qq][j] = want_pre ? *reinterpret_cast<const float*>(rpre + yo[qq][j]) : 0.f;
            r2[qq][j] = want_post ? *reinterpret_cast<const float*>(rpost + yo[qq][j]) : 0.f;
          }
        } else if constexpr (X::kFused) {
          bs[qq] = (!a.prev && a.bias) ? a.bias[o] : 0.f;
          sl[qq] = (a.final_pass && a.act >= LSQ_ACT_PRELU) ? a.slope[a.act == LSQ_ACT_PRELU ? 0 : o] : 0.f;
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            ok[qq][j] = rok && pok[j];
            yo[qq][j] = ok[qq][j] ? pbase[j] + (long long)olu * HoWo : 0ll;
            prev[qq][j] = a.prev ? a.prev[yo[qq][j]] : 0.f;
            r1[qq][j] = half_to_f32<X::kF16>(hpre[want_pre ? yo[qq][j] : 0ll]);
            r2[qq][j] = half_to_f32<X::kF16>(hpost[want_post ? yo[qq][j] : 0ll]);
          }
        } else {
          bs[qq] = (!a.prev && a.bias) ? a.bias[o] : 0.f;
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            ok[qq][j] = rok && pok[j];
            yo[qq][j] = ok[qq][j] ? pbase[j] + (long long)olu * HoWo : 0ll;
            prev[qq][j] = a.prev ? a.prev[yo[qq][j]] : 0.f;
          }
        }
      }
#pragma unroll
      for (int qq = 0; qq < 8; ++qq) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          if constexpr (X::kFp32) {
            float out = (a.accumulate ? prev[qq][j] : bs[qq]) + acc[i][j][qh * 8 + qq] * ws[qq];
            if (a.final_pass) {
              out += r1[qq][j];
              if (a.relu == LSQ_ACT_RELU) out = fmaxf(out, 0.f);
              else if (a.relu >= LSQ_ACT_PRELU) out = out > 0.f ? out : sl[qq] * out;
              out += r2[qq][j];
            }
            if (ok[qq][j]) *reinterpret_cast<float*>(yb + yo[qq][j]) = out;
          } else if constexpr (X::kFused) {
            float out = (a.prev ? prev[qq][j] : bs[qq]) + acc[i][j][qh * 8 + qq] * ws[qq];
            if (a.final_pass) {              // (an absent operand adds nothing: a -0 sum stays -0, as in the unfused call)
              if (want_pre) out += r1[qq][j];
              if (a.act == LSQ_ACT_RELU) out = fmaxf(out, 0.f);
              else if (a.act >= LSQ_ACT_PRELU) out = out > 0.f ? out : sl[qq] * out;
              if (want_post) out += r2[qq][j];
            }
            if (ok[qq][j]) a.store(yo[qq][j], out);
          } else {
            const float out = (a.prev ? prev[qq][j] : bs[qq]) + acc[i][j][qh * 8 + qq] * ws[qq];
            if (ok[qq][j]) a.store(yo[qq][j], out);
          }
        }
      }
    }
  }
}

// Tile shapes: 256 threads, four waves of TM x TN 32x32 tiles (TM = 2).  Out-channel groups wider than 64 take BM = 128 out
// channels per workgroup (2 x 2 waves), the others 64 (1 x 4 waves).
constexpr int kTM = 2;
constexpr int tile_bm(bool wide) { return wide ? 128 : 64; }
// pixels per workgroup of conv_patch.  Stride 1: 128 x 128, or 64 x 256 for narrow layers (the patch conversion is shared
// by more pixels), 64 x 64 per wave.  Other strides: only every second entry of a row feeds a given tap, so the same pixels
// would need a patch stride^2 times as long: 128 x 64 or 64 x 128 tiles (64 x 32 per wave).
constexpr int patch_bn(bool wide, bool unit) { return unit ? (wide ? 128 : 256) : (wide ? 64 : 128); }
// PMAX: patch entries the LDS planes hold; PREMAX: channels per group the folded-batch-norm table holds
constexpr int patch_pmax(bool unit) { return unit ? 512 : 640; }
constexpr int patch_premax(bool unit) { return unit ? 512 : 256; }

// ---------------------------------------------------------------------------------------------
// Tiled (im2col) kernel: a 256-thread workgroup computes BM out-channels x 128 pixels.  Per K-chunk (one tap, 32 channels)
// the block stages into LDS, ONCE for its four waves, (a) the +-1 weight fragment expanded from 4 bytes of the packed plane
// per out-channel and (b) the converted activation chunk (fp32: clamped / batch-norm-folded and split into bf16 hi and lo
// planes), both as [row][32 k] with a 16-byte row pad so that the 16-byte MFMA fragment reads of a 32-lane group hit
// distinct banks.  Global loads of chunk i+1 are issued before the MFMAs of chunk i and written to LDS after them (one
// buffer, two barriers per chunk: half the LDS, three workgroups per CU, measured faster than two buffers and one barrier).
// Each wave owns TM x TN 32x32 tiles: kPlanes*TM*TN*2 MFMAs per chunk against (TM + kPlanes*TN)*2 fragment reads.
constexpr int kKC = 32;                         // channels per K-chunk
constexpr int kRowB = kKC * 2 + 16;             // LDS row pitch in bytes (64 data + 16 pad)
constexpr int kBN = 128;                        // pixels per block

template <class X, bool WIDE>
__global__ __launch_bounds__(256) void conv_tiled(typename X::Args a) {
  constexpr int BM = tile_bm(WIDE), WM = BM / 64, WN = 4 / WM, TM = kTM, TN = kBN / (32 * WN);
  static_assert(WM * WN == 4 && WM * TM * 32 == BM && WN * TN * 32 == kBN, "tile shape");
  constexpr int kPlaneB = kBN * kRowB;          // bytes of an activation plane
  __shared__ __attribute__((aligned(16))) unsigned char smem[BM * kRowB + X::kPlanes * kPlaneB];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid - wm * WN;
  const int col = lane & 31, kh8 = lane >> 5;
  const int tile = blockIdx.y;
  const int grp = tile / a.tiles_per_group;
  const int t = tile - grp * a.tiles_per_group;
  const int o_pad0 = grp * a.og_pad + t * BM;
  const int o0 = grp * a.og + t * BM;
  const int HoWo = a.Ho * a.Wo, HW = a.H * a.W;
  const long long total = (long long)a.N * HoWo;
  const int taps = a.KH * a.KW;
  const int cchunks = (a.cg + kKC - 1) / kKC;
  const int nchunks = taps * cchunks;

  // ---- staging roles
  // activations: thread -> pixel (tid & 127), k half (tid >> 7) of 16 channels
  const int sp = tid & (kBN - 1), skh = tid >> 7;
  const long long spix = (long long)blockIdx.x * kBN + sp;
  const bool sp_valid = spix < total;
  const long long spc = sp_valid ? spix : 0;
  const int sn = (int)(spc / HoWo);
  const int sr = (int)(spc - (long long)sn * HoWo);
  const int sho = sr / a.Wo, swo = sr - sho * a.Wo;
  const typename X::T* xg = a.x + ((long long)sn * a.C + (long long)grp * a.cg) * HW;
  // weights: thread -> out-channel (tid % BM), k part (tid / BM) of KC / (256 / BM) channels
  constexpr int WPARTS = 256 / BM;              // 2 (BM = 128) or 4 (BM = 64)
  constexpr int WK = kKC / WPARTS;              // 16 or 8 channels per thread
  const int so = tid % BM, swp = tid / BM;
  const bool so_valid = t * BM + so < a.og_pad;

  typename X::Raw xr[16 / X::kPerReg];            // 16 converted activations (16-bit: two a dword)
  unsigned wr = 0;
  auto load_chunk = [&](int ch) {
    const int tap = ch / cchunks, cc = ch - tap * cchunks;
    const int kh = tap / a.KW, kw = tap - kh * a.KW;
    const int hi = sho * a.sh - a.ph + kh * a.dh, wi = swo * a.sw - a.pw + kw * a.dw;
    const bool inb = sp_valid && hi >= 0 && hi < a.H && wi >= 0 && wi < a.W;
    const int cbase = cc * kKC + skh * 16;
    // all 16 loads are issued unconditionally (out-of-image / padded channels read a valid dummy
    // address and are zeroed afterwards): a load inside a divergent branch is waited for on the spot,
    // which serialises 16 memory latencies per chunk
    const typename X::T* xp = inb ? xg + (long long)hi * a.W + wi : xg;
    typename X::Raw raw[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) raw[j] = xp[(long long)min(cbase + j, a.cg - 1) * HW];
    if constexpr (X::kFp32) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int c = cbase + j;
        float v = raw[j];
        if (a.pre_scale) {
          // the channel is the same for all lanes of a wave (k half = tid >> 7): scalar loads
          const int cs = __builtin_amdgcn_readfirstlane(grp * a.cg + min(c, a.cg - 1));
          v = fmaf(v, a.pre_scale[cs], a.pre_shift[cs]);
        }
        v = clamp_sym(v, a.alpha);
        xr[j] = (inb && c < a.cg) ? v : 0.f;
      }
    } else if constexpr (X::kFused) {
      // the folded batch norm of the 16 channels being staged: the channel is the same for all lanes of a wave (k half =
      // tid >> 7), scalar loads; the padding is of the folded value: zeroed after the fold
      float ps[16], pb[16];
      if (a.pre_scale) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int cs = __builtin_amdgcn_readfirstlane(grp * a.cg + min(cbase + j, a.cg - 1));
          ps[j] = a.pre_scale[cs];
          pb[j] = a.pre_shift[cs];
        }
      }
#pragma unroll
      for (int p = 0; p < 8; ++p) {
        const unsigned d = a.pre_scale ? fold2<X::kF16>(raw[2 * p], raw[2 * p + 1], ps[2 * p], pb[2 * p], ps[2 * p + 1], pb[2 * p + 1])
                                       : raw[2 * p] | raw[2 * p + 1] << 16;
        const unsigned lo = (inb && cbase + 2 * p < a.cg) ? d & 0xFFFFu : 0u;
        const unsigned hi16 = (inb && cbase + 2 * p + 1 < a.cg) ? d & 0xFFFF0000u : 0u;
        xr[p] = clamp2<X::kF16>(lo | hi16, a);
      }
    } else {
#pragma unroll
      for (int p = 0; p < 8; ++p) {
        const unsigned lo = (inb && cbase + 2 * p < a.cg) ? raw[2 * p] : 0u;
        const unsigned hi16 = (inb && cbase + 2 * p + 1 < a.cg) ? raw[2 * p + 1] : 0u;
        xr[p] = clamp2<X::kF16>(lo | hi16 << 16, a);
      }
    }
    const int c0 = cc * kKC;
    const int g = c0 >> 6;
    const int bit0 = (c0 & 63) + swp * WK;
    const unsigned long long wv =
        so_valid ? a.wbits[((long long)tap * a.Gg + g) * a.opad_total + o_pad0 + so] : 0ull;
    wr = (unsigned)(wv >> bit0) & ((1u << WK) - 1u);
  };
  auto store_chunk = [&]() {
    unsigned char* sA = smem;
    unsigned char* sB = sA + BM * kRowB;
    if constexpr (X::kFp32) {
      // activations -> bf16 hi and lo = bf16(x - hi) (x - hi is exact in fp32; |x - hi - lo| <= 2^-18 |x|),
      // 16 values = 32 bytes each
      unsigned hi[8], lo[8];
#pragma unroll
      for (int p = 0; p < 8; ++p) split_pair(xr[2 * p], xr[2 * p + 1], hi[p], lo[p]);
      uint4* dh = reinterpret_cast<uint4*>(sB + sp * kRowB + skh * 32);
      uint4* dl = reinterpret_cast<uint4*>(sB + kPlaneB + sp * kRowB + skh * 32);
      dh[0] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
      dh[1] = make_uint4(hi[4], hi[5], hi[6], hi[7]);
      dl[0] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
      dl[1] = make_uint4(lo[4], lo[5], lo[6], lo[7]);
    } else {
      uint4* db = reinterpret_cast<uint4*>(sB + sp * kRowB + skh * 32);
      db[0] = make_uint4(xr[0], xr[1], xr[2], xr[3]);
      db[1] = make_uint4(xr[4], xr[5], xr[6], xr[7]);
    }
    // weights: WK sign bits -> WK values +-1
    unsigned* dw = reinterpret_cast<unsigned*>(sA + so * kRowB + swp * WK * 2);
#pragma unroll
    for (int p = 0; p < WK / 2; ++p) {
      const unsigned b0 = (wr >> (2 * p)) & 1u, b1 = (wr >> (2 * p + 1)) & 1u;
      dw[p] = kOne2<X::kF16> | ((b0 ^ 1u) << 15) | ((b1 ^ 1u) << 31);
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

  load_chunk(0);
  store_chunk();
  __syncthreads();
  for (int ch = 0; ch < nchunks; ++ch) {
    if (ch + 1 < nchunks) load_chunk(ch + 1);          // in flight during the MFMAs below
    const unsigned char* sA = smem;
    const unsigned char* sB = sA + BM * kRowB;
#pragma unroll
    for (int ks = 0; ks < kKC / 16; ++ks) {
      if constexpr (X::kPlanes == 2) {
        const unsigned char* sBh = sB;
        const unsigned char* sBl = sBh + kBN * kRowB;
        Frag af[TM], bh[TN], bl[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const uint4 v = *reinterpret_cast<const uint4*>(sA + ((wm * TM + i) * 32 + col) * kRowB + ks * 32 + kh8 * 16);
          af[i].u[0] = v.x; af[i].u[1] = v.y; af[i].u[2] = v.z; af[i].u[3] = v.w;
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int row = ((wn * TN + j) * 32 + col) * kRowB + ks * 32 + kh8 * 16;
          const uint4 vh = *reinterpret_cast<const uint4*>(sBh + row);
          const uint4 vl = *reinterpret_cast<const uint4*>(sBl + row);
          bh[j].u[0] = vh.x; bh[j].u[1] = vh.y; bh[j].u[2] = vh.z; bh[j].u[3] = vh.w;
          bl[j].u[0] = vl.x; bl[j].u[1] = vl.y; bl[j].u[2] = vl.z; bl[j].u[3] = vl.w;
        }
        // hi and lo of a tile back to back
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            acc[i][j] = mfma16<X::kF16>(af[i], bh[j], acc[i][j]);
            acc[i][j] = mfma16<X::kF16>(af[i], bl[j], acc[i][j]);
          }
      } else {
        Frag af[TM], bf[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = lds_frag(sA + ((wm * TM + i) * 32 + col) * kRowB + ks * 32 + kh8 * 16);
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[j] = lds_frag(sB + ((wn * TN + j) * 32 + col) * kRowB + ks * 32 + kh8 * 16);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = mfma16<X::kF16>(af[i], bf[j], acc[i][j]);
      }
    }
    __syncthreads();                             // everyone is done reading before the single buffer is rewritten
    if (ch + 1 < nchunks) store_chunk();
    __syncthreads();
  }

  store_tiles<X, typename X::template Off<false>, BM, kBN, TM, TN>(a, acc, blockIdx.x, t, o0, wm, wn, col, kh8);
}

// ---------------------------------------------------------------------------------------------
// Patch kernel (any stride / padding / dilation).  Padded coordinates hp = hi + pad_h, wp = wi + pad_w
// and the linear index L = (n*Hp + hp)*Wp + wp: output pixel (n, ho, wo) and tap (kh, kw) read
// L = B + T with B = (n*Hp + ho*stride_h)*Wp + wo*stride_w and T = kh*dil_h*Wp + kw*dil_w.  The BN consecutive output
// pixels of a workgroup therefore touch the contiguous range [B_first, B_last + T_max] of L -- the patch,
// at most PLr <= PMAX entries (host-side bound, multiple of 128).  Per 16-channel chunk (one MFMA k-step)
// the workgroup
//   1. converts the patch once: lanes = consecutive entries = consecutive addresses of one channel
//      (coalesced), X::stage8 (fp32: folded batch norm + clamp + bf16 hi / lo split; 16-bit: clamp), LDS rows
//      [entry][16 channels] of 32 bytes in kPlanes planes;
//   2. expands the +-1 weights of up to 9 taps x BM out-channels x 16 channels from the packed plane
//      into LDS rows of 32 bytes, cooperatively (each 16-bit piece once per workgroup);
//   3. runs the taps back to back: A fragments at compile-time LDS offsets, B fragments at per-lane
//      addresses (entry of the lane's pixel + T) computed once per workgroup -- no address arithmetic,
//      no barrier and no global access inside the tap loop.
// The global loads of chunk i+1 (activations and weight words) are issued right before the tap loop of
// chunk i and consumed after it.  Rows have no padding: the two 16-byte halves of row r are swapped when
// bit 3 of r is set, which makes any 16 consecutive rows hit 16 distinct 4-bank groups.
// Each wave owns a 64 x 32 TN tile (2 x TN MFMA tiles); at TN = 2 and two planes: 16 MFMAs per tap against 6 fragment reads.
constexpr int kTapGroup = 9;                     // taps whose weights are resident at a time

template <class X, bool WIDE, bool UNIT, bool MANY_TAPS>
__global__ __launch_bounds__(256) void conv_patch(typename X::Args a, int Hp, int Wp, int PLr) {
  constexpr int BM = tile_bm(WIDE), BN = patch_bn(WIDE, UNIT), WM = BM / 64, WN = 4 / WM, TM = kTM, TN = BN / (32 * WN);
  constexpr int kPMaxEntries = patch_pmax(UNIT), kPlane = kPMaxEntries * kPRow, kMaxPre = patch_premax(UNIT);
  static_assert(WM * WN == 4 && WM * TM * 32 == BM && WN * TN * 32 == BN, "tile shape");
  constexpr int kItems = (kPMaxEntries * 2 + 255) / 256; // (entry, octet) items per thread, at most
  constexpr int WPARTS = 256 / BM;                       // threads per weight row
  constexpr int WTAPS = (kTapGroup + WPARTS - 1) / WPARTS;   // taps per thread and group
  __shared__ __attribute__((aligned(16))) unsigned char sP[X::kPlanes * kPlane];
  __shared__ __attribute__((aligned(16))) unsigned char sW[kTapGroup * BM * kPRow];
  __shared__ __attribute__((aligned(16))) float sPre[2 * kMaxPre];   // (fp32 only: never referenced otherwise)
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid - wm * WN;
  const int col = lane & 31, kh8 = lane >> 5;
  const int tile = blockIdx.y;
  const int grp = tile / a.tiles_per_group;
  const int t = tile - grp * a.tiles_per_group;
  const int o_pad0 = grp * a.og_pad + t * BM;
  const int o0 = grp * a.og + t * BM;
  const int HoWo = a.Ho * a.Wo, HW = a.H * a.W, HpWp = Hp * Wp;
  const int total = a.N * HoWo;
  const int taps = a.KH * a.KW;
  const int cchunks = (a.cg + kPC - 1) / kPC;
  const bool ragged = (a.cg % kPC) != 0;
  [[maybe_unused]] float lim = 0.f;                      // fp32: the clamp bound (clamp_identity: no-op bounds)
  if constexpr (X::kFp32) lim = a.alpha >= 0.f ? a.alpha : __builtin_inff();

  // 32-bit index math throughout: the host takes this kernel only when N*Hp*Wp and N*C*H*W fit in 31 bits (patch_plan)
  auto base_of = [&](int p) {
    const int n = p / HoWo;
    const int r = p - n * HoWo;
    const int ho = r / a.Wo;
    return (n * Hp + ho * a.sh) * Wp + (r - ho * a.Wo) * a.sw;
  };
  const int p0 = blockIdx.x * BN;
  const int bmin = base_of(p0);
  const typename X::T* xg = a.x + (long long)grp * a.cg * HW;

  if constexpr (X::kFp32) {
    if (a.pre_scale) {
      for (int c = tid; c < cchunks * kPC; c += 256) {
        const int cs = grp * a.cg + min(c, a.cg - 1);
        sPre[c] = a.pre_scale[cs];
        sPre[kMaxPre + c] = a.pre_shift[cs];
      }
    }
  }

  // ---- per-lane fragment addresses (fixed for the whole kernel)
  int e_pix[TN];                                         // patch entry of this lane's pixel, per column tile
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int pix = p0 + (wn * TN + j) * 32 + col;
    e_pix[j] = pix < total ? base_of(pix) - bmin : 0;
  }
  int b_addr[kTapGroup][TN];                             // first-plane byte address of the B fragment, first tap group
  {
    int kh = 0, kw = 0;
#pragma unroll
    for (int tt = 0; tt < kTapGroup; ++tt) {
      const int toff = kh * a.dh * Wp + kw * a.dw;
#pragma unroll
      for (int j = 0; j < TN; ++j) b_addr[tt][j] = swz(e_pix[j] + (tt < taps ? toff : 0), kh8);
      if (++kw == a.KW) { kw = 0; ++kh; }
    }
  }
  int a_addr[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) a_addr[i] = swz((wm * TM + i) * 32 + col, kh8);

  // ---- patch staging roles: item = (entry, channel octet); the octet is uniform per wave (PLr % 128 == 0)
  const int n_items = PLr >> 7;
  int it_off[kItems], it_dst[kItems];
#pragma unroll
  for (int u = 0; u < kItems; ++u) {
    const int i = tid + 256 * u;
    const int oct = i >= PLr;
    const int e = i - oct * PLr;
    const int L = bmin + e;
    const int n = L / HpWp;
    const int rem = L - n * HpWp;
    const int hp = rem / Wp;
    const int hi = hp - a.ph, wi = rem - hp * Wp - a.pw;
    const bool inside = u < n_items && n < a.N && hi >= 0 && hi < a.H && wi >= 0 && wi < a.W;
    it_off[u] = inside ? n * a.C * HW + hi * a.W + wi : -1;
    it_dst[u] = swz(e, oct) | (oct << 30);               // bit 30 carries the octet
  }
  typename X::Raw raw[kItems][8];
  auto issue_xloads = [&](int cc) {
    // address = wave-uniform channel base (scalar registers) + the lane's 32-bit byte offset, which never
    // changes: no vector address arithmetic.  Halo / padded channels read a valid dummy address and are
    // zeroed at conversion.
#pragma unroll
    for (int u = 0; u < kItems; ++u) {
      if (u < n_items) {
        const int c0 = __builtin_amdgcn_readfirstlane(cc * kPC + (it_dst[u] >> 30) * 8);
        const unsigned boff = it_off[u] < 0 ? 0u : (unsigned)it_off[u] * (unsigned)sizeof(typename X::T);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const char* cbase = reinterpret_cast<const char*>(xg + (long long)min(c0 + j, a.cg - 1) * HW);
          raw[u][j] = *reinterpret_cast<const typename X::T*>(cbase + boff);
        }
      }
    }
  };
  auto convert_store = [&](int cc) {
#pragma unroll
    for (int u = 0; u < kItems; ++u) {
      if (u < n_items) {
        const int c0 = cc * kPC + (it_dst[u] >> 30) * 8;
        if constexpr (X::kFp32) {                        // folded batch norm, v_med3 clamp, hi / lo split
          float v[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = raw[u][j];
          if (a.pre_scale) {                             // wave-uniform addresses: broadcast LDS reads
            const float4* ps = reinterpret_cast<const float4*>(sPre + c0);
            const float4* pb = reinterpret_cast<const float4*>(sPre + kMaxPre + c0);
            const float4 s0 = ps[0], s1 = ps[1], b0 = pb[0], b1 = pb[1];
            v[0] = fmaf(v[0], s0.x, b0.x); v[1] = fmaf(v[1], s0.y, b0.y);
            v[2] = fmaf(v[2], s0.z, b0.z); v[3] = fmaf(v[3], s0.w, b0.w);
            v[4] = fmaf(v[4], s1.x, b1.x); v[5] = fmaf(v[5], s1.y, b1.y);
            v[6] = fmaf(v[6], s1.z, b1.z); v[7] = fmaf(v[7], s1.w, b1.w);
          }
#pragma unroll
          for (int j = 0; j < 8; ++j)
            v[j] = (it_off[u] >= 0 && (!ragged || c0 + j < a.cg)) ? __builtin_amdgcn_fmed3f(v[j], -lim, lim) : 0.f;
          unsigned hi[4], lo[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) split_pair(v[2 * q], v[2 * q + 1], hi[q], lo[q]);
          const int dst = it_dst[u] & 0xFFFFF;
          *reinterpret_cast<uint4*>(sP + dst) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
          *reinterpret_cast<uint4*>(sP + kPlane + dst) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        } else if constexpr (X::kFused) {                // folded batch norm of this octet's channels, then as below
          float ps[8], pb[8];
          if (a.pre_scale) {                             // wave-uniform addresses: scalar loads
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const int cs = __builtin_amdgcn_readfirstlane(grp * a.cg + min(c0 + j, a.cg - 1));
              ps[j] = a.pre_scale[cs];
              pb[j] = a.pre_shift[cs];
            }
          }
          unsigned d[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const unsigned f = a.pre_scale ? fold2<X::kF16>(raw[u][2 * q], raw[u][2 * q + 1], ps[2 * q], pb[2 * q], ps[2 * q + 1], pb[2 * q + 1])
                                           : raw[u][2 * q] | raw[u][2 * q + 1] << 16;
            const unsigned lo = (it_off[u] >= 0 && (!ragged || c0 + 2 * q < a.cg)) ? f & 0xFFFFu : 0u;
            const unsigned hi16 = (it_off[u] >= 0 && (!ragged || c0 + 2 * q + 1 < a.cg)) ? f & 0xFFFF0000u : 0u;
            d[q] = clamp2<X::kF16>(lo | hi16, a);
          }
          *reinterpret_cast<uint4*>(sP + (it_dst[u] & 0xFFFFF)) = make_uint4(d[0], d[1], d[2], d[3]);
        } else {                                         // clamp in the activations' own type
          unsigned d[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const unsigned lo = (it_off[u] >= 0 && (!ragged || c0 + 2 * q < a.cg)) ? raw[u][2 * q] : 0u;
            const unsigned hi16 = (it_off[u] >= 0 && (!ragged || c0 + 2 * q + 1 < a.cg)) ? raw[u][2 * q + 1] : 0u;
            d[q] = clamp2<X::kF16>(lo | hi16 << 16, a);
          }
          *reinterpret_cast<uint4*>(sP + (it_dst[u] & 0xFFFFF)) = make_uint4(d[0], d[1], d[2], d[3]);
        }
      }
    }
  };

  // ---- weight staging roles: thread -> out-channel row (tid % BM), taps part + WPARTS * k of the group
  const int so = tid % BM, part = tid / BM;
  const bool so_valid = t * BM + so < a.og_pad;
  const unsigned* wcol = reinterpret_cast<const unsigned*>(a.wbits + o_pad0 + (so_valid ? so : 0));
  unsigned one_bf16x2 = 0;                               // fp32: 0x3F803F80 held in a vector register (one scalar operand per VALU op)
  if constexpr (X::kFp32) asm volatile("v_mov_b32 %0, 0x3f803f80" : "=v"(one_bf16x2));
  unsigned wraw[WTAPS];
  auto issue_wloads = [&](unsigned (&dst)[WTAPS], int tg, int cc) {
    const int c0 = cc * kPC;
#pragma unroll
    for (int k = 0; k < WTAPS; ++k) {
      const int tap = min(tg + part + WPARTS * k, taps - 1);
      dst[k] = wcol[2 * ((tap * a.Gg + (c0 >> 6)) * a.opad_total) + ((c0 >> 5) & 1)];
    }
  };
  auto expand_store = [&](const unsigned (&src)[WTAPS], int tg, int cc) {
    const int sh = (cc * kPC) & 16;
#pragma unroll
    for (int k = 0; k < WTAPS; ++k) {
      const int ts = part + WPARTS * k;
      if (ts < kTapGroup && tg + ts < taps) {
        // 16 sign bits (set = +1) -> 16 values +-1.  The inverted bits replicated into both 16-bit halves, one
        // packed 16-bit shift moves bit 2q / 2q+1 to the sign position of the low / high half, one
        // and-or merges it into 1.0: two VALU ops per pair of weights.
        const unsigned m = so_valid ? ~(src[k] >> sh) & 0xFFFFu : 0xFFFFu;     // rows past the group: -1 * 0 anyway
        const u16x2 rep = __builtin_bit_cast(u16x2, m | (m << 16));
        unsigned d[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const u16x2 shq = {(unsigned short)(15 - 2 * q), (unsigned short)(14 - 2 * q)};
          const unsigned xq = __builtin_bit_cast(unsigned, rep << shq);
          if constexpr (X::kFp32) asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(d[q]) : "v"(xq), "s"(0x80008000u), "v"(one_bf16x2));
          else d[q] = (xq & 0x80008000u) | kOne2<X::kF16>;
        }
        unsigned char* row = sW + ts * (BM * kPRow);
        *reinterpret_cast<uint4*>(row + swz(so, 0)) = make_uint4(d[0], d[1], d[2], d[3]);
        *reinterpret_cast<uint4*>(row + swz(so, 1)) = make_uint4(d[4], d[5], d[6], d[7]);
      }
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

  auto mfma_tap = [&](int tt, const int (&baddr)[TN]) {
    if constexpr (X::kPlanes == 2) {
      Frag af[TM], bh[TN], bl[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const uint4 v = *reinterpret_cast<const uint4*>(sW + tt * (BM * kPRow) + a_addr[i]);
        af[i].u[0] = v.x; af[i].u[1] = v.y; af[i].u[2] = v.z; af[i].u[3] = v.w;
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const uint4 vh = *reinterpret_cast<const uint4*>(sP + baddr[j]);
        const uint4 vl = *reinterpret_cast<const uint4*>(sP + kPlane + baddr[j]);
        bh[j].u[0] = vh.x; bh[j].u[1] = vh.y; bh[j].u[2] = vh.z; bh[j].u[3] = vh.w;
        bl[j].u[0] = vl.x; bl[j].u[1] = vl.y; bl[j].u[2] = vl.z; bl[j].u[3] = vl.w;
      }
      // hi products of all tiles first, then lo: dependent MFMAs on one accumulator are TM * TN apart
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = mfma16<X::kF16>(af[i], bh[j], acc[i][j]);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = mfma16<X::kF16>(af[i], bl[j], acc[i][j]);
    } else {
      Frag af[TM], bf[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = lds_frag(sW + tt * (BM * kPRow) + a_addr[i]);
#pragma unroll
      for (int j = 0; j < TN; ++j) bf[j] = lds_frag(sP + baddr[j]);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = mfma16<X::kF16>(af[i], bf[j], acc[i][j]);
    }
  };

  issue_xloads(0);
  issue_wloads(wraw, 0, 0);
  if constexpr (X::kFp32) __syncthreads();               // sPre visible
  for (int cc = 0; cc < cchunks; ++cc) {
    convert_store(cc);
    expand_store(wraw, 0, cc);
    __syncthreads();                                     // patch and first tap group of this chunk visible
    if constexpr (!MANY_TAPS) {
      if (cc + 1 < cchunks) {                            // next chunk's loads fly during the MFMAs below
        issue_xloads(cc + 1);
        issue_wloads(wraw, 0, cc + 1);
      }
#pragma unroll
      for (int tt = 0; tt < kTapGroup; ++tt)
        if (tt < taps) mfma_tap(tt, b_addr[tt]);
    } else {
      // more than 9 taps (5x5 ...): later groups are staged in place, B addresses recomputed per tap
      int kh = 0, kw = 0;
      for (int tg = 0; tg < taps; tg += kTapGroup) {
        if (tg) {
          unsigned wtmp[WTAPS];
          issue_wloads(wtmp, tg, cc);
          __syncthreads();                               // previous group's fragment reads finished
          expand_store(wtmp, tg, cc);
          __syncthreads();
        }
        for (int tt = 0; tt < kTapGroup && tg + tt < taps; ++tt) {
          const int toff = kh * a.dh * Wp + kw * a.dw;
          int baddr[TN];
#pragma unroll
          for (int j = 0; j < TN; ++j) baddr[j] = swz(e_pix[j] + toff, kh8);
          mfma_tap(tt, baddr);                           // (tt is not a compile-time constant here: the A offset is an add)
          if (++kw == a.KW) { kw = 0; ++kh; }
        }
      }
      if (cc + 1 < cchunks) {
        issue_xloads(cc + 1);
        issue_wloads(wraw, 0, cc + 1);
      }
    }
    __syncthreads();                                     // every wave is done reading before LDS is rewritten
  }
  store_tiles<X, typename X::template Off<true>, BM, BN, TM, TN>(a, acc, blockIdx.x, t, o0, wm, wn, col, kh8);
}

// ---------------------------------------------------------------------------------------------
// Host side.  The geometry fields every operand struct has (x, weights, scales and the epilogue's operands are the entry's).
template <class A>
void fill_geom(A& a, const lsq_conv_geom* g, int Ho, int Wo) {
  a.N = g->N; a.C = g->C; a.H = g->H; a.W = g->W; a.O = g->O; a.KH = g->KH; a.KW = g->KW;
  a.sh = g->stride_h; a.sw = g->stride_w; a.ph = g->pad_h; a.pw = g->pad_w; a.dh = g->dil_h; a.dw = g->dil_w;
  a.cg = g->C / g->groups;
  a.Gg = (a.cg + 63) / 64;
  a.Ho = Ho; a.Wo = Wo;
  a.og = g->O / g->groups;
  a.og_pad = (a.og + 15) / 16 * 16;
  a.opad_total = g->groups * a.og_pad;
  a.tiles_per_group = (a.og + tile_bm(a.og > 64) - 1) / tile_bm(a.og > 64);
}

struct PatchPlan {
  bool wide;                           // 128 out-channels per workgroup, else 64
  bool patch;                          // conv_patch, else conv_tiled; the fields below hold for conv_patch only
  bool unit, many;                     // unit stride; more than kTapGroup taps
  int pbn, PLr, Hp, Wp;                // pixels per workgroup, patch entries (multiple of 128), padded image
};

// THE rule that decides patch or tiled, for both libraries (tests/golden/conv_half_cases.py restates it as the check).  g has
// passed check_geom and Ho, Wo are its (positive) output size; has_pre: a folded batch norm, whose table must hold a group's
// channels.  Layers whose input patch fits the LDS planes take the patch kernel.  All in 64 bits: the patch kernel's own
// 32-bit index math is what the 2^30 / 2^31 limits guard.
inline PatchPlan patch_plan(const lsq_conv_geom* g, long long Ho, long long Wo, bool has_pre) {
  PatchPlan p = {};
  const int cg = g->C / g->groups;
  p.wide = g->O / g->groups > 64;
  const bool unit = g->stride_h == 1 && g->stride_w == 1;
  const long long Hp = (long long)g->H + 2ll * g->pad_h, Wp = (long long)g->W + 2ll * g->pad_w;
  const int pbn = patch_bn(p.wide, unit);
  const long long row_gap = (long long)g->stride_h * Wp - Wo * g->stride_w;
  const long long img_gap = (Hp - Ho * g->stride_h) * Wp;
  const long long patch = (long long)(pbn - 1) * g->stride_w + ((pbn - 1) / Wo + 1) * (row_gap > 0 ? row_gap : 0) +
                          ((pbn - 1) / (Ho * Wo) + 1) * (img_gap > 0 ? img_gap : 0) +
                          (long long)(g->KH - 1) * g->dil_h * Wp + (long long)(g->KW - 1) * g->dil_w + 1;
  const long long PLr = (patch + 127) / 128 * 128;
  p.patch = PLr <= patch_pmax(unit) && (!has_pre || (cg + kPC - 1) / kPC * kPC <= patch_premax(unit)) &&
            (long long)g->N * g->C * g->H * g->W < (1ll << 30) && (long long)g->N * Hp * Wp + PLr < (1ll << 31) &&
            (long long)g->N * g->O * Ho * Wo < (1ll << 30);
  if (p.patch) {
    p.unit = unit; p.many = (long long)g->KH * g->KW > kTapGroup;
    p.pbn = pbn; p.PLr = (int)PLr; p.Hp = (int)Hp; p.Wp = (int)Wp;
  }
  return p;
}

// one launch (one weight plane) of the kernel the plan names; a holds the operands of fill_geom's geometry
template <class X>
int launch(const typename X::Args& a, const PatchPlan& p, hipStream_t st) {
  typedef typename X::Args A;
  static constexpr void (*kPatch[2][2][2])(A, int, int, int) = {   // [wide][unit][many]
      {{conv_patch<X, false, false, false>, conv_patch<X, false, false, true>},
       {conv_patch<X, false, true, false>, conv_patch<X, false, true, true>}},
      {{conv_patch<X, true, false, false>, conv_patch<X, true, false, true>},
       {conv_patch<X, true, true, false>, conv_patch<X, true, true, true>}}};
  static constexpr void (*kTiled[2])(A) = {conv_tiled<X, false>, conv_tiled<X, true>};
  const long long total = (long long)a.N * a.Ho * a.Wo;
  const unsigned otiles = (unsigned)(a.opad_total / a.og_pad * a.tiles_per_group);
  if (p.patch)
    hipLaunchKernelGGL(kPatch[p.wide][p.unit][p.many], dim3((unsigned)((total + p.pbn - 1) / p.pbn), otiles), dim3(256), 0,
                       st, a, p.Hp, p.Wp, p.PLr);
  else
    hipLaunchKernelGGL(kTiled[p.wide], dim3((unsigned)((total + kBN - 1) / kBN), otiles), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace
}  // namespace signw
}  // namespace lsq
