// lsq_signw_conv2d_half: bf16 / fp16 activations x sign-weight planes, the convolution, on the 16-bit matrix cores of gfx950
// (v_mfma_f32_32x32x16_bf16 / v_mfma_f32_32x32x16_f16).
//
// lsq_signw_conv2d (csrc/lsq_signw_conv.hip) with a B operand that already is 16-bit: the same implicit GEMM
// D[o][pixel] = sum_k S[o][k] * X[k][pixel], k = (tap, channel), the same two kernels, tile shapes and choice between them,
// but the activations are read as they are (half the bytes), clamped in their own type and staged as ONE LDS plane -- no
// hi / lo split, one MFMA per (16 channels, tap) and tile where that kernel issues two.  The weights stay at one bit each
// in memory and are expanded to +-1.0 of the activations' type in the kernel (0x3F80 / 0x3C00 with the sign bit merged in).
//   conv_patch  (the input patch of the workgroup's output pixels fits PMAX LDS rows): per 16-channel chunk the patch is
//               staged once, clamped, as rows [entry][16 channels] of 32 bytes with swz's half-swap, next to the expanded
//               weights of up to 9 taps; the taps then run back to back at precomputed addresses while the next chunk's
//               global loads are in flight.  More than 9 taps: later tap groups are staged in place.
//   conv_tiled  (everything else): im2col staging per (tap, 32-channel chunk), 128 pixels per workgroup.
// Activations are loaded element by element (2-byte loads, lanes on consecutive addresses of one channel), so any
// 2-byte-aligned x gives the same bits.  Out-of-image entries, padded channels and pixels past the end read a valid address
// and are zeroed: zero padding is exact.
// Epilogue (restated from store_tiles of lsq_signw_conv.h, which stores float only): out = base + I * ws[o] with a separate
// multiply and add, base = bias[o] (or 0) at the first plane and the fp32 sum of the planes before it afterwards; a launch
// holds one plane.  The sum is stored as fp32 (into y, or into the workspace while launches of a 16-bit y remain) or rounded
// once into the 16-bit y by the last launch, one element per store.

#include <math.h>
#include <string.h>

#include "lsq_hip_conv_half.h"
#include "../lsq_signw_conv.h"

namespace lsq {
namespace signw {
namespace {

typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

struct HArgs {
  const unsigned short* x;             // [N][C][H][W], bf16 or fp16 bits
  const unsigned long long* wbits;     // [taps][Gg][Opad]  (the weight plane of this launch)
  const float* wscale;                 // [O], the plane of this launch
  const float* bias;                   // [O] or null
  const float* prev;                   // [N][O][Ho][Wo] fp32 sum of the launches before this one, or null (base = bias or 0)
  void* out;                           // [N][O][Ho][Wo] of odt
  int odt;                             // LSQ_DTYPE_* of out
  float lim;                           // clamp bound, a value of the activations' type (+inf: identity)
  unsigned lim2;                       // fp16: its bits in both halves
  int clamp;                           // 0: no bound (negative or +inf): the values pass as they are, NaN and inf included
  int N, C, H, W, O, KH, KW, sh, sw, ph, pw, dh, dw;
  int Gg, Ho, Wo, cg, og, og_pad, opad_total, tiles_per_group;
};

// two 16-bit activations in a dword, clamped: bf16 through fp32 (v_med3_f32 of the value shifted up; the bound is a bf16
// value, so the result is one), fp16 packed (v_pk_max_f16 / v_pk_min_f16).  Both return the non-NaN operand: under a finite
// bound a NaN activation becomes -bound (stated in the header)
template <bool F16>
__device__ __forceinline__ unsigned clamp2(unsigned d, const HArgs& a) {
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

// the epilogue's store: fp32, or rounded to nearest even into the 16-bit type (one element: nothing beside it is written)
__device__ __forceinline__ void store_out(const HArgs& a, long long i, float v) {
  if (a.odt == LSQ_DTYPE_F32) static_cast<float*>(a.out)[i] = v;
  else if (a.odt == LSQ_DTYPE_BF16) static_cast<__bf16*>(a.out)[i] = (__bf16)v;
  else static_cast<_Float16*>(a.out)[i] = (_Float16)v;
}

// Epilogue of both kernels: lane = pixel column, registers = out-channel rows (consecutive elements of a row per half-wave).
template <int BM, int BN, int TM, int TN>
__device__ __forceinline__ void store_tiles_half(const HArgs& a, const f32x16 (&acc)[TM][TN], int ptile, int t, int o0,
                                                 int wm, int wn, int col, int kh8) {
  const int HoWo = a.Ho * a.Wo;
  const long long total = (long long)a.N * HoWo;
  long long pbase[TN];                                 // element index of (n, out-channel o0 + 4*kh8, pixel)
  bool pok[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const long long pix = (long long)ptile * BN + (wn * TN + j) * 32 + col;
    pok[j] = pix < total;
    const int n = pok[j] ? (int)(pix / HoWo) : 0;
    const int r = pok[j] ? (int)(pix - (long long)n * HoWo) : 0;
    pbase[j] = ((long long)n * a.O + o0 + 4 * kh8) * HoWo + r;
  }
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int qh = 0; qh < 2; ++qh) {
      // batch of 8 out-channel rows x TN pixel tiles: every load of the batch is issued before the first use
      float ws[8], bs[8], prev[8][TN];
      long long yo[8][TN];
      bool ok[8][TN];
#pragma unroll
      for (int qq = 0; qq < 8; ++qq) {
        const int q = qh * 8 + qq;
        const int olu = (wm * TM + i) * 32 + (q & 3) + 8 * (q >> 2);      // wave-uniform part of the row
        const int ol = olu + 4 * kh8;                                     // C/D layout of the 32x32 MFMA
        const bool rok = t * BM + ol < a.og;
        const int o = o0 + (rok ? ol : 0);
        ws[qq] = a.wscale[o];
        bs[qq] = (!a.prev && a.bias) ? a.bias[o] : 0.f;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          ok[qq][j] = rok && pok[j];
          yo[qq][j] = ok[qq][j] ? pbase[j] + (long long)olu * HoWo : 0ll;
          prev[qq][j] = a.prev ? a.prev[yo[qq][j]] : 0.f;
        }
      }
#pragma unroll
      for (int qq = 0; qq < 8; ++qq) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const float out = (a.prev ? prev[qq][j] : bs[qq]) + acc[i][j][qh * 8 + qq] * ws[qq];
          if (ok[qq][j]) store_out(a, yo[qq][j], out);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Tiled (im2col) kernel: a 256-thread workgroup computes BM out-channels x 128 pixels.  Per K-chunk (one tap, 32 channels)
// the block stages into LDS, once for its four waves, the +-1 weight fragment expanded from 4 bytes of the packed plane per
// out-channel and the clamped activation chunk, both as [row][32 k] with a 16-byte row pad.  Global loads of chunk i + 1 are
// issued before the MFMAs of chunk i and written to LDS after them (one buffer, two barriers per chunk).
constexpr int kKC = 32;                         // channels per K-chunk
constexpr int kRowB = kKC * 2 + 16;             // LDS row pitch in bytes (64 data + 16 pad)
constexpr int kBN = 128;                        // pixels per block

template <bool F16, int BM, int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(256) void conv_tiled(HArgs a) {
  static_assert(WM * WN == 4 && WM * TM * 32 == BM && WN * TN * 32 == kBN, "tile shape");
  __shared__ __attribute__((aligned(16))) unsigned char smem[(BM + kBN) * kRowB];
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
  const unsigned short* xg = a.x + ((long long)sn * a.C + (long long)grp * a.cg) * HW;
  // weights: thread -> out-channel (tid % BM), k part (tid / BM) of KC / (256 / BM) channels
  constexpr int WPARTS = 256 / BM;              // 2 (BM = 128) or 4 (BM = 64)
  constexpr int WK = kKC / WPARTS;              // 16 or 8 channels per thread
  const int so = tid % BM, swp = tid / BM;
  const bool so_valid = t * BM + so < a.og_pad;

  unsigned xr[8];                               // 16 clamped activations, two a dword
  unsigned wr = 0;
  auto load_chunk = [&](int ch) {
    const int tap = ch / cchunks, cc = ch - tap * cchunks;
    const int kh = tap / a.KW, kw = tap - kh * a.KW;
    const int hi = sho * a.sh - a.ph + kh * a.dh, wi = swo * a.sw - a.pw + kw * a.dw;
    const bool inb = sp_valid && hi >= 0 && hi < a.H && wi >= 0 && wi < a.W;
    const int cbase = cc * kKC + skh * 16;
    // all 16 loads are issued unconditionally (out-of-image / padded channels read a valid dummy address and are zeroed
    // afterwards)
    const unsigned short* xp = inb ? xg + (long long)hi * a.W + wi : xg;
    unsigned raw[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) raw[j] = xp[(long long)min(cbase + j, a.cg - 1) * HW];
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const unsigned lo = (inb && cbase + 2 * p < a.cg) ? raw[2 * p] : 0u;
      const unsigned hi16 = (inb && cbase + 2 * p + 1 < a.cg) ? raw[2 * p + 1] : 0u;
      xr[p] = clamp2<F16>(lo | hi16 << 16, a);
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
    uint4* db = reinterpret_cast<uint4*>(sB + sp * kRowB + skh * 32);
    db[0] = make_uint4(xr[0], xr[1], xr[2], xr[3]);
    db[1] = make_uint4(xr[4], xr[5], xr[6], xr[7]);
    // weights: WK sign bits -> WK values +-1
    unsigned* dw = reinterpret_cast<unsigned*>(sA + so * kRowB + swp * WK * 2);
#pragma unroll
    for (int p = 0; p < WK / 2; ++p) {
      const unsigned b0 = (wr >> (2 * p)) & 1u, b1 = (wr >> (2 * p + 1)) & 1u;
      dw[p] = kOne2<F16> | ((b0 ^ 1u) << 15) | ((b1 ^ 1u) << 31);
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
      Frag af[TM], bf[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = lds_frag(sA + ((wm * TM + i) * 32 + col) * kRowB + ks * 32 + kh8 * 16);
#pragma unroll
      for (int j = 0; j < TN; ++j) bf[j] = lds_frag(sB + ((wn * TN + j) * 32 + col) * kRowB + ks * 32 + kh8 * 16);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = mfma16<F16>(af[i], bf[j], acc[i][j]);
    }
    __syncthreads();                             // everyone is done reading before the single buffer is rewritten
    if (ch + 1 < nchunks) store_chunk();
    __syncthreads();
  }

  store_tiles_half<BM, kBN, TM, TN>(a, acc, blockIdx.x, t, o0, wm, wn, col, kh8);
}

// ---------------------------------------------------------------------------------------------
// Patch kernel (any stride / padding / dilation).  Padded coordinates hp = hi + pad_h, wp = wi + pad_w and the linear index
// L = (n*Hp + hp)*Wp + wp: output pixel (n, ho, wo) and tap (kh, kw) read L = B + T with B = (n*Hp + ho*stride_h)*Wp +
// wo*stride_w and T = kh*dil_h*Wp + kw*dil_w.  The BN consecutive output pixels of a workgroup touch the contiguous range
// [B_first, B_last + T_max] of L -- the patch, at most PLr <= PMAX entries (host-side bound, multiple of 128).  Per
// 16-channel chunk (one MFMA k-step) the workgroup
//   1. stages the patch once: lanes = consecutive entries = consecutive addresses of one channel, clamp, LDS rows
//      [entry][16 channels] of 32 bytes in ONE plane;
//   2. expands the +-1 weights of up to 9 taps x BM out-channels x 16 channels from the packed plane into LDS rows of 32 bytes;
//   3. runs the taps back to back: A fragments at compile-time LDS offsets, B fragments at per-lane addresses (entry of the
//      lane's pixel + T) computed once per workgroup.
// The global loads of chunk i + 1 are issued right before the tap loop of chunk i and consumed after it.
constexpr int kTapGroup = 9;                     // taps whose weights are resident at a time

template <bool F16, int BM, int BN, int WM, int WN, int TN, int PMAX, bool MANY_TAPS>
__global__ __launch_bounds__(256) void conv_patch(HArgs a, int Hp, int Wp, int PLr) {
  constexpr int TM = 2;
  static_assert(WM * WN == 4 && WM * TM * 32 == BM && WN * TN * 32 == BN, "tile shape");
  constexpr int kItems = (PMAX * 2 + 255) / 256;         // (entry, octet) items per thread, at most
  constexpr int WPARTS = 256 / BM;                       // threads per weight row
  constexpr int WTAPS = (kTapGroup + WPARTS - 1) / WPARTS;   // taps per thread and group
  __shared__ __attribute__((aligned(16))) unsigned char sP[PMAX * kPRow];
  __shared__ __attribute__((aligned(16))) unsigned char sW[kTapGroup * BM * kPRow];
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

  // 32-bit index math throughout: the host takes this kernel only when N*Hp*Wp and N*C*H*W fit (see plan_of)
  auto base_of = [&](int p) {
    const int n = p / HoWo;
    const int r = p - n * HoWo;
    const int ho = r / a.Wo;
    return (n * Hp + ho * a.sh) * Wp + (r - ho * a.Wo) * a.sw;
  };
  const int p0 = blockIdx.x * BN;
  const int bmin = base_of(p0);
  const unsigned short* xg = a.x + (long long)grp * a.cg * HW;

  // ---- per-lane fragment addresses (fixed for the whole kernel)
  int e_pix[TN];                                         // patch entry of this lane's pixel, per column tile
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int pix = p0 + (wn * TN + j) * 32 + col;
    e_pix[j] = pix < total ? base_of(pix) - bmin : 0;
  }
  int b_addr[kTapGroup][TN];                             // byte address of the B fragment, first tap group
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
  unsigned raw[kItems][8];
  auto issue_xloads = [&](int cc) {
    // address = wave-uniform channel base + the lane's 32-bit byte offset, which never changes.  Halo / padded channels read
    // a valid dummy address and are zeroed at the clamp.
#pragma unroll
    for (int u = 0; u < kItems; ++u) {
      if (u < n_items) {
        const int c0 = __builtin_amdgcn_readfirstlane(cc * kPC + (it_dst[u] >> 30) * 8);
        const unsigned boff = it_off[u] < 0 ? 0u : (unsigned)it_off[u] * 2u;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const char* cbase = reinterpret_cast<const char*>(xg + (long long)min(c0 + j, a.cg - 1) * HW);
          raw[u][j] = *reinterpret_cast<const unsigned short*>(cbase + boff);
        }
      }
    }
  };
  auto clamp_store = [&](int cc) {
#pragma unroll
    for (int u = 0; u < kItems; ++u) {
      if (u < n_items) {
        const int c0 = cc * kPC + (it_dst[u] >> 30) * 8;
        unsigned d[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const unsigned lo = (it_off[u] >= 0 && (!ragged || c0 + 2 * q < a.cg)) ? raw[u][2 * q] : 0u;
          const unsigned hi16 = (it_off[u] >= 0 && (!ragged || c0 + 2 * q + 1 < a.cg)) ? raw[u][2 * q + 1] : 0u;
          d[q] = clamp2<F16>(lo | hi16 << 16, a);
        }
        *reinterpret_cast<uint4*>(sP + (it_dst[u] & 0xFFFFF)) = make_uint4(d[0], d[1], d[2], d[3]);
      }
    }
  };

  // ---- weight staging roles: thread -> out-channel row (tid % BM), taps part + WPARTS * k of the group
  const int so = tid % BM, part = tid / BM;
  const bool so_valid = t * BM + so < a.og_pad;
  const unsigned* wcol = reinterpret_cast<const unsigned*>(a.wbits + o_pad0 + (so_valid ? so : 0));
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
        // 16 sign bits (set = +1) -> 16 values +-1.  The inverted bits replicated into both 16-bit halves, one packed 16-bit
        // shift moves bit 2q / 2q+1 to the sign position of the low / high half, one and-or merges it into 1.0.
        const unsigned m = so_valid ? ~(src[k] >> sh) & 0xFFFFu : 0xFFFFu;     // rows past the group: never stored
        const u16x2 rep = __builtin_bit_cast(u16x2, m | (m << 16));
        unsigned d[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const u16x2 shq = {(unsigned short)(15 - 2 * q), (unsigned short)(14 - 2 * q)};
          d[q] = (__builtin_bit_cast(unsigned, rep << shq) & 0x80008000u) | kOne2<F16>;
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
    Frag af[TM], bf[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) af[i] = lds_frag(sW + tt * (BM * kPRow) + a_addr[i]);
#pragma unroll
    for (int j = 0; j < TN; ++j) bf[j] = lds_frag(sP + baddr[j]);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = mfma16<F16>(af[i], bf[j], acc[i][j]);
  };

  issue_xloads(0);
  issue_wloads(wraw, 0, 0);
  for (int cc = 0; cc < cchunks; ++cc) {
    clamp_store(cc);
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
  store_tiles_half<BM, BN, TM, TN>(a, acc, blockIdx.x, t, o0, wm, wn, col, kh8);
}

// ---- host side
struct Plan {
  int kind;                            // LSQ_CONV_HALF_* bits
  int Ho, Wo, Hp, Wp, PLr, pbn;
};

bool half_type(int t) { return t == LSQ_DTYPE_BF16 || t == LSQ_DTYPE_F16; }

// 0 and *p filled, or a negative LSQ_E_* code.  The patch rule is lsq_signw_conv2d's (same tiles, same PMAX 512 / 640), so
// that both libraries take a patch kernel for the same geometries.
int plan_of(const lsq_conv_geom* g, Plan* p) {
  if (int e = check_geom(g)) return e;
  const long long Hp = (long long)g->H + 2ll * g->pad_h, Wp = (long long)g->W + 2ll * g->pad_w;
  const long long Ho64 = (Hp - (long long)g->dil_h * (g->KH - 1) - 1) / g->stride_h + 1;
  const long long Wo64 = (Wp - (long long)g->dil_w * (g->KW - 1) - 1) / g->stride_w + 1;
  if (Hp - (long long)g->dil_h * (g->KH - 1) - 1 < 0 || Wp - (long long)g->dil_w * (g->KW - 1) - 1 < 0) return LSQ_E_SHAPE;
  const long long lim = 1ll << 31;
  if (Hp >= lim || Wp >= lim || Ho64 >= lim || Wo64 >= lim) return LSQ_E_UNSUPPORTED;
  // (products of at most three factors below 2^31 each: checked step by step)
  auto prod_fits = [&](long long a, long long b, long long c, long long d) {
    long long v = a;
    for (long long f : {b, c, d}) {
      if (v >= lim) return false;
      v *= f;
    }
    return v < lim;
  };
  const int cg = g->C / g->groups, og = g->O / g->groups;
  const long long Gg = (cg + 63) / 64, og_pad = (og + 15) / 16 * 16;
  if (!prod_fits(g->N, g->C, g->H, g->W) || !prod_fits(g->N, g->O, Ho64, Wo64) || !prod_fits(g->N, Hp, Wp, 1)) return LSQ_E_UNSUPPORTED;
  if (!prod_fits(g->KH, g->KW, Gg, (long long)g->groups * og_pad) ||
      (long long)g->KH * g->KW * Gg * g->groups * og_pad >= (1ll << 28))
    return LSQ_E_UNSUPPORTED;
  const bool wide = og > 64;
  const int bm = wide ? 128 : 64;
  if ((long long)g->groups * ((og + bm - 1) / bm) > 65535) return LSQ_E_UNSUPPORTED;
  const int Ho = (int)Ho64, Wo = (int)Wo64;
  const bool unit = g->stride_h == 1 && g->stride_w == 1;
  const int pbn = unit ? (wide ? 128 : 256) : (wide ? 64 : 128);
  const int pmax = unit ? 512 : 640;
  const long long row_gap = (long long)g->stride_h * Wp - (long long)Wo * g->stride_w;
  const long long img_gap = (Hp - (long long)Ho * g->stride_h) * Wp;
  const long long patch = (long long)(pbn - 1) * g->stride_w + ((pbn - 1) / Wo + 1) * (row_gap > 0 ? row_gap : 0) +
                          ((pbn - 1) / ((long long)Ho * Wo) + 1) * (img_gap > 0 ? img_gap : 0) +
                          (long long)(g->KH - 1) * g->dil_h * Wp + (long long)(g->KW - 1) * g->dil_w + 1;
  const long long PLr = (patch + 127) / 128 * 128;
  const bool use_patch = PLr <= pmax && (long long)g->N * g->C * g->H * g->W < (1ll << 30) &&
                         (long long)g->N * Hp * Wp + PLr < (1ll << 31) && (long long)g->N * g->O * Ho * Wo < (1ll << 30);
  p->kind = wide ? LSQ_CONV_HALF_WIDE : 0;
  if (use_patch)
    p->kind |= LSQ_CONV_HALF_PATCH | (unit ? LSQ_CONV_HALF_UNIT_STRIDE : 0) | (g->KH * g->KW > kTapGroup ? LSQ_CONV_HALF_MANY_TAPS : 0);
  p->Ho = Ho; p->Wo = Wo; p->Hp = (int)Hp; p->Wp = (int)Wp; p->PLr = use_patch ? (int)PLr : 0; p->pbn = pbn;
  return LSQ_OK;
}

template <bool F16>
int launch(const HArgs& a, const Plan& p, hipStream_t st) {
  const long long total = (long long)a.N * p.Ho * p.Wo;
  const unsigned otiles = (unsigned)(a.opad_total / a.og_pad * a.tiles_per_group);
  const bool wide = p.kind & LSQ_CONV_HALF_WIDE;
  if (p.kind & LSQ_CONV_HALF_PATCH) {
    dim3 grid((unsigned)((total + p.pbn - 1) / p.pbn), otiles);
    const bool many = p.kind & LSQ_CONV_HALF_MANY_TAPS, unit = p.kind & LSQ_CONV_HALF_UNIT_STRIDE;
#define LSQ_PATCH(BM_, BN_, WM_, WN_, TN_, PM_)                                                                                \
  do {                                                                                                                         \
    if (many) hipLaunchKernelGGL((conv_patch<F16, BM_, BN_, WM_, WN_, TN_, PM_, true>), grid, dim3(256), 0, st, a, p.Hp, p.Wp, p.PLr); \
    else hipLaunchKernelGGL((conv_patch<F16, BM_, BN_, WM_, WN_, TN_, PM_, false>), grid, dim3(256), 0, st, a, p.Hp, p.Wp, p.PLr);     \
  } while (0)
    if (unit && wide) LSQ_PATCH(128, 128, 2, 2, 2, 512);
    else if (unit) LSQ_PATCH(64, 256, 1, 4, 2, 512);
    else if (wide) LSQ_PATCH(128, 64, 2, 2, 1, 640);
    else LSQ_PATCH(64, 128, 1, 4, 1, 640);
#undef LSQ_PATCH
  } else {
    dim3 grid((unsigned)((total + kBN - 1) / kBN), otiles);
    if (wide) hipLaunchKernelGGL((conv_tiled<F16, 128, 2, 2, 2, 2>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((conv_tiled<F16, 64, 1, 4, 2, 1>), grid, dim3(256), 0, st, a);
  }
  return (int)hipGetLastError();
}

}  // namespace
}  // namespace signw
}  // namespace lsq

using namespace lsq;
using namespace lsq::signw;

extern "C" int lsq_conv_half_abi_version(void) { return LSQ_CONV_HALF_ABI_VERSION; }

extern "C" int lsq_signw_conv2d_half_plan(const lsq_conv_geom* g) {
  Plan p;
  if (int e = plan_of(g, &p)) return e;
  return p.kind;
}

// A launch holds one plane: the fp32 running sum of a 16-bit y of more than one plane lives in the workspace.
extern "C" int64_t lsq_signw_conv2d_half_workspace_bytes(const lsq_conv_geom* g, int kw_planes, int y_dtype) {
  Plan p;
  if (!half_type(y_dtype) || kw_planes <= 1 || plan_of(g, &p)) return 0;
  return 4ll * g->N * g->O * p.Ho * p.Wo;
}

extern "C" int lsq_signw_conv2d_half(const void* x, int x_dtype, float clamp_alpha, const uint64_t* wbits, int kw_planes,
                                     const float* wscales, const float* bias, const lsq_conv_geom* g, void* y, int y_dtype,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !wbits || !wscales || !y) return LSQ_E_NULL;
  if (int e = check_geom(g)) return e;
  if (!half_type(x_dtype) || (y_dtype != LSQ_DTYPE_F32 && y_dtype != x_dtype)) return LSQ_E_UNSUPPORTED;
  if (kw_planes < 1 || kw_planes > LSQ_MAX_PLANES) return LSQ_E_UNSUPPORTED;
  Plan p;
  if (int e = plan_of(g, &p)) return e;
  const size_t need = (size_t)lsq_signw_conv2d_half_workspace_bytes(g, kw_planes, y_dtype);
  if (need && (!workspace || ((uintptr_t)workspace & 3) || workspace_bytes < need)) return LSQ_E_WORKSPACE;
  const bool f16 = x_dtype == LSQ_DTYPE_F16;
  HArgs a = {};
  a.x = static_cast<const unsigned short*>(x);
  a.bias = bias;
  // the bound is used as given: the caller has rounded it into the activations' type (a NaN or negative one: identity)
  a.lim = clamp_alpha >= 0.f ? clamp_alpha : INFINITY;
  a.clamp = !isinf(a.lim);
  {
    const _Float16 h = (_Float16)a.lim;
    uint16_t hb;
    memcpy(&hb, &h, 2);
    a.lim2 = (uint32_t)hb << 16 | hb;
  }
  a.N = g->N; a.C = g->C; a.H = g->H; a.W = g->W; a.O = g->O; a.KH = g->KH; a.KW = g->KW;
  a.sh = g->stride_h; a.sw = g->stride_w; a.ph = g->pad_h; a.pw = g->pad_w; a.dh = g->dil_h; a.dw = g->dil_w;
  a.cg = g->C / g->groups;
  a.Gg = (a.cg + 63) / 64;
  a.Ho = p.Ho; a.Wo = p.Wo;
  a.og = g->O / g->groups;
  a.og_pad = (a.og + 15) / 16 * 16;
  a.opad_total = g->groups * a.og_pad;
  const int bm = (p.kind & LSQ_CONV_HALF_WIDE) ? 128 : 64;
  a.tiles_per_group = (a.og + bm - 1) / bm;
  const long long wplane_words = (long long)g->KH * g->KW * a.Gg * a.opad_total;
  float* const sum = need ? static_cast<float*>(workspace) : static_cast<float*>(y);   // the fp32 sum between launches
  hipStream_t st = (hipStream_t)stream;
  for (int q = 0; q < kw_planes; ++q) {
    const bool last = q == kw_planes - 1;
    a.wbits = (const unsigned long long*)wbits + (long long)q * wplane_words;
    a.wscale = wscales + (long long)q * g->O;
    a.prev = q ? sum : nullptr;
    a.out = last ? y : sum;
    a.odt = last ? y_dtype : LSQ_DTYPE_F32;
    if (int e = f16 ? launch<true>(a, p, st) : launch<false>(a, p, st)) return e;
  }
  return LSQ_OK;
}
