// liblsq_hip_conv_xnor_narrow.so: lsq_xnor_conv2d_narrow, the fp4 matrix-core XNOR convolution for ANY channel count -- input
// channels that are no multiple of 64, out-channels that are no multiple of 32 (LeNet's 20 -> 50 conv2, ResNets of width 16,
// 48, 80, 96, ...) -- with an optional 2 x 2 / stride-2 max-pool behind the activation.  Same operands and layouts as
// lsq_xnor_conv2d and -- the integers being exact, the fp32 arithmetic in that kernel's order -- the same result, bit for bit.
//
// The arithmetic is that of csrc/conv_xnor_gen/lsq_conv_xnor_gen.hip (see there for the why): v_mfma_scale_f32_32x32x64_f8f6f4
// on fp4 operands, a set activation bit = E2M1 0.5 / 1 / 2 (a clear bit -- a negative value, the zero halo or a padded channel
// -- is 0), the weight nibble +-(4, 2, 1, 4), an accumulator that starts at minus the inside-rectangle sum of wsum, read from
// a 2-D prefix table in LDS; a tile of 32 output pixels per wave, 8 waves per workgroup on 32 MT out-channels.
//
// What is this kernel's own:
//   * a FLAT K LOOP OVER 32-CHANNEL DWORDS.  D = ceil(C / 32) dwords per tap, units u = tap * D + j.  MFMA step s covers units
//     2 s and 2 s + 1: lane half hh = lane >> 5 supplies unit 2 s + hh, which is half j & 1 of channel word j >> 1 of its tap.
//     For even D that is the gen kernel's step; for odd D steps straddle taps and no K slot is spent on the all-zero upper
//     dword of the last word (13 steps instead of 25 for 20 channels 5 x 5).  Each half advances its own (tap, j) by two units
//     per step; a unit past the end (taps * D odd) is a zero activation dword.
//   * the WEIGHTS ARE RESIDENT: all steps * MT fragments (1 KB each) of the workgroup's out-channels are expanded once per
//     weight plane into LDS, and the waves then run the whole K loop with no barrier and no ring; activation dwords are
//     requested a chunk of steps ahead.  Out-channel slots at or past O read the zero words lsq_pack_weight leaves up to
//     ceil16(O) (guarded beyond), get zero scale, bias and wsum, and store nothing.
//   * EVERY PLANE PASS IN ONE LAUNCH (as csrc/conv_xnor_gen_half): weight planes outside -- fragments, prefix table and scales
//     re-staged per plane --, pairs of activation planes inside, the fp32 running value in registers in the order
//     lsq_xnor_conv2d forms it in y.  One store, no workspace, no read-modify-write of y.
//   * POOL 2 IN REGISTERS: the 32 pixels of a tile are 8 windows of 2 x 2, four consecutive lanes one window (flat over
//     (n, Ho / 2, Wo / 2), (dy, dx) from the low two bits).  Behind the activation the maximum over the quad is two quad-permute
//     DPP moves and one lane of four stores; pixels of a dropped odd row or column are never computed.

#include <atomic>

#include "../lsq_common.h"
#include "lsq_hip_conv_xnor_narrow.h"

namespace lsq {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int kWaves = 8;                        // pixel tiles (of 32) per workgroup
constexpr int kThreads = 64 * kWaves;
constexpr int kAheadMfma = 8;                    // K steps x activation planes requested ahead
constexpr int kMaxTaps = 64, kMaxK = 8;
constexpr int kMaxUnits = 128;                   // taps * D: at most 64 steps, 64 KB of fragments with MT = 1
constexpr int kPlainLds = 64 * 1024;             // dynamic LDS above this needs the function attribute
constexpr int kMaxLds = 96 * 1024;

struct NarrowArgs {
  const unsigned* xd;                  // every activation plane as dwords: [kx][N][Gg][Hp][Wp][2]
  const float* xscales;                // [kx][N]
  const unsigned* wd;                  // every weight plane as dwords: [kw_planes][taps][Gg][Opad][2]
  const int* wsum;                     // [kw_planes][O][taps]
  const float* wscales;                // [kw_planes][O]
  const float* bias;                   // [O] or null
  const float* slope;                  // PReLU slope(s)
  const float* res_pre;                // [N][O][Ho][Wo] or null
  const float* res_post;
  float* y;                            // [N][O][Ho][Wo], or [N][O][Ho / 2][Wo / 2] with pool 2
  unsigned plane_dwords;               // dwords of one activation plane
  unsigned word_dwords;                // 2 Hp Wp: dwords between two channel words of a sample
  unsigned wplane_dwords;              // dwords of one weight plane
  int N, H, W, O, Opad, KH, KW, sh, sw, ph, pw, dh, dw, Gg, Hp, Wp, Ho, Wo;
  int Hy, Wy;                          // the extent of y: (Ho, Wo) / pool
  int D, units, steps;                 // ceil(C / 32), taps D, ceil(units / 2)
  int kx, kw_planes, act, pool;
  int tap_xoff[kMaxTaps];              // dwords: 2 ((kh dil_h) Wp + kw dil_w)
};

// max over the 2 x 2 window held by four consecutive lanes (every lane of the quad gets it)
__device__ __forceinline__ float quad_max(float v) {
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false)));      // quad_perm:[1,0,3,2]
  return fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false)));   // quad_perm:[2,3,0,1]
}

// KX: activation planes of a full pass (2 where the call has at least two, else 1); MULTI: more than one pass
template <int KX, int MT, bool MULTI>
__global__ __launch_bounds__(kThreads, 4) void xnor_narrow_kernel(NarrowArgs a) {
  constexpr int OC = 32 * MT;                    // out-channels of the workgroup
  // dynamic LDS: [steps MT][64] fragments | prefix table [(KH + 1)(KW + 1)][OC] | scale, bias, slope [OC] | tap offsets
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int W1 = a.KW + 1, taps = a.KH * a.KW;
  v4i* const s_w = reinterpret_cast<v4i*>(smem);
  int* const s_pre = reinterpret_cast<int*>(s_w + a.steps * MT * 64);      // [a (KW + 1) + b][o]: sum over kh < a, kw < b
  float* const s_scale = reinterpret_cast<float*>(s_pre + (a.KH + 1) * W1 * OC);
  float* const s_bias = s_scale + OC;
  float* const s_slope = s_bias + OC;
  int* const s_tap = reinterpret_cast<int*>(s_slope + OC);                 // [kMaxTaps]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int col = lane & 31, hh = lane >> 5;
  const int o0 = blockIdx.y * OC;
  const int ob = 4 * hh;                         // the lane's out-channel of register i of tile mt: 32 mt + ob + (i & 3) + 8 (i >> 2)

  // ---- the lane's pixel.  No pool: the tile is 32 consecutive outputs, flat over (n, ho, wo).  Pool 2: 8 consecutive windows,
  // flat over (n, ho / 2, wo / 2), four lanes each.  Lanes past the last one compute pixel 0 and store nothing.
  const bool pooled = a.pool == 2;
  const int HyWy = a.Hy * a.Wy;
  const unsigned total = (unsigned)(a.N * HyWy);                 // outputs per channel of y
  const unsigned pix = ((unsigned)blockIdx.x * kWaves + (unsigned)wid) * 32u + (unsigned)col;
  const unsigned cell = pooled ? pix >> 2 : pix;                 // the lane's element of y
  const bool valid = cell < total;
  const unsigned cc = valid ? cell : 0u;
  const int n = (int)(cc / (unsigned)HyWy);
  const int r = (int)(cc - (unsigned)n * (unsigned)HyWy);        // offset of the lane's element inside its channel of y
  const int hy = (int)((unsigned)r / (unsigned)a.Wy), wy = r - hy * a.Wy;
  const int ho = pooled ? 2 * hy + ((col >> 1) & 1) : hy, wo = pooled ? 2 * wy + (col & 1) : wy;
  const unsigned xpix = 2u * (unsigned)((n * a.Gg * a.Hp + ho * a.sh) * a.Wp + wo * a.sw);
  const int hi0 = ho * a.sh - a.ph, wi0 = wo * a.sw - a.pw;      // the input row / column of tap (0, 0)

  if (tid < kMaxTaps) s_tap[tid] = tid < taps ? a.tap_xoff[tid] : 0;
  __syncthreads();

  // ---- per weight plane q: every fragment of the workgroup's out-channels, the scales and the prefix sums of wsum (bias and
  // slope with plane 0).  The last phase is left open: the caller's barrier closes it.
  auto stage = [&](int q) {
    if (q > 0) __syncthreads();                  // the passes of plane q - 1 have read the fragments, s_pre and s_scale
    int t = tid;
    asm volatile("" : "+v"(t));                  // (opaque: keeps this index arithmetic out of the registers of the K loops)
    // entry (fragment f = s MT + tile, lane L of the wave that will read it): L supplies out-channel L & 31 of the tile and
    // unit 2 s + (L >> 5), the K half its activation lanes supply
    const unsigned* __restrict__ wd = a.wd + (size_t)q * a.wplane_dwords;
    for (int idx = t; idx < a.steps * MT * 64; idx += kThreads) {
      const int L = idx & 63, f = idx >> 6;
      const int s = f / MT, mt = f - s * MT;
      const int u = 2 * s + (L >> 5), o = o0 + 32 * mt + (L & 31);
      unsigned d = 0u;
      if (u < a.units && o < a.Opad) {           // (slots in [O, Opad) hold zero words; past Opad there is no word)
        const int tap = u / a.D, j = u - tap * a.D;
        d = wd[2u * (unsigned)((tap * a.Gg + (j >> 1)) * a.Opad + o) + (unsigned)(j & 1)];
      }
      // nibble e of register g = channel g + 4 e: +-(4, 2, 1, 4) as E2M1 codes 6 / 4 / 2 / 6, sign bit 8 where the weight is -1
      v4i out;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const unsigned mag = (g == 1 ? 0x4u : (g == 2 ? 0x2u : 0x6u)) * 0x11111111u;
        const unsigned ones = (d >> g) & 0x11111111u;
        out[g] = (int)(mag | ((ones ^ 0x11111111u) << 3));
      }
      s_w[idx] = out;
    }
    if (t < OC) {
      const bool real = o0 + t < a.O;
      s_scale[t] = real ? a.wscales[(long long)q * a.O + o0 + t] : 0.f;
      if (q == 0) {
        s_bias[t] = real && a.bias ? a.bias[o0 + t] : 0.f;
        s_slope[t] = real && a.act >= LSQ_ACT_PRELU ? a.slope[a.act == LSQ_ACT_PRELU ? 0 : o0 + t] : 0.f;
      }
    }
    const int* __restrict__ ws = a.wsum + ((long long)q * a.O + o0) * taps;
    const int oreal = min(OC, a.O - o0);         // out-channels of the tile that exist
    for (int i = t; i < (a.KH + 1) * W1 * OC; i += kThreads) s_pre[i] = 0;
    __syncthreads();
    for (int i = t; i < oreal * taps; i += kThreads) {          // (consecutive threads, consecutive addresses: wsum is [O][taps])
      const int o = i / taps, tp = i - o * taps;
      const int kh = tp / a.KW, kw = tp - kh * a.KW;
      s_pre[((kh + 1) * W1 + kw + 1) * OC + o] = ws[i];
    }
    __syncthreads();
    for (int i = t; i < a.KH * OC; i += kThreads) {             // along kw
      const int o = i % OC, row = (i / OC + 1) * W1;
      int sum = 0;
      for (int b = 1; b <= a.KW; ++b) {
        sum += s_pre[(row + b) * OC + o];
        s_pre[(row + b) * OC + o] = sum;
      }
    }
    __syncthreads();
    for (int i = t; i < a.KW * OC; i += kThreads) {             // along kh
      const int o = i % OC, b = i / OC + 1;
      int sum = 0;
      for (int k = 1; k <= a.KH; ++k) {
        sum += s_pre[(k * W1 + b) * OC + o];
        s_pre[(k * W1 + b) * OC + o] = sum;
      }
    }
  };

  // ---- epilogue, once: residuals, activation, the pool's quad maximum, one store per output.
  // value(mt, i): the fp32 value of output register i of tile mt behind the last fold.  Every lane runs it (the quad moves
  // want whole quads); a lane stores where its element and its channel exist and, pooled, where it is the first of its quad.
  auto epilogue = [&](auto value) {
    const bool want_pre = a.res_pre != nullptr, want_post = a.res_post != nullptr;
    const bool relu = a.act == LSQ_ACT_RELU, prelu = a.act >= LSQ_ACT_PRELU;
    const bool writer = valid && (!pooled || (col & 3) == 0);
    // 32-bit element offsets (the entry point admits outputs below 2^30 elements)
    const unsigned yoff = (unsigned)((n * a.O + o0 + ob) * HyWy + r);
    const int olim = a.O - o0 - ob;              // channel ch of the lane exists where ch < olim
    // (eight outputs at a time: their loads go out together, and the operand arrays stay small beside the accumulators)
#pragma unroll
    for (int h = 0; h < 2 * MT; ++h) {
      const int mt = h >> 1, i0 = 8 * (h & 1);
      float pre[8], post[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int i = i0 + k, ch = 32 * mt + (i & 3) + 8 * (i >> 2);
        const unsigned at = yoff + (unsigned)(ch * HyWy);
        const bool here = writer && ch < olim;
        pre[k] = want_pre && here ? a.res_pre[at] : 0.f;       // (residuals come with pool 1 only)
        post[k] = want_post && here ? a.res_post[at] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int i = i0 + k, ch = 32 * mt + (i & 3) + 8 * (i >> 2);
        float out = value(mt, i);
        if (want_pre) out += pre[k];
        if (relu) out = fmaxf(out, 0.f);
        if (prelu) {
          const float neg = s_slope[ob + ch] * out;
          out = out > 0.f ? out : neg;
        }
        if (want_post) out += post[k];
        if (pooled) out = quad_max(out);
        if (writer && ch < olim) a.y[yoff + (unsigned)(ch * HyWy)] = out;
      }
    }
  };

  // several passes: the running value of the lane's 16 MT outputs, bias + the passes so far
  float run[MT][16];
  if constexpr (MULTI) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int o = o0 + ob + 32 * mt + (i & 3) + 8 * (i >> 2);
        run[mt][i] = a.bias && o < a.O ? a.bias[o] : 0.f;
      }
  }

  // ---- one pass: weight plane q against activation planes p0 .. p0 + P - 1
  auto pass = [&](auto planes_of_pass, int q, int p0) {
    constexpr int P = decltype(planes_of_pass)::value;
    constexpr int kChunk = kAheadMfma / P;       // K steps requested together
    const unsigned* __restrict__ xd = a.xd + (size_t)p0 * a.plane_dwords;

    // the (tap, dword) of the lane half's next unit: unit hh first, two units further per step -- an add and up to two carries
    int ld_tap = hh >= a.D ? 1 : 0, ld_j = hh - ld_tap * a.D, ld_u = hh;
    auto request = [&](int s0, unsigned (&x)[kChunk * P]) {
#pragma unroll
      for (int k = 0; k < kChunk; ++k) {
#pragma unroll
        for (int p = 0; p < P; ++p) x[k * P + p] = 0u;
        if (s0 + k < a.steps) {                  // (uniform)
          if (ld_u < a.units) {                  // (false for the upper half of the last step where taps D is odd)
            const unsigned at = xpix + (unsigned)s_tap[ld_tap] + (unsigned)(ld_j >> 1) * a.word_dwords + (unsigned)(ld_j & 1);
#pragma unroll
            for (int p = 0; p < P; ++p) x[k * P + p] = xd[at + (unsigned)p * a.plane_dwords];
          }
          ld_u += 2;
          ld_j += 2;
          if (ld_j >= a.D) { ld_j -= a.D; ++ld_tap; }
          if (ld_j >= a.D) { ld_j -= a.D; ++ld_tap; }
        }
      }
    };

    // ---- the first steps' activations go out before the plane is staged: their latency hides behind it
    unsigned xc[kChunk * P], xn[kChunk * P];
    request(0, xc);
    float xs[P];                                 // (several passes: requested here, a K loop ahead of the fold)
    if constexpr (MULTI) {
#pragma unroll
      for (int p = 0; p < P; ++p) xs[p] = a.xscales[(p0 + p) * a.N + n];
    }
    if (p0 == 0) {                               // (uniform)
      stage(q);
      __syncthreads();
    }

    // ---- the accumulators start at the border term: minus the rectangle sum of plane q's wsum over the taps inside the image.
    // hi and wi grow with the tap index, so the bounds of the rectangle are counts of taps below 0 and below the image's extent.
    v16f acc[P][MT];
    {
      int kh_lo = 0, kh_hi = 0, kw_lo = 0, kw_hi = 0;
      int h0 = hi0, w0 = wi0;
      asm volatile("" : "+v"(h0), "+v"(w0));     // (opaque: two registers across the passes, not four bounds and four addresses)
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) {
        const int hi = h0 + k * a.dh, wi = w0 + k * a.dw;
        kh_lo += (k < a.KH && hi < 0) ? 1 : 0;
        kh_hi += (k < a.KH && hi < a.H) ? 1 : 0;
        kw_lo += (k < a.KW && wi < 0) ? 1 : 0;
        kw_hi += (k < a.KW && wi < a.W) ? 1 : 0;
      }
      const int* __restrict__ p11 = s_pre + (kh_hi * W1 + kw_hi) * OC + ob;
      const int* __restrict__ p01 = s_pre + (kh_lo * W1 + kw_hi) * OC + ob;
      const int* __restrict__ p10 = s_pre + (kh_hi * W1 + kw_lo) * OC + ob;
      const int* __restrict__ p00 = s_pre + (kh_lo * W1 + kw_lo) * OC + ob;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int at = 32 * mt + 8 * g;
          const v4i inside = *reinterpret_cast<const v4i*>(p11 + at) - *reinterpret_cast<const v4i*>(p01 + at) -
                             *reinterpret_cast<const v4i*>(p10 + at) + *reinterpret_cast<const v4i*>(p00 + at);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int p = 0; p < P; ++p) acc[p][mt][4 * g + e] = (float)(-inside[e]);
          }
        }
    }

    // ---- the K loop: no barrier, the fragments stay where they are.  Per chunk: the next chunk's activation dwords first,
    // then this chunk's fragment reads, v_and and MFMAs.
    const int unit_scale = 0x7F7F7F7F;           // E8M0 127 = 2^0 in every byte: the block scales of both operands
    const int nchunks = (a.steps + kChunk - 1) / kChunk;
    for (int c = 0; c < nchunks; ++c) {
      const int s0 = c * kChunk;
      const bool more = c + 1 < nchunks;         // (uniform)
      if (more) request(s0 + kChunk, xn);
      __builtin_amdgcn_sched_barrier(0);
      const v4i* __restrict__ wb = s_w + s0 * MT * 64 + lane;
#pragma unroll
      for (int k = 0; k < kChunk; ++k) {
        if (s0 + k < a.steps) {                  // (uniform: the last chunk may be partial)
          v8i b8[P];
#pragma unroll
          for (int p = 0; p < P; ++p) {
            const unsigned d = xc[k * P + p];
            b8[p] = v8i{(int)(d & 0x11111111u), (int)(d & 0x22222222u), (int)(d & 0x44444444u), (int)((d >> 3) & 0x11111111u), 0, 0, 0, 0};
          }
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const v4i w4 = wb[(k * MT + mt) * 64];
            const v8i w8 = {w4[0], w4[1], w4[2], w4[3], 0, 0, 0, 0};      // (fp4 operands: the low four registers are read)
#pragma unroll
            for (int p = 0; p < P; ++p)
              acc[p][mt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(w8, b8[p], acc[p][mt], 4, 4, 0, unit_scale, 0, unit_scale);
          }
          // (an empty asm on the accumulators ties each step to its place: the scaled MFMA is a pure value to the selector)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int p = 0; p < P; ++p) asm volatile("" : "+v"(acc[p][mt]));
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (more) {
#pragma unroll
        for (int i = 0; i < kChunk * P; ++i) xc[i] = xn[i];
      }
    }

    // ---- the fold: the popcount kernel's arithmetic on the same integers -> the same floats
    auto fold = [&](int mt, int i, float base) {
      float v = xs[0] * acc[0][mt][i];
#pragma unroll
      for (int p = 1; p < P; ++p) v = fmaf(xs[p], acc[p][mt][i], v);
      return fmaf(v, s_scale[ob + 32 * mt + (i & 3) + 8 * (i >> 2)], base);
    };
    if constexpr (MULTI) {
      // (eight at a time: the scales of all 16 MT at once would stand beside the accumulators and the running values)
#pragma unroll
      for (int h = 0; h < 2 * MT; ++h) {
#pragma unroll
        for (int k = 0; k < 8; ++k) run[h >> 1][8 * (h & 1) + k] = fold(h >> 1, 8 * (h & 1) + k, run[h >> 1][8 * (h & 1) + k]);
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      // one pass: no running value, the accumulators go through the fold into the epilogue eight at a time
#pragma unroll
      for (int p = 0; p < P; ++p) xs[p] = a.xscales[p * a.N + n];
      epilogue([&](int mt, int i) { return fold(mt, i, s_bias[ob + 32 * mt + (i & 3) + 8 * (i >> 2)]); });
    }
  };

  if constexpr (MULTI) {
    for (int q = 0; q < a.kw_planes; ++q) {
      for (int p0 = 0; p0 < a.kx; p0 += 2) {
        if (KX == 2 && a.kx - p0 >= 2) pass(std::integral_constant<int, KX>{}, q, p0);
        else pass(std::integral_constant<int, 1>{}, q, p0);      // a lone last plane (or a call with one)
      }
    }
    epilogue([&](int mt, int i) { return run[mt][i]; });
  } else {
    pass(std::integral_constant<int, KX>{}, 0, 0);      // (its fold ends in the epilogue)
  }
}

// bytes of dynamic LDS of a launch with MT tiles of 32 out-channels per wave
long long lds_bytes(const NarrowArgs& a, int mt) {
  return 1024ll * a.steps * mt + 4ll * (a.KH + 1) * (a.KW + 1) * 32 * mt + 3 * 4ll * 32 * mt + 4ll * kMaxTaps;
}

// dynamic LDS above 64 KiB needs the function attribute: once per device and kernel
template <auto KERNEL>
hipError_t allow_lds() {
  static std::atomic<unsigned long long> allowed{0ull};
  int dev = 0;
  hipError_t rc = hipGetDevice(&dev);
  if (rc != hipSuccess) return rc;
  const unsigned long long bit = 1ull << (dev & 63);
  if (!(allowed.load(std::memory_order_acquire) & bit)) {
    rc = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
    if (rc != hipSuccess) return rc;
    allowed.fetch_or(bit, std::memory_order_release);
  }
  return hipSuccess;
}

template <int KX, int MT, bool MULTI>
int launch_one(const NarrowArgs& a, hipStream_t st) {
  const long long lds = lds_bytes(a, MT);
  if (lds > kPlainLds) {
    if (hipError_t rc = allow_lds<xnor_narrow_kernel<KX, MT, MULTI>>()) return (int)rc;
  }
  const long long lanes = (long long)a.N * a.Hy * a.Wy * (a.pool == 2 ? 4 : 1);
  const long long ntiles = (lanes + 31) >> 5;
  const unsigned gx = (unsigned)((ntiles + kWaves - 1) / kWaves), gy = (unsigned)((a.O + 32 * MT - 1) / (32 * MT));
  hipLaunchKernelGGL((xnor_narrow_kernel<KX, MT, MULTI>), dim3(gx, gy), dim3(kThreads), (size_t)lds, st, a);
  return (int)hipGetLastError();
}

int launch(const NarrowArgs& a, hipStream_t st) {
  const bool multi = a.kw_planes * ((a.kx + 1) / 2) > 1, two = a.kx >= 2;
  // a running value beside the accumulators of two tiles does not fit the 128 registers of four waves per SIMD
  if (multi) return two ? launch_one<2, 1, true>(a, st) : launch_one<1, 1, true>(a, st);
  // two tiles of 32 out-channels per wave where there are more than 32 and their fragments fit 64 KB
  const bool wide = a.O > 32 && 2 * a.steps <= 64;
  if (two) return wide ? launch_one<2, 2, false>(a, st) : launch_one<2, 1, false>(a, st);
  return wide ? launch_one<1, 2, false>(a, st) : launch_one<1, 1, false>(a, st);
}

// 0 where the kernel takes (g, kx, kw_planes, pool), else the code the entry point returns
int narrow_check(const lsq_conv_geom* g, int kx, int kw_planes, int pool) {
  if (int e = check_geom(g)) return e;
  if (kx < 1 || kx > LSQ_MAX_PLANES || kw_planes < 1 || kw_planes > LSQ_MAX_PLANES) return LSQ_E_SCHEME;
  const int Ho = out_h(g), Wo = out_w(g);
  if (Ho <= 0 || Wo <= 0) return LSQ_E_SHAPE;
  if (pool != 1 && pool != 2) return LSQ_E_UNSUPPORTED;
  if (pool == 2 && (Ho < 2 || Wo < 2)) return LSQ_E_SHAPE;                           // (an empty y)
  if (g->groups != 1) return LSQ_E_UNSUPPORTED;
  if (g->KH > kMaxK || g->KW > kMaxK || g->KH * g->KW > kMaxTaps) return LSQ_E_UNSUPPORTED;
  if ((long long)g->C * g->KH * g->KW >= (1ll << 23)) return LSQ_E_UNSUPPORTED;      // the fp32 accumulator holds the integer exactly
  if ((long long)g->KH * g->KW * ((g->C + 31ll) / 32) > kMaxUnits) return LSQ_E_UNSUPPORTED;      // the resident fragments
  if ((long long)g->N * g->O * Ho * Wo >= (1ll << 30)) return LSQ_E_UNSUPPORTED;     // 32-bit element offsets
  if ((g->O + 31) / 32 > 65535) return LSQ_E_UNSUPPORTED;                             // (grid.y)
  const long long Hp = g->H + 2ll * g->pad_h, Wp = g->W + 2ll * g->pad_w;
  if ((long long)g->N * ((g->C + 63) / 64) * Hp * Wp * kx >= (1ll << 30)) return LSQ_E_UNSUPPORTED;      // 32-bit dword offsets
  return LSQ_OK;
}

}  // namespace
}  // namespace lsq

using namespace lsq;

extern "C" int lsq_conv_xnor_narrow_abi_version(void) { return LSQ_CONV_XNOR_NARROW_ABI_VERSION; }

extern "C" int lsq_xnor_conv2d_narrow_supported(const lsq_conv_geom* g, int kx, int kw_planes, int pool) {
  return narrow_check(g, kx, kw_planes, pool) == LSQ_OK ? 1 : 0;
}

extern "C" int lsq_xnor_conv2d_narrow(const uint64_t* xplanes, int kx, const float* xscales, const uint64_t* wbits,
                                      const int32_t* wsum, int kw_planes, const float* wscales, const float* bias,
                                      const lsq_conv_geom* g, int act, const float* act_slope, const float* res_pre,
                                      const float* res_post, int pool, float* y, void* stream) {
  if (!xplanes || !xscales || !wbits || !wsum || !wscales || !y) return LSQ_E_NULL;
  if (int e = narrow_check(g, kx, kw_planes, pool)) return e;
  if (act < LSQ_ACT_NONE || act > LSQ_ACT_PRELU_CHANNEL || (act >= LSQ_ACT_PRELU && !act_slope)) return LSQ_E_SCHEME;
  if (pool == 2 && (res_pre || res_post)) return LSQ_E_UNSUPPORTED;
  NarrowArgs a = {};
  a.N = g->N; a.H = g->H; a.W = g->W; a.O = g->O; a.KH = g->KH; a.KW = g->KW;
  a.sh = g->stride_h; a.sw = g->stride_w; a.ph = g->pad_h; a.pw = g->pad_w; a.dh = g->dil_h; a.dw = g->dil_w;
  a.Gg = (g->C + 63) / 64;
  a.Opad = (g->O + 15) / 16 * 16;
  a.Hp = g->H + 2 * g->pad_h; a.Wp = g->W + 2 * g->pad_w;
  a.Ho = out_h(g); a.Wo = out_w(g);
  a.pool = pool;
  a.Hy = a.Ho / pool; a.Wy = a.Wo / pool;
  a.D = (g->C + 31) / 32;
  a.units = g->KH * g->KW * a.D;
  a.steps = (a.units + 1) / 2;
  const long long xplane_words = lsq_act_plane_words(g), wplane_words = lsq_weight_plane_words(g);
  // (the layouts this kernel indexes: [N][ceil(C / 64)][Hp][Wp] words per activation plane, [taps][ceil(C / 64)][ceil16(O)] per
  //  weight plane)
  if (xplane_words != (long long)a.N * a.Gg * a.Hp * a.Wp || wplane_words != (long long)g->KH * g->KW * a.Gg * a.Opad)
    return LSQ_E_UNSUPPORTED;
  if (2 * wplane_words >= (1ll << 31)) return LSQ_E_UNSUPPORTED;
  a.plane_dwords = (unsigned)(2 * xplane_words);
  a.word_dwords = 2u * (unsigned)(a.Hp * a.Wp);
  a.wplane_dwords = (unsigned)(2 * wplane_words);
  for (int kh = 0; kh < g->KH; ++kh)
    for (int kw = 0; kw < g->KW; ++kw) a.tap_xoff[kh * g->KW + kw] = 2 * (kh * g->dil_h * a.Wp + kw * g->dil_w);
  a.xd = reinterpret_cast<const unsigned*>(xplanes);
  a.xscales = xscales;
  a.wd = reinterpret_cast<const unsigned*>(wbits);
  a.wsum = wsum;
  a.wscales = wscales;
  a.bias = bias;
  a.slope = act_slope;
  a.act = act;
  a.res_pre = res_pre;
  a.res_post = res_post;
  a.y = y;
  a.kx = kx;
  a.kw_planes = kw_planes;
  return launch(a, (hipStream_t)stream);
}
