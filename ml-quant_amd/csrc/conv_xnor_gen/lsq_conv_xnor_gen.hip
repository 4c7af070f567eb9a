// liblsq_hip_conv_xnor_gen.so: lsq_xnor_conv2d_gen, the binary x binary convolution as an implicit GEMM on
// v_mfma_scale_f32_32x32x64_f8f6f4 (fp4 operands, exact) for the geometries the tuned 3x3 kernel of csrc/lsq_xnor_mfma.hip
// does not take: any kernel up to 8 x 8 (64 taps), any stride, dilation and padding, any multiple of 64 input channels.
// Same operands, same layouts and -- the integers being exact -- the same fp32 result, bit for bit, as lsq_xnor_conv2d.
//
// The fp4 encoding is the tuned kernel's: register q of a lane holds channels q + 4 j of its dword; a set
// activation bit becomes E2M1 code 1 / 2 / 4 = 0.5 / 1 / 2 with one v_and_b32 per eight channels (a clear bit -- a negative
// value or the zero halo -- is 0), the weight nibble of the same slot is +-(4, 2, 1, 4), every product is +-2 or 0, and an
// accumulator that starts at minus the tap sums of the taps inside the image ends as the integer (b * s).
//
// What is this kernel's own:
//   * a FLAT K LOOP over steps s = tap * Gg + word (the order of the weight plane [taps][Gg][O]), one MFMA per step,
//     activation plane and 32 out-channels; the step count is a kernel argument.  Steps go in chunks of 8 / KX.
//   * the WEIGHTS ARE STREAMED: a workgroup's waves share its out-channel tile (32 MT channels) and walk the K loop in
//     lockstep over kWaves different pixel tiles.  The packed sign words of chunk c + 1 are requested from global memory
//     before the MFMAs of chunk c, expanded to fp4 fragments by the thread that loaded them (once per workgroup, not once
//     per wave: four VALU instructions per register would otherwise outweigh the MFMAs they feed) and written into the
//     other half of a double-buffered LDS ring behind those MFMAs: one barrier per chunk, at most 8 MT KB per buffer whatever the
//     layer's size.
//   * MT = 2 tiles of 32 out-channels per wave where O is a multiple of 64: an activation register set feeds two MFMAs.
//   * the ACTIVATIONS never touch LDS: a lane reads the dword of its pixel and its half of the channel word, at
//     pixel base + tap_xoff[tap] + word * Hp * Wp (stride and dilation are in the address only), a whole chunk ahead.
//   * the BORDER TERM for any kernel: the taps inside the image form a rectangle [kh_lo, kh_hi) x [kw_lo, kw_hi), so the
//     term is four reads of a 2-D prefix-sum table of wsum, (KH + 1) x (KW + 1) x 32 MT ints in LDS.
// The epilogue is the popcount kernel's (csrc/lsq_xnor_conv.hip), fmaf for fmaf; one launch per (weight plane, pair of
// activation planes) with the running sum in y, as lsq_xnor_conv2d does.

#include "../lsq_common.h"
#include "lsq_hip_conv_xnor_gen.h"

namespace lsq {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int kWaves = 8;                        // pixel tiles (of 32) per workgroup
constexpr int kThreads = 64 * kWaves;
constexpr int kChunkMfma = 8;                    // K steps x activation planes between two barriers
constexpr int kMaxTaps = 64, kMaxK = 8;

struct GenArgs {
  const unsigned* xd;                  // this pass's activation planes as dwords: [KX][N][Gg][Hp][Wp][2]
  const float* xscales;                // [KX][N]
  const unsigned long long* wbits;     // [steps][O]  (one weight plane)
  const int* wsum;                     // [O][taps]
  const float* wscale;                 // [O]
  const float* bias;                   // [O] or null
  const float* slope;                  // PReLU slope(s)
  const float* res_pre;                // [N][O][Ho][Wo] or null
  const float* res_post;
  float* y;
  unsigned plane_dwords;               // dwords of one activation plane
  unsigned word_dwords;                // 2 Hp Wp: dwords between two channel words of a sample
  int N, H, W, O, KH, KW, sh, sw, ph, pw, dh, dw, Gg, Hp, Wp, Ho, Wo;
  int steps;                           // KH KW Gg
  int accumulate, final_pass, act;
  int tap_xoff[kMaxTaps];              // dwords: 2 ((kh dil_h) Wp + kw dil_w)
};

template <int KX, int MT>
__global__ __launch_bounds__(kThreads, 4) void xnor_gen_kernel(GenArgs a) {
  constexpr int OC = 32 * MT;                    // out-channels of the workgroup
  constexpr int kChunk = kChunkMfma / KX;        // K steps between two barriers: as many MFMAs per chunk with one plane as with two
  constexpr int kFrag = kChunk * MT;             // 1 KB fragments per buffer: [step of the chunk][tile]
  constexpr int kEnt = (kFrag * 64 + kThreads - 1) / kThreads;      // (fragment, lane) entries a thread expands per chunk
  __shared__ v4i s_w[2][kFrag][64];
  __shared__ __attribute__((aligned(16))) int s_pre[(kMaxK + 1) * (kMaxK + 1)][OC];      // [a (KW + 1) + b][o]: sum over kh < a, kw < b
  __shared__ __attribute__((aligned(16))) float s_scale[OC], s_bias[OC], s_slope[OC];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int col = lane & 31, hh = lane >> 5;
  const int o0 = blockIdx.y * OC;
  const int ob = 4 * hh;                         // the lane's out-channel of register i of tile mt: 32 mt + ob + (i & 3) + 8 (i >> 2)

  // ---- the lane's pixel: tile = 32 consecutive outputs, flat over (n, ho, wo); lanes past the last one compute pixel 0 and
  // store nothing (a whole wave of them still takes part in the staging and the barriers)
  const unsigned total = (unsigned)(a.N * a.Ho * a.Wo);
  const int HoWo = a.Ho * a.Wo;
  const unsigned pix = ((unsigned)blockIdx.x * kWaves + (unsigned)wid) * 32u + (unsigned)col;
  const bool valid = pix < total;
  const unsigned pc = valid ? pix : 0u;
  const int n = (int)(pc / (unsigned)HoWo);
  const int r = (int)(pc - (unsigned)n * (unsigned)HoWo);
  const int ho = (int)((unsigned)r / (unsigned)a.Wo), wo = r - ho * a.Wo;
  const unsigned xbase = 2u * (unsigned)((n * a.Gg * a.Hp + ho * a.sh) * a.Wp + wo * a.sw) + (unsigned)hh;

  // the (tap, word) of the next step to request: steps are requested in order, so the pair follows with an add and a carry
  int ld_tap = 0, ld_j = 0;
  auto request = [&](int s0, unsigned (&x)[kChunk * KX]) {
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
      if (s0 + k < a.steps) {                    // (uniform)
        const unsigned at = xbase + (unsigned)a.tap_xoff[ld_tap] + (unsigned)ld_j * a.word_dwords;
#pragma unroll
        for (int p = 0; p < KX; ++p) x[k * KX + p] = a.xd[at + (unsigned)p * a.plane_dwords];
        if (++ld_j == a.Gg) {
          ld_j = 0;
          ++ld_tap;
        }
      } else {
#pragma unroll
        for (int p = 0; p < KX; ++p) x[k * KX + p] = 0u;
      }
    }
  };
  // entry e of a thread: fragment f = (step of the chunk) MT + tile, lane L of the wave that will read it; L supplies
  // out-channel L & 31 and dword L >> 5 of the weight word (the k half its activation lanes supply)
  auto wload = [&](int s0, unsigned long long (&w)[kEnt]) {
#pragma unroll
    for (int e = 0; e < kEnt; ++e) {
      const int idx = tid + e * kThreads, L = idx & 63, f = idx >> 6;
      const int s = s0 + f / MT, mt = f % MT;
      w[e] = (idx < kFrag * 64 && s < a.steps) ? a.wbits[(long long)s * a.O + o0 + 32 * mt + (L & 31)] : 0ull;
    }
  };
  auto wstore = [&](int buf, const unsigned long long (&w)[kEnt]) {
#pragma unroll
    for (int e = 0; e < kEnt; ++e) {
      const int idx = tid + e * kThreads, L = idx & 63, f = idx >> 6;
      const unsigned d = (L >> 5) ? (unsigned)(w[e] >> 32) : (unsigned)w[e];
      // nibble j of register q = channel q + 4 j: +-(4, 2, 1, 4) as E2M1 codes 6 / 4 / 2 / 6, sign bit 8 where the weight is -1
      v4i out;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned mag = (q == 1 ? 0x4u : (q == 2 ? 0x2u : 0x6u)) * 0x11111111u;
        const unsigned ones = (d >> q) & 0x11111111u;
        out[q] = (int)(mag | ((ones ^ 0x11111111u) << 3));
      }
      if (idx < kFrag * 64) s_w[buf][f][L] = out;
    }
  };

  // ---- the first chunk's operands go out before the tables are built: their latency hides behind it
  unsigned xc[kChunk * KX], xn[kChunk * KX];
  unsigned long long wreg[kEnt];
  request(0, xc);
  wload(0, wreg);

  // ---- once per workgroup: scale / bias / slope and the prefix sums of wsum of its OC out-channels
  const int taps = a.KH * a.KW, W1 = a.KW + 1;
  if (tid < OC) {
    s_scale[tid] = a.wscale[o0 + tid];
    s_bias[tid] = a.bias ? a.bias[o0 + tid] : 0.f;
    s_slope[tid] = a.act >= LSQ_ACT_PRELU ? a.slope[a.act == LSQ_ACT_PRELU ? 0 : o0 + tid] : 0.f;
  }
  for (int i = tid; i < (a.KH + 1) * W1 * OC; i += kThreads) s_pre[i / OC][i % OC] = 0;
  __syncthreads();
  for (int i = tid; i < OC * taps; i += kThreads) {          // (consecutive threads, consecutive addresses: wsum is [O][taps])
    const int o = i / taps, tp = i - o * taps;
    const int kh = tp / a.KW, kw = tp - kh * a.KW;
    s_pre[(kh + 1) * W1 + kw + 1][o] = a.wsum[(long long)o0 * taps + i];
  }
  __syncthreads();
  for (int i = tid; i < a.KH * OC; i += kThreads) {           // along kw
    const int o = i % OC, row = (i / OC + 1) * W1;
    int run = 0;
    for (int b = 1; b <= a.KW; ++b) {
      run += s_pre[row + b][o];
      s_pre[row + b][o] = run;
    }
  }
  __syncthreads();
  for (int i = tid; i < a.KW * OC; i += kThreads) {           // along kh
    const int o = i % OC, b = i / OC + 1;
    int run = 0;
    for (int k = 1; k <= a.KH; ++k) {
      run += s_pre[k * W1 + b][o];
      s_pre[k * W1 + b][o] = run;
    }
  }
  wstore(0, wreg);
  __syncthreads();

  // ---- the accumulators start at the border term: minus the rectangle sum of wsum over the taps inside the image.  hi and
  // wi grow with the tap index, so the bounds of the rectangle are counts of taps below 0 and below the image's extent.
  v16f acc[KX][MT];
  {
    const int hi0 = ho * a.sh - a.ph, wi0 = wo * a.sw - a.pw;
    int kh_lo = 0, kh_hi = 0, kw_lo = 0, kw_hi = 0;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      const int hi = hi0 + k * a.dh, wi = wi0 + k * a.dw;
      kh_lo += (k < a.KH && hi < 0) ? 1 : 0;
      kh_hi += (k < a.KH && hi < a.H) ? 1 : 0;
      kw_lo += (k < a.KW && wi < 0) ? 1 : 0;
      kw_hi += (k < a.KW && wi < a.W) ? 1 : 0;
    }
    const int* __restrict__ p11 = &s_pre[kh_hi * W1 + kw_hi][ob];
    const int* __restrict__ p01 = &s_pre[kh_lo * W1 + kw_hi][ob];
    const int* __restrict__ p10 = &s_pre[kh_hi * W1 + kw_lo][ob];
    const int* __restrict__ p00 = &s_pre[kh_lo * W1 + kw_lo][ob];
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
          for (int p = 0; p < KX; ++p) acc[p][mt][4 * g + e] = (float)(-inside[e]);
        }
      }
  }

  // ---- the K loop.  Order of issue per chunk, pinned with scheduling barriers: the next chunk's activation dwords and weight
  // words first, then this chunk's fragment reads, v_and and MFMAs, then the next chunk's fragments into the other buffer.
  const int unit_scale = 0x7F7F7F7F;             // E8M0 127 = 2^0 in every byte: the block scales of both operands
  const int nchunks = (a.steps + kChunk - 1) / kChunk;
  for (int c = 0; c < nchunks; ++c) {
    const int s0 = c * kChunk;
    const bool more = c + 1 < nchunks;           // (uniform)
    if (more) {
      request(s0 + kChunk, xn);
      wload(s0 + kChunk, wreg);
    }
    __builtin_amdgcn_sched_barrier(0);
    const v4i (*__restrict__ wb)[64] = s_w[c & 1];
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
      if (s0 + k < a.steps) {                    // (uniform: the last chunk may be partial)
        v8i b8[KX];
#pragma unroll
        for (int p = 0; p < KX; ++p) {
          const unsigned d = xc[k * KX + p];
          b8[p] = v8i{(int)(d & 0x11111111u), (int)(d & 0x22222222u), (int)(d & 0x44444444u), (int)((d >> 3) & 0x11111111u), 0, 0, 0, 0};
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const v4i w4 = wb[k * MT + mt][lane];
          const v8i w8 = {w4[0], w4[1], w4[2], w4[3], 0, 0, 0, 0};      // (fp4 operands: the low four registers are read)
#pragma unroll
          for (int p = 0; p < KX; ++p)
            acc[p][mt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(w8, b8[p], acc[p][mt], 4, 4, 0, unit_scale, 0, unit_scale);
        }
        // (an empty asm on the accumulators ties each step to its place: the scaled MFMA is a pure value to the selector)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int p = 0; p < KX; ++p) asm volatile("" : "+v"(acc[p][mt]));
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (more) {
      wstore((c + 1) & 1, wreg);
#pragma unroll
      for (int i = 0; i < kChunk * KX; ++i) xc[i] = xn[i];
    }
    // buffer (c + 1) & 1 was last read in iteration c - 1, in front of that iteration's barrier; this one publishes it and
    // retires the reads of buffer c & 1 before iteration c + 1 overwrites it
    lds_barrier();
  }

  // ---- epilogue: the popcount kernel's arithmetic on the same integers -> the same floats
  if (!valid) return;
  float xs[KX];
#pragma unroll
  for (int p = 0; p < KX; ++p) xs[p] = a.xscales[p * a.N + n];
  const bool fin = a.final_pass != 0, acc_in = a.accumulate != 0;
  const bool want_pre = fin && a.res_pre, want_post = fin && a.res_post;
  const bool relu = fin && a.act == LSQ_ACT_RELU, prelu = fin && a.act >= LSQ_ACT_PRELU;
  // 32-bit element offsets (the entry point admits outputs below 2^30 elements)
  const unsigned yoff = (unsigned)((n * a.O + o0 + ob) * HoWo + r);
  // (eight outputs at a time: their loads go out together, and the three operand arrays stay small beside the accumulators)
#pragma unroll
  for (int h = 0; h < 2 * MT; ++h) {
    const int mt = h >> 1, i0 = 8 * (h & 1);
    float basev[8], pre[8], post[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = i0 + k, ch = 32 * mt + (i & 3) + 8 * (i >> 2);
      const unsigned at = yoff + (unsigned)(ch * HoWo);
      basev[k] = acc_in ? a.y[at] : s_bias[ob + ch];
      pre[k] = want_pre ? a.res_pre[at] : 0.f;
      post[k] = want_post ? a.res_post[at] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = i0 + k, ch = 32 * mt + (i & 3) + 8 * (i >> 2);
      float v = xs[0] * acc[0][mt][i];
#pragma unroll
      for (int p = 1; p < KX; ++p) v = fmaf(xs[p], acc[p][mt][i], v);
      float out = fmaf(v, s_scale[ob + ch], basev[k]);
      if (want_pre) out += pre[k];
      if (relu) out = fmaxf(out, 0.f);
      if (prelu) {
        const float neg = s_slope[ob + ch] * out;
        out = out > 0.f ? out : neg;
      }
      if (want_post) out += post[k];
      a.y[yoff + (unsigned)(ch * HoWo)] = out;
    }
  }
}

template <int KX>
int launch(const GenArgs& a, hipStream_t st) {
  const long long ntiles = ((long long)a.N * a.Ho * a.Wo + 31) >> 5;
  const unsigned gx = (unsigned)((ntiles + kWaves - 1) / kWaves);
  if (a.O % 64 == 0) hipLaunchKernelGGL((xnor_gen_kernel<KX, 2>), dim3(gx, (unsigned)(a.O / 64)), dim3(kThreads), 0, st, a);
  else hipLaunchKernelGGL((xnor_gen_kernel<KX, 1>), dim3(gx, (unsigned)(a.O / 32)), dim3(kThreads), 0, st, a);
  return (int)hipGetLastError();
}

// 0 where the kernel takes (g, kx, kw_planes), else the code the entry point returns
int gen_check(const lsq_conv_geom* g, int kx, int kw_planes) {
  if (int e = check_geom(g)) return e;
  if (kx < 1 || kx > LSQ_MAX_PLANES || kw_planes < 1 || kw_planes > LSQ_MAX_PLANES) return LSQ_E_SCHEME;
  const int Ho = out_h(g), Wo = out_w(g);
  if (Ho <= 0 || Wo <= 0) return LSQ_E_SHAPE;
  if (g->groups != 1 || g->C % 64 || g->O % 32) return LSQ_E_UNSUPPORTED;
  if (g->KH > kMaxK || g->KW > kMaxK || g->KH * g->KW > kMaxTaps) return LSQ_E_UNSUPPORTED;
  if ((long long)g->C * g->KH * g->KW >= (1ll << 23)) return LSQ_E_UNSUPPORTED;      // the fp32 accumulator holds the integer exactly
  if ((long long)g->N * g->O * Ho * Wo >= (1ll << 30)) return LSQ_E_UNSUPPORTED;     // 32-bit element offsets
  if (g->O / 32 > 65535) return LSQ_E_UNSUPPORTED;                                    // (grid.y)
  const long long Hp = g->H + 2ll * g->pad_h, Wp = g->W + 2ll * g->pad_w;
  if ((long long)g->N * (g->C / 64) * Hp * Wp * kx >= (1ll << 30)) return LSQ_E_UNSUPPORTED;      // 32-bit dword offsets
  return LSQ_OK;
}

}  // namespace
}  // namespace lsq

using namespace lsq;

extern "C" int lsq_conv_xnor_gen_abi_version(void) { return LSQ_CONV_XNOR_GEN_ABI_VERSION; }

extern "C" int lsq_xnor_conv2d_gen_supported(const lsq_conv_geom* g, int kx, int kw_planes) {
  return gen_check(g, kx, kw_planes) == LSQ_OK ? 1 : 0;
}

extern "C" int lsq_xnor_conv2d_gen(const uint64_t* xplanes, int kx, const float* xscales, const uint64_t* wbits,
                                   const int32_t* wsum, int kw_planes, const float* wscales, const float* bias,
                                   const lsq_conv_geom* g, int act, const float* act_slope, const float* res_pre,
                                   const float* res_post, float* y, void* stream) {
  if (!xplanes || !xscales || !wbits || !wsum || !wscales || !y) return LSQ_E_NULL;
  if (int e = gen_check(g, kx, kw_planes)) return e;
  if (act < LSQ_ACT_NONE || act > LSQ_ACT_PRELU_CHANNEL || (act >= LSQ_ACT_PRELU && !act_slope)) return LSQ_E_SCHEME;
  GenArgs a = {};
  a.N = g->N; a.H = g->H; a.W = g->W; a.O = g->O; a.KH = g->KH; a.KW = g->KW;
  a.sh = g->stride_h; a.sw = g->stride_w; a.ph = g->pad_h; a.pw = g->pad_w; a.dh = g->dil_h; a.dw = g->dil_w;
  a.Gg = g->C / 64;
  a.Hp = g->H + 2 * g->pad_h; a.Wp = g->W + 2 * g->pad_w;
  a.Ho = out_h(g); a.Wo = out_w(g);
  a.steps = g->KH * g->KW * a.Gg;
  const long long xplane_words = lsq_act_plane_words(g), wplane_words = lsq_weight_plane_words(g);
  // (the layouts this kernel indexes: [N][C/64][Hp][Wp] words per activation plane, [taps][C/64][O] per weight plane)
  if (xplane_words != (long long)a.N * a.Gg * a.Hp * a.Wp || wplane_words != (long long)a.steps * a.O) return LSQ_E_UNSUPPORTED;
  a.plane_dwords = (unsigned)(2 * xplane_words);
  a.word_dwords = 2u * (unsigned)(a.Hp * a.Wp);
  for (int kh = 0; kh < g->KH; ++kh)
    for (int kw = 0; kw < g->KW; ++kw) a.tap_xoff[kh * g->KW + kw] = 2 * (kh * g->dil_h * a.Wp + kw * g->dil_w);
  a.bias = bias;
  a.slope = act_slope;
  a.act = act;
  a.res_pre = res_pre;
  a.res_post = res_post;
  a.y = y;
  const int taps = g->KH * g->KW;
  hipStream_t st = (hipStream_t)stream;
  bool first = true;
  // one launch per (weight plane, pair of activation planes), the running sum carried through y: lsq_xnor_conv2d's passes
  for (int q = 0; q < kw_planes; ++q) {
    for (int p0 = 0; p0 < kx; p0 += 2) {
      const int np = (kx - p0) >= 2 ? 2 : 1;
      a.xd = reinterpret_cast<const unsigned*>(xplanes + (long long)p0 * xplane_words);
      a.xscales = xscales + (long long)p0 * g->N;
      a.wbits = reinterpret_cast<const unsigned long long*>(wbits) + (long long)q * wplane_words;
      a.wsum = wsum + (long long)q * g->O * taps;
      a.wscale = wscales + (long long)q * g->O;
      a.accumulate = first ? 0 : 1;
      a.final_pass = (q == kw_planes - 1 && p0 + np >= kx) ? 1 : 0;
      if (int e = np == 2 ? launch<2>(a, st) : launch<1>(a, st)) return e;
      first = false;
    }
  }
  return LSQ_OK;
}
