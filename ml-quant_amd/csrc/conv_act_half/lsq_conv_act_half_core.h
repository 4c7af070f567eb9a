// The kernels of the 16-bit activation quantizers of QuantConv2d, one source for two libraries:
//   BN = false  lsq_act_quant_half     (conv_act_half/lsq_conv_act_half.hip)       reads x as it is
//   BN = true   lsq_act_quant_bn_half  (conv_act_bn_half/lsq_conv_act_bn_half.hip) reads t = round_to_dtype(x * s[c] + b[c])
// Sign planes and per-sample scales of a bf16 / fp16 NCHW batch in the convolution's plane layout
// (include/lsq_hip.h: bit b of word (n, grp Gg + j, h + pad_h, w + pad_w) is channel grp cg + 64 j + b at pixel (h, w)) --
// the activation operand of lsq_xnor_conv2d from a 16-bit input, every scheme of lsq_act_quant, in ONE launch.
//
// One workgroup of 1024 threads owns a sample from its first load to its last plane word (grid = N): no workspace, no row
// shared between workgroups, integer atomics in LDS only.
//   * PLANE SWEEP (the lane = pixels, loop over the 64 channels of a word sweep of lsq_act_quant.hip): an ITEM is one word
//     index j and PIX consecutive pixels, PIX = 8, 4, 2 or 1 -- the largest that divides H W, so that a lane's pixels lie
//     in one channel row.  A lane walks the item's channels, converts each value to fp32 (exactly; subnormals kept), clamps
//     it, runs the chain of lsq_act_quant's chain_eval and assembles PIX words in registers; consecutive lanes hold
//     consecutive pixels: a wave's loads are contiguous in a channel, its stores consecutive w.  Eight loads are requested
//     before any is consumed.  A row with fewer items than half the threads is shared 2, 4 or 8 lanes an item:
//     each lane walks 32, 16 or 8 channels and the lanes' partial words are ORed together (they sit in one wave).
//   * LOAD: PIX elements in one 2 PIX-byte load where x is aligned to 2 PIX bytes (VEC; H W % PIX == 0 makes every channel
//     row of every sample as aligned as x), PIX 2-byte loads otherwise.  The same lane owns the same pixels either way, so
//     neither the words nor the scales depend on the alignment.
//   * SCALE SUMS are folded into the sweep: the fp32 magnitudes |res_q| of a GROUP of 8 consecutive channels at one pixel
//     (fewer in the last group of cg % 8) are added in fp32 in channel order, a lane's groups in fp64 in the order it meets
//     them, the wave's lanes by xor butterfly, the workgroup's waves in wave order.  Items, PIX and the lane sharing depend
//     on (C, H, W, groups) alone -- not on N, the sample's position, the address or the call.  v_q = (float)(S_q / M).
//   * PASSES: ls-1 / gf-1 -> one sweep.  gf-k -> k sweeps (the row again from L2), sweep q writes plane q.  Given scales ->
//     one sweep for k <= 2 (both planes), k sweeps of one plane beyond (k x PIX words would not fit a lane's registers).
//   * ls-2 / ls-T free-running: solve_v1 of linear_act_solve/lsq_half_table.h -- the count table (one count per
//     15-bit magnitude key, dynamic LDS bounded by key(alpha), swizzled index) over the flat sub-sample row[::skip], its plan /
//     test / argmin on lsq_solver_math.h; lsq_linear_act_solve.hip holds the same statements in line --, then one sweep for both
//     planes and S_1.  Only these kernels carry the table.
//   * BN: every element read -- in the table's pass 1 and in every sweep -- goes through fold_bits first: the
//     affine map of its channel in two fp32 operations, rounded once to the bits of the type.  The rounded value is a value
//     of the type, so keys, the clamp-bound key and the chain see a 16-bit tensor exactly as without BN.  Scale and shift are
//     read from global memory where the element is consumed (a lane's 8 loads in flight carry their channels' pairs); no LDS.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "lsq_hip.h"
#include "lsq_hip_linear_half.h" /* LSQ_DTYPE_* */
#include "../linear_act_solve/lsq_half_table.h"

namespace {

using namespace lsq_half;                             // to_f32, clamp_sym, load_group, wave_sum
using namespace lsq_half_table;                       // Shared, solve_v1, Best, kNoKey, top_key, table_bytes, allow_full_table

constexpr int kThreads = 1024, kWaves = kThreads / 64;   // (the first 512 threads plan the table's slices, every wave tests)
constexpr int kBatch = 8;                             // loads a lane requests before it consumes any of them
constexpr int kMaxSplitLog2 = 3;                      // at most 8 lanes an item: a lane keeps whole groups of 8 channels

enum { kGiven = 0, kFree = 1, kSolve = 2 };           // scales given | ls-1 / gf-k sums | ls-2 / ls-T table solve

struct Args {
  const unsigned short* x;            // [N][C][H][W], bf16 or fp16 bits
  const float* forced;                // [k][N] or null
  unsigned long long* planes;         // [k][N][Gt][Hp][Wp]
  float* scales;                      // [k][N]
  int* status;                        // [N] or null
  long long M, plane_words, row_words;   // M = C H W;  words of one plane;  words of one sample of one plane
  int N, HW, W, cg, Gg, Gt, Hp, Wp, pad_h, pad_w;
  int k, skip, ternary;
  int csl;                            // 2^csl lanes share an item
  unsigned n;                         // keys of the sub-sample: ceil(M / skip)
  unsigned kmax;                      // the largest key a clamped value has; the table holds the slices up to it
  float alpha;                        // clamp bound (negative: none)
};

struct ArgsBN : Args {
  const float* pre_scale;             // [C]
  const float* pre_shift;             // [C]
};

template <bool BN>
using ArgsOf = std::conditional_t<BN, ArgsBN, Args>;

// fl32(fl32(x * s) + b) rounded to nearest even into the type, as its 16 bits (as Tensor.to(dtype) rounds: subnormals of the
// type kept, fp16 overflow -> +-inf; a NaN is outside the contract)
template <bool F16>
__device__ __forceinline__ unsigned fold_bits(unsigned h, float s, float b) {
  const float t = __fadd_rn(__fmul_rn(to_f32<F16>(h), s), b);
  if constexpr (F16) {
    return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)t);   // the hardware's RNE convert
  } else {
    unsigned u = __float_as_uint(t);
    if ((u & 0x7F800000u) != 0x7F800000u) u += 0x7FFFu + ((u >> 16) & 1u);
    return u >> 16;
  }
}

// The element transform solve_v1 applies to what it counts: the folded batch norm of the element's channel.
template <bool F16>
struct FoldBN {
  const float* scale;
  const float* shift;
  int HW;
  struct Channel {
    float s, b;
  };
  __device__ __forceinline__ Channel channel(long long index) const {   // index: the element's position in the sample
    const int c = (int)((unsigned)index / (unsigned)HW);
    return {scale[c], shift[c]};
  }
  __device__ __forceinline__ unsigned operator()(unsigned h, const Channel& ch) const { return fold_bits<F16>(h, ch.s, ch.b); }
};

// PIX consecutive elements as 16-bit halves of 32-bit words
template <int PIX>
struct Raw {
  unsigned d[(PIX + 1) / 2];
};

template <int PIX, bool VEC>
__device__ __forceinline__ Raw<PIX> load_pixels(const unsigned short* p) {
  Raw<PIX> r;
  if constexpr (PIX == 1) {
    r.d[0] = p[0];
  } else if constexpr (!VEC) {
#pragma unroll
    for (int i = 0; i < PIX / 2; ++i) r.d[i] = (unsigned)p[2 * i] | (unsigned)p[2 * i + 1] << 16;
  } else if constexpr (PIX == 8) {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    r.d[0] = t.x; r.d[1] = t.y; r.d[2] = t.z; r.d[3] = t.w;
  } else if constexpr (PIX == 4) {
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    r.d[0] = t.x; r.d[1] = t.y;
  } else {
    r.d[0] = *reinterpret_cast<const unsigned*>(p);
  }
  return r;
}

// One sweep over the sample.  NP = 1: plane q (chain depth q) and, with SUM, the thread's share of S_q.  NP = 2: planes 0
// and 1 with v[0] and, with SUM, the thread's share of S_1.
template <bool BN, bool F16, int PIX, bool VEC, int NP, bool SUM>
__device__ __forceinline__ double sweep(const ArgsOf<BN>& a, const unsigned short* __restrict__ xrow,
                                        unsigned long long* __restrict__ prow, int q, const float (&v)[LSQ_MAX_PLANES]) {
  const int HW = a.HW;
  const int PV = HW / PIX;                            // (PIX divides H W)
  const int items = a.Gt * PV;
  const int csl = a.csl, cs = 1 << csl;
  const int part = (int)(threadIdx.x & (unsigned)(cs - 1));
  const int cper = 64 >> csl;
  double acc = 0.0;
  for (int item = (int)(threadIdx.x >> csl); item < items; item += kThreads >> csl) {
    const int j = item / PV;
    const int p = (item - j * PV) * PIX;
    const int grp = j / a.Gg;
    const int jj = j - grp * a.Gg;
    const int cfirst = part * cper;                   // the lane's first channel inside the 64-channel word
    const int c0 = grp * a.cg + jj * 64 + cfirst;
    const int nch = max(0, min(cper, a.cg - jj * 64 - cfirst));
    const unsigned short* src = xrow + (long long)c0 * HW + p;
    unsigned long long word0[PIX], word1[PIX];
    float facc[PIX];                                  // fp32 over one group of 8 channels, folded into fp64 per group
#pragma unroll
    for (int e = 0; e < PIX; ++e) {
      word0[e] = 0ull;
      word1[e] = 0ull;
      facc[e] = 0.f;
    }
    for (int cb = 0; cb < nch; cb += kBatch) {
      Raw<PIX> raw[kBatch];
      [[maybe_unused]] float ps[kBatch], pb[kBatch];  // BN: scale and shift of the channels of the loads in flight
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        raw[u] = load_pixels<PIX, VEC>(src + (long long)min(cb + u, nch - 1) * HW);
        if constexpr (BN) {
          ps[u] = a.pre_scale[c0 + min(cb + u, nch - 1)];
          pb[u] = a.pre_shift[c0 + min(cb + u, nch - 1)];
        }
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int cc = cb + u;                        // bit position relative to the lane's first channel
        if (cc < nch) {
#pragma unroll
          for (int e = 0; e < PIX; ++e) {
            unsigned bits = (raw[u].d[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
            if constexpr (BN) bits = fold_bits<F16>(bits, ps[u], pb[u]);
            const float c = clamp_sym(to_f32<F16>(bits), a.alpha);
            float result = 0.f, res = c;
            if constexpr (NP == 2) {
              const bool b0 = (c - result) >= 0.f;
              word0[e] |= (unsigned long long)b0 << cc;
              result = result + (b0 ? v[0] : -v[0]);
              res = res - ((res >= 0.f) ? v[0] : -v[0]);
              word1[e] |= (unsigned long long)((c - result) >= 0.f) << cc;
            } else {
#pragma unroll
              for (int i = 0; i < LSQ_MAX_PLANES - 1; ++i) {
                if (i >= q) break;
                result = result + ((c - result >= 0.f) ? v[i] : -v[i]);
                res = res - ((res >= 0.f) ? v[i] : -v[i]);
              }
              word0[e] |= (unsigned long long)((c - result) >= 0.f) << cc;
            }
            if constexpr (SUM) facc[e] = facc[e] + fabsf(res);
          }
          if constexpr (SUM) {
            if ((cc & 7) == 7) {                      // (cc counts from the lane's first channel, a multiple of 8)
#pragma unroll
              for (int e = 0; e < PIX; ++e) {
                acc += (double)facc[e];
                facc[e] = 0.f;
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int e = 0; e < PIX; ++e) {
      if constexpr (SUM) acc += (double)facc[e];      // (a last group of fewer than 8 channels; else +0: exact)
      unsigned long long w0 = word0[e] << cfirst, w1 = word1[e] << cfirst;
      for (int d = 1; d < cs; d <<= 1) {              // the lanes that share the item each hold some of its channels' bits
        w0 |= ((unsigned long long)(unsigned)__shfl_xor((int)(w0 >> 32), d) << 32) | (unsigned)__shfl_xor((int)(unsigned)w0, d);
        if constexpr (NP == 2)
          w1 |= ((unsigned long long)(unsigned)__shfl_xor((int)(w1 >> 32), d) << 32) | (unsigned)__shfl_xor((int)(unsigned)w1, d);
      }
      if (part == 0) {
        const int pix = p + e;
        const int h = pix / a.W;
        const int w = pix - h * a.W;
        const long long at = ((long long)j * a.Hp + h + a.pad_h) * a.Wp + w + a.pad_w;
        if constexpr (NP == 2) {
          prow[at] = w0;
          prow[a.plane_words + at] = w1;
        } else {
          prow[(long long)q * a.plane_words + at] = w0;
        }
      }
    }
  }
  return acc;
}

// the workgroup's sum in a fixed order: lanes by butterfly, waves in wave order (slot: kWaves doubles nobody else uses)
__device__ __forceinline__ double block_sum(double acc, double* slot) {
  const double w = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = w;
  __syncthreads();
  double tot = 0.0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) tot += slot[i];
  return tot;
}

template <bool BN, bool F16, int PIX, bool VEC, int MODE>
__global__ __launch_bounds__(kThreads) void conv_quant_rows(ArgsOf<BN> a) {
  __shared__ double s_red[LSQ_MAX_PLANES][kWaves];    // (one slot per sweep: one barrier per sweep)
  const int tid = threadIdx.x;
  const long long row = blockIdx.x;                   // one workgroup a sample: see launch()
  const unsigned short* xrow = a.x + row * a.M;
  unsigned long long* prow = a.planes + row * a.row_words;   // the sample's words in plane 0
  float v[LSQ_MAX_PLANES];
#pragma unroll
  for (int i = 0; i < LSQ_MAX_PLANES; ++i) v[i] = 0.f;
  if constexpr (MODE == kGiven) {
#pragma unroll
    for (int i = 0; i < LSQ_MAX_PLANES; ++i) {
      if (i >= a.k) break;
      v[i] = a.forced[(long long)i * a.N + row];
      if (tid == 0) a.scales[(long long)i * a.N + row] = v[i];
    }
    if (tid == 0 && a.status) a.status[row] = 1;
    if (a.k == 2) {
      sweep<BN, F16, PIX, VEC, 2, false>(a, xrow, prow, 1, v);
    } else {
      for (int q = 0; q < a.k; ++q) sweep<BN, F16, PIX, VEC, 1, false>(a, xrow, prow, q, v);
    }
  } else if constexpr (MODE == kFree) {
    for (int q = 0; q < a.k; ++q) {
      const double acc = sweep<BN, F16, PIX, VEC, 1, true>(a, xrow, prow, q, v);
      const float vq = (float)(block_sum(acc, s_red[q]) / (double)a.M);
#pragma unroll
      for (int i = 0; i < LSQ_MAX_PLANES; ++i)
        if (i == q) v[i] = vq;
      if (tid == 0) a.scales[(long long)q * a.N + row] = vq;
    }
    if (tid == 0 && a.status) a.status[row] = 1;
  } else {
    extern __shared__ __attribute__((aligned(16))) unsigned hist[];   // [slices * 64] counts, swizzled by phys()
    __shared__ Shared<kThreads> sh;
    double total;
    Best best;
    if constexpr (BN) {                               // pass 1 counts the keys of the folded values
      const FoldBN<F16> fold = {a.pre_scale, a.pre_shift, a.HW};
      best = solve_v1<F16, PIX == 8 && VEC, kThreads>(a, xrow, a.M, hist, sh, total, fold);
    } else {
      best = solve_v1<F16, PIX == 8 && VEC, kThreads>(a, xrow, a.M, hist, sh, total);
    }
    // a sub-sample of zeros only (+-0): its candidates are all 0, so it is reported as a sample without one (v1 = 0 either
    // way; `total` is the same bits in every thread)
    if (!(total > 0.0)) best.order = kNoKey;
    v[0] = best.value;                                // 0 where the row has no candidate
    const double acc = sweep<BN, F16, PIX, VEC, 2, true>(a, xrow, prow, 1, v);
    const double tot = block_sum(acc, s_red[0]);
    if (tid == 0) {
      a.scales[row] = v[0];
      a.scales[a.N + row] = a.ternary ? v[0] : (float)(tot / (double)a.M);
      if (a.status) a.status[row] = best.order != kNoKey ? 1 : 0;
    }
  }
}

template <bool BN, bool F16, int PIX, bool VEC, int MODE>
int launch(ArgsOf<BN> a, hipStream_t st) {
  unsigned lds = 0u;
  if constexpr (MODE == kSolve) {
    a.kmax = top_key<F16>(a.alpha);
    lds = table_bytes(a.kmax);
    const hipError_t rc = allow_full_table<&conv_quant_rows<BN, F16, PIX, VEC, MODE>>();
    if (rc != hipSuccess) return (int)rc;
  }
  // One workgroup a sample, N < 2^31 workgroups: the hardware takes them in turn.
  hipLaunchKernelGGL((conv_quant_rows<BN, F16, PIX, VEC, MODE>), dim3((unsigned)a.N), dim3(kThreads), lds, st, a);
  return (int)hipGetLastError();
}

template <bool BN, bool F16, int PIX, bool VEC>
int launch_mode(const ArgsOf<BN>& a, bool solve, hipStream_t st) {
  if (a.forced) return launch<BN, F16, PIX, VEC, kGiven>(a, st);
  return solve ? launch<BN, F16, PIX, VEC, kSolve>(a, st) : launch<BN, F16, PIX, VEC, kFree>(a, st);
}

template <bool BN, bool F16>
int launch_path(const ArgsOf<BN>& a, bool solve, hipStream_t st) {
  // PIX: the largest of 8, 4, 2, 1 that divides H W (fixed by the shape).  VEC: x on 2 PIX bytes (the same bits either way).
  const uintptr_t at = (uintptr_t)a.x;
  if (a.HW % 8 == 0) return (at & 15) == 0 ? launch_mode<BN, F16, 8, true>(a, solve, st) : launch_mode<BN, F16, 8, false>(a, solve, st);
  if (a.HW % 4 == 0) return (at & 7) == 0 ? launch_mode<BN, F16, 4, true>(a, solve, st) : launch_mode<BN, F16, 4, false>(a, solve, st);
  if (a.HW % 2 == 0) return (at & 3) == 0 ? launch_mode<BN, F16, 2, true>(a, solve, st) : launch_mode<BN, F16, 2, false>(a, solve, st);
  return launch_mode<BN, F16, 1, false>(a, solve, st);
}

// The argument checks and the launch of lsq_act_quant_half (BN = false: pre_scale / pre_shift are not read) and of
// lsq_act_quant_bn_half with both arrays (BN = true).
template <bool BN>
int act_quant_rows(const void* x, int x_dtype, const lsq_conv_geom* g, int scheme, int k, int skip, float clamp_alpha,
                   const float* pre_scale, const float* pre_shift, const float* forced, uint64_t* planes, float* scales,
                   int32_t* status, void* stream) {
  if (!x || !g || !planes || !scales) return LSQ_E_NULL;
  const int rc = lsq::check_geom(g);                  // (the geometry checks of lsq_act_quant)
  if (rc != LSQ_OK) return rc;
  if (skip <= 0) return LSQ_E_SHAPE;
  if (k < 1 || k > LSQ_MAX_PLANES || scheme < LSQ_SCHEME_LS1 || scheme > LSQ_SCHEME_GF) return LSQ_E_SCHEME;
  const bool solver = scheme == LSQ_SCHEME_LS2 || scheme == LSQ_SCHEME_LST;
  if ((scheme == LSQ_SCHEME_LS1 && k != 1) || (solver && k != 2)) return LSQ_E_SCHEME;
  if (x_dtype != LSQ_DTYPE_BF16 && x_dtype != LSQ_DTYPE_F16) return LSQ_E_UNSUPPORTED;
  const long long HW = (long long)g->H * g->W, M = (long long)g->C * HW;
  if (M >= (1ll << 31)) return LSQ_E_UNSUPPORTED;
  ArgsOf<BN> a = {};
  a.x = static_cast<const unsigned short*>(x);
  a.forced = forced;
  a.planes = reinterpret_cast<unsigned long long*>(planes);
  a.scales = scales;
  a.status = status;
  a.N = g->N;
  a.HW = (int)HW;
  a.W = g->W;
  a.M = M;
  a.cg = g->C / g->groups;
  a.Gg = (a.cg + 63) / 64;
  a.Gt = g->groups * a.Gg;
  a.Hp = g->H + 2 * g->pad_h;
  a.Wp = g->W + 2 * g->pad_w;
  a.pad_h = g->pad_h;
  a.pad_w = g->pad_w;
  a.row_words = (long long)a.Gt * a.Hp * a.Wp;
  a.plane_words = a.row_words * g->N;
  a.k = k;
  a.skip = skip;
  a.ternary = scheme == LSQ_SCHEME_LST;
  a.n = (unsigned)((M + skip - 1) / skip);
  a.alpha = clamp_alpha;
  if constexpr (BN) {
    a.pre_scale = pre_scale;
    a.pre_shift = pre_shift;
  }
  // lanes an item: as many (up to 8) as keep the items within the workgroup -- fixed by (C, H, W, groups) alone
  const int pix = HW % 8 == 0 ? 8 : (HW % 4 == 0 ? 4 : (HW % 2 == 0 ? 2 : 1));
  const long long items = (long long)a.Gt * (HW / pix);
  while (a.csl < kMaxSplitLog2 && (items << (a.csl + 1)) <= kThreads) ++a.csl;
  hipStream_t st = (hipStream_t)stream;
  const bool solve = solver && !forced;
  return x_dtype == LSQ_DTYPE_F16 ? launch_path<BN, true>(a, solve, st) : launch_path<BN, false>(a, solve, st);
}

}  // namespace
