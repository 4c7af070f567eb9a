// The input gradient of QuantLinear as one set of kernels, instantiated by liblsq_hip_linear_train.so (lsq_linear_signw_dgrad:
// fp32 gradients, plain fp32 stores) and by liblsq_hip_linear_train_half.so (lsq_linear_signw_dgrad_half: bf16 / fp16
// gradients converted exactly to fp32 as they are read, the straight-through estimator and the rounding into the type in the
// epilogue).  Templated on the gradient's element type GY and on an epilogue EPI; the tile rule, staging and the order of
// summation do not depend on either, so every instantiation computes the same fp32 accumulators.  Each library compiles its
// own copy (anonymous namespace); neither links the other's objects.
//   EPI:  struct Row;                                             what the epilogue keeps per sample (the sample's scales)
//         int sample(long long m) const;                          the sample that owns row m (0 where no row state is kept)
//         void row(int n, Row&) const;                            called when a lane's rows reach another sample
//         void store(long long i, const Row&, float acc) const;   element i of gx = f(acc)
//
// Gradient rows x sign-weight planes with the sum over the OUTPUT features, on the bf16 matrix cores of gfx950
// (v_mfma_f32_32x32x16_bf16) -- lsq_linear_signw transposed.
//
// As a GEMM:  gx[m][f] = sum_q sum_o (gy[m][o] ws[q][o]) s_q[o][f],  M = rows, K = O output features (per plane), N = F.
// Gradient rows are operand A (rows m), weights operand B (columns f); fragment layout, the hi / lo split and the sign-bit
// expansion: csrc/linear/lsq_signw_mma.h.
//   * WEIGHT: the forward's planes hold the bits of 64 FEATURES in a word; here k runs over o, so a first kernel
//     (transpose_planes) writes the transposed image T[q][ceil(O / 64)][ceil16(F)] into the caller's workspace: one wave
//     per 64 x 64 bit block, lane j reads the word of output feature 64 w + j, ballot i collects bit i of all lanes =
//     the word of input feature i.  After it a lane's B fragment is 8 consecutive bits of one word of its column, as in
//     the forward: one bit per weight in memory throughout.
//   * GRADIENT: a = fl32(gy ws[q][o]) -- the scale is per (plane, k) here, so it goes into A and all planes add into ONE
//     accumulator --, then split.  Output features past O are staged as 0: the padded slots of a plane are zero words and
//     would read as -1.
//   * Rows past M and columns past F read a valid row / column and are never stored.
// Two kernels behind the one entry point (selected from M and F, tile_rule):
//   dgrad_tiled  M x F tiles of 128 x 128 or 64 x 64, four waves (2 x 2), over the kw * ceil(O / 64) stages (plane-major);
//                per stage the workgroup scales and splits its rows' gradients ONCE into LDS; the next stage's gradients,
//                scales and weight words are loaded into registers while the MFMAs of this one run.
//   dgrad_split  few tiles (LeNet fc1, the ResNet head): one 32 x 32 tile of gx per workgroup, the stages split over 8
//                waves, each reading, scaling, splitting and multiplying its own range straight from global memory; the
//                partial sums meet in LDS and are added in wave order.
// VEC: a staging role's values in one load -- fp32: 16 bytes (4 values; the split kernel's 8 values in two), where gy is
// 16-byte aligned and O % 4 == 0; 16-bit: the tiled kernel's 4 values in 8 bytes where gy is 8-byte aligned and O % 4 == 0,
// the split kernel's 8 values in 16 bytes where gy is 16-byte aligned and O % 8 == 0 (every row then starts on the load's
// size).  Otherwise one load per element: the same values, the same bits.

#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "lsq_hip_linear_train.h"
#include "../linear/lsq_signw_mma.h"

namespace {

// plain fp32 stores: lsq_linear_signw_dgrad
struct EpiStore {
  float* gx;                          // [M][F]
  struct Row {};
  __device__ __forceinline__ int sample(long long) const { return 0; }
  __device__ __forceinline__ void row(int, Row&) const {}
  __device__ __forceinline__ void store(long long i, const Row&, float acc) const { gx[i] = acc; }
};

template <class GY, class EPI>
struct Args {
  const GY* gy;                       // [M][O]
  const unsigned long long* tbits;    // transposed planes [kw][nwo][fpad]
  const float* wscales;               // [kw][O]
  EPI epi;                            // gx [M][F] and what becomes of an accumulator
  long long M;
  int F, O, fpad, nwo, stages;        // fpad = ceil16(F); nwo = ceil(O / 64); stages = kw * nwo
};

template <class GY, int N>
struct alignas(N * sizeof(GY)) Pack {
  GY v[N];
};

// load_rows4 of lsq_signw_mma.h for a 16-bit matrix: VEC = one 8-byte load a row (every row starts on 8 bytes).
template <bool VEC, int ROWS, class GY>
__device__ __forceinline__ void load_rows4_half(const GY* base, long long row, long long M, int K, int k,
                                                float (&v)[ROWS][4]) {
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const long long mi = row + 16 * i;
    const GY* p = base + (mi < M ? mi : M - 1) * K;
    if constexpr (VEC) {
      const Pack<GY, 4> t = *reinterpret_cast<const Pack<GY, 4>*>(p + min(k, K - 4));
#pragma unroll
      for (int j = 0; j < 4; ++j) v[i][j] = (float)t.v[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[i][j] = (float)p[min(k + j, K - 1)];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// T[q][w][f] bit j = wbits[q][f / 64][64 w + j] bit f % 64: one wave per 64 x 64 bit block (grid-stride over the blocks).
// Output features past ceil16(O) read as zero words (their A operand is 0 in the GEMM); columns f < ceil16(F) are written.
__global__ __launch_bounds__(256) void transpose_planes(const unsigned long long* __restrict__ wbits,
                                                        unsigned long long* __restrict__ tbits, int nwf, int opad, int nwo,
                                                        int fpad, long long blocks) {
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * 4;
  for (long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); b < blocks; b += stride) {
    const int fw = (int)(b % nwf);
    const long long t = b / nwf;
    const int ow = (int)(t % nwo);
    const long long q = t / nwo;
    const int o = ow * 64 + lane;
    const unsigned long long w = o < opad ? wbits[(q * nwf + fw) * opad + o] : 0ull;
    unsigned long long out = 0;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      const unsigned long long m = __ballot((int)((w >> i) & 1ull));
      if (lane == i) out = m;
    }
    const int f = fw * 64 + lane;
    if (f < fpad) tbits[(q * nwo + ow) * fpad + f] = out;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
template <int RB, int CB, bool VEC, class GY, class EPI>
__global__ __launch_bounds__(256, 2) void dgrad_tiled(Args<GY, EPI> a) {
  constexpr int BM = 64 * RB;
  constexpr int kRows = BM / 16;                      // staged rows per thread and stage (16 threads x 4 values a row)
  __shared__ __attribute__((aligned(16))) unsigned char s_a[2 * BM * kPitch];    // hi rows [BM], then lo rows [BM]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int col = lane & 31, hh = lane >> 5;
  const int wr = wid >> 1, wc = wid & 1;              // the wave's block of rows / columns in the tile
  const long long m0 = (long long)blockIdx.x * BM;
  const int f0 = blockIdx.y * 64 * CB;
  const int sf = (tid & 15) * 4, sr = tid >> 4;       // staging role: output features sf .. sf + 3 of rows sr + 16 i

  float gr[kRows][4], sc[4];
  unsigned long long wn[1][CB], wcur[1][CB];      // [1]: one accumulator set for all planes (mma_stage<NQ = 1>)
  auto load = [&](int it) {
    const int q = it / a.nwo, st = it - q * a.nwo;
    const int o = st * 64 + sf;
    if constexpr (std::is_same<GY, float>::value) load_rows4<VEC>(a.gy, m0 + sr, a.M, a.O, o, gr);
    else load_rows4_half<VEC>(a.gy, m0 + sr, a.M, a.O, o, gr);
#pragma unroll
    for (int j = 0; j < 4; ++j) sc[j] = a.wscales[(long long)q * a.O + min(o + j, a.O - 1)];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
      const int f = min(f0 + wc * 32 * CB + cb * 32 + col, a.fpad - 1);
      wn[0][cb] = a.tbits[(long long)it * a.fpad + f];
    }
  };
  auto stash = [&](int it) {
    const int q = it / a.nwo, st = it - q * a.nwo;
    const int o = st * 64 + sf;
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      float c[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) c[j] = o + j < a.O ? __fmul_rn(gr[i][j], sc[j]) : 0.f;
      stash_hi_lo(s_a + (sr + 16 * i) * kPitch + sf * 2, BM * kPitch, c);
    }
  };

  f32x16 acc[1][RB][CB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[0][rb][cb][i] = 0.f;

  load(0);
  for (int it = 0; it < a.stages; ++it) {
    __syncthreads();                                  // every wave is done reading the previous stage
    stash(it);
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) wcur[0][cb] = wn[0][cb];
    __syncthreads();
    if (it + 1 < a.stages) load(it + 1);              // in flight during the MFMAs below
    mma_stage(s_a, BM * kPitch, wr * 32 * RB, col, hh, wcur, acc);
  }

  // a lane stores its column's 16 rows of every block, each as it comes through the epilogue (nothing of the epilogue is
  // computed on the whole accumulator array); the sample's row state is fetched again only where the rows reach another sample
  typename EPI::Row er;
  int ern = -1;
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
    const int f = f0 + wc * 32 * CB + cb * 32 + col;
    if (f >= a.F) continue;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const long long m = d_row(m0 + wr * 32 * RB + rb * 32, i, hh);
        if (m >= a.M) continue;
        const int n = a.epi.sample(m);
        if (n != ern) {
          a.epi.row(n, er);
          ern = n;
        }
        a.epi.store(m * a.F + f, er, acc[0][rb][cb][i]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
template <bool VEC, class GY, class EPI>
__global__ __launch_bounds__(64 * kSplitWaves) void dgrad_split(Args<GY, EPI> a) {
  __shared__ float s_red[kSplitWaves][1][16][64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int col = lane & 31, hh = lane >> 5;
  const int f0 = blockIdx.x * 32;
  const long long m0 = (long long)blockIdx.y * 32;
  const int per = (a.stages + kSplitWaves - 1) / kSplitWaves;
  const int i0 = wid * per, i1 = min(a.stages, i0 + per);        // this wave's stages (64 output features of one plane each)
  const long long mr = m0 + col < a.M ? m0 + col : a.M - 1;      // the lane's A row
  const GY* grow = a.gy + mr * a.O;
  const int fw = min(f0 + col, a.fpad - 1);                      // the lane's B column

  f32x16 acc[1];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[0][i] = 0.f;

  float gn[32], sn[32];
  unsigned long long wn;
  auto load = [&](int it) {
    const int q = it / a.nwo, st = it - q * a.nwo;
    const float* ws = a.wscales + (long long)q * a.O;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int o = st * 64 + 16 * s + 8 * hh;
      if constexpr (!VEC) {
#pragma unroll
        for (int j = 0; j < 8; ++j) gn[8 * s + j] = (float)grow[min(o + j, a.O - 1)];
      } else if constexpr (std::is_same<GY, float>::value) {
        const float4 v0 = *reinterpret_cast<const float4*>(grow + min(o, a.O - 4));
        const float4 v1 = *reinterpret_cast<const float4*>(grow + min(o + 4, a.O - 4));
        gn[8 * s + 0] = v0.x; gn[8 * s + 1] = v0.y; gn[8 * s + 2] = v0.z; gn[8 * s + 3] = v0.w;
        gn[8 * s + 4] = v1.x; gn[8 * s + 5] = v1.y; gn[8 * s + 6] = v1.z; gn[8 * s + 7] = v1.w;
      } else {
        const Pack<GY, 8> t = *reinterpret_cast<const Pack<GY, 8>*>(grow + min(o, a.O - 8));
#pragma unroll
        for (int j = 0; j < 8; ++j) gn[8 * s + j] = (float)t.v[j];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) sn[8 * s + j] = ws[min(o + j, a.O - 1)];
    }
    wn = a.tbits[(long long)it * a.fpad + fw];
  };

  if (i0 < i1) load(i0);
  for (int it = i0; it < i1; ++it) {
    float gv[32], sv[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) { gv[j] = gn[j]; sv[j] = sn[j]; }
    const unsigned long long wv = wn;
    const int st = it % a.nwo;
    if (it + 1 < i1) load(it + 1);                    // in flight during the MFMAs below
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int o = st * 64 + 16 * s + 8 * hh;
      float c[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) c[j] = o + j < a.O ? __fmul_rn(gv[8 * s + j], sv[8 * s + j]) : 0.f;
      Frag hi, lo;
#pragma unroll
      for (int d = 0; d < 4; ++d) split_pair(c[2 * d], c[2 * d + 1], hi.u[d], lo.u[d]);
      const Frag bw = expand8((unsigned)(wv >> (16 * s + 8 * hh)));
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hi.v, bw.v, acc[0], 0, 0, 0);
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lo.v, bw.v, acc[0], 0, 0, 0);
    }
  }

  split_reduce(s_red, acc, wid, lane);

  // wave g finishes registers 2 g and 2 g + 1 of the tile: the partial sums added in wave order
  const int f = f0 + col;
  if (f >= a.F) return;
  typename EPI::Row er;
  int ern = -1;
#pragma unroll
  for (int ii = 0; ii < 2; ++ii) {
    const int i = 2 * wid + ii;
    const long long m = m0 + (i & 3) + 8 * (i >> 2) + 4 * hh;       // d_row of lsq_signw_mma.h, written out (see there)
    if (m >= a.M) continue;
    const int n = a.epi.sample(m);
    if (n != ern) {
      a.epi.row(n, er);
      ern = n;
    }
    a.epi.store(m * a.F + f, er, split_sum(s_red, 0, i, lane));
  }
}

// ---- host side: shared by the entry points of both libraries
bool in_limits(int kw_planes, int64_t F, int64_t O) {
  return kw_planes >= 1 && kw_planes <= LSQ_MAX_PLANES && F > 0 && O > 0 && F < (1ll << 22) && O < (1ll << 21);
}

size_t workspace_bytes_of(int kw_planes, int64_t F, int64_t O) {
  if (!in_limits(kw_planes, F, O)) return 0;
  return (size_t)kw_planes * (size_t)((O + 63) / 64) * (size_t)((F + 15) / 16 * 16) * sizeof(unsigned long long);
}

// The checks every entry point makes after its own NULL checks: 0, or the code to return.
int check_call(int kw_planes, int64_t M, int64_t F, int64_t O, const void* workspace, size_t workspace_bytes) {
  if (M <= 0 || F <= 0 || O <= 0) return LSQ_E_SHAPE;
  if (!in_limits(kw_planes, F, O) || M >= (1ll << 31)) return LSQ_E_UNSUPPORTED;
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < workspace_bytes_of(kw_planes, F, O))
    return LSQ_E_WORKSPACE;
  return LSQ_OK;
}

// transpose_planes into the workspace, then the kernel tile_rule(M, F) names: the launches of a call whose operands passed
// check_call.
template <class GY, class EPI>
int launch_dgrad(const GY* gy, const uint64_t* wbits, int kw_planes, const float* wscales, int64_t M, int64_t F, int64_t O,
                 const EPI& epi, void* workspace, hipStream_t st) {
  typedef Args<GY, EPI> A;
  A a = {};
  a.gy = gy;
  a.tbits = (const unsigned long long*)workspace;
  a.wscales = wscales;
  a.epi = epi;
  a.M = M;
  a.F = (int)F;
  a.O = (int)O;
  a.fpad = (int)((F + 15) / 16 * 16);
  a.nwo = (int)((O + 63) / 64);
  a.stages = kw_planes * a.nwo;

  const int nwf = (int)((F + 63) / 64), opad = (int)((O + 15) / 16 * 16);
  const long long blocks = (long long)a.stages * nwf;             // 64 x 64 bit blocks, one wave each
  const long long tgrid = (blocks + 3) / 4;
  hipLaunchKernelGGL(transpose_planes, dim3((unsigned)(tgrid < (1ll << 20) ? tgrid : (1ll << 20))), dim3(256), 0, st,
                     (const unsigned long long*)wbits, (unsigned long long*)workspace, nwf, opad, a.nwo, a.fpad, blocks);
  int e = (int)hipGetLastError();
  if (e) return e;

  // wide gradient loads where every row starts on the load's size (same values, same bits as the per-element loads)
  const TileRule rule = tile_rule(M, F);
  bool vec;
  if (sizeof(GY) == 4) vec = ((uintptr_t)gy & 15) == 0 && O % 4 == 0;
  else if (rule.split) vec = ((uintptr_t)gy & 15) == 0 && O % 8 == 0;
  else vec = ((uintptr_t)gy & 7) == 0 && O % 4 == 0;

  const TileKernels<A> k = {{dgrad_split<false, GY, EPI>, dgrad_split<true, GY, EPI>},
                            {dgrad_tiled<2, 2, false, GY, EPI>, dgrad_tiled<2, 2, true, GY, EPI>},
                            {dgrad_tiled<1, 1, false, GY, EPI>, dgrad_tiled<1, 1, true, GY, EPI>}};
  auto grid = [&](int t) {                            // split: x = columns, y = rows; tiled: x = rows, y = columns
    const unsigned rows = (unsigned)((a.M + t - 1) / t), cols = (unsigned)((a.F + t - 1) / t);
    return t == 32 ? dim3(cols, rows) : dim3(rows, cols);
  };
  return launch_tiles(k, a, rule, vec, grid, st);
}

}  // namespace
