// The weight gradient of QuantLinear with binary activations as one set of kernels, instantiated by liblsq_hip_linear_wgrad.so
// (lsq_linear_signx_wgrad: fp32 gradients and input, plain fp32 stores) and by liblsq_hip_linear_wgrad_half.so
// (lsq_linear_signx_wgrad_half: bf16 / fp16 gradients and input converted exactly to fp32 as they are read, optionally the
// straight-through estimator of the weight quantizer in the epilogue).  Templated on the element type GY of gy and x and on an
// epilogue EPI; the sign image, the tile rule, staging and the order of summation do not depend on either, so every
// instantiation computes the same fp32 accumulators.  Each library compiles its own copy (anonymous namespace); neither links
// the other's objects.
//   EPI:  struct Row;                                             what the epilogue keeps per output feature (its weight scales)
//         void row(int o, Row&) const;                            called once per stored row o < O of a lane
//         float operand(long long i) const;                       what the epilogue reads at element i = o F + f; o < O, f < F
//         void store(long long i, const Row&, float acc, float operand) const;   element i of the output = f(acc, operand)
//
// fp32 gradient rows (transposed) x the sign planes of the quantized input with the sum over the ROWS, on the bf16 matrix
// cores of gfx950 (v_mfma_f32_32x32x16_bf16).
//
// As a GEMM:  gwq[o][f] = sum_p sum_m (gy[m][o] xs[p][m / T]) b_p[m][f],  D rows = O output features, K = M rows (per
// plane), D columns = F input features; fragment layout, the hi / lo split and the sign-bit expansion:
// csrc/linear/lsq_signw_mma.h.
//   * INPUT: a first kernel (sign_image) walks x row-major and writes X[p][ceil(M / 64)][ceil16(F)]: bit j of word
//     [p][w][f] = the chain's sign b_p at row 64 w + j, feature f.  A lane owns one feature and ORs the bits of 64 rows into
//     its kx words -- the layout the GEMM wants is the natural one, no ballot, no LDS.  After it a lane's B fragment is 8
//     consecutive bits of one word of its column.  One feature a lane for every element type: a wave reads 256 (fp32) or 128
//     (16-bit) consecutive bytes of a row, single-element loads that any element-aligned address and any F serve.
//   * GRADIENT: a = fl32(gy xs[p][m / T]) -- the scale is per (plane, k), so it goes into A and all planes add into ONE
//     accumulator --, then split.  The A fragment is 8 consecutive m of one o while gy is contiguous in o: the tile goes
//     through LDS transposed.  Rows past M are staged as 0 (their image bits are 0 and would read as -1).
//   * Output features past O and columns past F read a valid row / column and are never stored; the epilogue is handed
//     o < O and f < F only.
// Three kernels behind the one entry point (selected from O and F, tile_rule):
//   sign_image   one wave per 64 rows x 64 features.
//   wgrad_tiled  O x F tiles of 128 x 128 or 64 x 64, four waves (2 x 2), over ceil(M / 64) * kx stages (word-major, the
//                planes of a word inside it: the gradient rows of a word are loaded ONCE for all planes); per stage the
//                workgroup scales and splits its gradient tile into LDS, o-major.  A staging thread holds rows m, m + 1 of
//                four output features and stores four packed bf16 pairs; the lanes of a half-wave are 2 groups of four
//                output features x 16 row pairs, which puts the 32 stores of an instruction on 32 different banks.  The
//                next stage's gradients, scales and image words are loaded into registers while the MFMAs of this one run.
//   wgrad_split  few tiles (LeNet fc1, the ResNet head): one 32 x 32 tile of gwq per workgroup, the (word, plane, 16-row
//                step) units split over 8 waves, each reading, scaling, splitting and multiplying its own range straight from
//                global memory; the partial sums meet in LDS and are added in wave order.
// VEC (wgrad_tiled): a staging thread's four output features of a row in one load -- fp32: 16 bytes where gy is 16-byte
// aligned and O % 4 == 0; 16-bit: 8 bytes where gy is 8-byte aligned and O % 4 == 0 (every row then starts on the load's size
// and O >= 4, so min(o, O - 4) stays inside the row).  Otherwise one load per element, each index clamped to O - 1: the same
// values, the same bits.  wgrad_split and sign_image read single elements only.

#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "lsq_hip.h"
#include "../linear/lsq_signw_mma.h"

namespace {

// plain fp32 stores: lsq_linear_signx_wgrad, and lsq_linear_signx_wgrad_half without w
struct EpiStore {
  float* out;                         // [O][F]
  struct Row {};
  __device__ __forceinline__ void row(int, Row&) const {}
  __device__ __forceinline__ float operand(long long) const { return 0.f; }
  __device__ __forceinline__ void store(long long i, const Row&, float acc, float) const { out[i] = acc; }
};

template <class GY, class EPI>
struct Args {
  const GY* gy;                       // [M][O]
  const unsigned long long* img;      // sign image [kx][nwm][fpad]
  const float* xscales;               // [kx][N]
  EPI epi;                            // the output [O][F] and what becomes of an accumulator
  int M, N, T, F, O, kx, fpad, nwm;   // fpad = ceil16(F); nwm = ceil(M / 64)
  int ntf;                            // wgrad_split: tiles of 32 columns
};

template <class GY, int N>
struct alignas(N * sizeof(GY)) Pack {
  GY v[N];
};

// Values o .. o + 3 of the row p of O elements as fp32 (exact): VEC = one 16-byte (fp32) or 8-byte (16-bit) load, which the
// caller grants only where every row starts on that size and O % 4 == 0.
template <bool VEC, class GY>
__device__ __forceinline__ void load4(const GY* p, int o, int O, float (&v)[4]) {
  if constexpr (!VEC) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (float)p[min(o + j, O - 1)];
  } else if constexpr (std::is_same<GY, float>::value) {
    const float4 t = *reinterpret_cast<const float4*>(p + min(o, O - 4));
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    const Pack<GY, 4> t = *reinterpret_cast<const Pack<GY, 4>*>(p + min(o, O - 4));
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (float)t.v[j];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// X[p][w][f] bit j = [d_p >= 0] of the quantizer chain at row 64 w + j, feature f (lsq_ste.hip: ste_one): one wave per
// block of 64 rows x 64 features (grid-stride over the blocks).  Rows >= M and features >= F leave zero bits; the words of
// columns f < ceil16(F) are written.
template <class GY>
__global__ __launch_bounds__(256) void sign_image(const GY* __restrict__ x, const float* __restrict__ xs,
                                                  unsigned long long* __restrict__ img, int kx, float alpha, int M, int N,
                                                  int T, int F, int fpad, int nwm, int nwf, long long blocks) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long stride = (long long)gridDim.x * 4;
  for (long long b = (long long)blockIdx.x * 4 + wave; b < blocks; b += stride) {
    const int fw = (int)(b % nwf);
    const int w = (int)(b / nwf);
    const int f = fw * 64 + lane;
    const bool live = f < F;
    const GY* __restrict__ xcol = x + (live ? f : 0);
    unsigned long long word[LSQ_MAX_PLANES];
#pragma unroll
    for (int i = 0; i < LSQ_MAX_PLANES; ++i) word[i] = 0ull;
    const int mb = w * 64;
    int n = T == 1 ? mb : mb / T;
    int rem = mb - n * T;
    for (int j0 = 0; j0 < 64 && mb + j0 < M; j0 += 8) {
      float xv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int m = min(mb + j0 + j, M - 1);
        xv[j] = (float)xcol[(long long)m * F];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (mb + j0 + j < M) {
          const float xc = alpha >= 0.f ? fminf(fmaxf(xv[j], -alpha), alpha) : xv[j];
          float r = 0.f;
#pragma unroll
          for (int i = 0; i < LSQ_MAX_PLANES; ++i) {
            if (i < kx) {
              const float v = xs[(long long)i * N + n];
              const float d = xc - r;
              const bool pos = d >= 0.f;                           // sign(+-0) = +1
              word[i] |= (unsigned long long)pos << (j0 + j);
              r = r + v * (pos ? 1.f : -1.f);
            }
          }
          if (++rem == T) { rem = 0; ++n; }
        }
      }
    }
    if (f < fpad) {
#pragma unroll
      for (int i = 0; i < LSQ_MAX_PLANES; ++i)
        if (i < kx) img[((long long)i * nwm + w) * fpad + f] = live ? word[i] : 0ull;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// (the element-load variant of the 128 x 128 tile keeps 32 clamped addresses live: one workgroup per CU, no scratch)
template <int RB, int CB, bool VEC, class GY, class EPI>
__global__ __launch_bounds__(256, (RB == 2 && !VEC) ? 1 : 2) void wgrad_tiled(Args<GY, EPI> a) {
  constexpr int BO = 64 * RB;
  constexpr int kPass = BO / 32;                      // wave tasks (16 output features x 32 rows) per wave and stage
  __shared__ __attribute__((aligned(16))) unsigned char s_a[2 * BO * kPitch];    // hi rows [BO], then lo rows [BO]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int col = lane & 31, hh = lane >> 5;
  const int wr = wid >> 1, wc = wid & 1;              // the wave's block of rows / columns in the tile
  const int f0 = blockIdx.x * 64 * CB;
  const int o0 = blockIdx.y * BO;
  // staging role: four output features (sq) and one pair of rows (sp) of every task; a half-wave = 2 quads x 16 pairs
  const int sq = ((lane & 1) + 2 * hh) * 4, sp = (lane >> 1) & 15;

  float gr[kPass][2][4], sc[kPass][2];
  unsigned long long wn[1][CB], wcur[1][CB];      // [1]: one accumulator set for all planes (mma_stage<NQ = 1>)
  auto load_g = [&](int w) {
#pragma unroll
    for (int i = 0; i < kPass; ++i) {
      const int t = wid + 4 * i;
      const int o = o0 + (t >> 1) * 16 + sq;
      const int m = w * 64 + (t & 1) * 32 + 2 * sp;
#pragma unroll
      for (int e = 0; e < 2; ++e) load4<VEC>(a.gy + (long long)min(m + e, a.M - 1) * a.O, o, a.O, gr[i][e]);
    }
  };
  auto load_sw = [&](int w, int p) {
#pragma unroll
    for (int i = 0; i < kPass; ++i) {
      const int t = wid + 4 * i;
      const int m = w * 64 + (t & 1) * 32 + 2 * sp;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int mm = min(m + e, a.M - 1);
        sc[i][e] = a.xscales[(long long)p * a.N + (a.T == 1 ? mm : mm / a.T)];
      }
    }
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
      const int f = min(f0 + wc * 32 * CB + cb * 32 + col, a.fpad - 1);
      wn[0][cb] = a.img[((long long)p * a.nwm + w) * a.fpad + f];
    }
  };
  auto stash = [&](int w) {
#pragma unroll
    for (int i = 0; i < kPass; ++i) {
      const int t = wid + 4 * i;
      const int ol = (t >> 1) * 16 + sq;
      const int mp = (t & 1) * 16 + sp;
      const int m = w * 64 + 2 * mp;
      unsigned char* d = s_a + ol * kPitch + mp * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float c0 = m < a.M ? __fmul_rn(gr[i][0][j], sc[i][0]) : 0.f;
        const float c1 = m + 1 < a.M ? __fmul_rn(gr[i][1][j], sc[i][1]) : 0.f;
        unsigned h, l;
        split_pair(c0, c1, h, l);
        *reinterpret_cast<unsigned*>(d + j * kPitch) = h;
        *reinterpret_cast<unsigned*>(d + j * kPitch + BO * kPitch) = l;
      }
    }
  };

  f32x16 acc[1][RB][CB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[0][rb][cb][i] = 0.f;

  load_g(0);
  load_sw(0, 0);
  for (int w = 0; w < a.nwm; ++w) {
    for (int p = 0; p < a.kx; ++p) {
      __syncthreads();                                // every wave is done reading the previous stage
      stash(w);
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) wcur[0][cb] = wn[0][cb];
      __syncthreads();
      if (p + 1 < a.kx) {                             // in flight during the MFMAs below
        load_sw(w, p + 1);
      } else if (w + 1 < a.nwm) {
        load_g(w + 1);
        load_sw(w + 1, 0);
      }
      mma_stage(s_a, BO * kPitch, wr * 32 * RB, col, hh, wcur, acc);
    }
  }

  // a lane stores its columns' element of each of its 16 rows of every block, each as it comes through the epilogue.  The
  // epilogue's operands (nothing for the plain store) are addressed only behind the o < O and f < F guards, and they are
  // loaded AHEAD of the stores they could alias for the compiler: a block's operands all at once, a row's state while the row
  // before it is stored.
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    const int ob = o0 + wr * 32 * RB + rb * 32;
    float ov[16][CB];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int o = d_row(ob, i, hh);
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        const int f = f0 + wc * 32 * CB + cb * 32 + col;
        ov[i][cb] = (o < a.O && f < a.F) ? a.epi.operand((long long)o * a.F + f) : 0.f;
      }
    }
    typename EPI::Row er, en;
    if (d_row(ob, 0, hh) < a.O) a.epi.row(d_row(ob, 0, hh), en);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int o = d_row(ob, i, hh);
      if (o >= a.O) continue;
      er = en;
      if (i + 1 < 16 && d_row(ob, i + 1, hh) < a.O) a.epi.row(d_row(ob, i + 1, hh), en);
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        const int f = f0 + wc * 32 * CB + cb * 32 + col;
        if (f >= a.F) continue;
        a.epi.store((long long)o * a.F + f, er, acc[0][rb][cb][i], ov[i][cb]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
template <class GY, class EPI>
__global__ __launch_bounds__(64 * kSplitWaves) void wgrad_split(Args<GY, EPI> a) {
  __shared__ float s_red[kSplitWaves][1][16][64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int col = lane & 31, hh = lane >> 5;
  const int f0 = ((int)blockIdx.x % a.ntf) * 32;
  const int o0 = ((int)blockIdx.x / a.ntf) * 32;
  const int units = a.nwm * a.kx * 4;                 // (word, plane, 16-row step), in this order
  const int per = (units + kSplitWaves - 1) / kSplitWaves;
  const int u0 = wid * per, u1 = min(units, u0 + per);
  const GY* gcol = a.gy + min(o0 + col, a.O - 1);     // the lane's A row (an output feature)
  const int fl = min(f0 + col, a.fpad - 1);           // the lane's B column
  const unsigned char* bytes = reinterpret_cast<const unsigned char*>(a.img);

  f32x16 acc[1];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[0][i] = 0.f;

  float gn[8], sn[8];
  unsigned bn = 0;
  int mbn = 0;
  int w = 0, p = 0, s = 0;                            // the unit `load` reads next
  if (u0 < u1) {
    w = u0 / (4 * a.kx);
    const int rest = u0 - w * 4 * a.kx;
    p = rest >> 2;
    s = rest & 3;
  }
  auto load = [&]() {
    const int mb = w * 64 + 16 * s + 8 * hh;
    const int mc = min(mb, a.M - 1);
    int n = a.T == 1 ? mc : mc / a.T;
    int rem = mc - n * a.T;
    const float* xs = a.xscales + (long long)p * a.N;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      gn[j] = (float)gcol[(long long)min(mb + j, a.M - 1) * a.O];
      sn[j] = xs[min(n, a.N - 1)];
      if (++rem == a.T) { rem = 0; ++n; }
    }
    bn = bytes[(((long long)p * a.nwm + w) * a.fpad + fl) * 8 + 2 * s + hh];
    mbn = mb;
    if (++s == 4) {
      s = 0;
      if (++p == a.kx) { p = 0; ++w; }
    }
  };

  if (u0 < u1) load();
  for (int u = u0; u < u1; ++u) {
    float c[8];
    const int mb = mbn;
#pragma unroll
    for (int j = 0; j < 8; ++j) c[j] = mb + j < a.M ? __fmul_rn(gn[j], sn[j]) : 0.f;
    const Frag bw = expand8(bn);
    if (u + 1 < u1) load();                           // in flight during the MFMAs below
    Frag hi, lo;
#pragma unroll
    for (int d = 0; d < 4; ++d) split_pair(c[2 * d], c[2 * d + 1], hi.u[d], lo.u[d]);
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hi.v, bw.v, acc[0], 0, 0, 0);
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lo.v, bw.v, acc[0], 0, 0, 0);
  }

  split_reduce(s_red, acc, wid, lane);

  // wave g finishes registers 2 g and 2 g + 1 of the tile: the partial sums added in wave order.  The epilogue's operands
  // are addressed only behind the f < F and o < O guards.
  const int f = f0 + col;
  if (f >= a.F) return;
  const int i0 = 2 * wid;
  const int oa = o0 + (i0 & 3) + 8 * (i0 >> 2) + 4 * hh;      // d_row of lsq_signw_mma.h, written out (see there)
  const int ob = oa + 1;                                      // (register 2 wid + 1: the next row)
  typename EPI::Row ra, rb;
  float va = 0.f, vb = 0.f;
  if (oa < a.O) {
    a.epi.row(oa, ra);
    va = a.epi.operand((long long)oa * a.F + f);
  }
  if (ob < a.O) {
    a.epi.row(ob, rb);
    vb = a.epi.operand((long long)ob * a.F + f);
  }
  if (oa < a.O) a.epi.store((long long)oa * a.F + f, ra, split_sum(s_red, 0, i0, lane), va);
  if (ob < a.O) a.epi.store((long long)ob * a.F + f, rb, split_sum(s_red, 0, i0 + 1, lane), vb);
}

// ---- host side: shared by the entry points of both libraries
bool in_limits(int kx, int64_t N, int64_t T, int64_t F, int64_t O) {
  return kx >= 1 && kx <= LSQ_MAX_PLANES && N > 0 && T > 0 && F > 0 && O > 0 && N <= 65535 && T < (1ll << 31) &&
         N * T < (1ll << 31) && F < (1ll << 22) && O < (1ll << 21);
}

size_t workspace_bytes_of(int kx, int64_t N, int64_t T, int64_t F, int64_t O) {
  if (!in_limits(kx, N, T, F, O)) return 0;
  return (size_t)kx * (size_t)((N * T + 63) / 64) * (size_t)((F + 15) / 16 * 16) * sizeof(unsigned long long);
}

// The checks every entry point makes after its own NULL checks: 0, or the code to return.
int check_call(int kx, int64_t N, int64_t T, int64_t F, int64_t O, const void* workspace, size_t workspace_bytes) {
  if (N <= 0 || T <= 0 || F <= 0 || O <= 0) return LSQ_E_SHAPE;
  if (!in_limits(kx, N, T, F, O)) return LSQ_E_UNSUPPORTED;
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < workspace_bytes_of(kx, N, T, F, O)) return LSQ_E_WORKSPACE;
  return LSQ_OK;
}

template <class GY, class EPI>
int launch(const Args<GY, EPI>& a, TileRule rule, bool vec, hipStream_t st) {
  typedef Args<GY, EPI> A;
  const TileKernels<A> k = {{wgrad_split<GY, EPI>, wgrad_split<GY, EPI>},
                            {wgrad_tiled<2, 2, false, GY, EPI>, wgrad_tiled<2, 2, true, GY, EPI>},
                            {wgrad_tiled<1, 1, false, GY, EPI>, wgrad_tiled<1, 1, true, GY, EPI>}};
  auto grid = [&](int t) {                            // split: the tiles in x, columns fastest; tiled: x = columns, y = rows
    const unsigned rows = (unsigned)((a.O + t - 1) / t), cols = (unsigned)((a.F + t - 1) / t);
    return t == 32 ? dim3((unsigned)a.ntf * rows) : dim3(cols, rows);
  };
  return launch_tiles(k, a, rule, vec, grid, st);
}

// sign_image into the workspace, then the kernel tile_rule(O, F) names: the launches of a call whose operands passed
// check_call.
template <class GY, class EPI>
int launch_wgrad(const GY* gy, const GY* x, int kx, const float* xscales, float clamp_alpha, int64_t N, int64_t T, int64_t F,
                 int64_t O, const EPI& epi, void* workspace, hipStream_t st) {
  Args<GY, EPI> a = {};
  a.gy = gy;
  a.img = (const unsigned long long*)workspace;
  a.xscales = xscales;
  a.epi = epi;
  a.M = (int)(N * T);
  a.N = (int)N;
  a.T = (int)T;
  a.F = (int)F;
  a.O = (int)O;
  a.kx = kx;
  a.fpad = (int)((F + 15) / 16 * 16);
  a.nwm = (a.M + 63) / 64;
  a.ntf = (a.F + 31) / 32;

  const int nwf = (a.F + 63) / 64;
  const long long blocks = (long long)a.nwm * nwf;                // blocks of 64 rows x 64 features, one wave each
  const long long sgrid = (blocks + 3) / 4;
  hipLaunchKernelGGL(sign_image<GY>, dim3((unsigned)(sgrid < (1ll << 20) ? sgrid : (1ll << 20))), dim3(256), 0, st, x, xscales,
                     (unsigned long long*)workspace, kx, clamp_alpha, a.M, a.N, a.T, a.F, a.fpad, a.nwm, nwf, blocks);
  int e = (int)hipGetLastError();
  if (e) return e;

  // wide gradient loads where every row starts on the load's size (same values, same bits as the per-element loads)
  const bool vec = ((uintptr_t)gy & (4 * sizeof(GY) - 1)) == 0 && O % 4 == 0;
  return launch(a, tile_rule(O, F), vec, st);
}

}  // namespace
