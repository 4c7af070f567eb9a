// lsq_linear_signw: fp32 activations x sign-weight planes on the bf16 matrix cores of gfx950 (v_mfma_f32_32x32x16_bf16).
//
// As a GEMM:  I_q[m][o] = sum_f c(x[m][f]) s_q[o][f]  per weight plane q, M = rows, K = F features, N = O outputs, then
// y = bias + sum_q ws[q][o] I_q.  Activations are operand A (rows m), weights operand B (columns o), the orientation of
// csrc/linear/lsq_linear.hip; fragment layout, the hi / lo split and the sign-bit expansion: csrc/linear/lsq_signw_mma.h.
//   * ACTIVATION: clamped (v_med3), then split.  Features past F are staged as 0: they contribute 0 whatever the weight
//     bits hold.
//   * WEIGHT: the plane words as lsq_pack_weight wrote them, so the weight stream stays at one bit per weight (no 16-bit
//     image in memory).  One accumulator per weight plane: ws[q][o] is per column AND plane.
//   * Rows past M and columns past O read a valid row / column and are never stored (a row of D depends only on its row of
//     A, a column only on its column of B).
// Two kernels behind the one entry point (selected from M and O, see lsq_linear_signw):
//   signw_tiled  M x O tiles of 128 x 128 or 64 x 64 over the whole F, four waves (2 x 2); per stage of 64 features the
//                workgroup splits its rows' activations ONCE into LDS; the next stage's activations and weight words are
//                loaded into registers while the MFMAs of this one run.
//   signw_split  weight-streaming shapes (few rows): one 32 x 32 output tile per workgroup with its F split over 8 waves,
//                each wave reading, splitting and multiplying its own feature range straight from global memory (every x
//                element once per workgroup); the partial sums meet in LDS and are added in wave order.
// Epilogue (both): y = fma(I_q, ws[q][o], base) over the planes in order, base = bias (or 0) at the first launch and the y
// of the previous launch after it (a launch takes one or two planes).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lsq_hip_linear_fp.h"
#include "../linear/lsq_signw_mma.h"

namespace {

struct Args {
  const float* x;                     // [M][F]
  const unsigned long long* wbits;    // first weight plane of this launch: [nw][opad]
  const float* wscales;               // [.][O], first plane of this launch
  const float* bias;                  // [O] or null
  float* y;                           // [M][O]
  long long M, wplane;                // rows; words per weight plane (nw * opad)
  int F, O, opad, nw;
  float lim;                          // clamp bound (+inf: identity)
  int accumulate;                     // 0: base = bias (or 0); 1: base = y
};

__device__ __forceinline__ float clampv(float v, float lim) { return __builtin_amdgcn_fmed3f(v, -lim, lim); }

// ---------------------------------------------------------------------------------------------------------------------
template <int KP, int RB, int CB, bool VEC>
__global__ __launch_bounds__(256, 2) void signw_tiled(Args a) {
  constexpr int BM = 64 * RB, BN = 64 * CB;
  constexpr int kRows = BM / 16;                      // staged rows per thread and stage (16 threads x 4 features a row)
  __shared__ __attribute__((aligned(16))) unsigned char s_x[2 * BM * kPitch];    // hi rows [BM], then lo rows [BM]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int col = lane & 31, hh = lane >> 5;
  const int wr = wid >> 1, wc = wid & 1;              // the wave's block of rows / columns in the tile
  const long long m0 = (long long)blockIdx.x * BM;
  const int o0 = blockIdx.y * BN;
  const int sf = (tid & 15) * 4, sr = tid >> 4;       // staging role: features sf .. sf + 3 of rows sr + 16 i

  float xr[kRows][4];
  unsigned long long wn[KP][CB], wcur[KP][CB];
  auto load = [&](int st) {
    const int f = st * 64 + sf;
    load_rows4<VEC>(a.x, m0 + sr, a.M, a.F, f, xr);
#pragma unroll
    for (int q = 0; q < KP; ++q)
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        const int o = min(o0 + wc * 32 * CB + cb * 32 + col, a.opad - 1);
        wn[q][cb] = a.wbits[q * a.wplane + (long long)st * a.opad + o];
      }
  };
  auto stash = [&](int st) {
    const int f = st * 64 + sf;
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      float c[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) c[j] = f + j < a.F ? clampv(xr[i][j], a.lim) : 0.f;
      stash_hi_lo(s_x + (sr + 16 * i) * kPitch + sf * 2, BM * kPitch, c);
    }
  };

  f32x16 acc[KP][RB][CB];
#pragma unroll
  for (int q = 0; q < KP; ++q)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[q][rb][cb][i] = 0.f;

  load(0);
  for (int st = 0; st < a.nw; ++st) {
    __syncthreads();                                  // every wave is done reading the previous stage
    stash(st);
#pragma unroll
    for (int q = 0; q < KP; ++q)
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) wcur[q][cb] = wn[q][cb];
    __syncthreads();
    if (st + 1 < a.nw) load(st + 1);                  // in flight during the MFMAs below
    mma_stage(s_x, BM * kPitch, wr * 32 * RB, col, hh, wcur, acc);
  }

#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
    const int o = o0 + wc * 32 * CB + cb * 32 + col;
    if (o >= a.O) continue;
    float ws[KP];
#pragma unroll
    for (int q = 0; q < KP; ++q) ws[q] = a.wscales[(long long)q * a.O + o];
    const float b = a.bias ? a.bias[o] : 0.f;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const long long m = d_row(m0 + wr * 32 * RB + rb * 32, i, hh);
        if (m >= a.M) continue;
        float* yp = a.y + m * a.O + o;
        float v = a.accumulate ? *yp : b;
#pragma unroll
        for (int q = 0; q < KP; ++q) v = fmaf(acc[q][rb][cb][i], ws[q], v);
        *yp = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
template <int KP, bool VEC>
__global__ __launch_bounds__(64 * kSplitWaves) void signw_split(Args a) {
  __shared__ float s_red[kSplitWaves][KP][16][64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int col = lane & 31, hh = lane >> 5;
  const int o0 = blockIdx.x * 32;
  const long long m0 = (long long)blockIdx.y * 32;
  const int per = (a.nw + kSplitWaves - 1) / kSplitWaves;
  const int w0 = wid * per, w1 = min(a.nw, w0 + per);            // this wave's plane words (64 features each)
  const long long mr = m0 + col < a.M ? m0 + col : a.M - 1;      // the lane's A row
  const float* xrow = a.x + mr * a.F;
  const int ow = min(o0 + col, a.opad - 1);                      // the lane's B column

  f32x16 acc[KP];
#pragma unroll
  for (int q = 0; q < KP; ++q)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;

  float xn[32];
  unsigned long long wn[KP];
  auto load = [&](int w) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int f = w * 64 + 16 * s + 8 * hh;
      if constexpr (VEC) {
        const float4 v0 = *reinterpret_cast<const float4*>(xrow + min(f, a.F - 4));
        const float4 v1 = *reinterpret_cast<const float4*>(xrow + min(f + 4, a.F - 4));
        xn[8 * s + 0] = v0.x; xn[8 * s + 1] = v0.y; xn[8 * s + 2] = v0.z; xn[8 * s + 3] = v0.w;
        xn[8 * s + 4] = v1.x; xn[8 * s + 5] = v1.y; xn[8 * s + 6] = v1.z; xn[8 * s + 7] = v1.w;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) xn[8 * s + j] = xrow[min(f + j, a.F - 1)];
      }
    }
#pragma unroll
    for (int q = 0; q < KP; ++q) wn[q] = a.wbits[q * a.wplane + (long long)w * a.opad + ow];
  };

  if (w0 < w1) load(w0);
  for (int w = w0; w < w1; ++w) {
    float xv[32];
    unsigned long long wv[KP];
#pragma unroll
    for (int j = 0; j < 32; ++j) xv[j] = xn[j];
#pragma unroll
    for (int q = 0; q < KP; ++q) wv[q] = wn[q];
    if (w + 1 < w1) load(w + 1);                      // in flight during the MFMAs below
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int f = w * 64 + 16 * s + 8 * hh;
      float c[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) c[j] = f + j < a.F ? clampv(xv[8 * s + j], a.lim) : 0.f;
      Frag hi, lo;
#pragma unroll
      for (int d = 0; d < 4; ++d) split_pair(c[2 * d], c[2 * d + 1], hi.u[d], lo.u[d]);
#pragma unroll
      for (int q = 0; q < KP; ++q) {
        const Frag bw = expand8((unsigned)(wv[q] >> (16 * s + 8 * hh)));
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hi.v, bw.v, acc[q], 0, 0, 0);
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lo.v, bw.v, acc[q], 0, 0, 0);
      }
    }
  }

  split_reduce(s_red, acc, wid, lane);

  // wave g finishes registers 2 g and 2 g + 1 of the tile: the partial sums added in wave order, then the epilogue
  const int o = o0 + col;
  if (o >= a.O) return;
  float ws[KP];
#pragma unroll
  for (int q = 0; q < KP; ++q) ws[q] = a.wscales[(long long)q * a.O + o];
  const float b = a.bias ? a.bias[o] : 0.f;
#pragma unroll
  for (int ii = 0; ii < 2; ++ii) {
    const int i = 2 * wid + ii;
    const long long m = m0 + (i & 3) + 8 * (i >> 2) + 4 * hh;       // d_row of lsq_signw_mma.h, written out (see there)
    if (m >= a.M) continue;
    float* yp = a.y + m * a.O + o;
    float v = a.accumulate ? *yp : b;
#pragma unroll
    for (int q = 0; q < KP; ++q) v = fmaf(split_sum(s_red, q, i, lane), ws[q], v);
    *yp = v;
  }
}

template <int KP>
int launch(const Args& a, TileRule rule, bool vec, hipStream_t st) {
  const TileKernels<Args> k = {{signw_split<KP, false>, signw_split<KP, true>},
                               {signw_tiled<KP, 2, 2, false>, signw_tiled<KP, 2, 2, true>},
                               {signw_tiled<KP, 1, 1, false>, signw_tiled<KP, 1, 1, true>}};
  auto grid = [&](int t) {                            // split: x = columns, y = rows; tiled: x = rows, y = columns
    const unsigned rows = (unsigned)((a.M + t - 1) / t), cols = (unsigned)((a.O + t - 1) / t);
    return t == 32 ? dim3(cols, rows) : dim3(rows, cols);
  };
  return launch_tiles(k, a, rule, vec, grid, st);
}

}  // namespace

extern "C" int lsq_linear_fp_abi_version(void) { return LSQ_LINEAR_FP_ABI_VERSION; }

extern "C" int lsq_linear_signw(const float* x, float clamp_alpha, const uint64_t* wbits, int kw_planes,
                                const float* wscales, const float* bias, int64_t M, int64_t F, int64_t O, float* y,
                                void* stream) {
  if (!x || !wbits || !wscales || !y) return LSQ_E_NULL;
  if (M <= 0 || F <= 0 || O <= 0) return LSQ_E_SHAPE;
  if (kw_planes < 1 || kw_planes > LSQ_MAX_PLANES) return LSQ_E_UNSUPPORTED;
  if (F >= (1ll << 22) || M >= (1ll << 31) || O >= (1ll << 21)) return LSQ_E_UNSUPPORTED;
  Args a = {};
  a.x = x;
  a.bias = bias;
  a.y = y;
  a.M = M;
  a.F = (int)F;
  a.O = (int)O;
  a.opad = (int)((O + 15) / 16 * 16);
  a.nw = (int)((F + 63) / 64);
  a.wplane = (long long)a.nw * a.opad;
  a.lim = clamp_alpha >= 0.f ? clamp_alpha : INFINITY;
  // 16-byte activation loads where every row starts on 16 bytes (same values, same bits as the 4-byte loads)
  const bool vec = ((uintptr_t)x & 15) == 0 && F % 4 == 0;
  const TileRule rule = tile_rule(M, O);
  hipStream_t st = (hipStream_t)stream;
  for (int q0 = 0; q0 < kw_planes; q0 += 2) {         // planes in pairs: two accumulators share every A fragment
    a.wbits = (const unsigned long long*)wbits + (long long)q0 * a.wplane;
    a.wscales = wscales + (long long)q0 * O;
    a.accumulate = q0 ? 1 : 0;
    const int e = kw_planes - q0 >= 2 ? launch<2>(a, rule, vec, st) : launch<1>(a, rule, vec, st);
    if (e) return e;
  }
  return LSQ_OK;
}
