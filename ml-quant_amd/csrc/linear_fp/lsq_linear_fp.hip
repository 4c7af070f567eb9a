// lsq_linear_signw: fp32 activations x sign-weight planes on the bf16 matrix cores of gfx950 (v_mfma_f32_32x32x16_bf16).
//
// As a GEMM:  I_q[m][o] = sum_f c(x[m][f]) s_q[o][f]  per weight plane q, M = rows, K = F features, N = O outputs, then
// y = bias + sum_q ws[q][o] I_q.  Activations are operand A (rows m), weights operand B (columns o), the orientation of
// csrc/linear/lsq_linear.hip: a lane of D holds ONE column o (lane & 31) and 16 rows, so a store instruction writes 32
// consecutive floats of a row of y per half-wave.  Lane (r = lane & 31, h = lane >> 5) holds A[row r][k = 8 h + j] and
// B[k = 8 h + j][col r] in element j = 0..7 of its fragments.
//   * ACTIVATION: clamped (v_med3), split into hi = bf16(v) and lo = bf16(v - hi); two MFMAs per k-step (hi, then lo) into
//     the same fp32 accumulator.  Features past F are staged as 0: they contribute 0 whatever the weight bits hold.
//   * WEIGHT: the 8 sign bits of a lane's fragment (bits 16 s + 8 h .. + 7 of its column's plane word for k-step s) become
//     8 bf16 +-1.0 in registers -- one packed 16-bit shift and one and-or per pair --, so the weight stream stays at one bit
//     per weight (no 16-bit image in memory).  One accumulator per weight plane: ws[q][o] is per column AND plane.
//   * Rows past M and columns past O read a valid row / column and are never stored (a row of D depends only on its row of
//     A, a column only on its column of B).
// Two kernels behind the one entry point (selected from M and O, see lsq_linear_signw):
//   signw_tiled  M x O tiles of 128 x 128 or 64 x 64 over the whole F, four waves (2 x 2); per stage of 64 features the
//                workgroup splits its rows' activations ONCE into LDS (hi and lo rows of 144 bytes: 16-byte pad, conflict-
//                free ds_read_b128 fragments); the next stage's activations and weight words are loaded into registers
//                while the MFMAs of this one run.
//   signw_split  weight-streaming shapes (few rows): one 32 x 32 output tile per workgroup with its F split over 8 waves,
//                each wave reading, splitting and multiplying its own feature range straight from global memory (every x
//                element once per workgroup); the partial sums meet in LDS and are added in wave order.
// Epilogue (both): y = fma(I_q, ws[q][o], base) over the planes in order, base = bias (or 0) at the first launch and the y
// of the previous launch after it (a launch takes one or two planes).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lsq_hip_linear_fp.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) unsigned short u16x2;

union Frag {
  unsigned u[4];
  bf16x8 v;
};

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

constexpr int kPitch = 144;           // LDS bytes per staged row of signw_tiled: 64 bf16 + 16 bytes of pad
constexpr int kSplitWaves = 8;        // waves of signw_split, one feature range each

// v = hi + lo in bf16: hi = bf16(v) (round to nearest even), lo = bf16(v - hi); v - hi is exact in fp32, so
// |v - hi - lo| <= 2^-18 |v|
__device__ __forceinline__ void split_pair(float v0, float v1, unsigned& hi, unsigned& lo) {
  const f32x2 v = {v0, v1};
  const bf16x2 h = __builtin_convertvector(v, bf16x2);
  const f32x2 r = v - __builtin_convertvector(h, f32x2);
  const bf16x2 l = __builtin_convertvector(r, bf16x2);
  hi = __builtin_bit_cast(unsigned, h);
  lo = __builtin_bit_cast(unsigned, l);
}

// 8 sign bits (bit j set = +1) -> B fragment: element j = +-1.0 in bf16, half (j & 1) of dword j >> 1.  The inverted bits
// in both 16-bit halves, one packed shift brings bit 2d / 2d + 1 to the sign position of the low / high half.
__device__ __forceinline__ Frag expand8(unsigned bits) {
  const unsigned short m = (unsigned short)(~bits & 0xFFu);
  const u16x2 rep = {m, m};
  Frag f;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const u16x2 sh = {(unsigned short)(15 - 2 * d), (unsigned short)(14 - 2 * d)};
    const u16x2 s = rep << sh;
    f.u[d] = (__builtin_bit_cast(unsigned, s) & 0x80008000u) | 0x3F803F80u;
  }
  return f;
}

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
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      const long long mi = m0 + sr + 16 * i;
      const float* p = a.x + (mi < a.M ? mi : a.M - 1) * a.F;
      if constexpr (VEC) {
        const float4 v = *reinterpret_cast<const float4*>(p + min(f, a.F - 4));
        xr[i][0] = v.x; xr[i][1] = v.y; xr[i][2] = v.z; xr[i][3] = v.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) xr[i][j] = p[min(f + j, a.F - 1)];
      }
    }
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
      unsigned h0, l0, h1, l1;
      split_pair(c[0], c[1], h0, l0);
      split_pair(c[2], c[3], h1, l1);
      unsigned char* d = s_x + (sr + 16 * i) * kPitch + sf * 2;
      *reinterpret_cast<uint2*>(d) = make_uint2(h0, h1);
      *reinterpret_cast<uint2*>(d + BM * kPitch) = make_uint2(l0, l1);
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
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      Frag ah[RB], al[RB], bw[KP][CB];
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        const unsigned char* r = s_x + (wr * 32 * RB + rb * 32 + col) * kPitch + 32 * s + 16 * hh;
        const uint4 vh = *reinterpret_cast<const uint4*>(r);
        const uint4 vl = *reinterpret_cast<const uint4*>(r + BM * kPitch);
        ah[rb].u[0] = vh.x; ah[rb].u[1] = vh.y; ah[rb].u[2] = vh.z; ah[rb].u[3] = vh.w;
        al[rb].u[0] = vl.x; al[rb].u[1] = vl.y; al[rb].u[2] = vl.z; al[rb].u[3] = vl.w;
      }
#pragma unroll
      for (int q = 0; q < KP; ++q)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) bw[q][cb] = expand8((unsigned)(wcur[q][cb] >> (16 * s + 8 * hh)));
      // hi products of every tile first, then lo: dependent MFMAs on one accumulator are KP * RB * CB apart
#pragma unroll
      for (int q = 0; q < KP; ++q)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
          for (int cb = 0; cb < CB; ++cb)
            acc[q][rb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[rb].v, bw[q][cb].v, acc[q][rb][cb], 0, 0, 0);
#pragma unroll
      for (int q = 0; q < KP; ++q)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
          for (int cb = 0; cb < CB; ++cb)
            acc[q][rb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[rb].v, bw[q][cb].v, acc[q][rb][cb], 0, 0, 0);
    }
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
        const long long m = m0 + wr * 32 * RB + rb * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh;
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
  __shared__ float s_red[kSplitWaves][KP][16][64];    // every wave's partial sums, [register][lane]
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

#pragma unroll
  for (int q = 0; q < KP; ++q)
#pragma unroll
    for (int i = 0; i < 16; ++i) s_red[wid][q][i][lane] = acc[q][i];
  __syncthreads();

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
    const long long m = m0 + (i & 3) + 8 * (i >> 2) + 4 * hh;
    if (m >= a.M) continue;
    float* yp = a.y + m * a.O + o;
    float v = a.accumulate ? *yp : b;
#pragma unroll
    for (int q = 0; q < KP; ++q) {
      float sum = s_red[0][q][i][lane];
#pragma unroll
      for (int w = 1; w < kSplitWaves; ++w) sum += s_red[w][q][i][lane];
      v = fmaf(sum, ws[q], v);
    }
    *yp = v;
  }
}

template <int KP>
int launch(const Args& a, bool split, bool big, bool vec, hipStream_t st) {
  if (split) {
    const dim3 grid((unsigned)((a.O + 31) / 32), (unsigned)((a.M + 31) / 32));
    if (vec) hipLaunchKernelGGL((signw_split<KP, true>), grid, dim3(64 * kSplitWaves), 0, st, a);
    else hipLaunchKernelGGL((signw_split<KP, false>), grid, dim3(64 * kSplitWaves), 0, st, a);
  } else if (big) {
    const dim3 grid((unsigned)((a.M + 127) / 128), (unsigned)((a.O + 127) / 128));
    if (vec) hipLaunchKernelGGL((signw_tiled<KP, 2, 2, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((signw_tiled<KP, 2, 2, false>), grid, dim3(256), 0, st, a);
  } else {
    const dim3 grid((unsigned)((a.M + 63) / 64), (unsigned)((a.O + 63) / 64));
    if (vec) hipLaunchKernelGGL((signw_tiled<KP, 1, 1, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((signw_tiled<KP, 1, 1, false>), grid, dim3(256), 0, st, a);
  }
  return (int)hipGetLastError();
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
  // fewer 64 x 64 tiles than CUs: the weight stream bounds the call, so the F of each 32 x 32 tile is split over 8 waves;
  // 128 x 128 tiles where there are at least 256 of them (one per CU), 64 x 64 otherwise
  const bool split = ((M + 63) / 64) * ((O + 63) / 64) < 256;
  const bool big = ((M + 127) / 128) * ((O + 127) / 128) >= 256;
  hipStream_t st = (hipStream_t)stream;
  for (int q0 = 0; q0 < kw_planes; q0 += 2) {         // planes in pairs: two accumulators share every A fragment
    a.wbits = (const unsigned long long*)wbits + (long long)q0 * a.wplane;
    a.wscales = wscales + (long long)q0 * O;
    a.accumulate = q0 ? 1 : 0;
    const int e = kw_planes - q0 >= 2 ? launch<2>(a, split, big, vec, st) : launch<1>(a, split, big, vec, st);
    if (e) return e;
  }
  return LSQ_OK;
}
