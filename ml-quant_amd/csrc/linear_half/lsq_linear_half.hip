// lsq_linear_signw_half: bf16 / fp16 activations x sign-weight planes on the 16-bit matrix cores of gfx950
// (v_mfma_f32_32x32x16_bf16 / v_mfma_f32_32x32x16_f16).
//
// lsq_linear_signw (csrc/linear_fp/lsq_linear_fp.hip) with an A operand that already is 16-bit: the same GEMM orientation,
// tile rule, kernels and epilogue, but the rows are read as they are (half the bytes), clamped in their own type and used as
// ONE fragment per k-step -- no hi / lo split, one MFMA where that kernel issues two (mma_stage1 of
// csrc/linear/lsq_signw_mma.h).  The weight stream stays at one bit per weight.
//   * ACTIVATION: eight 16-bit values = one 16-byte load (VEC: every row starts on 16 bytes) or eight 2-byte loads; values
//     past F become 0 (they contribute 0 whatever the weight bits hold), then the clamp: bf16 through fp32 (v_med3_f32 of
//     the value shifted up; the bound is a bf16 value, so the result is one), fp16 packed (v_pk_max_f16 / v_pk_min_f16).
//   * Rows past M and columns past O read a valid row / column and are never stored.
//   signw_tiled  M x O tiles of 128 x 128 or 64 x 64 over the whole F, four waves (2 x 2); per stage of 64 features the
//                workgroup puts its rows' clamped activations ONCE into LDS (8 threads x 16 bytes a row); the next stage's
//                activations and weight words are loaded into registers while the MFMAs of this one run.
//   signw_split  weight-streaming shapes: one 32 x 32 output tile per workgroup with its F split over 8 waves, each lane
//                reading its own row's 8 features per k-step straight from global memory; the partial sums meet in LDS
//                and are added in wave order.
// Epilogue (both): v = fma(I_q, ws[q][o], base) over the planes in order in fp32, base = bias (or 0) at the first launch
// and the fp32 sum of the previous launch after it (a launch takes one or two planes); v is stored as fp32 (into y, or
// into the workspace while launches of a 16-bit y remain) or rounded once into the 16-bit y by the last launch.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "lsq_hip_linear_half.h"
#include "../linear/lsq_signw_mma.h"

namespace {

typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;

struct Args {
  const unsigned short* x;            // [M][F], bf16 or fp16 bits
  const unsigned long long* wbits;    // first weight plane of this launch: [nw][opad]
  const float* wscales;               // [.][O], first plane of this launch
  const float* bias;                  // [O] or null
  const float* base;                  // [M][O] fp32 sum of the launches before this one, or null (base = bias or 0)
  void* out;                          // [M][O] of odt
  long long M, wplane;                // rows; words per weight plane (nw * opad)
  int F, O, opad, nw;
  float lim;                          // clamp bound, a value of the activations' type (+inf: identity)
  unsigned lim2;                      // fp16: its bits in both halves
  int odt;                            // LSQ_DTYPE_* of out
};

// two 16-bit activations in a dword, clamped
template <bool F16>
__device__ __forceinline__ unsigned clamp2(unsigned d, const Args& a) {
  if constexpr (F16) {
    const f16x2 v = __builtin_bit_cast(f16x2, d), l = __builtin_bit_cast(f16x2, a.lim2);
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_elementwise_max(v, -l), l));
  } else {
    const float lo = __builtin_amdgcn_fmed3f(__builtin_bit_cast(float, d << 16), -a.lim, a.lim);
    const float hi = __builtin_amdgcn_fmed3f(__builtin_bit_cast(float, d & 0xFFFF0000u), -a.lim, a.lim);
    return (__builtin_bit_cast(unsigned, hi) & 0xFFFF0000u) | (__builtin_bit_cast(unsigned, lo) >> 16);
  }
}

// Eight 16-bit values as they come from memory: one 16-byte load or eight 2-byte loads.
template <bool VEC>
struct Raw8;
template <>
struct Raw8<true> {
  uint4 v;
};
template <>
struct Raw8<false> {
  unsigned short h[8];
};

// values k .. k + 7 of the row p of K values; indices clamped into the row (VEC: K % 8 == 0 and k % 8 == 0)
template <bool VEC>
__device__ __forceinline__ void load8(const unsigned short* p, int K, int k, Raw8<VEC>& r) {
  if constexpr (VEC) {
    r.v = *reinterpret_cast<const uint4*>(p + min(k, K - 8));
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) r.h[j] = p[min(k + j, K - 1)];
  }
}

// -> the A fragment's four dwords: values at k + j >= K are 0, the others clamped
template <bool F16, bool VEC>
__device__ __forceinline__ void finish8(const Raw8<VEC>& r, int K, int k, const Args& a, unsigned (&d)[4]) {
  if constexpr (VEC) {
    const bool in = k < K;
    d[0] = in ? r.v.x : 0u; d[1] = in ? r.v.y : 0u; d[2] = in ? r.v.z : 0u; d[3] = in ? r.v.w : 0u;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned lo = k + 2 * j < K ? r.h[2 * j] : 0u, hi = k + 2 * j + 1 < K ? r.h[2 * j + 1] : 0u;
      d[j] = lo | hi << 16;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) d[j] = clamp2<F16>(d[j], a);
}

// the epilogue's store: fp32, or rounded to nearest even into the 16-bit type (one element: nothing beside it is written)
__device__ __forceinline__ void store_out(const Args& a, long long i, float v) {
  if (a.odt == LSQ_DTYPE_F32) static_cast<float*>(a.out)[i] = v;
  else if (a.odt == LSQ_DTYPE_BF16) static_cast<__bf16*>(a.out)[i] = (__bf16)v;
  else static_cast<_Float16*>(a.out)[i] = (_Float16)v;
}

// ---------------------------------------------------------------------------------------------------------------------
template <bool F16, int KP, int RB, int CB, bool VEC>
__global__ __launch_bounds__(256, 2) void signw_tiled(Args a) {
  constexpr int BM = 64 * RB, BN = 64 * CB;
  constexpr int kRows = BM / 32;                      // staged rows per thread and stage (8 threads x 8 features a row)
  __shared__ __attribute__((aligned(16))) unsigned char s_x[BM * kPitch];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int col = lane & 31, hh = lane >> 5;
  const int wr = wid >> 1, wc = wid & 1;              // the wave's block of rows / columns in the tile
  const long long m0 = (long long)blockIdx.x * BM;
  const int o0 = blockIdx.y * BN;
  const int sf = (tid & 7) * 8, sr = tid >> 3;        // staging role: features sf .. sf + 7 of rows sr + 32 i

  Raw8<VEC> xr[kRows];
  unsigned long long wn[KP][CB], wcur[KP][CB];
  auto load = [&](int st) {
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      const long long mi = m0 + sr + 32 * i;
      load8<VEC>(a.x + (mi < a.M ? mi : a.M - 1) * a.F, a.F, st * 64 + sf, xr[i]);
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
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      unsigned d[4];
      finish8<F16, VEC>(xr[i], a.F, st * 64 + sf, a, d);
      *reinterpret_cast<uint4*>(s_x + (sr + 32 * i) * kPitch + sf * 2) = make_uint4(d[0], d[1], d[2], d[3]);
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
    mma_stage1<F16>(s_x, wr * 32 * RB, col, hh, wcur, acc);
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
        float v = a.base ? a.base[m * a.O + o] : b;
#pragma unroll
        for (int q = 0; q < KP; ++q) v = fmaf(acc[q][rb][cb][i], ws[q], v);
        store_out(a, m * a.O + o, v);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
template <bool F16, int KP, bool VEC>
__global__ __launch_bounds__(64 * kSplitWaves) void signw_split(Args a) {
  __shared__ float s_red[kSplitWaves][KP][16][64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int col = lane & 31, hh = lane >> 5;
  const int o0 = blockIdx.x * 32;
  const long long m0 = (long long)blockIdx.y * 32;
  const int per = (a.nw + kSplitWaves - 1) / kSplitWaves;
  const int w0 = wid * per, w1 = min(a.nw, w0 + per);            // this wave's plane words (64 features each)
  const long long mr = m0 + col < a.M ? m0 + col : a.M - 1;      // the lane's A row
  const unsigned short* xrow = a.x + mr * a.F;
  const int ow = min(o0 + col, a.opad - 1);                      // the lane's B column

  f32x16 acc[KP];
#pragma unroll
  for (int q = 0; q < KP; ++q)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;

  Raw8<VEC> xn[4];
  unsigned long long wn[KP];
  auto load = [&](int w) {
#pragma unroll
    for (int s = 0; s < 4; ++s) load8<VEC>(xrow, a.F, w * 64 + 16 * s + 8 * hh, xn[s]);
#pragma unroll
    for (int q = 0; q < KP; ++q) wn[q] = a.wbits[q * a.wplane + (long long)w * a.opad + ow];
  };

  if (w0 < w1) load(w0);
  for (int w = w0; w < w1; ++w) {
    Raw8<VEC> xv[4];
    unsigned long long wv[KP];
#pragma unroll
    for (int s = 0; s < 4; ++s) xv[s] = xn[s];
#pragma unroll
    for (int q = 0; q < KP; ++q) wv[q] = wn[q];
    if (w + 1 < w1) load(w + 1);                      // in flight during the MFMAs below
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      Frag af;
      finish8<F16, VEC>(xv[s], a.F, w * 64 + 16 * s + 8 * hh, a, af.u);
#pragma unroll
      for (int q = 0; q < KP; ++q)
        acc[q] = mfma16<F16>(af, expand8_as<F16>((unsigned)(wv[q] >> (16 * s + 8 * hh))), acc[q]);
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
    float v = a.base ? a.base[m * a.O + o] : b;
#pragma unroll
    for (int q = 0; q < KP; ++q) v = fmaf(split_sum(s_red, q, i, lane), ws[q], v);
    store_out(a, m * a.O + o, v);
  }
}

template <bool F16, int KP>
int launch(const Args& a, TileRule rule, bool vec, hipStream_t st) {
  const TileKernels<Args> k = {{signw_split<F16, KP, false>, signw_split<F16, KP, true>},
                               {signw_tiled<F16, KP, 2, 2, false>, signw_tiled<F16, KP, 2, 2, true>},
                               {signw_tiled<F16, KP, 1, 1, false>, signw_tiled<F16, KP, 1, 1, true>}};
  auto grid = [&](int t) {                            // split: x = columns, y = rows; tiled: x = rows, y = columns
    const unsigned rows = (unsigned)((a.M + t - 1) / t), cols = (unsigned)((a.O + t - 1) / t);
    return t == 32 ? dim3(cols, rows) : dim3(rows, cols);
  };
  return launch_tiles(k, a, rule, vec, grid, st);
}

bool half_type(int t) { return t == LSQ_DTYPE_BF16 || t == LSQ_DTYPE_F16; }

// v rounded to nearest even into bf16 (v >= 0, finite or +inf), as the float of that value
float round_bf16(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  if ((u & 0x7F800000u) != 0x7F800000u) u += 0x7FFFu + ((u >> 16) & 1u);
  u &= 0xFFFF0000u;
  memcpy(&v, &u, 4);
  return v;
}

}  // namespace

extern "C" int lsq_linear_half_abi_version(void) { return LSQ_LINEAR_HALF_ABI_VERSION; }

// The fp32 running sum of a 16-bit y with more than one launch (two planes a launch) lives in the workspace.
extern "C" int64_t lsq_linear_signw_half_workspace_bytes(int64_t M, int64_t O, int kw_planes, int y_dtype) {
  if (!half_type(y_dtype) || kw_planes <= 2 || M <= 0 || O <= 0) return 0;
  return 4 * M * O;
}

extern "C" int lsq_linear_signw_half(const void* x, int x_dtype, float clamp_alpha, const uint64_t* wbits, int kw_planes,
                                     const float* wscales, const float* bias, int64_t M, int64_t F, int64_t O, void* y,
                                     int y_dtype, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !wbits || !wscales || !y) return LSQ_E_NULL;
  if (M <= 0 || F <= 0 || O <= 0) return LSQ_E_SHAPE;
  if (!half_type(x_dtype) || (y_dtype != LSQ_DTYPE_F32 && y_dtype != x_dtype)) return LSQ_E_UNSUPPORTED;
  if (kw_planes < 1 || kw_planes > LSQ_MAX_PLANES) return LSQ_E_UNSUPPORTED;
  if (F >= (1ll << 22) || M >= (1ll << 31) || O >= (1ll << 21)) return LSQ_E_UNSUPPORTED;
  const size_t need = (size_t)lsq_linear_signw_half_workspace_bytes(M, O, kw_planes, y_dtype);
  if (need && (!workspace || ((uintptr_t)workspace & 3) || workspace_bytes < need)) return LSQ_E_WORKSPACE;
  const bool f16 = x_dtype == LSQ_DTYPE_F16;
  Args a = {};
  a.x = static_cast<const unsigned short*>(x);
  a.bias = bias;
  a.M = M;
  a.F = (int)F;
  a.O = (int)O;
  a.opad = (int)((O + 15) / 16 * 16);
  a.nw = (int)((F + 63) / 64);
  a.wplane = (long long)a.nw * a.opad;
  // the bound rounded to nearest even into the activations' type: what Tensor.clamp does with a 16-bit tensor
  if (!(clamp_alpha >= 0.f)) {
    a.lim = INFINITY;
    a.lim2 = 0x7C007C00u;
  } else if (f16) {
    const _Float16 h = (_Float16)clamp_alpha;         // (above 65504 + half an ulp: +inf, the identity)
    uint16_t hb;
    memcpy(&hb, &h, 2);
    a.lim = (float)h;
    a.lim2 = (uint32_t)hb << 16 | hb;
  } else {
    a.lim = round_bf16(clamp_alpha);
  }
  // 16-byte activation loads where every row starts on 16 bytes (same values, same bits as the 2-byte loads)
  const bool vec = ((uintptr_t)x & 15) == 0 && F % 8 == 0;
  const TileRule rule = tile_rule(M, O);
  hipStream_t st = (hipStream_t)stream;
  float* const sum = need ? static_cast<float*>(workspace) : static_cast<float*>(y);   // the fp32 sum between launches
  for (int q0 = 0; q0 < kw_planes; q0 += 2) {         // planes in pairs: two accumulators share every A fragment
    const bool last = q0 + 2 >= kw_planes;
    a.wbits = (const unsigned long long*)wbits + (long long)q0 * a.wplane;
    a.wscales = wscales + (long long)q0 * O;
    a.base = q0 ? sum : nullptr;
    a.out = last ? y : sum;
    a.odt = last ? y_dtype : LSQ_DTYPE_F32;
    const int kp = kw_planes - q0 >= 2 ? 2 : 1;
    const int e = f16 ? (kp == 2 ? launch<true, 2>(a, rule, vec, st) : launch<true, 1>(a, rule, vec, st))
                      : (kp == 2 ? launch<false, 2>(a, rule, vec, st) : launch<false, 1>(a, rule, vec, st));
    if (e) return e;
  }
  return LSQ_OK;
}
