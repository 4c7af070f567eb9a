// lsq_linear_xnor: binary x binary linear layer on the fp4 matrix cores of gfx950 (v_mfma_scale_f32_32x32x64_f8f6f4).
//
// As a GEMM:  D_pq[m][o] = sum_f a_p[m][f] w_q[o][f]  over the sign planes, M = rows, K = F features, N = O outputs.
// One uint64 plane word is the K = 64 of one MFMA row: lane (r = lane & 31, h = lane >> 5) holds k-slots 32 h + 4 j + q in
// nibble j of register q, for both operands (the convention of csrc/lsq_xnor_mfma.hip, "FP4"; known-answer test
// scripts/ubench/fp4_mfma_check.hip).
//   * ACTIVATION (operand A, rows m): the bit becomes an indicator code with one v_and_b32 per 8 channels: registers
//     d & 0x11111111, d & 0x22222222, d & 0x44444444, (d >> 3) & 0x11111111 hold 0 or 0.5 / 1 / 2 / 0.5 (E2M1 codes 1, 2, 4, 1).
//   * WEIGHT (operand B, columns o): the nibble of the same slot is +-(4, 2, 1, 4) -- sign bit 8 where the weight is -1 --,
//     so every product is +-2 or 0 and the accumulator sums 2 sum_f w_f [a_f = 1].
//   * Started at -wsum[q][o] = -sum_f w_f, the fp32 accumulator ends at I = 2 sum_f w_f [a_f = 1] - sum_f w_f = sum_f a_f w_f,
//     and every partial sum is an integer of magnitude below 3 F < 2^24: exact in any order for F < 2^22.  Channels past F
//     have activation bit 0 (lsq_act_quant writes them so) and contribute 0 whatever the weight bits hold; the words past
//     the end of K and the rows / columns past the matrix are staged as zeros.
// Epilogue: the fp32 arithmetic of the popcount kernel (csrc/lsq_xnor_conv.hip) in its order -- one launch per weight plane
// q and pair of activation planes (p0, p0 + 1), v = xs[p0] I_p0q (+ fma xs[p0 + 1] I_(p0+1)q), y = fma(v, ws[q][o], base)
// with base = bias (or 0) at the first launch and the y of the previous launch after it -- so y is bit for bit what
// lsq_xnor_conv2d returns for the 1x1 convolution over (M, F, 1, 1).
//
// Tiles: a workgroup of four waves (2 x 2) owns BM = 64 RB rows x BN = 64 CB columns; a wave owns RB x CB blocks of
// 32 x 32, KX accumulators of 16 registers each.  The lane of the D layout holds ONE column o (lane & 31) and 16 rows, so a
// store instruction writes 32 consecutive floats of a row of y per half-wave.  Per stage of kStageW plane words (256
// features) the workgroup loads the activation words of its rows (row-strided: 32 contiguous bytes per row and plane) and
// the weight words of its columns into LDS; the next stage's words are loaded into registers while the MFMAs of this one
// run.  Every lane builds its operands from the dwords it reads from LDS: 4 v_and per activation fragment, 12 VALU per
// weight fragment.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsq_hip_linear.h"

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kStageW = 4;            // plane words (64 features each) per stage

struct Args {
  const unsigned long long* xplanes;  // first plane of this launch's pair
  const float* xscales;               // [.][N], first plane of this launch's pair
  const unsigned long long* wbits;    // weight plane q: [nw][opad]
  const int* wsum;                    // [O] of plane q
  const float* wscale;                // [O] of plane q
  const float* bias;
  float* y;
  long long M, xplane_words;          // rows; words per activation plane (M * nw)
  int O, opad, nw, N, T;
  int accumulate;                     // 0: base = bias; 1: base = y
};

template <int KX, int RB, int CB>
__global__ __launch_bounds__(kThreads, 2) void linear_xnor_kernel(Args a) {
  constexpr int BM = 64 * RB, BN = 64 * CB;
  constexpr int kAW = BM * kStageW / kThreads;        // activation words per thread, plane and stage
  constexpr int kWW = BN * kStageW / kThreads;        // weight words per thread and stage
  // (one __shared__ array: the staged activation words [p][w][BM], then the weight words [w][BN])
  __shared__ unsigned long long s_buf[KX * kStageW * BM + kStageW * BN];
  unsigned long long* s_x = s_buf;
  unsigned long long* s_w = s_buf + KX * kStageW * BM;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int col = lane & 31, hh = lane >> 5;
  const int wr = wid >> 1, wc = wid & 1;              // the wave's block of rows / columns in the tile
  const long long m0 = (long long)blockIdx.x * BM;
  const int o0 = blockIdx.y * BN;
  const int nstages = (a.nw + kStageW - 1) / kStageW;

  // global -> registers: activation word (row e / kStageW, word e % kStageW) and weight word (word e / BN, column e % BN)
  unsigned long long rx[KX][kAW], rw[kWW];
  auto load = [&](int st) {
    const int w0 = st * kStageW;
#pragma unroll
    for (int i = 0; i < kAW; ++i) {
      const int e = tid + i * kThreads;
      const long long m = m0 + e / kStageW;
      const int w = w0 + e % kStageW;
      const bool in = m < a.M && w < a.nw;
#pragma unroll
      for (int p = 0; p < KX; ++p)
        rx[p][i] = in ? a.xplanes[(long long)p * a.xplane_words + m * a.nw + w] : 0ull;
    }
#pragma unroll
    for (int i = 0; i < kWW; ++i) {
      const int e = tid + i * kThreads;
      const int w = w0 + e / BN, o = o0 + e % BN;
      rw[i] = (w < a.nw && o < a.opad) ? a.wbits[(long long)w * a.opad + o] : 0ull;
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int i = 0; i < kAW; ++i) {
      const int e = tid + i * kThreads;
#pragma unroll
      for (int p = 0; p < KX; ++p) s_x[(p * kStageW + e % kStageW) * BM + e / kStageW] = rx[p][i];
    }
#pragma unroll
    for (int i = 0; i < kWW; ++i) s_w[tid + i * kThreads] = rw[i];
  };

  // accumulators start at -wsum of their column: they end at I = sum_f a_f w_f
  v16f acc[KX][RB][CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
    const int o = o0 + wc * 32 * CB + cb * 32 + col;
    const float init = o < a.O ? -(float)a.wsum[o] : 0.f;
#pragma unroll
    for (int p = 0; p < KX; ++p)
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[p][rb][cb][i] = init;
  }

  const int unit_scale = 0x7F7F7F7F;                  // E8M0 127 = 2^0: the block scales of both operands
  const unsigned* s_x32 = reinterpret_cast<const unsigned*>(s_x);
  const unsigned* s_w32 = reinterpret_cast<const unsigned*>(s_w);
  load(0);
  for (int st = 0; st < nstages; ++st) {
    __syncthreads();                                  // the previous stage's reads are done
    stash();
    __syncthreads();
    if (st + 1 < nstages) load(st + 1);
#pragma unroll
    for (int w = 0; w < kStageW; ++w) {
      v8i bw[CB];
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        const unsigned d = s_w32[2 * (w * BN + wc * 32 * CB + cb * 32 + col) + hh];
        // nibble j of register q = feature q + 4 j: +-(4, 2, 1, 4) as E2M1 codes 6 / 4 / 2 / 6, sign bit 8 where the weight is -1
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const unsigned mag = (q == 1 ? 0x4u : (q == 2 ? 0x2u : 0x6u)) * 0x11111111u;
          const unsigned ones = (d >> q) & 0x11111111u;
          bw[cb][q] = (int)(mag | ((ones ^ 0x11111111u) << 3));
        }
#pragma unroll
        for (int q = 4; q < 8; ++q) bw[cb][q] = 0;    // (fp4 operands: the low four registers are read)
      }
#pragma unroll
      for (int p = 0; p < KX; ++p)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          const unsigned d = s_x32[2 * ((p * kStageW + w) * BM + wr * 32 * RB + rb * 32 + col) + hh];
          const v8i ax = {(int)(d & 0x11111111u), (int)(d & 0x22222222u), (int)(d & 0x44444444u),
                          (int)((d >> 3) & 0x11111111u), 0, 0, 0, 0};
#pragma unroll
          for (int cb = 0; cb < CB; ++cb)
            acc[p][rb][cb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ax, bw[cb], acc[p][rb][cb], 4, 4, 0, unit_scale,
                                                                             0, unit_scale);
        }
    }
  }

  // ---- epilogue: the popcount kernel's arithmetic on the same integers -> the same floats -----------------------------
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
    const int o = o0 + wc * 32 * CB + cb * 32 + col;
    if (o >= a.O) continue;
    const float ws = a.wscale[o];
    const float b = a.bias ? a.bias[o] : 0.f;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const long long m = m0 + wr * 32 * RB + rb * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh;
        if (m >= a.M) continue;
        const long long n = m / a.T;
        float* yp = a.y + m * a.O + o;
        float v = a.xscales[n] * acc[0][rb][cb][i];
#pragma unroll
        for (int p = 1; p < KX; ++p) v = fmaf(a.xscales[(long long)p * a.N + n], acc[p][rb][cb][i], v);
        const float base = a.accumulate ? *yp : b;
        *yp = fmaf(v, ws, base);
      }
    }
  }
}

template <int KX>
int launch(const Args& a, bool big, hipStream_t st) {
  // 128 x 128 tiles where the matrix has enough of them to fill the chip, 64 x 64 otherwise
  if (big) {
    const dim3 grid((unsigned)((a.M + 127) / 128), (unsigned)((a.O + 127) / 128));
    hipLaunchKernelGGL((linear_xnor_kernel<KX, 2, 2>), grid, dim3(kThreads), 0, st, a);
  } else {
    const dim3 grid((unsigned)((a.M + 63) / 64), (unsigned)((a.O + 63) / 64));
    hipLaunchKernelGGL((linear_xnor_kernel<KX, 1, 1>), grid, dim3(kThreads), 0, st, a);
  }
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int lsq_linear_abi_version(void) { return LSQ_LINEAR_ABI_VERSION; }

extern "C" int lsq_linear_xnor(const uint64_t* xplanes, int kx, const float* xscales, int64_t rows_per_scale,
                               const uint64_t* wbits, const int32_t* wsum, int kw_planes, const float* wscales,
                               const float* bias, int64_t M, int64_t F, int64_t O, float* y, void* stream) {
  if (!xplanes || !xscales || !wbits || !wsum || !wscales || !y) return LSQ_E_NULL;
  if (M <= 0 || F <= 0 || O <= 0 || rows_per_scale <= 0 || M % rows_per_scale) return LSQ_E_SHAPE;
  if (kx < 1 || kx > LSQ_MAX_PLANES || kw_planes < 1 || kw_planes > LSQ_MAX_PLANES) return LSQ_E_UNSUPPORTED;
  if (F >= (1ll << 22) || M >= (1ll << 31) || O >= (1ll << 21)) return LSQ_E_UNSUPPORTED;   // (O: the grid's y extent)
  if (rows_per_scale > 1 && F % 64) return LSQ_E_UNSUPPORTED;      // the rows of a sample must start on whole words
  Args a = {};
  a.M = M;
  a.O = (int)O;
  a.opad = (int)((O + 15) / 16 * 16);
  a.nw = (int)((F + 63) / 64);
  a.T = (int)rows_per_scale;
  a.N = (int)(M / rows_per_scale);
  a.xplane_words = M * a.nw;
  a.bias = bias;
  a.y = y;
  const long long wplane_words = (long long)a.nw * a.opad;
  const bool big = ((M + 127) / 128) * ((O + 127) / 128) >= 256;    // one 128 x 128 tile per CU at least
  hipStream_t st = (hipStream_t)stream;
  bool first = true;
  for (int q = 0; q < kw_planes; ++q) {
    for (int p0 = 0; p0 < kx; p0 += 2) {              // planes in pairs, as the popcount kernel takes them
      const int np = (kx - p0) >= 2 ? 2 : 1;
      a.xplanes = (const unsigned long long*)xplanes + (long long)p0 * a.xplane_words;
      a.xscales = xscales + (long long)p0 * a.N;
      a.wbits = (const unsigned long long*)wbits + (long long)q * wplane_words;
      a.wsum = wsum + (long long)q * O;
      a.wscale = wscales + (long long)q * O;
      a.accumulate = first ? 0 : 1;
      const int e = np == 2 ? launch<2>(a, big, st) : launch<1>(a, big, st);
      if (e) return e;
      first = false;
    }
  }
  return LSQ_OK;
}
