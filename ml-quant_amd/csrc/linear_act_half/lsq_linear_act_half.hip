// lsq_linear_act_quant_half: sign planes and per-sample scales of bf16 / fp16 rows, for the schemes without a scale solve
// (ls-1, gf-k, and any scheme with given scales) -- the activation operand of lsq_linear_xnor from a 16-bit input.
//
// A streaming kernel: the row is read once (once per plane for gf-k without given scales), 8 elements a lane.
//   * GROUP g of a row = its elements 8 g .. 8 g + 7 = byte g of its plane words (bit i of word w is element 64 w + i, so
//     byte b of word w holds elements 64 w + 8 b ..): one lane owns a group, converts it to fp32 (exactly; subnormals kept),
//     clamps it, runs the chain of lsq_act_quant's chain_eval on each element and stores ONE BYTE per plane.  Consecutive
//     lanes own consecutive groups: a wave's loads are 1 KiB contiguous, its byte stores 64 bytes contiguous.  A row has
//     8 ceil(L / 64) groups, so every byte of every word is written; elements past L give bit 0.
//   * LOAD: one 16-byte load where every row starts on 16 bytes (VEC), eight 2-byte loads otherwise; the same lane owns
//     the same group either way, so neither the planes nor the scales depend on the alignment.
//   * SCALE (no given scales): the lane adds the 8 fp32 magnitudes |res_q| of its group in fp32 in element order (0 past
//     L), its groups' sums in fp64 in group order, the wave's lanes by xor butterfly, the workgroup's waves in wave order:
//     an order fixed by L alone.  v_q = (float)(S_q / L).
//   * PASSES: given scales -> one pass writes all k planes.  ls-1 / gf-1 -> one pass.  gf-k -> k passes; pass 0 leaves the
//     raw groups in LDS (each thread reads back only what it wrote itself: no barrier) where the row fits, later passes
//     read them from there, or from global memory (L2) again where it does not.
//   quant_wave_rows   rows of up to kWaveRowMax elements: one wave a row, four rows a workgroup (8192 rows of 4096)
//   quant_block_rows  longer rows: one workgroup of 256 threads a row

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "lsq_hip_linear_act_half.h"
#include "../lsq_half_rows.h"

namespace {

using namespace lsq_half;                             // to_f32, clamp_sym, load_group, wave_sum

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kWaveRowMax = 4096;                     // elements: longer rows take a workgroup each
constexpr int kWaveStash = kWaveRowMax / 8;           // groups a wave keeps in LDS between passes (8 KiB)
constexpr int kBlockStash = 2048;                     // groups a workgroup keeps (32 KiB): rows of up to 16384 elements
constexpr long long kMaxGrid = 1ll << 22;
constexpr int kWaveBatch = 8, kBlockBatch = 4;        // groups a thread requests before it consumes any of them

enum { kGiven = 0, kOnePass = 1, kPasses = 2 };       // scales given | one plane to compute | k planes, k passes

struct Args {
  const unsigned short* x;            // [N][L], bf16 or fp16 bits
  const float* forced;                // [k][N] or null
  unsigned char* planes;              // [k][N][nw] words, addressed by byte
  float* scales;                      // [k][N]
  long long N, L, plane_bytes;        // plane_bytes = 8 N nw
  int nw, k;
  float alpha;                        // clamp bound (negative: none)
};

// One row by T threads (t = the thread's index among them).  reduce(acc, q): the sum of acc over the T threads, the same
// value in every thread.  stash: the threads' LDS room for `stash_groups` groups (kPasses only).
template <bool F16, bool VEC, int MODE, int T, int U, class Reduce>
__device__ __forceinline__ void quant_row(const Args& a, long long row, int t, uint4* stash, int stash_groups, Reduce reduce) {
  const unsigned short* xrow = a.x + row * a.L;
  unsigned char* prow = a.planes + row * a.nw * 8;    // the row's bytes in plane 0
  const int G = a.nw * 8;
  float v[LSQ_MAX_PLANES];
#pragma unroll
  for (int i = 0; i < LSQ_MAX_PLANES; ++i) v[i] = 0.f;
  if constexpr (MODE == kGiven) {
#pragma unroll
    for (int i = 0; i < LSQ_MAX_PLANES; ++i) {
      if (i >= a.k) break;
      v[i] = a.forced[i * a.N + row];
      if (t == 0) a.scales[i * a.N + row] = v[i];
    }
  }
  const int passes = MODE == kPasses ? a.k : 1;
  const bool stashed = MODE == kPasses && G <= stash_groups;
  for (int q = 0; q < passes; ++q) {
    double acc = 0.0;
    for (int g0 = 0; g0 < G; g0 += T * U) {
      uint4 raw[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int g = min(g0 + u * T + t, G - 1);
        if (MODE == kPasses && stashed && q > 0) raw[u] = stash[g];
        else raw[u] = load_group<VEC>(xrow, a.L, g);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int g = g0 + u * T + t;
        if (g >= G) continue;
        if (MODE == kPasses && stashed && q == 0) stash[g] = raw[u];
        const long long left = a.L - 8ll * g;          // elements of the group inside the row
        const int n = left >= 8 ? 8 : (left > 0 ? (int)left : 0);
        const unsigned mask = (1u << n) - 1u;
        const unsigned d[4] = {raw[u].x, raw[u].y, raw[u].z, raw[u].w};
        float c[8], result[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          c[j] = clamp_sym(to_f32<F16>((d[j >> 1] >> (16 * (j & 1))) & 0xFFFFu), a.alpha);
          result[j] = 0.f;
        }
        if constexpr (MODE == kGiven) {
#pragma unroll
          for (int i = 0; i < LSQ_MAX_PLANES; ++i) {
            if (i >= a.k) break;
            unsigned byte = 0u;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const bool b = (c[j] - result[j]) >= 0.f;
              byte |= (unsigned)b << j;
              result[j] = result[j] + (b ? v[i] : -v[i]);
            }
            prow[i * a.plane_bytes + g] = (unsigned char)(byte & mask);
          }
        } else {
          float res[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) res[j] = c[j];
#pragma unroll
          for (int i = 0; i < LSQ_MAX_PLANES - 1; ++i) {
            if (i >= q) break;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              result[j] = result[j] + ((c[j] - result[j] >= 0.f) ? v[i] : -v[i]);
              res[j] = res[j] - ((res[j] >= 0.f) ? v[i] : -v[i]);
            }
          }
          unsigned byte = 0u;
          float s = 0.f;                              // |res| of elements 0 .. 7 in order (+0 past L: exact)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            byte |= (unsigned)((c[j] - result[j]) >= 0.f) << j;
            s = s + (j < n ? fabsf(res[j]) : 0.f);
          }
          acc += (double)s;
          prow[q * a.plane_bytes + g] = (unsigned char)(byte & mask);
        }
      }
    }
    if constexpr (MODE != kGiven) {
      const float vq = (float)(reduce(acc, q) / (double)a.L);
#pragma unroll
      for (int i = 0; i < LSQ_MAX_PLANES; ++i)
        if (i == q) v[i] = vq;
      if (t == 0) a.scales[q * a.N + row] = vq;
    }
  }
}

template <bool F16, bool VEC, int MODE>
__global__ __launch_bounds__(kThreads) void quant_wave_rows(Args a) {
  __shared__ __attribute__((aligned(16))) uint4 s_stash[MODE == kPasses ? kWaves * kWaveStash : 1];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  // (no barrier in this kernel: a wave is on its own)
  for (long long row = (long long)blockIdx.x * kWaves + wid; row < a.N; row += (long long)gridDim.x * kWaves)
    quant_row<F16, VEC, MODE, 64, kWaveBatch>(a, row, lane, s_stash + (MODE == kPasses ? wid * kWaveStash : 0), kWaveStash,
                                              [](double acc, int) { return wave_sum(acc); });
}

template <bool F16, bool VEC, int MODE>
__global__ __launch_bounds__(kThreads) void quant_block_rows(Args a) {
  __shared__ __attribute__((aligned(16))) uint4 s_stash[MODE == kPasses ? kBlockStash : 1];
  __shared__ double s_sum[LSQ_MAX_PLANES][kWaves];    // (one slot per pass: one barrier per pass)
  const int tid = threadIdx.x;
  for (long long row = blockIdx.x; row < a.N; row += gridDim.x) {
    quant_row<F16, VEC, MODE, kThreads, kBlockBatch>(a, row, tid, s_stash, kBlockStash, [&](double acc, int q) {
      const double w = wave_sum(acc);
      if ((tid & 63) == 0) s_sum[q][tid >> 6] = w;
      __syncthreads();
      double tot = 0.0;
#pragma unroll
      for (int i = 0; i < kWaves; ++i) tot += s_sum[q][i];
      return tot;
    });
    __syncthreads();                                  // (the next row's sums reuse the slots)
  }
}

template <bool F16, bool VEC, int MODE>
int launch(const Args& a, hipStream_t st) {
  // (at most kMaxGrid workgroups: beyond, a workgroup takes several rows in turn)
  if (a.L <= kWaveRowMax)
    hipLaunchKernelGGL((quant_wave_rows<F16, VEC, MODE>), dim3((unsigned)std::min<long long>((a.N + kWaves - 1) / kWaves, kMaxGrid)),
                       dim3(kThreads), 0, st, a);
  else
    hipLaunchKernelGGL((quant_block_rows<F16, VEC, MODE>), dim3((unsigned)std::min<long long>(a.N, kMaxGrid)), dim3(kThreads), 0, st, a);
  return (int)hipGetLastError();
}

template <bool F16, bool VEC>
int launch_mode(const Args& a, hipStream_t st) {
  if (a.forced) return launch<F16, VEC, kGiven>(a, st);
  return a.k == 1 ? launch<F16, VEC, kOnePass>(a, st) : launch<F16, VEC, kPasses>(a, st);
}

}  // namespace

extern "C" int lsq_linear_act_half_abi_version(void) { return LSQ_LINEAR_ACT_HALF_ABI_VERSION; }

extern "C" int lsq_linear_act_quant_half(const void* x, int x_dtype, int64_t N, int64_t L, int scheme, int k, float clamp_alpha,
                                         const float* forced, uint64_t* planes, float* scales, void* stream) {
  if (!x || !planes || !scales) return LSQ_E_NULL;
  if (N <= 0 || L <= 0) return LSQ_E_SHAPE;
  if (k < 1 || k > LSQ_MAX_PLANES || scheme < LSQ_SCHEME_LS1 || scheme > LSQ_SCHEME_GF) return LSQ_E_SCHEME;
  const bool solver = scheme == LSQ_SCHEME_LS2 || scheme == LSQ_SCHEME_LST;
  if ((scheme == LSQ_SCHEME_LS1 && k != 1) || (solver && k != 2)) return LSQ_E_SCHEME;
  if (x_dtype != LSQ_DTYPE_BF16 && x_dtype != LSQ_DTYPE_F16) return LSQ_E_UNSUPPORTED;
  if (L >= (1ll << 31) || N >= (1ll << 31)) return LSQ_E_UNSUPPORTED;
  if (solver && !forced) return LSQ_E_UNSUPPORTED;    // the free-running ls-2 / ls-T solve is lsq_act_quant's (fp32 rows)
  Args a = {};
  a.x = static_cast<const unsigned short*>(x);
  a.forced = forced;
  a.planes = reinterpret_cast<unsigned char*>(planes);
  a.scales = scales;
  a.N = N;
  a.L = L;
  a.nw = (int)((L + 63) / 64);
  a.plane_bytes = 8ll * N * a.nw;
  a.k = k;
  a.alpha = clamp_alpha;
  // 16-byte loads where every row starts on 16 bytes (same groups, same lanes, same bits as the 2-byte loads)
  const bool vec = ((uintptr_t)x & 15) == 0 && L % 8 == 0;
  hipStream_t st = (hipStream_t)stream;
  if (x_dtype == LSQ_DTYPE_F16) return vec ? launch_mode<true, true>(a, st) : launch_mode<true, false>(a, st);
  return vec ? launch_mode<false, true>(a, st) : launch_mode<false, false>(a, st);
}
