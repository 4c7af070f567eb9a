// lsq_linear_act_quant_solve_half: free-running ls-2 / ls-T on bf16 / fp16 rows -- the optimal v1 of quant/binary/optimal.py,
// v2 and both sign planes in ONE launch, one workgroup of 512 threads a row from its first load to its last plane word
// (grid = N).
//
// The magnitude of a clamped 16-bit value is a 15-bit KEY, so a table of one count per key fits in LDS (2^15 x 4 B = 128 KiB;
// with a clamp only the keys up to key(alpha): the table is dynamic LDS).  A key's sum is count x value, exact in fp64, and
// the whole solve runs on the table with the arithmetic of lsq_solver_math.h (shared with lsq_act_quant): no radix
// refinement, no key registers, no fallback solve, no workspace.
//   PASS 1   the sub-sample row[::skip] into the table, one 32-bit LDS atomic add per key.  Keys 0 and key(alpha) -- where a
//            zero-padded or heavily clamped row puts a large share of its elements -- are counted in registers and added once
//            per wave.  16-byte loads (a lane picks the sub-sampled elements of its groups) or 2-byte loads of the
//            sub-sampled elements alone: the same counts.
//   PLAN     SLICE t = keys 64 t .. 64 t + 63 belongs to thread t: its count, its sum (64 consecutive keys span at most two
//            binades: the fp64 sum of count x value is exact), its first and last non-empty key.  The table is swizzled
//            (low 5 bits ^ slice number) so that both a thread walking its slice and a wave reading one slice are free of
//            bank conflicts.  A workgroup scan in thread order gives every slice its sorted position r0 and prefix sum p0:
//            an order that depends on nothing but the table.
//   TEST     may_hold_candidate on each slice as a whole (reciprocal divisions, conservative); the few slices that pass are
//            listed, and a wave takes a listed slice with one key per lane: run_has_candidate (exact divisions) on each
//            non-empty key against the next non-empty key's value, cost_of, better.  The ternary extra candidate, then the
//            workgroup argmin over (cost, first sorted position of the run): the order of the list does not matter.
// (kSlice, phys(), key_value and the host helpers are lsq_half_table.h's; pass 1 to the argmin below is the text of its
// solve_v1 written in line: calling it here changed this kernel's instruction stream and cost time)
//   PASS 2   the row again (from L2): plane 0, plane 1 and S_1 by the per-group code of lsq_linear_act_quant_half's pass q = 1
//            with v_0 = v1; the same summation rule (fp32 in a group, fp64 across groups: thread, wave butterfly, waves in order).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lsq_hip_linear_act_solve.h"
#include "lsq_half_table.h"

namespace {

using namespace lsq_half;                             // to_f32, clamp_sym, load_group, wave_sum
using lsq::Best;
using lsq::kNoKey;
namespace table = lsq_half_table;                     // what this file shares with lsq_conv_act_half.hip
using table::kSlice;
using table::phys;
using table::key_value;

constexpr int kThreads = 512, kWaves = kThreads / 64;
static_assert(table::kSlices == kThreads, "one slice per thread");

struct Args {
  const unsigned short* x;            // [N][L], bf16 or fp16 bits
  unsigned char* planes;              // [2][N][nw] words, addressed by byte
  float* scales;                      // [2][N]
  int* status;                        // [N] or null
  long long N, L, plane_bytes;        // plane_bytes = 8 N nw
  int nw, skip, ternary;
  unsigned n;                         // keys of the sub-sample: ceil(L / skip)
  unsigned kmax;                      // the largest key a clamped value has; the table holds the slices up to it
  float alpha;                        // clamp bound (negative: none)
};

struct Shared {
  unsigned first[kThreads];           // first non-empty key of slice t (kNoKey: the slice is empty)
  unsigned next[kThreads];            // first non-empty key above slice t (kNoKey: none)
  unsigned r0[kThreads];              // sorted position of slice t's first element
  double p0[kThreads];                // sum of the elements below slice t
  unsigned listed[kThreads];          // slices that may hold a candidate
  unsigned nlisted;
  unsigned wcnt[kWaves];
  double wsum[kWaves];
  double red[kWaves];
  Best wbest[kWaves];
};

template <bool F16, bool VEC>
__global__ __launch_bounds__(kThreads) void solve_quant_rows(Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned hist[];   // [slices * 64] counts, swizzled by phys()
  __shared__ Shared sh;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const unsigned slices = a.kmax / kSlice + 1u;       // <= kThreads
  const unsigned n = a.n;
  const bool ternary = a.ternary != 0;
  const long long row = blockIdx.x;                 // one workgroup a row: see launch()
  const unsigned short* xrow = a.x + row * a.L;
  for (unsigned i = tid; i < slices * kSlice; i += kThreads) hist[i] = 0u;
  if (tid == 0) sh.nlisted = 0u;
  __syncthreads();

  // ---- pass 1: the sub-sample into the table
  unsigned c_zero = 0u, c_top = 0u;
  auto count = [&](unsigned h) {
    const unsigned key = min(h & 0x7FFFu, a.kmax);  // the key of the clamped value; no bit pattern leaves the table
    if (key == 0u) ++c_zero;
    else if (key == a.kmax) ++c_top;
    else atomicAdd(&hist[phys(key)], 1u);
  };
  if constexpr (VEC) {
    const int G = (int)(a.L / 8);
    for (int g = tid; g < G; g += kThreads) {
      const uint4 raw = load_group<true>(xrow, a.L, g);
      const unsigned d[4] = {raw.x, raw.y, raw.z, raw.w};
      const unsigned r = (8u * (unsigned)g) % (unsigned)a.skip;
      unsigned pick = r ? (unsigned)a.skip - r : 0u;            // the group's first sub-sampled element
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if ((unsigned)j == pick) {
          count((d[j >> 1] >> (16 * (j & 1))) & 0xFFFFu);
          pick += (unsigned)a.skip;
        }
      }
    }
  } else {
    for (unsigned s = tid; s < n; s += kThreads) count(xrow[(long long)s * a.skip]);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    c_zero += __shfl_xor(c_zero, d);
    c_top += __shfl_xor(c_top, d);
  }
  if (lane == 0) {
    if (c_zero) atomicAdd(&hist[0], c_zero);
    if (c_top) atomicAdd(&hist[phys(a.kmax)], c_top);
  }
  __syncthreads();

  // ---- plan: every slice's count and sum, then their prefixes in slice order
  unsigned cnt = 0u, first = kNoKey, last = 0u;
  double sum = 0.0;
  if ((unsigned)tid < slices) {
    for (unsigned i = 0; i < kSlice; ++i) {
      const unsigned k = (unsigned)tid * kSlice + i;
      const unsigned c = hist[phys(k)];
      if (c) {
        if (first == kNoKey) first = k;
        last = k;
        cnt += c;
        sum += (double)c * key_value<F16>(k);
      }
    }
  }
  unsigned ic = cnt;
  double is = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned oc = __shfl_up(ic, d);
    const double os = __shfl_up(is, d);
    if (lane >= d) {
      ic += oc;
      is += os;
    }
  }
  unsigned ex_c = __shfl_up(ic, 1);
  double ex_s = __shfl_up(is, 1);
  if (lane == 0) {
    ex_c = 0u;
    ex_s = 0.0;
  }
  if (lane == 63) {
    sh.wcnt[wid] = ic;
    sh.wsum[wid] = is;
  }
  sh.first[tid] = first;
  __syncthreads();
  unsigned r0 = ex_c;
  double p0 = ex_s, total = 0.0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    if (w < wid) {
      r0 += sh.wcnt[w];
      p0 += sh.wsum[w];
    }
    total += sh.wsum[w];
  }

  // ---- test: slices as a whole, conservatively
  unsigned nk = kNoKey;
  if (cnt)
    for (unsigned t = (unsigned)tid + 1u; t < slices && nk == kNoKey; ++t) nk = sh.first[t];
  sh.next[tid] = nk;
  sh.r0[tid] = r0;
  sh.p0[tid] = p0;
  if (cnt && n >= 3u) {
    const double next_hi = nk != kNoKey ? key_value<F16>(nk) : (double)INFINITY;
    if (lsq::may_hold_candidate(r0, cnt, p0, sum, key_value<F16>(first), key_value<F16>(last), next_hi, n, total, ternary))
      sh.listed[atomicAdd(&sh.nlisted, 1u)] = (unsigned)tid;
  }
  __syncthreads();

  // ---- the listed slices exactly: a wave a slice, a lane a key
  Best best;
  best.cost = (double)INFINITY;
  best.order = kNoKey;
  best.value = 0.f;
  const unsigned nl = sh.nlisted;
  for (unsigned s = (unsigned)wid; s < nl; s += kWaves) {
    const unsigned t = sh.listed[s];
    const unsigned k = t * kSlice + (unsigned)lane;
    const unsigned c = hist[phys(k)];
    const double v = key_value<F16>(k);
    unsigned jc = c;
    double js = (double)c * v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned oc = __shfl_up(jc, d);
      const double os = __shfl_up(js, d);
      if (lane >= d) {
        jc += oc;
        js += os;
      }
    }
    unsigned below_c = __shfl_up(jc, 1);
    double below_s = __shfl_up(js, 1);
    if (lane == 0) {
      below_c = 0u;
      below_s = 0.0;
    }
    const unsigned long long filled = __ballot(c != 0u);
    const unsigned long long above = lane < 63 ? filled >> (lane + 1) : 0ull;
    const unsigned succ = above ? k + (unsigned)__ffsll((long long)above) : sh.next[t];
    const double succ_v = succ != kNoKey ? key_value<F16>(succ) : (double)INFINITY;
    const unsigned run_r0 = sh.r0[t] + below_c;
    const double run_p0 = sh.p0[t] + below_s;
    if (c && lsq::run_has_candidate(v, c, run_r0, run_p0, succ_v, n, total, ternary)) {
      Best cb;
      cb.cost = lsq::cost_of(v, run_r0, run_p0, c, n, total, ternary);
      cb.order = run_r0;
      cb.value = (float)v;
      if (lsq::better(cb, best)) best = cb;
    }
  }
  // the ternary scheme's extra candidate (optimal.py:86-118: min > mean / 2 adds fl32(mean) / 2)
  if (ternary && tid == 0) {
    unsigned minkey = kNoKey;
    for (unsigned t = 0; t < slices && minkey == kNoKey; ++t) minkey = sh.first[t];
    const double mean = total / (double)n;
    if (minkey != kNoKey && key_value<F16>(minkey) > 0.5 * mean) {
      const float half = (float)((double)((float)mean) / 2.0);
      Best cb;
      cb.cost = lsq::cost_of((double)half, 0u, 0.0, 0u, n, total, true);
      cb.order = n + 1u;
      cb.value = half;
      if (lsq::better(cb, best)) best = cb;
    }
  }
  // workgroup argmin: `better` is a total order on (cost, order), so every lane ends with the same candidate
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    Best o;
    o.cost = __shfl_xor(best.cost, d);
    o.order = __shfl_xor(best.order, d);
    o.value = __shfl_xor(best.value, d);
    if (lsq::better(o, best)) best = o;
  }
  if (lane == 0) sh.wbest[wid] = best;
  __syncthreads();
  best = sh.wbest[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) {
    const Best o = sh.wbest[w];
    if (lsq::better(o, best)) best = o;
  }
  const float v1 = best.value;                      // 0 where the row has no candidate

  // ---- pass 2: both planes and S_1 (lsq_linear_act_quant_half's pass q = 1 with v_0 = v1)
  unsigned char* prow = a.planes + row * a.nw * 8;
  const int G = a.nw * 8;
  double acc = 0.0;
  for (int g = tid; g < G; g += kThreads) {
    const uint4 raw = load_group<VEC>(xrow, a.L, g);
    const long long left = a.L - 8ll * g;           // elements of the group inside the row
    const int m = left >= 8 ? 8 : (left > 0 ? (int)left : 0);
    const unsigned mask = (1u << m) - 1u;
    const unsigned d[4] = {raw.x, raw.y, raw.z, raw.w};
    unsigned byte0 = 0u, byte1 = 0u;
    float s = 0.f;                                  // |res_1| of elements 0 .. 7 in order (+0 past L: exact)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float c = clamp_sym(to_f32<F16>((d[j >> 1] >> (16 * (j & 1))) & 0xFFFFu), a.alpha);
      float result = 0.f, res = c;
      byte0 |= (unsigned)((c - result) >= 0.f) << j;
      result = result + ((c - result >= 0.f) ? v1 : -v1);
      res = res - ((res >= 0.f) ? v1 : -v1);
      byte1 |= (unsigned)((c - result) >= 0.f) << j;
      s = s + (j < m ? fabsf(res) : 0.f);
    }
    acc += (double)s;
    prow[g] = (unsigned char)(byte0 & mask);
    prow[a.plane_bytes + g] = (unsigned char)(byte1 & mask);
  }
  const double w = wave_sum(acc);
  if (lane == 0) sh.red[wid] = w;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) tot += sh.red[i];
    a.scales[row] = v1;
    a.scales[a.N + row] = ternary ? v1 : (float)(tot / (double)a.L);
    if (a.status) a.status[row] = best.order != kNoKey ? 1 : 0;
  }
}

template <bool F16, bool VEC>
int launch(Args a, hipStream_t st) {
  a.kmax = table::top_key<F16>(a.alpha);
  const hipError_t rc = table::allow_full_table<&solve_quant_rows<F16, VEC>>();
  if (rc != hipSuccess) return (int)rc;
  // One workgroup a row, N < 2^31 workgroups: the hardware takes them in turn.  (A loop over rows inside the kernel lets the
  // compiler keep every row-invariant mask and bound live across it: 30 to 35 scalar registers spilled, 111 vector
  // registers against 76.)
  hipLaunchKernelGGL((solve_quant_rows<F16, VEC>), dim3((unsigned)a.N), dim3(kThreads), table::table_bytes(a.kmax), st, a);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int lsq_linear_act_solve_abi_version(void) { return LSQ_LINEAR_ACT_SOLVE_ABI_VERSION; }

extern "C" int lsq_linear_act_quant_solve_half(const void* x, int x_dtype, int64_t N, int64_t L, int scheme, int skip,
                                               float clamp_alpha, uint64_t* planes, float* scales, int32_t* status, void* stream) {
  if (!x || !planes || !scales) return LSQ_E_NULL;
  if (N <= 0 || L <= 0 || skip <= 0) return LSQ_E_SHAPE;
  if (scheme != LSQ_SCHEME_LS2 && scheme != LSQ_SCHEME_LST) return LSQ_E_SCHEME;
  if (x_dtype != LSQ_DTYPE_BF16 && x_dtype != LSQ_DTYPE_F16) return LSQ_E_UNSUPPORTED;
  if (L >= (1ll << 31) || N >= (1ll << 31)) return LSQ_E_UNSUPPORTED;
  Args a = {};
  a.x = static_cast<const unsigned short*>(x);
  a.planes = reinterpret_cast<unsigned char*>(planes);
  a.scales = scales;
  a.status = status;
  a.N = N;
  a.L = L;
  a.nw = (int)((L + 63) / 64);
  a.plane_bytes = 8ll * N * a.nw;
  a.skip = skip;
  a.ternary = scheme == LSQ_SCHEME_LST;
  a.n = (unsigned)((L + skip - 1) / skip);
  a.alpha = clamp_alpha;
  // 16-byte loads where every row starts on 16 bytes (same counts, same groups, same bits as the 2-byte loads)
  const bool vec = ((uintptr_t)x & 15) == 0 && L % 8 == 0;
  hipStream_t st = (hipStream_t)stream;
  if (x_dtype == LSQ_DTYPE_F16) return vec ? launch<true, true>(a, st) : launch<true, false>(a, st);
  return vec ? launch<false, true>(a, st) : launch<false, false>(a, st);
}
