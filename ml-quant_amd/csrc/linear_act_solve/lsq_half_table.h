// The count-table solve of the 16-bit quantizers: the optimal v1 of quant/binary/optimal.py (ls-2 / ls-T,
// free-running) of a bf16 / fp16 row.  conv_act_half/lsq_conv_act_half_core.h (1024 threads a sample; with the
// folded batch norm of DESIGN 4.30 as the element transform `xf`) calls solve_v1;
// lsq_linear_act_solve.hip (512 threads a row) shares the table's constants, phys(), key_value and the host side
// and keeps pass 1 to the argmin written in line -- the same statements: a change to either goes into both.
// The table (one count per 15-bit magnitude key, dynamic LDS up to key(alpha), swizzled by phys()) and the steps PASS 1, PLAN
// and TEST are described at the top of lsq_linear_act_solve.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>

#include "../lsq_half_rows.h"
#include "../lsq_solver_math.h"

namespace lsq_half_table {

using lsq::Best;
using lsq::kNoKey;
using namespace lsq_half;                             // to_f32, load_group

constexpr unsigned kKeys = 1u << 15;                  // magnitudes of a 16-bit type
constexpr unsigned kSlice = 64;                       // keys of a slice: one thread in the plan, one wave in the exact test
constexpr int kSlices = (int)(kKeys / kSlice);        // 512: the first 512 threads of the workgroup plan, every wave tests

template <int THREADS>
struct Shared {
  static_assert(THREADS % 64 == 0 && kSlices <= THREADS, "one slice per thread");
  unsigned first[kSlices];            // first non-empty key of slice t (kNoKey: the slice is empty)
  unsigned next[kSlices];             // first non-empty key above slice t (kNoKey: none)
  unsigned r0[kSlices];               // sorted position of slice t's first element
  double p0[kSlices];                 // sum of the elements below slice t
  unsigned listed[kSlices];           // slices that may hold a candidate
  unsigned nlisted;
  unsigned wcnt[THREADS / 64];
  double wsum[THREADS / 64];
  Best wbest[THREADS / 64];
};

__device__ __forceinline__ unsigned phys(unsigned key) { return key ^ ((key >> 6) & 31u); }

template <bool F16>
__device__ __forceinline__ double key_value(unsigned key) { return (double)to_f32<F16>(key); }

// The optimal v1 of the flat sub-sample xrow[::skip] of a row of len elements, by a workgroup of THREADS threads.  `a`: the
// caller's kernel arguments, with members int skip, unsigned n = ceil(len / skip), unsigned kmax (the largest key of a clamped
// value) and int ternary (read from it, not passed as four values: DESIGN 4.25).  hist: (kmax / kSlice + 1) * kSlice counts.
// VEC16: the row starts on 16 bytes, len % 8 == 0.  Every thread gets the same candidate (order == kNoKey: none, value 0)
// and the same sum `total` of the sub-sample's magnitudes.
// xf: an element transform applied to the 16 bits of every element pass 1 counts (the row is then the transformed row):
// xf.channel(index) is what the transform needs of the element at `index` of the row, xf(bits, that) the transformed bits.  On
// the VEC16 path channel() is asked once per group of 8 elements, at the group's first: a transform that depends on the index
// must be constant over aligned groups of 8.  The default is the identity and compiles to nothing.
struct Identity {
  struct Channel {};
  __device__ __forceinline__ Channel channel(long long) const { return {}; }
  __device__ __forceinline__ unsigned operator()(unsigned h, const Channel&) const { return h; }
};

template <bool F16, bool VEC16, int THREADS, class ARGS, class XF = Identity>
__device__ __forceinline__ Best solve_v1(const ARGS& a, const unsigned short* __restrict__ xrow, long long len, unsigned* hist,
                                         Shared<THREADS>& sh, double& total, const XF& xf = XF()) {
  static_assert(std::is_same_v<decltype(ARGS::skip), int> && std::is_same_v<decltype(ARGS::n), unsigned> &&
                    std::is_same_v<decltype(ARGS::kmax), unsigned> && std::is_same_v<decltype(ARGS::ternary), int>,
                "ARGS needs: int skip; unsigned n; unsigned kmax; int ternary");
  constexpr int kWaves = THREADS / 64;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int skip = a.skip;
  const unsigned kmax = a.kmax;
  const unsigned slices = kmax / kSlice + 1u;         // <= kSlices
  const unsigned n = a.n;
  const bool ternary = a.ternary != 0;
  for (unsigned i = tid; i < slices * kSlice; i += THREADS) hist[i] = 0u;
  if (tid == 0) sh.nlisted = 0u;
  __syncthreads();

  // ---- pass 1: the sub-sample into the table
  unsigned c_zero = 0u, c_top = 0u;
  auto count = [&](unsigned h) {
    const unsigned key = min(h & 0x7FFFu, kmax);      // the key of the clamped value; no bit pattern leaves the table
    if (key == 0u) ++c_zero;
    else if (key == kmax) ++c_top;
    else atomicAdd(&hist[phys(key)], 1u);
  };
  if constexpr (VEC16) {
    const int G = (int)(len / 8);
    for (int g = tid; g < G; g += THREADS) {
      const uint4 raw = load_group<true>(xrow, len, g);
      const unsigned d[4] = {raw.x, raw.y, raw.z, raw.w};
      const unsigned r = (unsigned)((8ll * g) % skip);
      unsigned pick = r ? (unsigned)skip - r : 0u;    // the group's first sub-sampled element
      const auto ch = xf.channel(8ll * g);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if ((unsigned)j == pick) {
          count(xf((d[j >> 1] >> (16 * (j & 1))) & 0xFFFFu, ch));
          pick += (unsigned)skip;
        }
      }
    }
  } else {
    for (unsigned s = tid; s < n; s += THREADS) {
      const long long at = (long long)s * skip;
      count(xf(xrow[at], xf.channel(at)));
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    c_zero += __shfl_xor(c_zero, d);
    c_top += __shfl_xor(c_top, d);
  }
  if (lane == 0) {
    if (c_zero) atomicAdd(&hist[0], c_zero);
    if (c_top) atomicAdd(&hist[phys(kmax)], c_top);
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
  if (tid < kSlices) sh.first[tid] = first;
  __syncthreads();
  unsigned r0 = ex_c;
  double p0 = ex_s;
  total = 0.0;
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
  if (tid < kSlices) {
    sh.next[tid] = nk;
    sh.r0[tid] = r0;
    sh.p0[tid] = p0;
  }
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
  return best;
}

// ---- host side

// the largest key whose value is <= alpha (alpha >= 0): the key of the clamp bound where the bound is a value of the type
template <bool F16>
inline unsigned key_of_bound(float alpha) {
  auto value = [](unsigned key) {
    if constexpr (F16) return (float)__builtin_bit_cast(_Float16, (unsigned short)key);
    else return __builtin_bit_cast(float, key << 16);
  };
  unsigned lo = 0u, hi = F16 ? 0x7C00u : 0x7F80u;     // 0 .. +inf
  while (lo < hi) {
    const unsigned mid = (lo + hi + 1u) >> 1;
    if (value(mid) <= alpha) lo = mid; else hi = mid - 1u;
  }
  return lo;
}

// the largest key a value clamped to alpha has (negative alpha: no clamp), and the bytes of the table of the slices up to it
template <bool F16>
inline unsigned top_key(float alpha) { return alpha >= 0.f ? key_of_bound<F16>(alpha) : kKeys - 1u; }

inline unsigned table_bytes(unsigned kmax) { return (kmax / kSlice + 1u) * kSlice * 4u; }

// Dynamic LDS above 64 KiB needs the function attribute: set once per device for KERNEL (one mask per instantiation, that is
// per kernel); hipGetDevice on every launch.
template <auto KERNEL>
inline hipError_t allow_full_table() {
  static std::atomic<unsigned long long> allowed{0ull};
  int dev = 0;
  hipError_t rc = hipGetDevice(&dev);
  if (rc != hipSuccess) return rc;
  const unsigned long long bit = 1ull << (dev & 63);
  if (!(allowed.load(std::memory_order_acquire) & bit)) {
    rc = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kKeys * 4u));
    if (rc != hipSuccess) return rc;
    allowed.fetch_or(bit, std::memory_order_release);
  }
  return hipSuccess;
}

}  // namespace lsq_half_table
