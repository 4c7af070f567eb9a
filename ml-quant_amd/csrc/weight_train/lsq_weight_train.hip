// lsq_weight_quant_pack: the weight side of a train step in one launch (include/lsq_hip_weight_train.h) for gfx950.
//
// What it replaces, once per quantized layer per step: the torch weight quantizer (abs / mean / sign / mul, and for ls-2 /
// ls-T lsq_solve_rows -- the activation solver, one 512-thread workgroup with a histogram radix select per row, built for
// rows of 10^5..10^6 keys -- plus a full w_q nobody reads), the stack of the scales, a memset and lsq_pack_weight (one
// thread per (out-channel, tap) walking a row with a stride of `taps` floats).
//
// Work split.  A workgroup of 16 waves owns R consecutive slots of the PADDED out-channel index o' (the innermost index of
// wbits): R = 16 rows with one wave each where a row has at most kWaveRowMax floats, one row with all 16 waves above.  The
// slots of a workgroup lie in one group and are 16-aligned, so its valid rows are one contiguous range of w, loaded once
// with 16-byte loads into LDS; a padded slot is a row of zeros whose words are written as zeros.  Both shapes run the same
// code (a "team" of T waves per row): trip counts depend on the row length alone, so every team reaches every barrier.
//
// Per row, all in LDS:
//   1. ls-2 / ls-T: |row[::skip]| as integer keys into a second array, bitonic sort over the next power of two, fp64 prefix
//      sums (each thread owns a run of consecutive sorted positions: wave scan on DPP + one hand-over per wave), every thread
//      tests its own positions with position_is_candidate and prices a hit with cost_of (csrc/lsq_solver_math.h: the
//      arithmetic and the tie rule are lsq_solve_rows's own), one reduction of Best.  below / equal counts of a hit come from
//      two binary searches of the sorted keys, its lower sum from the owner's prefix: candidates are a handful per row.
//   2. mean-type scales: v_q = mean |r_q|, fp64 sums in a fixed order.  The row in LDS is never overwritten: r_q is recomputed
//      from w and v_0..v_{q-1} in registers (k <= 8), because the planes are NOT the signs of r_q from plane 2 on --
//      lsq_pack_weight (as the torch quantizer) compares w against the ACCUMULATED approximation, which rounds differently.
//   3. packing: lane b reads channel 64 j + b of one tap, __ballot is the plane word, popcounts give wsum.  The words of a
//      step go through a small double-buffered LDS stage so that the 16 words of neighbouring out-channels leave as one
//      128-byte store; one barrier per step.
// The LDS row is skewed (element m at m + m / 32) so that the stride of `taps` floats between lanes is conflict-free for the
// even tap counts (2x2, 4x4, 8x8) too.

#include <atomic>

#include "lsq_hip_weight_train.h"
#include "../lsq_common.h"
#include "../lsq_solver_math.h"      // position_is_candidate, cost_of, Best / better: lsq_solve_rows's own

namespace lsq {
namespace {

constexpr int kThreads = 1024, kWaves = kThreads / kWave;
constexpr int kWaveRowMax = 1024;                 // rows up to here: a wave per row, 16 rows per workgroup
constexpr int kMaxDynamicLds = 144 * 1024;        // prefix bases + rows + keys (the static part is under 4 KB)

struct Args {
  const float* w;
  float* scales;
  unsigned long long* wbits;
  int* wsum;
  long long plane_words;
  int O, og, og_pad, opad_total, cg, taps, Gg, M, k, scheme;
  int skip, n, npow2;   // ls-2 / ls-T: keys per row, length of the sorted array (a power of two >= threads of a team)
  int pitch;            // floats of one skewed LDS row
};

__device__ __forceinline__ int skewed(int m) { return m + (m >> 5); }

// sum of `x` over the T waves of a team, the same value in every thread: butterfly inside the wave, then the wave sums in
// wave order (fixed order: bitwise repeatable)
template <int T>
__device__ __forceinline__ double team_sum(double x, double* wpart, int wave, int lane) {
  x = wave_sum(x);
  if constexpr (T > 1) {
    if (lane == 0) wpart[wave] = x;
    __syncthreads();
    x = 0.0;
#pragma unroll
    for (int i = 0; i < T; ++i) x += wpart[(wave / T) * T + i];
    __syncthreads();
  }
  return x;
}

template <int T>
__device__ __forceinline__ Best team_best(Best b, Best* wbest, int wave, int lane) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    Best o;
    o.cost = __shfl_xor(b.cost, d);
    o.order = __shfl_xor(b.order, d);
    o.value = __shfl_xor(b.value, d);
    if (better(o, b)) b = o;
  }
  if constexpr (T > 1) {
    if (lane == 0) wbest[wave] = b;
    __syncthreads();
    b = wbest[(wave / T) * T];
#pragma unroll
    for (int i = 1; i < T; ++i) {
      const Best o = wbest[(wave / T) * T + i];
      if (better(o, b)) b = o;
    }
    __syncthreads();
  }
  return b;
}

// optimal v1 of the team's row (quant/binary/optimal.py) from the row in LDS; every thread of the team returns it
template <int T>
__device__ float solve_v1(const Args& a, const float* row, unsigned* keys, double* base, double* wpart, Best* wbest, int t,
                          int wave, int lane) {
  constexpr int TT = T * kWave;
  const int n = a.n, np2 = a.npow2;
  const bool ternary = a.scheme == LSQ_SCHEME_LST;
  for (int i = t; i < np2; i += TT) keys[i] = i < n ? abs_key(row[skewed(i * a.skip)]) : kNoKey;
  __syncthreads();
  // bitonic sort, ascending; the padding keys (kNoKey) end above every real key
  for (int k2 = 2; k2 <= np2; k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int i = t; i < (np2 >> 1); i += TT) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
        const unsigned x = keys[lo], y = keys[hi];
        if ((x > y) == ((lo & k2) == 0)) {
          keys[lo] = y;
          keys[hi] = x;
        }
      }
      __syncthreads();
    }
  }
  // fp64 prefix: thread t owns the sorted positions [t * ch, (t + 1) * ch)
  const int ch = np2 / TT, p0 = t * ch;
  double local = 0.0;
  for (int p = p0; p < p0 + ch && p < n; ++p) local += (double)key_value(keys[p]);
  const double incl = wave_incl_scan(local);
  double excl = __shfl_up(incl, 1);
  if (lane == 0) excl = 0.0;
  double wave_off = 0.0, total = incl;
  if constexpr (T > 1) {
    if (lane == kWave - 1) wpart[wave] = incl;
    __syncthreads();
    total = 0.0;
#pragma unroll
    for (int i = 0; i < T; ++i) {
      if (i == wave % T) wave_off = total;
      total += wpart[(wave / T) * T + i];
    }
  } else {
    total = __shfl(incl, kWave - 1);
  }
  base[t] = wave_off + excl;
  __syncthreads();

  Best best;
  best.cost = INFINITY;
  best.order = kNoKey;
  best.value = 0.f;
  double run = wave_off + excl;
  for (int p = p0; p < p0 + ch && p < n; ++p) {
    const unsigned key = keys[p];
    const double v = (double)key_value(key);
    run += v;
    if (p < 1 || p > n - 2) continue;
    if (!position_is_candidate(v, (double)key_value(keys[p + 1]), (double)(p + 1), run, (double)n, total, ternary)) continue;
    // first position of the key's run (keys below it) and one past its last
    int lo = 0, hi = p;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    const int below = lo;
    lo = p + 1, hi = n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (keys[mid] <= key) lo = mid + 1; else hi = mid;
    }
    const int owner = below / ch;
    double below_sum = base[owner];
    for (int i = owner * ch; i < below; ++i) below_sum += (double)key_value(keys[i]);
    Best c;
    c.cost = cost_of(v, (unsigned)below, below_sum, (unsigned)(lo - below), (unsigned)n, total, ternary);
    c.order = (unsigned)below;
    c.value = key_value(key);
    if (better(c, best)) best = c;
  }
  // ternary: a row whose minimum exceeds half its mean adds mean / 2 (optimal.py:86-118)
  if (ternary && t == 0) {
    const double mean = total / (double)n;
    if ((double)key_value(keys[0]) > 0.5 * mean) {
      const float half = (float)((double)((float)mean) / 2.0);
      Best c;
      c.cost = cost_of((double)half, 0u, 0.0, 0u, (unsigned)n, total, true);
      c.order = (unsigned)n + 1u;
      c.value = half;
      if (better(c, best)) best = c;
    }
  }
  return team_best<T>(best, wbest, wave, lane).value;   // 0 when no candidate exists
}

template <int T>
__global__ __launch_bounds__(kThreads) void weight_quant_pack_kernel(Args a) {
  constexpr int R = kWaves / T, TT = T * kWave;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ double wpart[kWaves];
  __shared__ Best wbest[kWaves];
  __shared__ unsigned long long stage[2][kWaves][LSQ_MAX_PLANES];
  double* base_all = reinterpret_cast<double*>(smem);                       // [R][TT] = kThreads doubles
  float* rows = reinterpret_cast<float*>(smem + sizeof(double) * kThreads);    // [R][pitch]
  unsigned* keys_all = reinterpret_cast<unsigned*>(rows + (size_t)R * a.pitch);   // [R][npow2]

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int team = wave / T, tw = wave % T, t = tid - team * TT;
  const int slot0 = blockIdx.x * R;                       // first padded out-channel slot of the workgroup
  const int grp = slot0 / a.og_pad, oi0 = slot0 - grp * a.og_pad;
  const int nvalid = min(R, max(0, a.og - oi0)), o0 = grp * a.og + oi0;
  const bool valid = team < nvalid;
  const int M = a.M;
  float* row = rows + (size_t)team * a.pitch;

  // ---- the workgroup's rows: one contiguous range of w, 16-byte loads, read once
  if (!valid)
    for (int m = t; m < a.pitch; m += TT) row[m] = 0.f;
  {
    const float* src = a.w + (long long)o0 * M;
    const int count = nvalid * M;
    const int head = min(count, (int)((4u - (unsigned)(((uintptr_t)src >> 2) & 3u)) & 3u));
    const int nvec = (count - head) >> 2;
    if (tid < head) {
      const int r = tid / M, m = tid - r * M;
      rows[(size_t)r * a.pitch + skewed(m)] = src[tid];
    }
    for (int v = tid; v < nvec; v += kThreads) {
      const int e = head + 4 * v;
      const float4 x = *reinterpret_cast<const float4*>(src + e);
      const float xs[4] = {x.x, x.y, x.z, x.w};
      int r = e / M, m = e - r * M;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        rows[(size_t)r * a.pitch + skewed(m)] = xs[u];
        if (++m == M) {
          m = 0;
          ++r;
        }
      }
    }
    const int e = head + 4 * nvec + tid;
    if (e < count) {
      const int r = e / M, m = e - r * M;
      rows[(size_t)r * a.pitch + skewed(m)] = src[e];
    }
  }
  __syncthreads();

  // ---- scales
  float u[LSQ_MAX_PLANES];
#pragma unroll
  for (int q = 0; q < LSQ_MAX_PLANES; ++q) u[q] = 0.f;
  int q_first = 0;
  if (a.scheme == LSQ_SCHEME_LS2 || a.scheme == LSQ_SCHEME_LST) {
    u[0] = solve_v1<T>(a, row, keys_all + (size_t)team * a.npow2, base_all + team * TT, wpart, wbest, t, wave, lane);
    u[1] = u[0];
    q_first = a.scheme == LSQ_SCHEME_LS2 ? 1 : 2;
  }
#pragma unroll
  for (int q = 0; q < LSQ_MAX_PLANES; ++q) {
    if (q >= q_first && q < a.k) {         // (uniform over the workgroup: team_sum's barriers are reached by all)
      double s = 0.0;
      for (int m = t; m < M; m += TT) {
        float r = row[skewed(m)];
#pragma unroll
        for (int p = 0; p < q; ++p) r = r >= 0.f ? r - u[p] : r + u[p];
        s += (double)fabsf(r);
      }
      u[q] = (float)(team_sum<T>(s, wpart, wave, lane) / (double)M);
    }
  }
  if (valid && t < a.k) {
    float mine = 0.f;
#pragma unroll
    for (int q = 0; q < LSQ_MAX_PLANES; ++q)
      if (t == q) mine = u[q];
    a.scales[(long long)t * a.O + o0 + team] = mine;
  }

  // ---- planes and tap sums: per step the team's T waves take T words of one tap
  const int jsteps = (a.Gg + T - 1) / T;
  const int wq = tid >> 4, ws = tid & 15;                 // write-out thread: plane wq, stage entry ws
  const int wr = ws / T, wtw = ws % T;                    //   = row wr of the workgroup, wave wtw of its team
  int acc = 0, buf = 0;
  for (int tap = 0; tap < a.taps; ++tap) {
    for (int jb = 0; jb < jsteps; ++jb, buf ^= 1) {
      const int j = jb * T + tw, c = 64 * j + lane;
      const bool inb = valid && j < a.Gg && c < a.cg;
      const float x = inb ? row[skewed(c * a.taps + tap)] : 0.f;
      float result = 0.f;
      unsigned long long mine = 0ull;
#pragma unroll
      for (int q = 0; q < LSQ_MAX_PLANES; ++q) {
        if (q < a.k) {
          const bool bit = (x - result) >= 0.f;
          const unsigned long long word = __ballot(bit && inb);
          if (lane == q) mine = word;
          result = result + (bit ? u[q] : -u[q]);
        }
      }
      if (lane < a.k) stage[buf][wave][lane] = mine;
      __syncthreads();
      if (wq < a.k) {
        const int jw = jb * T + wtw;
        if (jw < a.Gg)
          a.wbits[(long long)wq * a.plane_words + ((long long)tap * a.Gg + jw) * a.opad_total + slot0 + wr] =
              stage[buf][ws][wq];
        if (wtw == 0) {
#pragma unroll
          for (int i = 0; i < T; ++i) acc += __popcll(stage[buf][wr * T + i][wq]);     // (words past Gg are zero)
          if (jb == jsteps - 1) {
            if (wr < nvalid) a.wsum[((long long)wq * a.O + o0 + wr) * a.taps + tap] = 2 * acc - a.cg;
            acc = 0;
          }
        }
      }
    }
  }
}

int next_pow2(int x) {
  int p = 1;
  while (p < x) p <<= 1;
  return p;
}

bool solver_scheme(int scheme) { return scheme == LSQ_SCHEME_LS2 || scheme == LSQ_SCHEME_LST; }

int check_scheme(int scheme, int k, int skip) {
  const bool ok = (scheme == LSQ_SCHEME_LS1 && k == 1) || (solver_scheme(scheme) && k == 2) ||
                  (scheme == LSQ_SCHEME_GF && k >= 1 && k <= LSQ_MAX_PLANES);
  return ok && skip >= 1 ? LSQ_OK : LSQ_E_SCHEME;
}

// fills what the kernel needs of `a` from the geometry; returns the dynamic LDS bytes, or -1 where the call is refused
long long plan(const lsq_conv_geom* g, int scheme, int k, int skip, Args* a) {
  a->O = g->O;
  a->og = g->O / g->groups;
  a->og_pad = (a->og + 15) / 16 * 16;
  a->opad_total = g->groups * a->og_pad;
  a->cg = g->C / g->groups;
  a->taps = g->KH * g->KW;
  a->Gg = (a->cg + 63) / 64;
  const long long M = (long long)a->cg * a->taps;
  a->plane_words = (long long)a->taps * a->Gg * a->opad_total;
  if (M > LSQ_WEIGHT_TRAIN_MAX_ROW || M * g->O >= (1ll << 31) || a->plane_words * k >= (1ll << 31)) return -1;
  a->M = (int)M;
  a->k = k;
  a->scheme = scheme;
  a->skip = skip;
  const int team_threads = a->M <= kWaveRowMax ? kWave : kThreads, rows = kThreads / team_threads;
  a->n = (a->M + skip - 1) / skip;
  a->npow2 = solver_scheme(scheme) ? (next_pow2(a->n) > team_threads ? next_pow2(a->n) : team_threads) : 0;
  a->pitch = a->M + (a->M >> 5) + 1;
  const long long bytes = (long long)sizeof(double) * kThreads + 4ll * rows * (a->pitch + a->npow2);
  return bytes <= kMaxDynamicLds ? bytes : -1;
}

// dynamic LDS above 64 KiB needs the function attribute: once per device and kernel
template <auto KERNEL>
hipError_t allow_lds() {
  static std::atomic<unsigned long long> allowed{0ull};
  int dev = 0;
  hipError_t rc = hipGetDevice(&dev);
  if (rc != hipSuccess) return rc;
  const unsigned long long bit = 1ull << (dev & 63);
  if (!(allowed.load(std::memory_order_acquire) & bit)) {
    rc = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds);
    if (rc != hipSuccess) return rc;
    allowed.fetch_or(bit, std::memory_order_release);
  }
  return hipSuccess;
}

template <int T>
int launch(const Args& a, long long lds, hipStream_t stream) {
  if (hipError_t rc = allow_lds<weight_quant_pack_kernel<T>>()) return (int)rc;
  hipLaunchKernelGGL(weight_quant_pack_kernel<T>, dim3(a.opad_total / (kWaves / T)), dim3(kThreads), (size_t)lds, stream, a);
  return (int)hipGetLastError();
}

}  // namespace
}  // namespace lsq

using namespace lsq;

extern "C" int lsq_weight_train_abi_version(void) { return LSQ_WEIGHT_TRAIN_ABI_VERSION; }

extern "C" int lsq_weight_quant_pack_supported(const lsq_conv_geom* g, int scheme, int k, int skip) {
  Args a;
  return check_geom(g) == LSQ_OK && check_scheme(scheme, k, skip) == LSQ_OK && plan(g, scheme, k, skip, &a) >= 0;
}

extern "C" int lsq_weight_quant_pack(const float* w, const lsq_conv_geom* g, int scheme, int k, int skip, float* scales,
                                     uint64_t* wbits, int32_t* wsum, void* stream) {
  if (!w || !scales || !wbits || !wsum) return LSQ_E_NULL;
  if (int e = check_geom(g)) return e;
  if (int e = check_scheme(scheme, k, skip)) return e;
  Args a;
  const long long lds = plan(g, scheme, k, skip, &a);
  if (lds < 0) return LSQ_E_UNSUPPORTED;
  a.w = w;
  a.scales = scales;
  a.wbits = (unsigned long long*)wbits;
  a.wsum = wsum;
  return a.M <= kWaveRowMax ? launch<1>(a, lds, (hipStream_t)stream) : launch<kWaves>(a, lds, (hipStream_t)stream);
}
