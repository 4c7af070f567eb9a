// liblsq_hip_conv_xnor_gen_half.so: lsq_xnor_conv2d_gen_half, the general fp4 matrix-core XNOR convolution of
// csrc/conv_xnor_gen/lsq_conv_xnor_gen.hip for 16-bit networks: bf16 / fp16 residuals and output, EVERY plane pass inside ONE
// launch, no workspace.  Same operands and layouts as lsq_xnor_conv2d_half and -- the integers being exact, the fp32
// arithmetic in that kernel's order, one rounding at the store -- the same 16-bit result, bit for bit.
//
// Kept from xnor_gen_kernel (see that file for the why of each): 8 waves per workgroup on 32 MT out-channels, one tile of 32
// output pixels per wave flat over (n, ho, wo); the fp4 encoding; the flat K loop over steps s = tap * Gg + word in chunks of
// 8 / (planes of the pass); the packed weight words streamed through a double-buffered LDS ring and expanded once per
// workgroup; activation dwords read straight from the bit planes a chunk ahead; the border term from a 2-D prefix-sum table of
// wsum.
//
// What is this kernel's own:
//   * the PLANE PASSES ARE A LOOP IN THE KERNEL: weight planes q outside, pairs of activation planes p0 inside (the order of
//     lsq_xnor_conv2d's launches: the bits depend on it).  A pass starts its accumulators at the border term of plane q, walks
//     the K loop over plane q's weight words and planes p0, p0 + 1 of the activations and folds into a per-lane fp32 running
//     value run[MT][16] in registers, which starts at the bias:  v = xs0 I0;  v = fmaf(xs1, I1, v);  run = fmaf(v, ws_q[o], run).
//     Nothing goes to memory between passes: lsq_xnor_conv2d_half writes and reads back an fp32 sum per extra launch.
//   * per weight plane the prefix table and the scales are REBUILT in LDS from that plane's wsum / wscales, behind a barrier
//     (the fold of the plane before reads the scales after its last K-loop barrier).
//   * an odd plane count ends every weight plane with a pass over ONE activation plane: the same pass body instantiated with
//     one plane (chunks of 8 steps), taken by a uniform branch.
//   * the 16-bit EPILOGUE runs once, behind the last pass: res_pre / res_post widened as they are read (exact), activation,
//     one rounding to T, one 2-byte store per output (32 consecutive pixels of a channel: 64 contiguous bytes per half-wave).
//   * MULTI = false (one pass: kw_planes * ceil(kx / 2) == 1) has no loop, no rebuild and no running value beside the
//     accumulators: xnor_gen_kernel with a 16-bit epilogue.
// Registers: run adds 16 MT beside the 16 KX MT accumulators.  With MT = 2 that does not fit the 128 registers of four waves
// per SIMD without scratch, so a call of several passes runs MT = 1 (the build record is in DESIGN 4.38).

#include "../lsq_xnor_conv.h"      // epi_load / epi_store, LSQ_DTYPE_*
#include "lsq_hip_conv_xnor_gen_half.h"

namespace lsq {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int kWaves = 8;                        // pixel tiles (of 32) per workgroup
constexpr int kThreads = 64 * kWaves;
constexpr int kChunkMfma = 8;                    // K steps x activation planes between two barriers
constexpr int kMaxTaps = 64, kMaxK = 8;

struct GenHalfArgs {
  const unsigned* xd;                  // every activation plane as dwords: [kx][N][Gg][Hp][Wp][2]
  const float* xscales;                // [kx][N]
  const unsigned long long* wbits;     // [kw_planes][steps][O]
  const int* wsum;                     // [kw_planes][O][taps]
  const float* wscales;                // [kw_planes][O]
  const float* bias;                   // [O] or null
  const float* slope;                  // PReLU slope(s)
  const void* res_pre;                 // [N][O][Ho][Wo] of T or null
  const void* res_post;
  void* y;                             // [N][O][Ho][Wo] of T
  unsigned plane_dwords;               // dwords of one activation plane
  unsigned word_dwords;                // 2 Hp Wp: dwords between two channel words of a sample
  int N, H, W, O, KH, KW, sh, sw, ph, pw, dh, dw, Gg, Hp, Wp, Ho, Wo;
  int steps;                           // KH KW Gg
  int kx, kw_planes, act;
  int tap_xoff[kMaxTaps];              // dwords: 2 ((kh dil_h) Wp + kw dil_w)
};

// KX: activation planes of a full pass (2 where the call has at least two, else 1); MULTI: more than one pass
template <typename T, int KX, int MT, bool MULTI>
__global__ __launch_bounds__(kThreads, 4) void xnor_gen_half_kernel(GenHalfArgs a) {
  constexpr int OC = 32 * MT;                    // out-channels of the workgroup
  // 1 KB fragments per ring buffer, [step of the chunk][tile]: a pass over one plane has chunks of 8 steps, over two of 4
  constexpr int kFragMax = ((KX == 1 || MULTI) ? kChunkMfma : kChunkMfma / 2) * MT;
  __shared__ v4i s_w[2 * kFragMax][64];
  __shared__ __attribute__((aligned(16))) int s_pre[(kMaxK + 1) * (kMaxK + 1)][OC];      // [a (KW + 1) + b][o]: sum over kh < a, kw < b
  __shared__ __attribute__((aligned(16))) float s_scale[OC], s_bias[OC], s_slope[OC];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int col = lane & 31, hh = lane >> 5;
  const int o0 = blockIdx.y * OC;
  const int ob = 4 * hh;                         // the lane's out-channel of register i of tile mt: 32 mt + ob + (i & 3) + 8 (i >> 2)

  // ---- the lane's pixel: tile = 32 consecutive outputs, flat over (n, ho, wo); lanes past the last one compute pixel 0 and
  // store nothing (a whole wave of them still takes part in the staging and the barriers)
  const unsigned total = (unsigned)(a.N * a.Ho * a.Wo);
  const int HoWo = a.Ho * a.Wo;
  const unsigned pix = ((unsigned)blockIdx.x * kWaves + (unsigned)wid) * 32u + (unsigned)col;
  const bool valid = pix < total;
  const unsigned pc = valid ? pix : 0u;
  const int n = (int)(pc / (unsigned)HoWo);
  const int r = (int)(pc - (unsigned)n * (unsigned)HoWo);
  const int ho = (int)((unsigned)r / (unsigned)a.Wo), wo = r - ho * a.Wo;
  const unsigned xbase = 2u * (unsigned)((n * a.Gg * a.Hp + ho * a.sh) * a.Wp + wo * a.sw) + (unsigned)hh;
  const int taps = a.KH * a.KW, W1 = a.KW + 1;

  const int hi0 = ho * a.sh - a.ph, wi0 = wo * a.sw - a.pw;      // the input row / column of tap (0, 0)

  // ---- per weight plane q: scale and the prefix sums of wsum of the workgroup's OC out-channels (bias and slope with plane 0).
  // The last phase is left open: the caller's barrier closes it.
  auto build_tables = [&](int q) {
    if (q > 0) lds_barrier();                    // the fold of plane q - 1 has read s_scale, its passes s_pre
    // (opaque: the index arithmetic below is the same for every plane, and hoisted out of the plane loop it would stand in
    //  registers beside the accumulators through every K loop)
    int t = tid;
    asm volatile("" : "+v"(t));
    if (t < OC) {
      s_scale[t] = a.wscales[(long long)q * a.O + o0 + t];
      if (q == 0) {
        s_bias[t] = a.bias ? a.bias[o0 + t] : 0.f;
        s_slope[t] = a.act >= LSQ_ACT_PRELU ? a.slope[a.act == LSQ_ACT_PRELU ? 0 : o0 + t] : 0.f;
      }
    }
    const int* __restrict__ ws = a.wsum + ((long long)q * a.O + o0) * taps;
    for (int i = t; i < (a.KH + 1) * W1 * OC; i += kThreads) s_pre[i / OC][i % OC] = 0;
    __syncthreads();
    for (int i = t; i < OC * taps; i += kThreads) {          // (consecutive threads, consecutive addresses: wsum is [O][taps])
      const int o = i / taps, tp = i - o * taps;
      const int kh = tp / a.KW, kw = tp - kh * a.KW;
      s_pre[(kh + 1) * W1 + kw + 1][o] = ws[i];
    }
    __syncthreads();
    for (int i = t; i < a.KH * OC; i += kThreads) {           // along kw
      const int o = i % OC, row = (i / OC + 1) * W1;
      int sum = 0;
      for (int b = 1; b <= a.KW; ++b) {
        sum += s_pre[row + b][o];
        s_pre[row + b][o] = sum;
      }
    }
    __syncthreads();
    for (int i = t; i < a.KW * OC; i += kThreads) {           // along kh
      const int o = i % OC, b = i / OC + 1;
      int sum = 0;
      for (int k = 1; k <= a.KH; ++k) {
        sum += s_pre[k * W1 + b][o];
        s_pre[k * W1 + b][o] = sum;
      }
    }
  };

  // ---- 16-bit epilogue, once: residuals widened as they are read, activation, one rounding, one store per output.
  // value(mt, i): the fp32 value of output register i of tile mt behind the last fold.
  auto epilogue = [&](auto value) {
    if (!valid) return;
    const bool want_pre = a.res_pre != nullptr, want_post = a.res_post != nullptr;
    const bool relu = a.act == LSQ_ACT_RELU, prelu = a.act >= LSQ_ACT_PRELU;
    const T* __restrict__ rpre = static_cast<const T*>(a.res_pre);
    const T* __restrict__ rpost = static_cast<const T*>(a.res_post);
    T* __restrict__ y = static_cast<T*>(a.y);
    // 32-bit element offsets (the entry point admits outputs below 2^30 elements)
    const unsigned yoff = (unsigned)((n * a.O + o0 + ob) * HoWo + r);
    // (eight outputs at a time: their loads go out together, and the operand arrays stay small beside the accumulators)
#pragma unroll
    for (int h = 0; h < 2 * MT; ++h) {
      const int mt = h >> 1, i0 = 8 * (h & 1);
      float pre[8], post[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int i = i0 + k, ch = 32 * mt + (i & 3) + 8 * (i >> 2);
        const unsigned at = yoff + (unsigned)(ch * HoWo);
        pre[k] = want_pre ? epi_load(rpre + at) : 0.f;
        post[k] = want_post ? epi_load(rpost + at) : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int i = i0 + k, ch = 32 * mt + (i & 3) + 8 * (i >> 2);
        float out = value(mt, i);
        if (want_pre) out += pre[k];
        if (relu) out = fmaxf(out, 0.f);
        if (prelu) {
          const float neg = s_slope[ob + ch] * out;
          out = out > 0.f ? out : neg;
        }
        if (want_post) out += post[k];
        epi_store(y + (yoff + (unsigned)(ch * HoWo)), out);
      }
    }
  };

  // several passes: the running value of the lane's 16 MT outputs, bias + the passes so far.  It starts at the bias (read
  // here, far ahead of the first fold), so every fold is the same fmaf.
  float run[MT][16];
  if constexpr (MULTI) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 16; ++i) run[mt][i] = a.bias ? a.bias[o0 + ob + 32 * mt + (i & 3) + 8 * (i >> 2)] : 0.f;
  }

  // ---- one pass: weight plane q against activation planes p0 .. p0 + P - 1
  auto pass = [&](auto planes_of_pass, int q, int p0) {
    constexpr int P = decltype(planes_of_pass)::value;
    constexpr int kChunk = kChunkMfma / P;       // K steps between two barriers: as many MFMAs per chunk with one plane as with two
    constexpr int kFrag = kChunk * MT;
    constexpr int kEnt = (kFrag * 64 + kThreads - 1) / kThreads;      // (fragment, lane) entries a thread expands per chunk
    static_assert(kFrag <= kFragMax, "ring buffer");
    const unsigned* __restrict__ xd = a.xd + (size_t)p0 * a.plane_dwords;
    const unsigned long long* __restrict__ wbits = a.wbits + (long long)q * a.steps * a.O;

    // the (tap, word) of the next step to request: steps are requested in order, so the pair follows with an add and a carry
    int ld_tap = 0, ld_j = 0;
    auto request = [&](int s0, unsigned (&x)[kChunk * P]) {
#pragma unroll
      for (int k = 0; k < kChunk; ++k) {
        if (s0 + k < a.steps) {                  // (uniform)
          const unsigned at = xbase + (unsigned)a.tap_xoff[ld_tap] + (unsigned)ld_j * a.word_dwords;
#pragma unroll
          for (int p = 0; p < P; ++p) x[k * P + p] = xd[at + (unsigned)p * a.plane_dwords];
          if (++ld_j == a.Gg) {
            ld_j = 0;
            ++ld_tap;
          }
        } else {
#pragma unroll
          for (int p = 0; p < P; ++p) x[k * P + p] = 0u;
        }
      }
    };
    // entry e of a thread: fragment f = (step of the chunk) MT + tile, lane L of the wave that will read it; L supplies
    // out-channel L & 31 and dword L >> 5 of the weight word (the k half its activation lanes supply)
    auto wload = [&](int s0, unsigned long long (&w)[kEnt]) {
#pragma unroll
      for (int e = 0; e < kEnt; ++e) {
        const int idx = tid + e * kThreads, L = idx & 63, f = idx >> 6;
        const int s = s0 + f / MT, mt = f % MT;
        w[e] = (idx < kFrag * 64 && s < a.steps) ? wbits[(long long)s * a.O + o0 + 32 * mt + (L & 31)] : 0ull;
      }
    };
    auto wstore = [&](int buf, const unsigned long long (&w)[kEnt]) {
#pragma unroll
      for (int e = 0; e < kEnt; ++e) {
        const int idx = tid + e * kThreads, L = idx & 63, f = idx >> 6;
        const unsigned d = (L >> 5) ? (unsigned)(w[e] >> 32) : (unsigned)w[e];
        // nibble j of register g = channel g + 4 j: +-(4, 2, 1, 4) as E2M1 codes 6 / 4 / 2 / 6, sign bit 8 where the weight is -1
        v4i out;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const unsigned mag = (g == 1 ? 0x4u : (g == 2 ? 0x2u : 0x6u)) * 0x11111111u;
          const unsigned ones = (d >> g) & 0x11111111u;
          out[g] = (int)(mag | ((ones ^ 0x11111111u) << 3));
        }
        if (idx < kFrag * 64) s_w[buf * kFrag + f][L] = out;
      }
    };

    // ---- the first chunk's operands go out before the tables are built: their latency hides behind it.  Both ring buffers
    // are free: every wave has passed the last barrier of the pass before, behind its last fragment read.
    unsigned xc[kChunk * P], xn[kChunk * P];
    unsigned long long wreg[kEnt];
    request(0, xc);
    wload(0, wreg);
    float xs[P];                                 // (several passes: requested here, a K loop ahead of the fold)
    if constexpr (MULTI) {
#pragma unroll
      for (int p = 0; p < P; ++p) xs[p] = a.xscales[(p0 + p) * a.N + n];
    }
    if (p0 == 0) build_tables(q);                // (uniform)
    wstore(0, wreg);
    __syncthreads();

    // ---- the accumulators start at the border term: minus the rectangle sum of plane q's wsum over the taps inside the image
    // hi and wi grow with the tap index, so the bounds of the rectangle are counts of taps below 0 and below the image's extent.
    v16f acc[P][MT];
    {
      int kh_lo = 0, kh_hi = 0, kw_lo = 0, kw_hi = 0;
      int h0 = hi0, w0 = wi0;                    // (opaque, as in build_tables: two registers across the passes, not four bounds
      asm volatile("" : "+v"(h0), "+v"(w0));     //  and four table addresses)
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) {
        const int hi = h0 + k * a.dh, wi = w0 + k * a.dw;
        kh_lo += (k < a.KH && hi < 0) ? 1 : 0;
        kh_hi += (k < a.KH && hi < a.H) ? 1 : 0;
        kw_lo += (k < a.KW && wi < 0) ? 1 : 0;
        kw_hi += (k < a.KW && wi < a.W) ? 1 : 0;
      }
      const int* __restrict__ p11 = &s_pre[kh_hi * W1 + kw_hi][ob];
      const int* __restrict__ p01 = &s_pre[kh_lo * W1 + kw_hi][ob];
      const int* __restrict__ p10 = &s_pre[kh_hi * W1 + kw_lo][ob];
      const int* __restrict__ p00 = &s_pre[kh_lo * W1 + kw_lo][ob];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int at = 32 * mt + 8 * g;
          const v4i inside = *reinterpret_cast<const v4i*>(p11 + at) - *reinterpret_cast<const v4i*>(p01 + at) -
                             *reinterpret_cast<const v4i*>(p10 + at) + *reinterpret_cast<const v4i*>(p00 + at);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int p = 0; p < P; ++p) acc[p][mt][4 * g + e] = (float)(-inside[e]);
          }
        }
    }

    // ---- the K loop.  Order of issue per chunk, pinned with scheduling barriers: the next chunk's activation dwords and
    // weight words first, then this chunk's fragment reads, v_and and MFMAs, then the next chunk's fragments into the other buffer.
    const int unit_scale = 0x7F7F7F7F;           // E8M0 127 = 2^0 in every byte: the block scales of both operands
    const int nchunks = (a.steps + kChunk - 1) / kChunk;
    for (int c = 0; c < nchunks; ++c) {
      const int s0 = c * kChunk;
      const bool more = c + 1 < nchunks;         // (uniform)
      if (more) {
        request(s0 + kChunk, xn);
        wload(s0 + kChunk, wreg);
      }
      __builtin_amdgcn_sched_barrier(0);
      const v4i (*__restrict__ wb)[64] = s_w + (c & 1) * kFrag;
#pragma unroll
      for (int k = 0; k < kChunk; ++k) {
        if (s0 + k < a.steps) {                  // (uniform: the last chunk may be partial)
          v8i b8[P];
#pragma unroll
          for (int p = 0; p < P; ++p) {
            const unsigned d = xc[k * P + p];
            b8[p] = v8i{(int)(d & 0x11111111u), (int)(d & 0x22222222u), (int)(d & 0x44444444u), (int)((d >> 3) & 0x11111111u), 0, 0, 0, 0};
          }
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const v4i w4 = wb[k * MT + mt][lane];
            const v8i w8 = {w4[0], w4[1], w4[2], w4[3], 0, 0, 0, 0};      // (fp4 operands: the low four registers are read)
#pragma unroll
            for (int p = 0; p < P; ++p)
              acc[p][mt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(w8, b8[p], acc[p][mt], 4, 4, 0, unit_scale, 0, unit_scale);
          }
          // (an empty asm on the accumulators ties each step to its place: the scaled MFMA is a pure value to the selector)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int p = 0; p < P; ++p) asm volatile("" : "+v"(acc[p][mt]));
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (more) {
        wstore((c + 1) & 1, wreg);
#pragma unroll
        for (int i = 0; i < kChunk * P; ++i) xc[i] = xn[i];
      }
      // buffer (c + 1) & 1 was last read in iteration c - 1, in front of that iteration's barrier; this one publishes it and
      // retires the reads of buffer c & 1 before iteration c + 1 (or the next pass) overwrites it
      lds_barrier();
    }

    // ---- the fold: the popcount kernel's arithmetic on the same integers -> the same floats
    auto fold = [&](int mt, int i, float base) {
      float v = xs[0] * acc[0][mt][i];
#pragma unroll
      for (int p = 1; p < P; ++p) v = fmaf(xs[p], acc[p][mt][i], v);
      return fmaf(v, s_scale[ob + 32 * mt + (i & 3) + 8 * (i >> 2)], base);
    };
    if constexpr (MULTI) {
      // (eight at a time: the scales of all 16 MT at once would stand beside the accumulators and the running values)
#pragma unroll
      for (int h = 0; h < 2 * MT; ++h) {
#pragma unroll
        for (int k = 0; k < 8; ++k) run[h >> 1][8 * (h & 1) + k] = fold(h >> 1, 8 * (h & 1) + k, run[h >> 1][8 * (h & 1) + k]);
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      // one pass: no running value, the accumulators go through the fold into the epilogue eight at a time
#pragma unroll
      for (int p = 0; p < P; ++p) xs[p] = a.xscales[p * a.N + n];
      epilogue([&](int mt, int i) { return fold(mt, i, s_bias[ob + 32 * mt + (i & 3) + 8 * (i >> 2)]); });
    }
  };

  if constexpr (MULTI) {
    for (int q = 0; q < a.kw_planes; ++q) {
      for (int p0 = 0; p0 < a.kx; p0 += 2) {
        if (KX == 2 && a.kx - p0 >= 2) pass(std::integral_constant<int, KX>{}, q, p0);
        else pass(std::integral_constant<int, 1>{}, q, p0);      // a lone last plane (or a call with one)
      }
    }
    epilogue([&](int mt, int i) { return run[mt][i]; });
  } else {
    pass(std::integral_constant<int, KX>{}, 0, 0);      // (its fold ends in the epilogue)
  }
}

template <typename T, int KX, int MT, bool MULTI>
int launch_one(const GenHalfArgs& a, hipStream_t st) {
  const long long ntiles = ((long long)a.N * a.Ho * a.Wo + 31) >> 5;
  const unsigned gx = (unsigned)((ntiles + kWaves - 1) / kWaves);
  hipLaunchKernelGGL((xnor_gen_half_kernel<T, KX, MT, MULTI>), dim3(gx, (unsigned)(a.O / (32 * MT))), dim3(kThreads), 0, st, a);
  return (int)hipGetLastError();
}

template <typename T>
int launch(const GenHalfArgs& a, hipStream_t st) {
  const bool multi = a.kw_planes * ((a.kx + 1) / 2) > 1, two = a.kx >= 2;
  // two tiles of 32 out-channels per wave where O allows it -- but not beside the running value of a call of several passes:
  // with 32 running values the MT = 2 instantiations do not fit the 128 registers of four waves per SIMD without scratch
  if (multi) return two ? launch_one<T, 2, 1, true>(a, st) : launch_one<T, 1, 1, true>(a, st);
  const bool wide = a.O % 64 == 0;
  if (two) return wide ? launch_one<T, 2, 2, false>(a, st) : launch_one<T, 2, 1, false>(a, st);
  return wide ? launch_one<T, 1, 2, false>(a, st) : launch_one<T, 1, 1, false>(a, st);
}

// 0 where the kernel takes (g, kx, kw_planes, dtype), else the code the entry point returns: the checks of
// lsq_xnor_conv2d_gen, then the dtype
int gen_half_check(const lsq_conv_geom* g, int kx, int kw_planes, int dtype) {
  if (int e = check_geom(g)) return e;
  if (kx < 1 || kx > LSQ_MAX_PLANES || kw_planes < 1 || kw_planes > LSQ_MAX_PLANES) return LSQ_E_SCHEME;
  const int Ho = out_h(g), Wo = out_w(g);
  if (Ho <= 0 || Wo <= 0) return LSQ_E_SHAPE;
  if (g->groups != 1 || g->C % 64 || g->O % 32) return LSQ_E_UNSUPPORTED;
  if (g->KH > kMaxK || g->KW > kMaxK || g->KH * g->KW > kMaxTaps) return LSQ_E_UNSUPPORTED;
  if ((long long)g->C * g->KH * g->KW >= (1ll << 23)) return LSQ_E_UNSUPPORTED;      // the fp32 accumulator holds the integer exactly
  if ((long long)g->N * g->O * Ho * Wo >= (1ll << 30)) return LSQ_E_UNSUPPORTED;     // 32-bit element offsets
  if (g->O / 32 > 65535) return LSQ_E_UNSUPPORTED;                                    // (grid.y)
  const long long Hp = g->H + 2ll * g->pad_h, Wp = g->W + 2ll * g->pad_w;
  if ((long long)g->N * (g->C / 64) * Hp * Wp * kx >= (1ll << 30)) return LSQ_E_UNSUPPORTED;      // 32-bit dword offsets
  if (dtype != LSQ_DTYPE_BF16 && dtype != LSQ_DTYPE_F16) return LSQ_E_UNSUPPORTED;
  return LSQ_OK;
}

}  // namespace
}  // namespace lsq

using namespace lsq;

extern "C" int lsq_conv_xnor_gen_half_abi_version(void) { return LSQ_CONV_XNOR_GEN_HALF_ABI_VERSION; }

extern "C" int lsq_xnor_conv2d_gen_half_supported(const lsq_conv_geom* g, int kx, int kw_planes, int dtype) {
  return gen_half_check(g, kx, kw_planes, dtype) == LSQ_OK ? 1 : 0;
}

extern "C" int lsq_xnor_conv2d_gen_half(const uint64_t* xplanes, int kx, const float* xscales, const uint64_t* wbits,
                                        const int32_t* wsum, int kw_planes, const float* wscales, const float* bias,
                                        const lsq_conv_geom* g, int act, const float* act_slope, const void* res_pre,
                                        const void* res_post, int dtype, void* y, void* stream) {
  if (!xplanes || !xscales || !wbits || !wsum || !wscales || !y) return LSQ_E_NULL;
  if (int e = gen_half_check(g, kx, kw_planes, dtype)) return e;
  if (act < LSQ_ACT_NONE || act > LSQ_ACT_PRELU_CHANNEL || (act >= LSQ_ACT_PRELU && !act_slope)) return LSQ_E_SCHEME;
  GenHalfArgs a = {};
  a.N = g->N; a.H = g->H; a.W = g->W; a.O = g->O; a.KH = g->KH; a.KW = g->KW;
  a.sh = g->stride_h; a.sw = g->stride_w; a.ph = g->pad_h; a.pw = g->pad_w; a.dh = g->dil_h; a.dw = g->dil_w;
  a.Gg = g->C / 64;
  a.Hp = g->H + 2 * g->pad_h; a.Wp = g->W + 2 * g->pad_w;
  a.Ho = out_h(g); a.Wo = out_w(g);
  a.steps = g->KH * g->KW * a.Gg;
  const long long xplane_words = lsq_act_plane_words(g), wplane_words = lsq_weight_plane_words(g);
  // (the layouts this kernel indexes: [N][C/64][Hp][Wp] words per activation plane, [taps][C/64][O] per weight plane)
  if (xplane_words != (long long)a.N * a.Gg * a.Hp * a.Wp || wplane_words != (long long)a.steps * a.O) return LSQ_E_UNSUPPORTED;
  a.plane_dwords = (unsigned)(2 * xplane_words);
  a.word_dwords = 2u * (unsigned)(a.Hp * a.Wp);
  for (int kh = 0; kh < g->KH; ++kh)
    for (int kw = 0; kw < g->KW; ++kw) a.tap_xoff[kh * g->KW + kw] = 2 * (kh * g->dil_h * a.Wp + kw * g->dil_w);
  a.xd = reinterpret_cast<const unsigned*>(xplanes);
  a.xscales = xscales;
  a.wbits = reinterpret_cast<const unsigned long long*>(wbits);
  a.wsum = wsum;
  a.wscales = wscales;
  a.bias = bias;
  a.slope = act_slope;
  a.act = act;
  a.res_pre = res_pre;
  a.res_post = res_post;
  a.y = y;
  a.kx = kx;
  a.kw_planes = kw_planes;
  hipStream_t st = (hipStream_t)stream;
  return dtype == LSQ_DTYPE_BF16 ? launch<__bf16>(a, st) : launch<_Float16>(a, st);
}
