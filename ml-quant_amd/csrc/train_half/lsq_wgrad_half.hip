// lsq_train_wgrad_half: weight and bias gradient of a binary-activation convolution from the activation sign planes and a
// 16-bit (bf16 / fp16) output gradient (gfx950).  The 16-bit counterpart of csrc/train/lsq_wgrad.hip, DESIGN 4.27.
//
// As a GEMM:  D[o][(c, tap)] = sum_p sum_n v_p[n] T_p,n[o][(c, tap)],  T_p,n = sum_(ho,wo) A[o][k] B_p[k][(c, tap)], with
//   A[o][k]           = grad_y[n][o][ho][wo] AS IT IS: a bf16 / fp16 value is an exact matrix-core operand, no scale, no split
//   B_p[k][(c, i, j)] = 2 bit_p - 1 of channel c at padded pixel (ho s + i, wo s + j): exactly +-1 in grad_y's type, or 0 on a
//                       halo word and past a sample's end
//   v_p[n]            = xscales[p][n], applied on the VALU to the partial sums of ONE sample (it is constant over them)
// so one v_mfma_f32_32x32x16_{bf16,f16} per sign fragment where the fp32 kernel issues three, and products without any rounding.
// Planes 2m, 2m + 1 whose scales are equal for a sample (ls-T) are one operand in {-2, 0, +2} with that one scale, so that
// x_q = 0 is an exact 0; the decision holds for all of a sample's positions.
//
// The reduction: every sample's Ho Wo positions are padded to whole k-steps of 16 with zero operands (sps steps a sample), so
// that a k-step never mixes two samples; the N sps steps are taken in chunks of four (64 k), which may hold up to four samples.
// Tiles: as lsq_wgrad.hip, a workgroup (4 waves) owns 64 output channels x 64 input channels (one plane word) x up to TT taps,
// every wave a 32 x 32 block of (o, c) for each of the tile's taps (TT accumulators of 16 registers).  Per chunk the workgroup
// stages A once (64 rows x 64 k of 16-bit values, for every plane) and per plane the sign words of its taps.  A wave then
// works the chunk one group of TG = 3 taps at a time: the group's partial sums t (3 x 16 registers, 48 beside the 144 of the
// accumulators) over the chunk's k-steps, re-reading the A fragments from LDS for every group, and
//   acc = fma(v_p[n], t, acc)
// where the sample changes inside the chunk and at the chunk's end.  (The alternative, partial sums of all TT taps kept over a
// whole sample, needs 288 accumulator registers and a staging of A per plane: DESIGN 4.27 holds the choice.)
// The bias gradient: the workgroups of channel word 0 and tap tile 0 sum the staged A rows in fp32, a fixed quarter row per
// thread, the four quarters added in a fixed order at the end.
// Split-K: the chunks are cut into S slices (S from the geometry alone: about kTargetGroups workgroups).  With S > 1 every
// workgroup stores its accumulators as a slab in MFMA order (coalesced) and its bias sums behind the slabs; a second launch
// sums the S partial sums of each output element in slice order -- bitwise deterministic, no atomics.  S = 1 writes grad_wq
// and grad_b directly.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsq_hip_train_half.h"
#include "../linear/lsq_signw_mma.h"     // Frag, f32x16, mfma16<F16>

namespace {

constexpr int kThreads = 256;
constexpr int kKC = 64;               // k per chunk: four k-steps
constexpr int kOT = 64;               // output channels per workgroup
constexpr int kApitch = kKC + 8;      // 16-bit values per staged A row (16-byte pad: the row reads of a wave fall on distinct banks)
constexpr int kTargetGroups = 512;    // workgroups the K split aims at (2 per CU)
constexpr int kTapTile = 9;           // taps per workgroup for kernels larger than 1x1
constexpr int kTapGroup = 3;          // taps whose partial sums a wave holds at a time

template <int TT>
struct alignas(16) Smem {
  unsigned short a[kOT][kApitch];     // grad_y of the chunk, as it is; 0 past a sample's end and past O
  unsigned p[TT][2][kKC];             // ~(word half) of tap tl at chunk position k; 0 on the halo / past the end
  unsigned z[TT][2][kKC];             // channels whose value is 0 (a folded pair of planes with opposite signs)
  unsigned short b0[TT][kKC];         // +1 (0x3F80 bf16, 0x3C00 fp16) or +2 (0x4000 in both, a folded pair) where the sign is real, else 0
};

struct Args {
  const uint64_t* planes;
  const float* scales;
  const unsigned short* gy;
  float* out;                         // the slabs (S > 1)
  float* bias_part;                   // [S][OB] behind the slabs (S > 1 and grad_b)
  float* grad_wq;
  float* grad_b;                      // or NULL
  long long plane_words;
  int N, C, H, W, O, KH, KW, s, ph, pw, Ho, Wo, Hp, Wp, Gt;
  unsigned HoWo, sps, KS, chunks;     // positions and k-steps of a sample, k-steps and chunks in all
  int kx, ntc, tiles, chunks_per_split, S, OB;
};

template <bool F16>
__device__ __forceinline__ float widen(unsigned short b) {
  if constexpr (F16) return (float)__builtin_bit_cast(_Float16, b);
  else return __uint_as_float((unsigned)b << 16);
}

template <int TT, bool FOLD, bool F16>
__global__ __launch_bounds__(kThreads) void wgrad_half_kernel(Args a) {
  constexpr int TG = TT == 1 ? 1 : kTapGroup;
  static_assert(TT % TG == 0, "whole tap groups");
  __shared__ Smem<TT> sm;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int split = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  const int tc = tile % a.ntc, g = (tile / a.ntc) % a.Gt, ot = tile / (a.ntc * a.Gt);
  const int KK = a.KH * a.KW;
  const int ntaps = min(TT, KK - tc * TT);
  const unsigned c_begin = (unsigned)split * (unsigned)a.chunks_per_split;
  const unsigned c_end = min(a.chunks, c_begin + (unsigned)a.chunks_per_split);
  const bool bias = a.grad_b != nullptr && g == 0 && tc == 0;      // (uniform over the workgroup)

  // staging roles: A rows r0 and r0 + 32 at chunk positions kq .. kq + 7 (one half of a k-step); sign words of chunk position
  // kp, taps t>>6 + 4m; bias: a quarter (16 k) of row t >> 2
  const int r0 = t >> 3, kq = (t & 7) * 8, kp = t & 63;
  // compute roles: wave (wo_, wc) owns rows 32 wo_ .. +31 and channels 32 wc .. +31 of the tile
  const int wo_ = w & 1, wc = w >> 1, lr = lane & 31, lh = lane >> 5;

  f32x16 acc[TT];
#pragma unroll
  for (int tl = 0; tl < TT; ++tl) acc[tl] = f32x16{};
  float bsum = 0.f;

  for (unsigned ch = c_begin; ch < c_end; ++ch) {
    // the sample of each of the chunk's k-steps (uniform); a step past the end takes the last sample's and holds zeros
    unsigned ns[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) ns[ks] = min(ch * 4 + ks, a.KS - 1) / a.sps;

    __syncthreads();                       // the previous chunk's fragments and rows have been read
    // ---- A operand: grad_y of this chunk, once for every plane
    {
      const unsigned ksi = ch * 4 + (unsigned)(kq >> 4);
      const unsigned n = ksi / a.sps, hw0 = (ksi - n * a.sps) * 16 + (unsigned)(kq & 15);
      const int cnt = ksi < a.KS && hw0 < a.HoWo ? (int)min(8u, a.HoWo - hw0) : 0;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int o = ot * kOT + r0 + 32 * r;
        uint4 q = make_uint4(0, 0, 0, 0);
        if (cnt > 0 && o < a.O) {
          const unsigned short* src = a.gy + ((size_t)n * a.O + o) * a.HoWo + hw0;
          if (cnt == 8 && ((uintptr_t)src & 15) == 0) {
            q = *(const uint4*)src;
          } else {
            unsigned short h[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) h[j] = j < cnt ? src[j] : (unsigned short)0;
            q = make_uint4(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16), h[4] | ((unsigned)h[5] << 16),
                           h[6] | ((unsigned)h[7] << 16));
          }
        }
        *(uint4*)&sm.a[r0 + 32 * r][kq] = q;
      }
    }
    // ---- sign words: this thread's chunk position
    long long wbase = -1;
    int pho = 0, pwo = 0, pn = 0;
    {
      const unsigned ksi = ch * 4 + (unsigned)(kp >> 4);
      const unsigned n = ksi / a.sps, hw = (ksi - n * a.sps) * 16 + (unsigned)(kp & 15);
      if (ksi < a.KS && hw < a.HoWo) {
        const int ho = (int)(hw / (unsigned)a.Wo), wo = (int)(hw - (unsigned)ho * a.Wo);
        pn = (int)n;
        pho = ho * a.s;
        pwo = wo * a.s;
        wbase = ((long long)n * a.Gt + g) * a.Hp * a.Wp + (long long)pho * a.Wp + pwo;
      }
    }

    for (int p = 0; p < a.kx; ++p) {
      // FOLD: planes 2m and 2m + 1 with equal scales for a sample (ls-T: v2 = v1) are one operand v (s_2m + s_2m+1) in
      // {-2v, 0, 2v} -- a value of 0 is then an exact 0, not v - v accumulated separately in fp32
      int fold = 0;                        // this thread's chunk position: 1 = plane p carries p + 1 too, 2 = folded away
      if (FOLD && wbase >= 0) {
        const int n = pn;
        if ((p & 1) == 0 && p + 1 < a.kx && a.scales[(size_t)p * a.N + n] == a.scales[(size_t)(p + 1) * a.N + n]) fold = 1;
        if ((p & 1) == 1 && a.scales[(size_t)p * a.N + n] == a.scales[(size_t)(p - 1) * a.N + n]) fold = 2;
      }
      if (p > 0) __syncthreads();          // the previous plane's sign words have been read
#pragma unroll
      for (int m = 0; m < (TT + 3) / 4; ++m) {
        const int tl = (t >> 6) + 4 * m;
        if (tl < TT) {
          unsigned plo = 0, phi = 0, zlo = 0, zhi = 0;
          unsigned short b0 = 0;
          if (wbase >= 0 && tl < ntaps && fold != 2) {
            const int tap = tc * TT + tl, i = tap / a.KW, j = tap - (tap / a.KW) * a.KW;
            const int hh = pho + i - a.ph, ww = pwo + j - a.pw;
            if (hh >= 0 && hh < a.H && ww >= 0 && ww < a.W) {
              const long long at = wbase + (long long)i * a.Wp + j;
              const uint64_t word = a.planes[p * a.plane_words + at];
              plo = ~(unsigned)word;
              phi = ~(unsigned)(word >> 32);
              b0 = F16 ? 0x3C00 : 0x3F80;
              if (FOLD && fold == 1) {
                const uint64_t diff = word ^ a.planes[(p + 1) * a.plane_words + at];
                zlo = (unsigned)diff;
                zhi = (unsigned)(diff >> 32);
                b0 = 0x4000;
              }
            }
          }
          sm.p[tl][0][kp] = plo;
          sm.p[tl][1][kp] = phi;
          if (FOLD) {
            sm.z[tl][0][kp] = zlo;
            sm.z[tl][1][kp] = zhi;
          }
          sm.b0[tl][kp] = b0;
        }
      }
      __syncthreads();

      if (p == 0 && bias) {                // the staged rows, widened exactly: 16 k of row t >> 2
        const uint4 q0 = *(const uint4*)&sm.a[t >> 2][16 * (t & 3)];
        const uint4 q1 = *(const uint4*)&sm.a[t >> 2][16 * (t & 3) + 8];
        const unsigned d[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          bsum += widen<F16>((unsigned short)(d[j] & 0xFFFFu));
          bsum += widen<F16>((unsigned short)(d[j] >> 16));
        }
      }

      float v[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) v[ks] = a.scales[(size_t)p * a.N + ns[ks]];

#pragma unroll
      for (int grp = 0; grp < TT / TG; ++grp) {
        if (grp * TG < ntaps) {
          f32x16 ts[TG];
#pragma unroll
          for (int j = 0; j < TG; ++j) ts[j] = f32x16{};
#pragma unroll
          for (int ks = 0; ks < kKC / 16; ++ks) {
            const int k8 = 16 * ks + 8 * lh;
            Frag fa;
            {
              const uint4 q = *(const uint4*)&sm.a[32 * wo_ + lr][k8];
              fa.u[0] = q.x; fa.u[1] = q.y; fa.u[2] = q.z; fa.u[3] = q.w;
            }
#pragma unroll
            for (int j = 0; j < TG; ++j) {
              const int tl = grp * TG + j;
              if (tl < ntaps) {
                const uint4 p0 = *(const uint4*)&sm.p[tl][wc][k8];
                const uint4 p1 = *(const uint4*)&sm.p[tl][wc][k8 + 4];
                const uint4 bb = *(const uint4*)&sm.b0[tl][k8];
                const unsigned pw_[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
                const unsigned b0_[4] = {bb.x, bb.y, bb.z, bb.w};
                Frag fb;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                  const unsigned e0 = (pw_[2 * q] >> lr) & 1u, e1 = (pw_[2 * q + 1] >> lr) & 1u;
                  fb.u[q] = b0_[q] + ((e0 | (e1 << 16)) << 15);
                }
                if (FOLD) {
                  const uint4 z0 = *(const uint4*)&sm.z[tl][wc][k8];
                  const uint4 z1 = *(const uint4*)&sm.z[tl][wc][k8 + 4];
                  const unsigned zw_[8] = {z0.x, z0.y, z0.z, z0.w, z1.x, z1.y, z1.z, z1.w};
#pragma unroll
                  for (int q = 0; q < 4; ++q) {
                    const unsigned d0 = (zw_[2 * q] >> lr) & 1u, d1 = (zw_[2 * q + 1] >> lr) & 1u;
                    fb.u[q] &= ~((d0 | (d1 << 16)) * 0xFFFFu);
                  }
                }
                ts[j] = mfma16<F16>(fa, fb, ts[j]);
              }
            }
            // the sample's scale, once for its partial sums: where the next k-step is another sample's, and at the chunk's end
            if (ks == kKC / 16 - 1 || ns[ks + 1 < 4 ? ks + 1 : 3] != ns[ks]) {
#pragma unroll
              for (int j = 0; j < TG; ++j) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg)
                  acc[grp * TG + j][reg] = __builtin_fmaf(v[ks], ts[j][reg], acc[grp * TG + j][reg]);
                ts[j] = f32x16{};
              }
            }
          }
        }
      }
    }
  }

  // ---- the bias gradient of rows t >> 2: quarters (0 + 1) + (2 + 3)
  if (bias) {
    bsum += __shfl_xor(bsum, 1);
    bsum += __shfl_xor(bsum, 2);
    const int row = t >> 2, o = ot * kOT + row;
    if ((t & 3) == 0) {
      if (a.S == 1) {
        if (o < a.O) a.grad_b[o] = bsum;
      } else {
        a.bias_part[(size_t)split * a.OB + o] = bsum;
      }
    }
  }

  // ---- epilogue: column c = lane & 31, row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int c = g * 64 + 32 * wc + lr;
  if (a.S == 1) {
#pragma unroll
    for (int tl = 0; tl < TT; ++tl) {
      if (tl < ntaps && c < a.C) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int o = d_row(ot * kOT + 32 * wo_, reg, lh);
          if (o < a.O) a.grad_wq[((size_t)o * a.C + c) * KK + tc * TT + tl] = acc[tl][reg];
        }
      }
    }
  } else {
    float* slab = a.out + ((((size_t)split * a.tiles + tile) * 4 + w) * TT) * 16 * 64 + lane;
#pragma unroll
    for (int tl = 0; tl < TT; ++tl) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) slab[(tl * 16 + reg) * 64] = acc[tl][reg];
    }
  }
}

// Sum of the S partial sums of every output element, in slice order.  Thread = one slab position (MFMA order), and behind
// the slab one bias element.
template <int TT>
__global__ __launch_bounds__(kThreads) void wgrad_half_reduce_kernel(Args a) {
  const size_t slab = (size_t)a.tiles * 4 * TT * 16 * 64;
  const size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= slab) {
    const size_t o = idx - slab;
    if (a.grad_b == nullptr || o >= (size_t)a.O) return;
    float sum = a.bias_part[o];
    for (int s = 1; s < a.S; ++s) sum += a.bias_part[(size_t)s * a.OB + o];
    a.grad_b[o] = sum;
    return;
  }
  const int lane = (int)(idx & 63), reg = (int)((idx >> 6) & 15);
  const size_t rest = idx >> 10;
  const int tl = (int)(rest % TT), w = (int)((rest / TT) % 4), tile = (int)(rest / (TT * 4));
  const int tc = tile % a.ntc, g = (tile / a.ntc) % a.Gt, ot = tile / (a.ntc * a.Gt);
  const int KK = a.KH * a.KW, tap = tc * TT + tl;
  const int c = g * 64 + 32 * (w >> 1) + (lane & 31);
  const int o = d_row(ot * kOT + 32 * (w & 1), reg, lane >> 5);
  if (tap >= KK || c >= a.C || o >= a.O) return;
  float sum = a.out[idx];
  for (int s = 1; s < a.S; ++s) sum += a.out[(size_t)s * slab + idx];
  a.grad_wq[((size_t)o * a.C + c) * KK + tap] = sum;
}

struct Plan {
  int TT, ntc, tiles, S, chunks_per_split, OB;
  unsigned HoWo, sps, KS, chunks;
  size_t slab_floats;
};

// the refusals of lsq_train_wgrad (csrc/train/lsq_wgrad.hip), with its codes
int check_geom(const lsq_conv_geom* g, int kx) {
  if (!g) return LSQ_E_NULL;
  if (kx < 1 || kx > LSQ_MAX_PLANES) return LSQ_E_SCHEME;
  if (g->N < 1 || g->C < 1 || g->H < 1 || g->W < 1 || g->O < 1 || g->KH < 1 || g->KW < 1 || g->stride_h < 1 ||
      g->stride_w < 1 || g->pad_h < 0 || g->pad_w < 0 || g->dil_h < 1 || g->dil_w < 1 || g->groups < 1)
    return LSQ_E_SHAPE;
  if (g->C % g->groups || g->O % g->groups) return LSQ_E_SHAPE;
  const long long ho = ((long long)g->H + 2 * g->pad_h - (long long)g->dil_h * (g->KH - 1) - 1) / g->stride_h + 1;
  const long long wo = ((long long)g->W + 2 * g->pad_w - (long long)g->dil_w * (g->KW - 1) - 1) / g->stride_w + 1;
  if (g->H + 2 * g->pad_h < g->dil_h * (g->KH - 1) + 1 || g->W + 2 * g->pad_w < g->dil_w * (g->KW - 1) + 1 || ho < 1 || wo < 1)
    return LSQ_E_SHAPE;
  if (g->groups != 1 || g->dil_h != 1 || g->dil_w != 1 || g->stride_h != g->stride_w || g->stride_h > 2)
    return LSQ_E_UNSUPPORTED;
  if (g->KH > 8 || g->KW > 8 || g->pad_h > g->KH - 1 || g->pad_w > g->KW - 1) return LSQ_E_UNSUPPORTED;
  if ((long long)g->N * ho * wo >= (1ll << 31) || g->O > 65535 || g->C > 65535) return LSQ_E_UNSUPPORTED;
  return LSQ_OK;
}

// N sps <= N Ho Wo < 2^31: k-step and chunk counts fit 32 bits (the padded positions 16 N sps are never formed)
Plan plan(const lsq_conv_geom* g) {
  Plan p;
  const int KK = g->KH * g->KW;
  const int ho = (g->H + 2 * g->pad_h - g->KH) / g->stride_h + 1, wo = (g->W + 2 * g->pad_w - g->KW) / g->stride_w + 1;
  p.HoWo = (unsigned)ho * (unsigned)wo;
  p.sps = (p.HoWo + 15) / 16;
  p.KS = (unsigned)g->N * p.sps;
  p.chunks = (p.KS + 3) / 4;
  p.TT = KK == 1 ? 1 : kTapTile;
  p.ntc = (KK + p.TT - 1) / p.TT;
  p.tiles = ((g->O + kOT - 1) / kOT) * ((g->C + 63) / 64) * p.ntc;
  p.OB = ((g->O + kOT - 1) / kOT) * kOT;
  const long long chunks = p.chunks;
  long long S = (kTargetGroups + p.tiles - 1) / p.tiles;
  if (S > chunks) S = chunks;
  if (S < 1) S = 1;
  p.chunks_per_split = (int)((chunks + S - 1) / S);
  p.S = (int)((chunks + p.chunks_per_split - 1) / p.chunks_per_split);
  p.slab_floats = (size_t)p.tiles * 4 * p.TT * 16 * 64;
  return p;
}

size_t workspace_need(const Plan& p, bool with_bias) {
  if (p.S <= 1) return 0;
  return ((size_t)p.S * p.slab_floats + (with_bias ? (size_t)p.S * p.OB : 0)) * sizeof(float);
}

template <int TT, bool F16>
void launch(const Args& a, const Plan& p, bool fold, hipStream_t st) {
  const dim3 grid((unsigned)(p.tiles * p.S)), block(kThreads);
  const dim3 rgrid((unsigned)((p.slab_floats + p.OB + kThreads - 1) / kThreads));
  if (fold) hipLaunchKernelGGL((wgrad_half_kernel<TT, true, F16>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((wgrad_half_kernel<TT, false, F16>), grid, block, 0, st, a);
  if (p.S > 1) hipLaunchKernelGGL(wgrad_half_reduce_kernel<TT>, rgrid, block, 0, st, a);
}

}  // namespace

extern "C" int lsq_train_half_abi_version(void) { return LSQ_TRAIN_HALF_ABI_VERSION; }

extern "C" size_t lsq_train_wgrad_half_workspace_bytes(const lsq_conv_geom* g, int kx, int with_bias) {
  if (check_geom(g, kx) != LSQ_OK) return 0;
  return workspace_need(plan(g), with_bias != 0);
}

extern "C" int lsq_train_wgrad_half(const uint64_t* xplanes, int kx, const float* xscales, const void* grad_y, int dtype,
                                    const lsq_conv_geom* g, float* grad_wq, float* grad_b, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  if (const int e = check_geom(g, kx)) return e;
  if (!xplanes || !xscales || !grad_y || !grad_wq) return LSQ_E_NULL;
  if (dtype != LSQ_DTYPE_BF16 && dtype != LSQ_DTYPE_F16) return LSQ_E_UNSUPPORTED;
  if (((uintptr_t)grad_y & 1) || ((uintptr_t)grad_wq & 3) || ((uintptr_t)grad_b & 3)) return LSQ_E_UNSUPPORTED;
  const Plan p = plan(g);
  const size_t need = workspace_need(p, grad_b != nullptr);
  if (need > 0 && !workspace) return LSQ_E_NULL;
  if (workspace_bytes < need || ((uintptr_t)workspace & 15)) return LSQ_E_WORKSPACE;
  Args a;
  a.planes = xplanes;
  a.scales = xscales;
  a.gy = (const unsigned short*)grad_y;
  a.grad_wq = grad_wq;
  a.grad_b = grad_b;
  a.out = (float*)workspace;
  a.bias_part = p.S > 1 ? (float*)workspace + (size_t)p.S * p.slab_floats : nullptr;
  a.N = g->N; a.C = g->C; a.H = g->H; a.W = g->W; a.O = g->O; a.KH = g->KH; a.KW = g->KW;
  a.s = g->stride_h; a.ph = g->pad_h; a.pw = g->pad_w;
  a.Ho = (g->H + 2 * g->pad_h - g->KH) / g->stride_h + 1;
  a.Wo = (g->W + 2 * g->pad_w - g->KW) / g->stride_w + 1;
  a.Hp = g->H + 2 * g->pad_h;
  a.Wp = g->W + 2 * g->pad_w;
  a.Gt = (g->C + 63) / 64;
  a.HoWo = p.HoWo;
  a.sps = p.sps;
  a.KS = p.KS;
  a.chunks = p.chunks;
  a.plane_words = (long long)g->N * a.Gt * a.Hp * a.Wp;
  a.kx = kx;
  a.ntc = p.ntc;
  a.tiles = p.tiles;
  a.chunks_per_split = p.chunks_per_split;
  a.S = p.S;
  a.OB = p.OB;
  hipStream_t st = (hipStream_t)stream;
  const bool fold = kx > 1, f16 = dtype == LSQ_DTYPE_F16;
  if (p.TT == 1) {
    if (f16) launch<1, true>(a, p, fold, st);
    else launch<1, false>(a, p, fold, st);
  } else {
    if (f16) launch<kTapTile, true>(a, p, fold, st);
    else launch<kTapTile, false>(a, p, fold, st);
  }
  return (int)hipGetLastError();
}
