// lsq_train_wgrad_half: weight and bias gradient of a binary-activation convolution from the activation sign planes and a
// 16-bit (bf16 / fp16) output gradient (gfx950).  The 16-bit counterpart of csrc/train/lsq_wgrad.hip, DESIGN 4.27.
//
// As a GEMM:  D[o][(c, tap)] = sum_p sum_n v_p[n] T_p,n[o][(c, tap)],  T_p,n = sum_(ho,wo) A[o][k] B_p[k][(c, tap)], with
//   A[o][k]           = grad_y[n][o][ho][wo] AS IT IS: a bf16 / fp16 value is an exact matrix-core operand, no scale, no split
//   B_p               = the sign operand of ../train/lsq_wgrad_core.h: exactly +-1 in grad_y's type, 0 on a halo word and past
//                       a sample's end
//   v_p[n]            = xscales[p][n], applied on the VALU to the partial sums of ONE sample (it is constant over them)
// so one v_mfma_f32_32x32x16_{bf16,f16} per sign fragment where the fp32 kernel issues three, and products without any rounding.
//
// Planes 2m, 2m + 1 whose scales are equal for a sample (ls-T) are one operand in {-2, 0, +2} with that one scale, so that
// x_q = 0 is an exact 0; the decision holds for all of a sample's positions.
//
// ../train/lsq_wgrad_core.h holds what this file shares with ../train/lsq_wgrad.hip: the constants, the tiles, the
// layout of the staged sign words, the K split, the reduce kernel (here with the bias rows) and the host rules.  Here: the
// main kernel; its sign-word steps (position, fold, staging, expansion, stores) read as in lsq_wgrad.hip and are kept in line in
// both files (lsq_wgrad_core.h says why).
// The reduction: every sample's Ho Wo positions are padded to whole k-steps of 16 with zero operands (sps steps a sample), so
// that a k-step never mixes two samples; the N sps steps are taken in chunks of four (64 k), which may hold up to four samples.
// Per chunk the workgroup stages A once (64 rows x 64 k of 16-bit values, for every plane) and per plane the sign words of its
// taps.  A wave then works the chunk one group of TG = 3 taps at a time: the group's partial sums t (3 x 16 registers, 48
// beside the 144 of the accumulators) over the chunk's k-steps, re-reading the A fragments from LDS for every group, and
//   acc = fma(v_p[n], t, acc)
// where the sample changes inside the chunk and at the chunk's end.  (The alternative, partial sums of all TT taps kept over a
// whole sample, needs 288 accumulator registers and a staging of A per plane: DESIGN 4.27 holds the choice.)
// The bias gradient: the workgroups of channel word 0 and tap tile 0 sum the staged A rows in fp32, a fixed quarter row per
// thread, the four quarters added in a fixed order at the end; with S > 1 the bias sums go behind the slabs and the reduce
// kernel adds them in slice order too.

#include "lsq_hip_train_half.h"
#include "../train/lsq_wgrad_core.h"

namespace {

constexpr int kTapGroup = 3;          // taps whose partial sums a wave holds at a time

template <int TT>
struct alignas(16) Smem {
  unsigned short a[kOT][kApitch];     // grad_y of the chunk, as it is; 0 past a sample's end and past O
  SignSmem<TT> s;
};

struct Args {
  const uint64_t* planes;
  const float* scales;
  const unsigned short* gy;
  float* out;                         // the slabs (S > 1)
  float* bias_part;                   // [S][OB] behind the slabs (S > 1 and grad_b)
  float* grad_wq;
  float* grad_b;                      // or NULL
  WgradGeom g;
  unsigned sps, KS, chunks;           // k-steps of a sample, k-steps and chunks in all
  WgradTiles t;
  int OB;
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
  const WgradGeom& e = a.g;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int split = blockIdx.x / a.t.tiles, tile = blockIdx.x % a.t.tiles;
  const int tc = tile % a.t.ntc, g = (tile / a.t.ntc) % e.Gt, ot = tile / (a.t.ntc * e.Gt);
  const int KK = e.KH * e.KW;
  const int ntaps = min(TT, KK - tc * TT);
  const unsigned c_begin = (unsigned)split * (unsigned)a.t.chunks_per_split;
  const unsigned c_end = min(a.chunks, c_begin + (unsigned)a.t.chunks_per_split);
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
      const int cnt = ksi < a.KS && hw0 < e.HoWo ? (int)min(8u, e.HoWo - hw0) : 0;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int o = ot * kOT + r0 + 32 * r;
        uint4 q = make_uint4(0, 0, 0, 0);
        if (cnt > 0 && o < e.O) {
          const unsigned short* src = a.gy + ((size_t)n * e.O + o) * e.HoWo + hw0;
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
      if (ksi < a.KS && hw < e.HoWo) {
        const int ho = (int)(hw / (unsigned)e.Wo), wo = (int)(hw - (unsigned)ho * e.Wo);
        pn = (int)n;
        pho = ho * e.s;
        pwo = wo * e.s;
        wbase = ((long long)n * e.Gt + g) * e.Hp * e.Wp + (long long)pho * e.Wp + pwo;
      }
    }

    for (int p = 0; p < a.t.kx; ++p) {
      // FOLD: planes 2m and 2m + 1 with equal scales for a sample (ls-T: v2 = v1) are one operand v (s_2m + s_2m+1) in
      // {-2v, 0, 2v} -- a value of 0 is then an exact 0, not v - v accumulated separately in fp32
      int fold = 0;                        // this thread's chunk position: 1 = plane p carries p + 1 too, 2 = folded away
      if (FOLD && wbase >= 0) {
        const int n = pn;
        if ((p & 1) == 0 && p + 1 < a.t.kx && a.scales[(size_t)p * e.N + n] == a.scales[(size_t)(p + 1) * e.N + n]) fold = 1;
        if ((p & 1) == 1 && a.scales[(size_t)p * e.N + n] == a.scales[(size_t)(p - 1) * e.N + n]) fold = 2;
      }
      if (p > 0) __syncthreads();          // the previous plane's sign words have been read
#pragma unroll
      for (int m = 0; m < (TT + 3) / 4; ++m) {
        const int tl = (t >> 6) + 4 * m;
        if (tl < TT) {
          unsigned plo = 0, phi = 0, zlo = 0, zhi = 0;
          unsigned short b0 = 0;
          if (wbase >= 0 && tl < ntaps && fold != 2) {
            const int tap = tc * TT + tl, i = tap / e.KW, j = tap - (tap / e.KW) * e.KW;
            const int hh = pho + i - e.ph, ww = pwo + j - e.pw;
            if (hh >= 0 && hh < e.H && ww >= 0 && ww < e.W) {
              const long long at = wbase + (long long)i * e.Wp + j;
              const uint64_t word = a.planes[p * e.plane_words + at];
              plo = ~(unsigned)word;
              phi = ~(unsigned)(word >> 32);
              b0 = F16 ? 0x3C00 : 0x3F80;
              if (FOLD && fold == 1) {
                const uint64_t diff = word ^ a.planes[(p + 1) * e.plane_words + at];
                zlo = (unsigned)diff;
                zhi = (unsigned)(diff >> 32);
                b0 = 0x4000;
              }
            }
          }
          sm.s.p[tl][0][kp] = plo;
          sm.s.p[tl][1][kp] = phi;
          if (FOLD) {
            sm.s.z[tl][0][kp] = zlo;
            sm.s.z[tl][1][kp] = zhi;
          }
          sm.s.b0[tl][kp] = b0;
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
      for (int ks = 0; ks < 4; ++ks) v[ks] = a.scales[(size_t)p * e.N + ns[ks]];

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
                const uint4 p0 = *(const uint4*)&sm.s.p[tl][wc][k8];
                const uint4 p1 = *(const uint4*)&sm.s.p[tl][wc][k8 + 4];
                const uint4 bb = *(const uint4*)&sm.s.b0[tl][k8];
                const unsigned pw_[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
                const unsigned b0_[4] = {bb.x, bb.y, bb.z, bb.w};
                Frag fb;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                  const unsigned e0 = (pw_[2 * q] >> lr) & 1u, e1 = (pw_[2 * q + 1] >> lr) & 1u;
                  fb.u[q] = b0_[q] + ((e0 | (e1 << 16)) << 15);
                }
                if (FOLD) {
                  const uint4 z0 = *(const uint4*)&sm.s.z[tl][wc][k8];
                  const uint4 z1 = *(const uint4*)&sm.s.z[tl][wc][k8 + 4];
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
      if (a.t.S == 1) {
        if (o < e.O) a.grad_b[o] = bsum;
      } else {
        a.bias_part[(size_t)split * a.OB + o] = bsum;
      }
    }
  }

  // ---- epilogue: column c = lane & 31, row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int c = g * 64 + 32 * wc + lr;
  if (a.t.S == 1) {
#pragma unroll
    for (int tl = 0; tl < TT; ++tl) {
      if (tl < ntaps && c < e.C) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int o = d_row(ot * kOT + 32 * wo_, reg, lh);
          if (o < e.O) a.grad_wq[((size_t)o * e.C + c) * KK + tc * TT + tl] = acc[tl][reg];
        }
      }
    }
  } else {
    float* slab = a.out + ((((size_t)split * a.t.tiles + tile) * 4 + w) * TT) * 16 * 64 + lane;
#pragma unroll
    for (int tl = 0; tl < TT; ++tl) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) slab[(tl * 16 + reg) * 64] = acc[tl][reg];
    }
  }
}

// N sps <= N Ho Wo < 2^31 (check_geom): k-step and chunk counts fit 32 bits (the padded positions 16 N sps are never formed)
struct Plan {
  unsigned sps, KS, chunks;
  int OB;
  TilePlan tp;
};

Plan plan(const WgradGeom& g, int kx) {
  Plan p;
  p.sps = (g.HoWo + 15) / 16;
  p.KS = (unsigned)g.N * p.sps;
  p.chunks = (p.KS + 3) / 4;
  p.OB = ((g.O + kOT - 1) / kOT) * kOT;
  p.tp = tile_plan(g, kx, p.chunks);
  return p;
}

size_t workspace_need(const Plan& p, bool with_bias) {
  if (p.tp.t.S <= 1) return 0;
  return ((size_t)p.tp.t.S * p.tp.slab_floats + (with_bias ? (size_t)p.tp.t.S * p.OB : 0)) * sizeof(float);
}

template <bool F16>
const WgradKernels<Args> kKernels = {
    {{wgrad_half_kernel<1, false, F16>, wgrad_half_kernel<1, true, F16>},
     {wgrad_half_kernel<kTapTile, false, F16>, wgrad_half_kernel<kTapTile, true, F16>}},
    {wgrad_reduce_kernel<1, true, Args>, wgrad_reduce_kernel<kTapTile, true, Args>}};

}  // namespace

extern "C" int lsq_train_half_abi_version(void) { return LSQ_TRAIN_HALF_ABI_VERSION; }

extern "C" size_t lsq_train_wgrad_half_workspace_bytes(const lsq_conv_geom* g, int kx, int with_bias) {
  if (check_geom(g, kx) != LSQ_OK) return 0;
  return workspace_need(plan(fill_geom(g), kx), with_bias != 0);
}

extern "C" int lsq_train_wgrad_half(const uint64_t* xplanes, int kx, const float* xscales, const void* grad_y, int dtype,
                                    const lsq_conv_geom* g, float* grad_wq, float* grad_b, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  if (const int e = check_geom(g, kx)) return e;
  if (!xplanes || !xscales || !grad_y || !grad_wq) return LSQ_E_NULL;
  if (dtype != LSQ_DTYPE_BF16 && dtype != LSQ_DTYPE_F16) return LSQ_E_UNSUPPORTED;
  if (((uintptr_t)grad_y & 1) || ((uintptr_t)grad_wq & 3) || ((uintptr_t)grad_b & 3)) return LSQ_E_UNSUPPORTED;
  Args a;
  a.g = fill_geom(g);
  const Plan p = plan(a.g, kx);
  if (const int e = check_workspace(workspace_need(p, grad_b != nullptr), workspace, workspace_bytes)) return e;
  a.t = p.tp.t;
  a.planes = xplanes;
  a.scales = xscales;
  a.gy = (const unsigned short*)grad_y;
  a.grad_wq = grad_wq;
  a.grad_b = grad_b;
  a.out = (float*)workspace;
  a.bias_part = p.tp.t.S > 1 ? (float*)workspace + (size_t)p.tp.t.S * p.tp.slab_floats : nullptr;
  a.sps = p.sps;
  a.KS = p.KS;
  a.chunks = p.chunks;
  a.OB = p.OB;
  const WgradKernels<Args>& k = dtype == LSQ_DTYPE_F16 ? kKernels<true> : kKernels<false>;
  return launch_wgrad(k, a, p.tp, kx > 1, p.OB, (hipStream_t)stream);
}
