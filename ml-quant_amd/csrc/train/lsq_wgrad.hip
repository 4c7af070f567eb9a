// lsq_train_wgrad: weight gradient of a binary-activation convolution from the activation sign planes (gfx950).
//
// As a GEMM:  D[o][(c, tap)] = sum_k A_p[o][k] B_p[k][(c, tap)], summed over the planes p, with
//   k = (n, ho, wo)                                  K = N Ho Wo, the reduction
//   A_p[o][k] = xscales[p][n] * grad_y[n][o][ho][wo] fp32, split into three bf16 terms hi + mid + lo
//   B_p                                              the sign operand of lsq_wgrad_core.h, +-1 in bf16
// One sign fragment serves the three terms (three v_mfma_f32_32x32x16_bf16 per fragment).  hi = bf16(a), mid = bf16(a - hi),
// lo = bf16(a - hi - mid): each subtraction is exact in fp32 and each term carries the next 8 bits, so hi + mid + lo is a
// to within 2^-24 |a| -- the products with +-1 are exact and the MFMA accumulates in fp32.  No scaling: bf16 has fp32's exponent range.
//
// Planes 2m, 2m + 1 whose scales are equal for a sample (ls-T) are folded into one operand in {-2, 0, +2}, so that x_q = 0 is an
// exact 0 rather than +v - v accumulated in fp32 (which misses sum |gy| |x_q| by far more than an fp32 rounding).
//
// lsq_wgrad_core.h holds what this file shares with ../train_half/lsq_wgrad_half.hip: the constants, the tiles,
// the layout of the staged sign words, the K split, the reduce kernel and the host rules.  Here: the main kernel.  A chunk is a
// run of 64 k of the N Ho Wo positions, across samples; per chunk the workgroup holds grad_y in registers and stages, per
// plane, A (64 rows x 64 k, three terms, bf16) beside the sign words of its taps; every lane expands its 8 signs per fragment
// with two bit extracts and one shift-add per pair.  The sign-word steps (position, fold, staging, expansion, stores) read as
// in lsq_wgrad_half.hip and are kept in line in both files (lsq_wgrad_core.h says why).

#include "lsq_hip_train.h"
#include "lsq_wgrad_core.h"

namespace {

template <int TT>
struct alignas(16) Smem {
  unsigned short a[3][kOT][kApitch];  // A_p terms hi, mid, lo
  SignSmem<TT> s;
};

struct Args {
  const uint64_t* planes;
  const float* scales;
  const float* gy;
  float* out;                         // the slabs (S > 1)
  float* grad_wq;
  WgradGeom g;
  unsigned K;
  WgradTiles t;
};

union Frag4 {                         // a staged A fragment: 16 bytes to and from LDS as one
  unsigned u[4];
  uint4 q;
  bf16x8 v;
};

__device__ __forceinline__ unsigned short bf16_bits(float x) { return __builtin_bit_cast(unsigned short, (__bf16)x); }
__device__ __forceinline__ float bf16_value(unsigned short b) { return __uint_as_float((unsigned)b << 16); }

template <int TT, bool FOLD>
__global__ __launch_bounds__(kThreads) void wgrad_kernel(Args a) {
  __shared__ Smem<TT> sm;
  const WgradGeom& e = a.g;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int split = blockIdx.x / a.t.tiles, tile = blockIdx.x % a.t.tiles;
  const int tc = tile % a.t.ntc, g = (tile / a.t.ntc) % e.Gt, ot = tile / (a.t.ntc * e.Gt);
  const int KK = e.KH * e.KW;
  const int ntaps = min(TT, KK - tc * TT);
  const unsigned k_begin = (unsigned)split * (unsigned)a.t.chunks_per_split * kKC;
  const unsigned k_end = min(a.K, k_begin + (unsigned)a.t.chunks_per_split * kKC);

  // staging roles: A rows r0 and r0 + 32 at chunk positions kq .. kq + 7; sign words of chunk position kp, taps t>>6 + 4m
  const int r0 = t >> 3, kq = (t & 7) * 8, kp = t & 63;
  // compute roles: wave (wo_, wc) owns rows 32 wo_ .. +31 and channels 32 wc .. +31 of the tile
  const int wo_ = w & 1, wc = w >> 1, lr = lane & 31, lh = lane >> 5;

  f32x16 acc[TT];
#pragma unroll
  for (int tl = 0; tl < TT; ++tl) acc[tl] = f32x16{};

  for (unsigned kb = k_begin; kb < k_end; kb += kKC) {
    const unsigned nb = kb / e.HoWo, hwb = kb - nb * e.HoWo;
    // ---- A operand: grad_y of this chunk, fp32 in registers for every plane
    float gv[2][8];
    int nn[8];
    {
      unsigned n = nb, hw = hwb + kq;
      if (hw >= e.HoWo) { n += hw / e.HoWo; hw %= e.HoWo; }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool valid = kb + kq + j < k_end;
        nn[j] = valid ? (int)n : -1;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int o = ot * kOT + r0 + 32 * r;
          gv[r][j] = (valid && o < e.O) ? a.gy[((size_t)n * e.O + o) * e.HoWo + hw] : 0.f;
        }
        if (++hw == e.HoWo) { hw = 0; ++n; }
      }
    }
    // ---- sign words: this thread's chunk position
    long long wbase = -1;
    int pho = 0, pwo = 0, pn = 0;
    {
      const unsigned k = kb + kp;
      if (k < k_end) {
        unsigned n = nb, hw = hwb + kp;
        if (hw >= e.HoWo) { n += hw / e.HoWo; hw %= e.HoWo; }
        pn = (int)n;
        const int ho = (int)(hw / (unsigned)e.Wo), wo = (int)(hw - (unsigned)ho * e.Wo);
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
      __syncthreads();                     // the previous plane's fragments have been read
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        Frag4 hi, mid, lo;
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
          unsigned short th[2], tm[2], tlo[2];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const float v = nn[j + h] >= 0 ? a.scales[(size_t)p * e.N + nn[j + h]] : 0.f;
            const float x = v * gv[r][j + h];
            th[h] = bf16_bits(x);
            const float r1 = x - bf16_value(th[h]);
            tm[h] = bf16_bits(r1);
            tlo[h] = bf16_bits(r1 - bf16_value(tm[h]));
          }
          hi.u[j / 2] = th[0] | ((unsigned)th[1] << 16);
          mid.u[j / 2] = tm[0] | ((unsigned)tm[1] << 16);
          lo.u[j / 2] = tlo[0] | ((unsigned)tlo[1] << 16);
        }
        *(uint4*)&sm.a[0][r0 + 32 * r][kq] = hi.q;
        *(uint4*)&sm.a[1][r0 + 32 * r][kq] = mid.q;
        *(uint4*)&sm.a[2][r0 + 32 * r][kq] = lo.q;
      }
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
              b0 = 0x3F80;
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

#pragma unroll
      for (int ks = 0; ks < kKC / 16; ++ks) {
        const int k8 = 16 * ks + 8 * lh;
        Frag4 fa[3];
#pragma unroll
        for (int h = 0; h < 3; ++h) fa[h].q = *(const uint4*)&sm.a[h][32 * wo_ + lr][k8];
#pragma unroll
        for (int tl = 0; tl < TT; ++tl) {
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
            acc[tl] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[2].v, fb.v, acc[tl], 0, 0, 0);      // lo, mid, hi
            acc[tl] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1].v, fb.v, acc[tl], 0, 0, 0);
            acc[tl] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0].v, fb.v, acc[tl], 0, 0, 0);
          }
        }
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

// N Ho Wo < 2^31 (check_geom)
TilePlan plan(const WgradGeom& g, int kx) { return tile_plan(g, kx, ((long long)g.N * g.HoWo + kKC - 1) / kKC); }

size_t workspace_need(const TilePlan& p) { return p.t.S > 1 ? (size_t)p.t.S * p.slab_floats * sizeof(float) : 0; }

const WgradKernels<Args> kKernels = {
    {{wgrad_kernel<1, false>, wgrad_kernel<1, true>}, {wgrad_kernel<kTapTile, false>, wgrad_kernel<kTapTile, true>}},
    {wgrad_reduce_kernel<1, false, Args>, wgrad_reduce_kernel<kTapTile, false, Args>}};

}  // namespace

extern "C" int lsq_train_abi_version(void) { return LSQ_TRAIN_ABI_VERSION; }

extern "C" size_t lsq_train_wgrad_workspace_bytes(const lsq_conv_geom* g, int kx) {
  if (check_geom(g, kx) != LSQ_OK) return 0;
  return workspace_need(plan(fill_geom(g), kx));
}

extern "C" int lsq_train_wgrad(const uint64_t* xplanes, int kx, const float* xscales, const float* grad_y,
                               const lsq_conv_geom* g, float* grad_wq, void* workspace, size_t workspace_bytes,
                               void* stream) {
  if (const int e = check_geom(g, kx)) return e;
  if (!xplanes || !xscales || !grad_y || !grad_wq) return LSQ_E_NULL;
  Args a;
  a.g = fill_geom(g);
  const TilePlan p = plan(a.g, kx);
  if (const int e = check_workspace(workspace_need(p), workspace, workspace_bytes)) return e;
  a.t = p.t;
  a.planes = xplanes;
  a.scales = xscales;
  a.gy = grad_y;
  a.grad_wq = grad_wq;
  a.out = (float*)workspace;
  a.K = (unsigned)g->N * a.g.HoWo;
  return launch_wgrad(kKernels, a, p, kx > 1, 0, (hipStream_t)stream);
}
