// lsq_train_wgrad: weight gradient of a binary-activation convolution from the activation sign planes (gfx950).
//
// As a GEMM:  D[o][(c, tap)] = sum_k A_p[o][k] B_p[k][(c, tap)], summed over the planes p, with
//   k = (n, ho, wo)                                  K = N Ho Wo, the reduction
//   A_p[o][k] = xscales[p][n] * grad_y[n][o][ho][wo] fp32, split into three bf16 terms hi + mid + lo
//   B_p[k][(c, i, j)] = 2 bit_p - 1 of channel c at padded pixel (ho s + i, wo s + j): exactly +-1 in bf16, or 0 on a halo
//                       word or past the end of K.
// One sign fragment serves the three terms (three v_mfma_f32_32x32x16_bf16 per fragment).  Planes 2m, 2m + 1 whose scales
// are equal for a sample (ls-T) are folded into one operand in {-2, 0, +2}, so that x_q = 0 is an exact 0 rather than
// +v - v accumulated in fp32 (which misses sum |gy| |x_q| by far more than an fp32 rounding).  hi = bf16(a), mid = bf16(a - hi),
// lo = bf16(a - hi - mid): each subtraction is exact in fp32 and each term carries the next 8 bits, so hi + mid + lo is a
// to within 2^-24 |a| -- the products with +-1 are exact and the MFMA accumulates in fp32.  No scaling: bf16 has fp32's exponent range.
//
// Tiles: a workgroup (4 waves) owns 64 output channels x 64 input channels (one plane word) x up to TT taps, every wave a
// 32 x 32 block of (o, c) for each of the tile's taps (TT accumulators of 16 registers).  Per chunk of 64 k the workgroup
// stages, per plane, A (64 rows x 64 k, three terms, bf16) and the sign words of its taps (complemented, 0 on the halo) in
// LDS; every lane expands its 8 signs per fragment with two bit extracts and one shift-add per pair.
// Split-K: K is cut into S slices of whole chunks (S from the geometry alone: about kTargetGroups workgroups).  With S > 1
// every workgroup stores its accumulators as a slab in MFMA order (coalesced) and a second launch sums the S slabs of each
// output element in slice order -- bitwise deterministic, no atomics, no inter-workgroup hand-off.  S = 1 writes grad_wq
// directly.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsq_hip_train.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int kThreads = 256;
constexpr int kKC = 64;               // k per chunk
constexpr int kOT = 64;               // output channels per workgroup
constexpr int kApitch = kKC + 8;      // bf16 per staged A row (16-byte pad: the row reads of a wave fall on distinct banks)
constexpr int kTargetGroups = 512;    // workgroups the K split aims at (2 per CU)
constexpr int kTapTile = 9;           // taps per workgroup for kernels larger than 1x1

union Frag {
  unsigned u[4];
  uint4 q;
  bf16x8 v;
};

template <int TT>
struct alignas(16) Smem {
  unsigned short a[3][kOT][kApitch];  // A_p terms hi, mid, lo
  unsigned p[TT][2][kKC];             // ~(word half) of tap tl at chunk position k; 0 on the halo / past the end
  unsigned z[TT][2][kKC];             // channels whose value is 0 (a folded pair of planes with opposite signs)
  unsigned short b0[TT][kKC];         // 0x3F80 (bf16 +1) or 0x4000 (+2, a folded pair) where the sign is real, else 0
};

struct Args {
  const uint64_t* planes;
  const float* scales;
  const float* gy;
  float* out;                         // grad_wq (S == 1) or the slabs
  float* grad_wq;
  long long plane_words;
  int N, C, H, W, O, KH, KW, s, ph, pw, Ho, Wo, Hp, Wp, Gt;
  unsigned HoWo, K;
  int kx, ntc, tiles, chunks_per_split, S;
};

__device__ __forceinline__ unsigned short bf16_bits(float x) { return __builtin_bit_cast(unsigned short, (__bf16)x); }
__device__ __forceinline__ float bf16_value(unsigned short b) { return __uint_as_float((unsigned)b << 16); }

template <int TT, bool FOLD>
__global__ __launch_bounds__(kThreads) void wgrad_kernel(Args a) {
  __shared__ Smem<TT> sm;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int split = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  const int tc = tile % a.ntc, g = (tile / a.ntc) % a.Gt, ot = tile / (a.ntc * a.Gt);
  const int KK = a.KH * a.KW;
  const int ntaps = min(TT, KK - tc * TT);
  const unsigned k_begin = (unsigned)split * (unsigned)a.chunks_per_split * kKC;
  const unsigned k_end = min(a.K, k_begin + (unsigned)a.chunks_per_split * kKC);

  // staging roles: A rows r0 and r0 + 32 at chunk positions kq .. kq + 7; sign words of chunk position kp, taps t>>6 + 4m
  const int r0 = t >> 3, kq = (t & 7) * 8, kp = t & 63;
  // compute roles: wave (wo_, wc) owns rows 32 wo_ .. +31 and channels 32 wc .. +31 of the tile
  const int wo_ = w & 1, wc = w >> 1, lr = lane & 31, lh = lane >> 5;

  f32x16 acc[TT];
#pragma unroll
  for (int tl = 0; tl < TT; ++tl) acc[tl] = f32x16{};

  for (unsigned kb = k_begin; kb < k_end; kb += kKC) {
    const unsigned nb = kb / a.HoWo, hwb = kb - nb * a.HoWo;
    // ---- A operand: grad_y of this chunk, fp32 in registers for every plane
    float gv[2][8];
    int nn[8];
    {
      unsigned n = nb, hw = hwb + kq;
      if (hw >= a.HoWo) { n += hw / a.HoWo; hw %= a.HoWo; }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool valid = kb + kq + j < k_end;
        nn[j] = valid ? (int)n : -1;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int o = ot * kOT + r0 + 32 * r;
          gv[r][j] = (valid && o < a.O) ? a.gy[((size_t)n * a.O + o) * a.HoWo + hw] : 0.f;
        }
        if (++hw == a.HoWo) { hw = 0; ++n; }
      }
    }
    // ---- sign words: this thread's chunk position
    long long wbase = -1;
    int pho = 0, pwo = 0, pn = 0;
    {
      const unsigned k = kb + kp;
      if (k < k_end) {
        unsigned n = nb, hw = hwb + kp;
        if (hw >= a.HoWo) { n += hw / a.HoWo; hw %= a.HoWo; }
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
      __syncthreads();                     // the previous plane's fragments have been read
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        Frag hi, mid, lo;
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
          unsigned short th[2], tm[2], tlo[2];
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const float v = nn[j + e] >= 0 ? a.scales[(size_t)p * a.N + nn[j + e]] : 0.f;
            const float x = v * gv[r][j + e];
            th[e] = bf16_bits(x);
            const float r1 = x - bf16_value(th[e]);
            tm[e] = bf16_bits(r1);
            tlo[e] = bf16_bits(r1 - bf16_value(tm[e]));
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
            const int tap = tc * TT + tl, i = tap / a.KW, j = tap - (tap / a.KW) * a.KW;
            const int hh = pho + i - a.ph, ww = pwo + j - a.pw;
            if (hh >= 0 && hh < a.H && ww >= 0 && ww < a.W) {
              const long long at = wbase + (long long)i * a.Wp + j;
              const uint64_t word = a.planes[p * a.plane_words + at];
              plo = ~(unsigned)word;
              phi = ~(unsigned)(word >> 32);
              b0 = 0x3F80;
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

#pragma unroll
      for (int ks = 0; ks < kKC / 16; ++ks) {
        const int k8 = 16 * ks + 8 * lh;
        Frag fa[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) fa[e].q = *(const uint4*)&sm.a[e][32 * wo_ + lr][k8];
#pragma unroll
        for (int tl = 0; tl < TT; ++tl) {
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
            acc[tl] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[2].v, fb.v, acc[tl], 0, 0, 0);
            acc[tl] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1].v, fb.v, acc[tl], 0, 0, 0);
            acc[tl] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0].v, fb.v, acc[tl], 0, 0, 0);
          }
        }
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
          const int o = ot * kOT + 32 * wo_ + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
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

// Sum of the S slabs of every output element, in slice order.  Thread = one slab position (MFMA order).
template <int TT>
__global__ __launch_bounds__(kThreads) void wgrad_reduce_kernel(Args a) {
  const size_t slab = (size_t)a.tiles * 4 * TT * 16 * 64;
  const size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= slab) return;
  const int lane = (int)(idx & 63), reg = (int)((idx >> 6) & 15);
  const size_t rest = idx >> 10;
  const int tl = (int)(rest % TT), w = (int)((rest / TT) % 4), tile = (int)(rest / (TT * 4));
  const int tc = tile % a.ntc, g = (tile / a.ntc) % a.Gt, ot = tile / (a.ntc * a.Gt);
  const int KK = a.KH * a.KW, tap = tc * TT + tl;
  const int c = g * 64 + 32 * (w >> 1) + (lane & 31);
  const int o = ot * kOT + 32 * (w & 1) + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
  if (tl >= TT || tap >= KK || c >= a.C || o >= a.O) return;
  float sum = a.out[idx];
  for (int s = 1; s < a.S; ++s) sum += a.out[(size_t)s * slab + idx];
  a.grad_wq[((size_t)o * a.C + c) * KK + tap] = sum;
}

struct Plan {
  int TT, ntc, tiles, S, chunks_per_split;
  size_t slab_floats;
};

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

Plan plan(const lsq_conv_geom* g) {
  Plan p;
  const int KK = g->KH * g->KW;
  const int ho = (g->H + 2 * g->pad_h - g->KH) / g->stride_h + 1, wo = (g->W + 2 * g->pad_w - g->KW) / g->stride_w + 1;
  p.TT = KK == 1 ? 1 : kTapTile;
  p.ntc = (KK + p.TT - 1) / p.TT;
  p.tiles = ((g->O + kOT - 1) / kOT) * ((g->C + 63) / 64) * p.ntc;
  const long long chunks = ((long long)g->N * ho * wo + kKC - 1) / kKC;
  long long S = (kTargetGroups + p.tiles - 1) / p.tiles;
  if (S > chunks) S = chunks;
  if (S < 1) S = 1;
  p.chunks_per_split = (int)((chunks + S - 1) / S);
  p.S = (int)((chunks + p.chunks_per_split - 1) / p.chunks_per_split);
  p.slab_floats = (size_t)p.tiles * 4 * p.TT * 16 * 64;
  return p;
}

}  // namespace

extern "C" int lsq_train_abi_version(void) { return LSQ_TRAIN_ABI_VERSION; }

extern "C" size_t lsq_train_wgrad_workspace_bytes(const lsq_conv_geom* g, int kx) {
  if (check_geom(g, kx) != LSQ_OK) return 0;
  const Plan p = plan(g);
  return p.S > 1 ? (size_t)p.S * p.slab_floats * sizeof(float) : 0;
}

extern "C" int lsq_train_wgrad(const uint64_t* xplanes, int kx, const float* xscales, const float* grad_y,
                               const lsq_conv_geom* g, float* grad_wq, void* workspace, size_t workspace_bytes,
                               void* stream) {
  if (const int e = check_geom(g, kx)) return e;
  if (!xplanes || !xscales || !grad_y || !grad_wq) return LSQ_E_NULL;
  const Plan p = plan(g);
  const size_t need = p.S > 1 ? (size_t)p.S * p.slab_floats * sizeof(float) : 0;
  if (need > 0 && !workspace) return LSQ_E_NULL;
  if (workspace_bytes < need || ((uintptr_t)workspace & 15)) return LSQ_E_WORKSPACE;
  Args a;
  a.planes = xplanes;
  a.scales = xscales;
  a.gy = grad_y;
  a.grad_wq = grad_wq;
  a.out = p.S > 1 ? (float*)workspace : grad_wq;
  a.N = g->N; a.C = g->C; a.H = g->H; a.W = g->W; a.O = g->O; a.KH = g->KH; a.KW = g->KW;
  a.s = g->stride_h; a.ph = g->pad_h; a.pw = g->pad_w;
  a.Ho = (g->H + 2 * g->pad_h - g->KH) / g->stride_h + 1;
  a.Wo = (g->W + 2 * g->pad_w - g->KW) / g->stride_w + 1;
  a.Hp = g->H + 2 * g->pad_h;
  a.Wp = g->W + 2 * g->pad_w;
  a.Gt = (g->C + 63) / 64;
  a.HoWo = (unsigned)a.Ho * (unsigned)a.Wo;
  a.K = (unsigned)g->N * a.HoWo;
  a.plane_words = (long long)g->N * a.Gt * a.Hp * a.Wp;
  a.kx = kx;
  a.ntc = p.ntc;
  a.tiles = p.tiles;
  a.chunks_per_split = p.chunks_per_split;
  a.S = p.S;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(p.tiles * p.S)), block(kThreads);
  const dim3 rgrid((unsigned)((p.slab_floats + kThreads - 1) / kThreads));
  const bool fold = kx > 1;
  if (p.TT == 1) {
    if (fold) hipLaunchKernelGGL((wgrad_kernel<1, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((wgrad_kernel<1, false>), grid, block, 0, st, a);
    if (p.S > 1) hipLaunchKernelGGL(wgrad_reduce_kernel<1>, rgrid, block, 0, st, a);
  } else {
    if (fold) hipLaunchKernelGGL((wgrad_kernel<kTapTile, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((wgrad_kernel<kTapTile, false>), grid, block, 0, st, a);
    if (p.S > 1) hipLaunchKernelGGL(wgrad_reduce_kernel<kTapTile>, rgrid, block, 0, st, a);
  }
  return (int)hipGetLastError();
}
