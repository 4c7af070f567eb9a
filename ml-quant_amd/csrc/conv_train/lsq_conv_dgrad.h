// The input gradient of QuantConv2d as one set of kernels, instantiated by liblsq_hip_conv_train.so (lsq_signw_conv2d_dgrad:
// fp32 gradients, plain fp32 stores) and by liblsq_hip_conv_train_half.so (lsq_signw_conv2d_dgrad_half: bf16 / fp16 gradients
// converted exactly to fp32 as they are read, the straight-through estimator and the rounding into the type in the
// epilogue).  Templated on the gradient's element type GY and on an epilogue EPI; plan, tile choice, staging and the order
// of summation do not depend on either, so every instantiation computes the same fp32 accumulators.  Each library compiles
// its own copy (anonymous namespace); neither links the other's objects.
//   EPI:  struct Row;                                             what the epilogue keeps per sample (the sample's scales)
//         void row(int n, Row&) const;                            called once per (lane, sample) after the last MFMA
//         void store(long long i, const Row&, float acc) const;   element i of grad_x = f(acc)
//
// Output gradients x sign-weight planes with the sum over the OUTPUT channels and the taps, on
// the bf16 matrix cores of gfx950 (v_mfma_f32_32x32x16_bf16) -- the input gradient of QuantConv2d, conv2d_input over the
// forward's own planes.
//
// As a GEMM per (residue class of pixels, group):  D[c'][pixel] = sum_tap sum_o sum_q S_q[c'][(tap, o)] A_q[(tap, o)][pixel],
//   rows = the group's channels c', columns = the class's pixels (n, h, w), k = (tap of the class, out-channel o, plane q).
// Fragment layout, the hi / lo split and the sign-bit expansion: csrc/linear/lsq_signw_mma.h.  The SIGNS are the row operand
// here and the gradients the column operand (the two fragments of the instruction have the same lane layout), so a lane of D
// holds ONE pixel and 16 channels: a store instruction writes 32 consecutive pixels of the class per half-wave.
//   * WEIGHT: the forward's planes hold 64 CHANNELS in a word; k runs over o, so transpose_planes first writes the image
//     T[q][tap][grp][ceil(og / 64)][ceil16(cg)] into the caller's workspace (one wave per 64 x 64 bit block, 64 ballots).
//     After it a lane's sign fragment is 8 consecutive bits of one word of its channel.
//   * GRADIENT: a = fl32(gy ws[q][o]) -- the scale is per (plane, k), so it goes into the gradient operand and all planes
//     add into ONE accumulator --, then split hi + lo into LDS (one row of 64 o per staged position).  Out-channels past og,
//     positions outside gy and pixels past the class's end are staged as 0.
//   * CLASSES: class (rh, rw) = the pixels with (h + pad_h) % stride_h == rh, (w + pad_w) % stride_w == rw.  Tap (i, j) reaches
//     only the class with (i dil_h) % stride_h == rh, (j dil_w) % stride_w == rw; the taps of a class along an axis are an
//     arithmetic progression i0 + t * stride / gcd(dil, stride).  A workgroup owns 128 pixels of one class (blockIdx.y) and
//     walks that class's taps only; a class without taps stores the zero accumulators.
// Two kernels, two instantiations each (CB = 1: 128 pixels x 64 channels for cg <= 64; CB = 2: 128 x 128).  Four waves: wave
// (wr, wc) holds pixels 64 wr .. + 63 (two blocks of 32) x channels 32 CB wc .. (CB blocks of 32).
//   dgrad_patch  a tile of NS samples x TH x TW pixels of the class; in class coordinates a tap is a pure shift, so per (word
//                of 64 o, plane) the patch the tile's taps read is scaled, split and staged ONCE and every tap reads its
//                fragments at its shift.  Taken where a patch of at most kMaxPos positions exists (shape_of).
//   dgrad_conv   128 consecutive pixels of the class; every (tap, word) gathers its 128 x 64 gradients into registers (kept
//                across the planes, the next gather in flight during the last plane's MFMAs) and stages them per plane: large
//                or widely dilated kernels, whose patch does not fit.

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsq_hip_conv_train.h"
#include "../lsq_common.h"
#include "../linear/lsq_signw_mma.h"

namespace {

constexpr int kPB = 2;                // 32-pixel blocks per wave
constexpr int kBM = 64 * kPB;         // pixels per workgroup
constexpr int kStageO = 32;           // out-channels a thread stages per (tap, word): 128 pixels x 64 o over 256 threads

// plain fp32 stores: lsq_signw_conv2d_dgrad
struct EpiStore {
  float* gx;                          // [N][C][H][W]
  struct Row {};
  __device__ __forceinline__ void row(int, Row&) const {}
  __device__ __forceinline__ void store(long long i, const Row&, float acc) const { gx[i] = acc; }
};

template <class GY, class EPI>
struct Args {
  const GY* gy;                       // [N][O][Ho][Wo]
  const unsigned long long* tbits;    // T[kw][taps][groups][nwo][cpad]
  const float* ws;                    // [kw][O]
  EPI epi;                            // grad_x [N][C][H][W] and what becomes of an accumulator
  int N, C, H, W, O, Ho, Wo;
  int KH, KW, sh, sw, ph, pw, dh, dw;
  int groups, cg, og, cpad, nwo, kw;
  int per_h, per_w;                   // distance of a class's taps along an axis: stride / gcd(dilation, stride)
  int ctiles;                         // channel tiles per group
  // dgrad_patch only: a tile is NS samples x TH x TW pixels of a class (powers of two, NS TH TW = 128)
  int lw, lh;                         // log2 TW, log2 TH
  int tiles_w, tiles_h;               // tiles along the columns / rows of the largest class
};

// ---------------------------------------------------------------------------------------------------------------------
// T[q][tap][grp][ow][c'] bit j = wbits[q][tap][c' / 64][grp og_pad + 64 ow + j] bit c' % 64: one wave per 64 x 64 bit block
// (grid-stride over the blocks).  Out-channel slots past og_pad read as zero words (their gradient operand is 0 in the GEMM);
// channels c' < cpad are written, so every word of T is.
__global__ __launch_bounds__(256) void transpose_planes(const unsigned long long* __restrict__ wbits,
                                                        unsigned long long* __restrict__ tbits, int taps, int groups, int nwc,
                                                        int og_pad, int nwo, int cpad, long long plane_words, long long blocks) {
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * 4;
  const long long opad_total = (long long)groups * og_pad;
  for (long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); b < blocks; b += stride) {
    const int cw = (int)(b % nwc);
    long long t = b / nwc;
    const int ow = (int)(t % nwo);
    t /= nwo;
    const int grp = (int)(t % groups);
    t /= groups;
    const int tap = (int)(t % taps);
    const long long q = t / taps;
    const int oo = ow * 64 + lane;
    const unsigned long long w =
        oo < og_pad ? wbits[q * plane_words + ((long long)tap * nwc + cw) * opad_total + (long long)grp * og_pad + oo] : 0ull;
    unsigned long long out = 0;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      const unsigned long long m = __ballot((int)((w >> i) & 1ull));
      if (lane == i) out = m;
    }
    const int cc = cw * 64 + lane;
    if (cc < cpad) tbits[((((q * taps + tap) * groups + grp) * nwo + ow) * cpad) + cc] = out;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
template <int CB, class GY, class EPI>
__global__ __launch_bounds__(256, 2) void dgrad_conv(Args<GY, EPI> a) {
  __shared__ __attribute__((aligned(16))) unsigned char s_a[2 * kBM * kPitch];    // hi rows [kBM], then lo rows [kBM]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int col = lane & 31, hh = lane >> 5;
  const int wr = wid >> 1, wc = wid & 1;
  const int rh = blockIdx.y / a.sw, rw = blockIdx.y - rh * a.sw;          // the class
  const int grp = blockIdx.z / a.ctiles, ct = blockIdx.z - grp * a.ctiles;
  const int c0 = ct * 64 * CB + wc * 32 * CB;                               // the wave's first channel in the group

  // the class's pixels: h = h0 + sh ah, w = w0 + sw aw
  const int h0 = ((rh - a.ph) % a.sh + a.sh) % a.sh, w0 = ((rw - a.pw) % a.sw + a.sw) % a.sw;
  const int Hc = h0 < a.H ? (a.H - 1 - h0) / a.sh + 1 : 0, Wc = w0 < a.W ? (a.W - 1 - w0) / a.sw + 1 : 0;
  const long long Mc = (long long)a.N * Hc * Wc;
  const long long m0 = (long long)blockIdx.x * kBM;
  if (m0 >= Mc) return;                                                     // (the whole workgroup)
  const int HcWc = Hc * Wc;

  // the class's taps: i = i0 + per_h t < KH, j = j0 + per_w t < KW
  int i0 = 0, j0 = 0;
  while (i0 < a.KH && (i0 * a.dh) % a.sh != rh) ++i0;
  while (j0 < a.KW && (j0 * a.dw) % a.sw != rw) ++j0;
  const int nti = i0 < a.KH ? (a.KH - 1 - i0) / a.per_h + 1 : 0, ntj = j0 < a.KW ? (a.KW - 1 - j0) / a.per_w + 1 : 0;
  const int steps = nti * ntj * a.nwo;                                      // gathers: (tap, word of 64 out-channels)

  // staging role: pixel sp of the tile, out-channels so .. so + 31 of the word
  const int sp = tid & (kBM - 1), so = (tid >> 7) * kStageO;
  const bool sp_in = m0 + sp < Mc;
  int sn, shp, swp;                                                         // sample, h + pad_h, w + pad_w of the staged pixel
  {
    const long long pm = sp_in ? m0 + sp : Mc - 1;
    sn = (int)(pm / HcWc);
    const int r = (int)(pm - (long long)sn * HcWc);
    const int ah = r / Wc;
    shp = h0 + a.sh * ah + a.ph;
    swp = w0 + a.sw * (r - ah * Wc) + a.pw;
  }

  float gn[kStageO], gcur[kStageO];
  bool okn = false;
  auto tap_of = [&](int s, int& tap, int& ow, int& i, int& j) {
    const int t = s / a.nwo;
    ow = s - t * a.nwo;
    const int ti = t / ntj;
    i = i0 + ti * a.per_h;
    j = j0 + (t - ti * ntj) * a.per_w;
    tap = i * a.KW + j;
  };
  auto gather = [&](int s) {
    int tap, ow, i, j;
    tap_of(s, tap, ow, i, j);
    const int hn = shp - i * a.dh, wn = swp - j * a.dw;
    const int ho = hn / a.sh, wo = wn / a.sw;                               // (exact: the tap belongs to the class)
    okn = sp_in && hn >= 0 && wn >= 0 && ho < a.Ho && wo < a.Wo;
    const int oo = ow * 64 + so;
    const long long plane = (long long)a.Ho * a.Wo;
    const GY* p = a.gy + ((long long)sn * a.O + (long long)grp * a.og + oo) * plane + (okn ? (long long)ho * a.Wo + wo : 0);
#pragma unroll
    for (int e = 0; e < kStageO; ++e) gn[e] = okn && oo + e < a.og ? (float)p[e * plane] : 0.f;
  };

  f32x16 acc[kPB][CB];
#pragma unroll
  for (int pb = 0; pb < kPB; ++pb)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[pb][cb][i] = 0.f;

  if (steps > 0) gather(0);
  for (int s = 0; s < steps; ++s) {
    int tap, ow, ti, tj;
    tap_of(s, tap, ow, ti, tj);
#pragma unroll
    for (int e = 0; e < kStageO; ++e) gcur[e] = gn[e];
    const int oo = ow * 64 + so;
    for (int q = 0; q < a.kw; ++q) {
      unsigned long long wcur[CB];
      const unsigned long long* tw = a.tbits + ((((long long)q * a.KH * a.KW + tap) * a.groups + grp) * a.nwo + ow) * a.cpad;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) wcur[cb] = tw[min(c0 + cb * 32 + col, a.cpad - 1)];
      const float* sc = a.ws + (long long)q * a.O + (long long)grp * a.og;
      __syncthreads();                                  // every wave is done reading the previous stage
#pragma unroll
      for (int e = 0; e < kStageO; e += 4) {
        float c[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) c[d] = oo + e + d < a.og ? __fmul_rn(gcur[e + d], sc[oo + e + d]) : 0.f;
        stash_hi_lo(s_a + sp * kPitch + (so + e) * 2, kBM * kPitch, c);
      }
      __syncthreads();
      if (q + 1 == a.kw && s + 1 < steps) gather(s + 1);          // in flight during the MFMAs below
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4) {
        Frag gh[kPB], gl[kPB], sg[CB];
#pragma unroll
        for (int pb = 0; pb < kPB; ++pb) {
          const unsigned char* r = s_a + (wr * 32 * kPB + pb * 32 + col) * kPitch + 32 * k4 + 16 * hh;
          const uint4 vh = *reinterpret_cast<const uint4*>(r);
          const uint4 vl = *reinterpret_cast<const uint4*>(r + kBM * kPitch);
          gh[pb].u[0] = vh.x; gh[pb].u[1] = vh.y; gh[pb].u[2] = vh.z; gh[pb].u[3] = vh.w;
          gl[pb].u[0] = vl.x; gl[pb].u[1] = vl.y; gl[pb].u[2] = vl.z; gl[pb].u[3] = vl.w;
        }
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) sg[cb] = expand8((unsigned)(wcur[cb] >> (16 * k4 + 8 * hh)));
#pragma unroll
        for (int pb = 0; pb < kPB; ++pb)
#pragma unroll
          for (int cb = 0; cb < CB; ++cb)
            acc[pb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sg[cb].v, gh[pb].v, acc[pb][cb], 0, 0, 0);
#pragma unroll
        for (int pb = 0; pb < kPB; ++pb)
#pragma unroll
          for (int cb = 0; cb < CB; ++cb)
            acc[pb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sg[cb].v, gl[pb].v, acc[pb][cb], 0, 0, 0);
      }
    }
  }

  // a lane stores its pixel's 16 channels of every block (a class without taps: the zero accumulators)
  const long long HW = (long long)a.H * a.W;
#pragma unroll
  for (int pb = 0; pb < kPB; ++pb) {
    const long long pm = m0 + wr * 32 * kPB + pb * 32 + col;
    if (pm >= Mc) continue;
    const int n = (int)(pm / HcWc);
    const int r = (int)(pm - (long long)n * HcWc);
    const int ah = r / Wc;
    const int h = h0 + a.sh * ah, w = w0 + a.sw * (r - ah * Wc);
    const long long out = ((long long)n * a.C + (long long)grp * a.cg) * HW + (long long)h * a.W + w;
    typename EPI::Row er;
    a.epi.row(n, er);
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int cc = d_row(c0 + cb * 32, i, hh);
        if (cc < a.cg) a.epi.store(out + cc * HW, er, acc[pb][cb][i]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The patch kernel: in class coordinates (h = h0 + sh ah) tap i is a pure shift, ho = ah + (h0 + pad_h - i dil_h) / sh, so
// the gradients a tile's taps read form a patch of (TH + dH) x (TW + dW) positions of gy per sample.  Per (word of 64 o,
// plane) the workgroup scales, splits and stages that patch ONCE (thread t = position t: at most kMaxPos positions), and every
// tap of the class reads its fragments from the staged rows at its shift.
constexpr int kMaxPos = 222;          // staged positions: 2 * 222 * kPitch = 63936 bytes of LDS

template <int CB, class GY, class EPI>
__global__ __launch_bounds__(256, 2) void dgrad_patch(Args<GY, EPI> a) {
  __shared__ __attribute__((aligned(16))) unsigned char s_a[2 * kMaxPos * kPitch];    // hi rows, then lo rows
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int col = lane & 31, hh = lane >> 5;
  const int wr = wid >> 1, wc = wid & 1;
  const int rh = blockIdx.y / a.sw, rw = blockIdx.y - rh * a.sw;
  const int grp = blockIdx.z / a.ctiles, ct = blockIdx.z - grp * a.ctiles;
  const int c0 = ct * 64 * CB + wc * 32 * CB;
  const int TW = 1 << a.lw, TH = 1 << a.lh, NS = kBM >> (a.lw + a.lh);

  const int h0 = ((rh - a.ph) % a.sh + a.sh) % a.sh, w0 = ((rw - a.pw) % a.sw + a.sw) % a.sw;
  const int Hc = h0 < a.H ? (a.H - 1 - h0) / a.sh + 1 : 0, Wc = w0 < a.W ? (a.W - 1 - w0) / a.sw + 1 : 0;
  int b = blockIdx.x;
  const int aw0 = (b % a.tiles_w) * TW;
  b /= a.tiles_w;
  const int ah0 = (b % a.tiles_h) * TH, n0 = (b / a.tiles_h) * NS;
  if (ah0 >= Hc || aw0 >= Wc) return;                                       // (the whole workgroup: a smaller class)

  int i0 = 0, j0 = 0;
  while (i0 < a.KH && (i0 * a.dh) % a.sh != rh) ++i0;
  while (j0 < a.KW && (j0 * a.dw) % a.sw != rw) ++j0;
  const int nti = i0 < a.KH ? (a.KH - 1 - i0) / a.per_h + 1 : 0, ntj = j0 < a.KW ? (a.KW - 1 - j0) / a.per_w + 1 : 0;
  const int ntaps = nti * ntj;
  // shifts of the class's taps: bh(i) = (h0 + pad_h - i dil_h) / sh (exact), smallest at the last tap
  const int bh_min = nti ? (h0 + a.ph - (i0 + (nti - 1) * a.per_h) * a.dh) / a.sh : 0;
  const int bw_min = ntj ? (w0 + a.pw - (j0 + (ntj - 1) * a.per_w) * a.dw) / a.sw : 0;
  const int PH = TH + (nti ? (nti - 1) * a.per_h * a.dh / a.sh : 0), PW = TW + (ntj ? (ntj - 1) * a.per_w * a.dw / a.sw : 0);
  const int npos = NS * PH * PW;                                            // <= kMaxPos (the host's choice of the tile)

  // staging role: position tid of the patch
  const long long plane = (long long)a.Ho * a.Wo;
  bool pos_ok = false;
  const GY* gpos = a.gy + (long long)grp * a.og * plane;                 // (a valid address for a position outside gy)
  if (tid < npos) {
    const int ns = tid / (PH * PW), r2 = tid - ns * PH * PW;
    const int r = r2 / PW, c = r2 - r * PW;
    const int n = n0 + ns, ho = ah0 + bh_min + r, wo = aw0 + bw_min + c;
    pos_ok = n < a.N && ho >= 0 && ho < a.Ho && wo >= 0 && wo < a.Wo;
    if (pos_ok) gpos = a.gy + ((long long)n * a.O + (long long)grp * a.og) * plane + (long long)ho * a.Wo + wo;
  }
  // MFMA role: the lane's pixel of each block and its first staged row
  int prow[kPB];
#pragma unroll
  for (int pb = 0; pb < kPB; ++pb) {
    const int p = wr * 32 * kPB + pb * 32 + col;
    prow[pb] = ((p >> (a.lw + a.lh)) * PH + ((p >> a.lw) & (TH - 1))) * PW + (p & (TW - 1));
  }

  f32x16 acc[kPB][CB];
#pragma unroll
  for (int pb = 0; pb < kPB; ++pb)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[pb][cb][i] = 0.f;

  const int taps = a.KH * a.KW;
  auto tap_at = [&](int t, int& tap, int& shift) {
    const int ti = t / ntj, i = i0 + ti * a.per_h, j = j0 + (t - ti * ntj) * a.per_w;
    tap = i * a.KW + j;
    shift = ((h0 + a.ph - i * a.dh) / a.sh - bh_min) * PW + (w0 + a.pw - j * a.dw) / a.sw - bw_min;
  };
  auto words = [&](int q, int ow, int tap, unsigned long long (&w)[CB]) {
    const unsigned long long* tw = a.tbits + ((((long long)q * taps + tap) * a.groups + grp) * a.nwo + ow) * a.cpad;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) w[cb] = tw[min(c0 + cb * 32 + col, a.cpad - 1)];
  };

  if (ntaps > 0) {
    for (int ow = 0; ow < a.nwo; ++ow) {
      for (int q = 0; q < a.kw; ++q) {
        unsigned long long wn[CB], wcur[CB];
        int tapn, shiftn;
        tap_at(0, tapn, shiftn);
        words(q, ow, tapn, wn);
        const float* sc = a.ws + (long long)q * a.O + (long long)grp * a.og;
        __syncthreads();                                // every wave is done reading the previous patch
        if (tid < npos) {
          // 32 unconditional loads in flight (a position outside gy reads the group's first element, a slot past og its
          // last out-channel: valid addresses, the values are dropped), then scaled, split and stored
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            float v[32];
#pragma unroll
            for (int e = 0; e < 32; ++e) v[e] = (float)gpos[min(ow * 64 + 32 * half + e, a.og - 1) * plane];
#pragma unroll
            for (int e = 0; e < 32; e += 4) {
              float c[4];
#pragma unroll
              for (int d = 0; d < 4; ++d) {
                const int oo = ow * 64 + 32 * half + e + d;
                c[d] = pos_ok && oo < a.og ? __fmul_rn(v[e + d], sc[min(oo, a.og - 1)]) : 0.f;
              }
              stash_hi_lo(s_a + tid * kPitch + (32 * half + e) * 2, kMaxPos * kPitch, c);
            }
          }
        }
        __syncthreads();
        for (int t = 0; t < ntaps; ++t) {
          const int shift = shiftn;
#pragma unroll
          for (int cb = 0; cb < CB; ++cb) wcur[cb] = wn[cb];
          if (t + 1 < ntaps) {                          // the next tap's words, in flight during the MFMAs below
            tap_at(t + 1, tapn, shiftn);
            words(q, ow, tapn, wn);
          }
#pragma unroll
          for (int k4 = 0; k4 < 4; ++k4) {
            Frag gh[kPB], gl[kPB], sg[CB];
#pragma unroll
            for (int pb = 0; pb < kPB; ++pb) {
              const unsigned char* r = s_a + (prow[pb] + shift) * kPitch + 32 * k4 + 16 * hh;
              const uint4 vh = *reinterpret_cast<const uint4*>(r);
              const uint4 vl = *reinterpret_cast<const uint4*>(r + kMaxPos * kPitch);
              gh[pb].u[0] = vh.x; gh[pb].u[1] = vh.y; gh[pb].u[2] = vh.z; gh[pb].u[3] = vh.w;
              gl[pb].u[0] = vl.x; gl[pb].u[1] = vl.y; gl[pb].u[2] = vl.z; gl[pb].u[3] = vl.w;
            }
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) sg[cb] = expand8((unsigned)(wcur[cb] >> (16 * k4 + 8 * hh)));
#pragma unroll
            for (int pb = 0; pb < kPB; ++pb)
#pragma unroll
              for (int cb = 0; cb < CB; ++cb)
                acc[pb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sg[cb].v, gh[pb].v, acc[pb][cb], 0, 0, 0);
#pragma unroll
            for (int pb = 0; pb < kPB; ++pb)
#pragma unroll
              for (int cb = 0; cb < CB; ++cb)
                acc[pb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sg[cb].v, gl[pb].v, acc[pb][cb], 0, 0, 0);
          }
        }
      }
    }
  }

  // The lane's coordinates are derived again from a thread index the compiler cannot connect with the one above: nothing
  // of the epilogue but the accumulators then stays in registers across the matrix loop (the wide instantiation is at 256).
  int etid = threadIdx.x;
  asm volatile("" : "+v"(etid));
  const int ecol = etid & 31, ehh = (etid >> 5) & 1, ewr = etid >> 7, ec0 = ct * 64 * CB + ((etid >> 6) & 1) * 32 * CB;
  const long long HW = (long long)a.H * a.W;
#pragma unroll
  for (int pb = 0; pb < kPB; ++pb) {
    const int p = ewr * 32 * kPB + pb * 32 + ecol;
    const int n = n0 + (p >> (a.lw + a.lh)), ah = ah0 + ((p >> a.lw) & (TH - 1)), aw = aw0 + (p & (TW - 1));
    if (n >= a.N || ah >= Hc || aw >= Wc) continue;
    const long long out = ((long long)n * a.C + (long long)grp * a.cg) * HW + (long long)(h0 + a.sh * ah) * a.W + w0 + a.sw * aw;
    typename EPI::Row er;
    a.epi.row(n, er);
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int cc = d_row(ec0 + cb * 32, i, ehh);
        if (cc < a.cg) a.epi.store(out + cc * HW, er, acc[pb][cb][i]);
      }
    }
  }
}

int gcd(int x, int y) {
  while (y) {
    const int t = x % y;
    x = y;
    y = t;
  }
  return x;
}

// What a call does, or why it is refused: shared by the entry points of both libraries.
struct Shape {
  int Ho, Wo, cg, og, og_pad, cpad, nwo, nwc, taps, ctiles, cb;
  long long t_words;                  // words of the transposed image of one plane
  int per_h, per_w;                   // distance of a class's taps along an axis
  bool patch;                         // the patch kernel's tile, where a patch of at most kMaxPos positions exists
  int lw, lh, tiles_w, tiles_h;
  long long tiles;                    // grid x
};

int shape_of(const lsq_conv_geom* g, Shape* s) {
  if (int e = lsq::check_geom(g)) return e;
  s->Ho = lsq::out_h(g);
  s->Wo = lsq::out_w(g);
  if ((long long)g->H + 2ll * g->pad_h - (long long)g->dil_h * (g->KH - 1) - 1 < 0 ||
      (long long)g->W + 2ll * g->pad_w - (long long)g->dil_w * (g->KW - 1) - 1 < 0 || s->Ho < 1 || s->Wo < 1)
    return LSQ_E_SHAPE;
  const long long lim = 1ll << 31;
  if ((long long)g->N * g->C * g->H * g->W >= lim || (long long)g->N * g->O * s->Ho * s->Wo >= lim) return LSQ_E_UNSUPPORTED;
  if ((long long)g->stride_h * g->stride_w > 65535) return LSQ_E_UNSUPPORTED;
  if ((long long)g->KH * g->dil_h >= lim || (long long)g->KW * g->dil_w >= lim) return LSQ_E_UNSUPPORTED;
  s->cg = g->C / g->groups;
  s->og = g->O / g->groups;
  s->og_pad = (s->og + 15) / 16 * 16;
  s->cpad = (s->cg + 15) / 16 * 16;
  s->nwo = (s->og + 63) / 64;
  s->nwc = (s->cg + 63) / 64;
  s->taps = g->KH * g->KW;
  s->cb = s->cg <= 64 ? 1 : 2;
  s->ctiles = (s->cg + 64 * s->cb - 1) / (64 * s->cb);
  if ((long long)g->groups * s->ctiles > 65535) return LSQ_E_UNSUPPORTED;
  const long long kk = (long long)g->KH * g->KW;
  if (kk >= (1ll << 28)) return LSQ_E_UNSUPPORTED;
  s->t_words = kk * g->groups * s->nwo * s->cpad;
  if (s->t_words >= (1ll << 28) || kk * s->nwc * g->groups * s->og_pad >= (1ll << 28)) return LSQ_E_UNSUPPORTED;
  s->per_h = g->stride_h / gcd(g->dil_h, g->stride_h);
  s->per_w = g->stride_w / gcd(g->dil_w, g->stride_w);
  // The largest class has hc x wc pixels a sample and (ntih x ntiw) taps, which span dH x dW positions beyond a tile.
  // Patch tile: the power-of-two split of 128 pixels into NS x TH x TW whose patch fits, at the least cost below (few tiles,
  // small patches, long rows); none fits (large or widely dilated kernels): the gather kernel, 128 consecutive pixels of the class.
  const long long hc = (g->H + g->stride_h - 1) / g->stride_h, wc = (g->W + g->stride_w - 1) / g->stride_w;
  const long long dH = (long long)((g->KH - 1) / s->per_h) * s->per_h * g->dil_h / g->stride_h;
  const long long dW = (long long)((g->KW - 1) / s->per_w) * s->per_w * g->dil_w / g->stride_w;
  s->patch = false;
  long long best = 0;
  for (int lw = 0; lw <= 7; ++lw) {
    for (int lh = 0; lw + lh <= 7; ++lh) {
      const long long TW = 1ll << lw, TH = 1ll << lh, NS = kBM >> (lw + lh);
      const long long npos = NS * (TH + dH) * (TW + dW);
      if (npos > kMaxPos) continue;
      const long long tw = (wc + TW - 1) / TW, th = (hc + TH - 1) / TH;
      const long long tiles = ((g->N + NS - 1) / NS) * th * tw;
      if (tiles >= (1ll << 31) || tw >= (1ll << 30) || th >= (1ll << 30)) continue;
      // per tile: the staged positions, weighted by the 64-byte sectors a row segment of TW + dW floats touches (one more
      // than its length: 1 + 16 / (TW + dW) per float), plus the tile's matrix work
      const long long cost = tiles * (npos * (16 + 256 / (TW + dW)) + 16 * 256);
      if (!s->patch || cost < best) {
        s->patch = true;
        best = cost;
        s->lw = lw; s->lh = lh; s->tiles_w = (int)tw; s->tiles_h = (int)th; s->tiles = tiles;
      }
    }
  }
  if (!s->patch) s->tiles = ((long long)g->N * hc * wc + kBM - 1) / kBM;
  return LSQ_OK;
}

bool planes_ok(int kw_planes) { return kw_planes >= 1 && kw_planes <= LSQ_MAX_PLANES; }

// The plan of a call: shared by lsq_signw_conv2d_dgrad_plan and lsq_signw_conv2d_dgrad_half_plan.
int plan_of(const lsq_conv_geom* g, lsq_conv_dgrad_plan* plan) {
  if (!g || !plan) return LSQ_E_NULL;
  Shape s;
  if (int e = shape_of(g, &s)) return e;
  // per axis: the taps of every residue, counted tap by tap
  int live_h = 0, live_w = 0, taps_h = 0, taps_w = 0;
  for (int r = 0; r < g->stride_h; ++r) {
    int n = 0;
    for (int i = 0; i < g->KH; ++i) n += (int)(((long long)i * g->dil_h) % g->stride_h == r);
    live_h += n > 0;
    taps_h += n;
  }
  for (int r = 0; r < g->stride_w; ++r) {
    int n = 0;
    for (int j = 0; j < g->KW; ++j) n += (int)(((long long)j * g->dil_w) % g->stride_w == r);
    live_w += n > 0;
    taps_w += n;
  }
  plan->kernel = (s.cb == 1 ? LSQ_CONV_DGRAD_NARROW : LSQ_CONV_DGRAD_WIDE) | (s.patch ? LSQ_CONV_DGRAD_PATCH : 0);
  plan->classes = g->stride_h * g->stride_w;
  plan->dead_classes = plan->classes - live_h * live_w;
  plan->tap_steps = taps_h * taps_w;                  // (sum over the classes (rh, rw) of taps_h[rh] * taps_w[rw])
  return LSQ_OK;
}

size_t workspace_bytes_of(const lsq_conv_geom* g, int kw_planes) {
  Shape s;
  if (!g || !planes_ok(kw_planes) || shape_of(g, &s)) return 0;
  return (size_t)kw_planes * (size_t)s.t_words * sizeof(unsigned long long);
}

// The checks every entry point makes after its own (g is not NULL): 0 and *s filled, or the code to return.
int check_call(const lsq_conv_geom* g, int kw_planes, const void* workspace, size_t workspace_bytes, Shape* s) {
  if (int e = shape_of(g, s)) return e;
  if (!planes_ok(kw_planes)) return LSQ_E_UNSUPPORTED;
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < (size_t)kw_planes * (size_t)s->t_words * 8)
    return LSQ_E_WORKSPACE;
  return LSQ_OK;
}

// transpose_planes into the workspace, then the plan's kernel: the launches of a call whose operands passed check_call.
template <class GY, class EPI>
int launch_dgrad(const GY* grad_y, const uint64_t* wbits, int kw_planes, const float* wscales, const lsq_conv_geom* g,
                 const Shape& s, const EPI& epi, void* workspace, hipStream_t st) {
  const long long plane_words = (long long)s.taps * s.nwc * g->groups * s.og_pad;
  const long long blocks = (long long)kw_planes * s.taps * g->groups * s.nwo * s.nwc;      // 64 x 64 bit blocks, one wave each
  const long long tgrid = (blocks + 3) / 4;
  hipLaunchKernelGGL(transpose_planes, dim3((unsigned)(tgrid < (1ll << 20) ? tgrid : (1ll << 20))), dim3(256), 0, st,
                     (const unsigned long long*)wbits, (unsigned long long*)workspace, s.taps, (int)g->groups, s.nwc, s.og_pad,
                     s.nwo, s.cpad, plane_words, blocks);
  int e = (int)hipGetLastError();
  if (e) return e;

  Args<GY, EPI> a = {};
  a.gy = grad_y;
  a.tbits = (const unsigned long long*)workspace;
  a.ws = wscales;
  a.epi = epi;
  a.N = g->N; a.C = g->C; a.H = g->H; a.W = g->W; a.O = g->O; a.Ho = s.Ho; a.Wo = s.Wo;
  a.KH = g->KH; a.KW = g->KW; a.sh = g->stride_h; a.sw = g->stride_w; a.ph = g->pad_h; a.pw = g->pad_w;
  a.dh = g->dil_h; a.dw = g->dil_w;
  a.groups = g->groups; a.cg = s.cg; a.og = s.og; a.cpad = s.cpad; a.nwo = s.nwo; a.kw = kw_planes;
  a.per_h = s.per_h;
  a.per_w = s.per_w;
  a.ctiles = s.ctiles;
  // grid x: the tiles of the LARGEST class; workgroups past a smaller class's end return
  const dim3 grid((unsigned)s.tiles, (unsigned)(g->stride_h * g->stride_w), (unsigned)(g->groups * s.ctiles));
  if (s.patch) {
    a.lw = s.lw; a.lh = s.lh; a.tiles_w = s.tiles_w; a.tiles_h = s.tiles_h;
    if (s.cb == 1) hipLaunchKernelGGL((dgrad_patch<1, GY, EPI>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((dgrad_patch<2, GY, EPI>), grid, dim3(256), 0, st, a);
  } else {
    if (s.cb == 1) hipLaunchKernelGGL((dgrad_conv<1, GY, EPI>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((dgrad_conv<2, GY, EPI>), grid, dim3(256), 0, st, a);
  }
  return (int)hipGetLastError();
}

}  // namespace
