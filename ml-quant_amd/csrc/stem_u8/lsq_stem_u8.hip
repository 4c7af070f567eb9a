// lsq_stem_conv_u8 for gfx950: the front convolution of a network on the uint8 pixels an image pipeline delivers, planar
// (NCHW) or interleaved (channels-last), with the input normalisation x * in_scale[c] + in_shift[c], bias, ReLU, a per-channel
// affine and a max-pool (none, 2x2 / 2, or the ImageNet stem's 3x3 / 2 / pad 1) in ONE launch; fp32 NCHW out.
// (include/lsq_hip_stem_u8.h: the contract and the work-split rule.)
//
// Arithmetic.  A byte is exact in ONE bf16 (eight significant bits), so the activation side is a single term: no split, no
// overflow guard.  in_scale is folded into the weights (w' = w * in_scale[c], one fp32 product) and w' is split into three
// bf16 terms h + m + l (24 significant bits: w' itself): three MFMA passes h x, m x, l x -- the leading products on one fp32
// accumulator, the two small ones on a second.  Every product is exact; the roundings are those of the fp32 accumulation.
// in_shift rides a synthetic input channel C: 1 inside the image, 0 in the zero padding, with the weights
// sum_c w[o][c][kh][kw] * in_shift[c] (fp32, c ascending).  A padded pixel therefore contributes 0, not in_shift, and the K
// loop has no border branch.  With in_shift == 0 for every c the channel is left out (a step count the kernel derives).
//
// GEMM view: D[out-channel][pixel] = A[out-channel][k] B[k][pixel] on v_mfma_f32_32x32x16_bf16.
//   M  = 32 out-channels (rows past O: zero weights, masked stores);
//   N  = 32 consecutive conv columns of ONE conv row: a lane holds column lane % 32 and sixteen out-channels;
//   K  = (c, kh, kw) with kw padded to 8 behind the taps (zero weights): the eight k-values of a lane's operand are eight
//        consecutive pixels of input row (c, kh), from column x stride - pad on.  A k-step of 16 is two (c, kh) rows, one per
//        lane half; ceil((C + 1) KH / 2) steps (3 x 7x7 + indicator: 14; 3 x 3x3: 6; 1 x 5x5: 5).
//
// Data flow of one workgroup (256 threads; one image, one strip of R conv rows, T out-channel tiles):
//   once     weights read, scaled, the indicator row summed, split, and written to LDS as ready A fragments
//            [tile][step][term][lane] of 16 bytes; bias / post tables and the dword offset of every (c, kh) row of the patch;
//   chunk    (32 conv columns; 30 for pool 3, whose windows overlap by one column) the byte patch is read with aligned dword
//            loads (head, tail and the tensor's ends guarded; bytes where a dword would leave the tensor), zero filled outside
//            the image, converted and stored as ONE plane of bf16 per channel: both layouts differ here only -- NCHW walks C
//            byte rows, channels-last walks one row of C W bytes and de-interleaves on the LDS write.  There is no second,
//            shifted copy for the odd windows of stride 1: a lane reads five aligned dwords and v_alignbyte assembles its
//            eight pixels in registers;
//   unit     wave w takes the units w, w + 4, ... of (tile, run of L row pairs).  Pool 3 first computes the conv row above
//            the run alone and carries it (sixteen registers); every pair then gives one pooled row and leaves the next carry;
//   epilogue in registers: + bias, ReLU, fmaf(v, s, t); columns and rows outside the conv output become -inf for pool 3;
//            vertical max between accumulators, horizontal max with lane ^ 1 (DPP) and lane + 2 (ds_bpermute).
// Barriers are LDS-only (lds_barrier): the stores of a chunk stay in flight while the next patch is staged.

#include "../lsq_common.h"
#include "lsq_hip_stem_u8.h"

namespace lsq {
namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) float f32x2;

union Frag {
  unsigned u[4];
  uint4 q;
  bf16x8 v;
};

constexpr int kTerms = 3;                    // bf16 terms of a weight
constexpr int kThreads = 256;
constexpr int kMaxKernel = 7, kMaxC = 3, kMaxO = 256;
constexpr int kMaxRows = 32;                 // (c, kh) rows of K rounded up to even: (3 + 1) * 7 = 28
constexpr int kLdsBudget = 64 * 1024;
constexpr int kMaxTiles = 4;                 // out-channel tiles per workgroup
constexpr int kMaxStrip = 32;
constexpr long long kGridTarget = 512;       // two workgroups per CU of an MI355X
constexpr unsigned kOne = 0x3F80u;           // bf16 1.0

struct Plan {
  int steps;      // k-steps of 16 with the indicator channel
  int tiles;      // out-channel tiles per workgroup (T)
  int groups;     // workgroups along O
  int R;          // conv rows per strip (even)
  int L;          // row pairs per unit
  int IR;         // patch rows
  int ICd;        // patch row length in dwords (bf16 pairs)
  int Hc, Wc, Ho, Wo;
  size_t lds;     // bytes
};

struct Args {
  const uint8_t* x;
  const float* w;
  const float* bias;
  const float* in_scale;
  const float* in_shift;
  const float* post_scale;
  const float* post_shift;
  float* y;
  int N, C, H, W, O, KH, KW, stride, pad_h, pad_w, relu, layout;
  int Hc, Wc, Ho, Wo;
  int steps, tiles, R, L, IR, ICd, strips;
};

// LDS: [A fragments: tiles * steps * 3 * 64 uint4][patch: (C + 1) * IR * ICd dwords][rowoff: kMaxRows ints]
//      [bias, scale, shift: 3 * tiles * 32 floats]
__host__ __device__ inline size_t lds_bytes(int tiles, int steps, int patch) {
  return (size_t)tiles * steps * kTerms * 64 * 16 + (size_t)patch * 4 + kMaxRows * 4 + (size_t)3 * tiles * 32 * 4;
}

// two fp32 values -> three packed bf16 pairs, leading term first; the remainders are exact in fp32
__device__ __forceinline__ void split_pair(float x0, float x1, unsigned (&t)[kTerms]) {
  f32x2 r = {x0, x1};
#pragma unroll
  for (int i = 0; i < kTerms; ++i) {
    const bf16x2 b = __builtin_convertvector(r, bf16x2);
    t[i] = __builtin_bit_cast(unsigned, b);
    r = r - __builtin_convertvector(b, f32x2);
  }
}

// NR conv rows of one tile: out[r] = sum over the K steps; xa is the lane's window in the first row, the next row is
// rowstep dwords on.  sh = 2 where the lane's window starts at an odd pixel (stride 1, odd column), else 0.
template <int NR>
__device__ __forceinline__ void conv_rows(const uint4* wf, const unsigned* xa, int rowstep, const int* rowoff, int steps, int g,
                                          unsigned sh, f32x16 (&out)[NR]) {
  f32x16 acc0[NR], acc1[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    acc0[r] = f32x16{};
    acc1[r] = f32x16{};
  }
  for (int s = 0; s < steps; ++s) {
    Frag af[kTerms], b[NR];
#pragma unroll
    for (int i = 0; i < kTerms; ++i) af[i].q = wf[(s * kTerms + i) * 64];
    const unsigned* xr = xa + rowoff[2 * s + g];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      unsigned d[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) d[j] = xr[r * rowstep + j];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[r].u[j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], sh);
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) acc0[r] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0].v, b[r].v, acc0[r], 0, 0, 0);
#pragma unroll
    for (int r = 0; r < NR; ++r) acc1[r] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1].v, b[r].v, acc1[r], 0, 0, 0);
#pragma unroll
    for (int r = 0; r < NR; ++r) acc1[r] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[2].v, b[r].v, acc1[r], 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < NR; ++r) out[r] = acc1[r] + acc0[r];
}

__device__ __forceinline__ float finish(float v, float b, float sc, float sh, int relu) {
  v += b;
  if (relu) v = fmaxf(v, 0.f);
  return fmaf(v, sc, sh);                                     // (without post: scale 1, shift 0 -- exact)
}

template <int POOL>
__global__ __launch_bounds__(kThreads, 2) void stem_u8_kernel(Args a) {
  extern __shared__ uint4 smem[];
  uint4* const wl = smem;
  unsigned* const xs = reinterpret_cast<unsigned*>(wl + a.tiles * a.steps * kTerms * 64);
  const int plane = a.IR * a.ICd;                             // dwords of one channel of the patch
  int* const rowoff = reinterpret_cast<int*>(xs + (a.C + 1) * plane);
  float* const epi = reinterpret_cast<float*>(rowoff + kMaxRows);

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int xl = lane & 31, g = lane >> 5;
  const int n = blockIdx.x / a.strips;
  const int r0 = (blockIdx.x - n * a.strips) * a.R;          // first conv row the strip owns
  const int o0 = blockIdx.y * a.tiles * 32;                   // first out-channel of the workgroup
  constexpr int kTop = POOL == 3 ? 1 : 0;                     // conv rows above the strip that pool 3 needs

  bool ind = false;                                           // (uniform) the indicator channel is needed
  for (int c = 0; c < a.C; ++c) ind |= a.in_shift[c] != 0.f;
  const int krows = (a.C + (ind ? 1 : 0)) * a.KH;
  const int steps = (krows + 1) / 2;                          // <= a.steps, the count the LDS plan was made for

  // ---- once: A fragments, tables
  for (int e = tid; e < a.tiles * steps * 64; e += kThreads) {
    const int l = e & 63, ms = e >> 6;                        // ms = tile * steps + step
    const int m = ms / steps, s = ms - m * steps;
    const int o = o0 + m * 32 + (l & 31), row = 2 * s + (l >> 5);
    const bool live = o < a.O && row < krows;
    const int c = live ? row / a.KH : 0, kh = live ? row - c * a.KH : 0;
    const float* wo = a.w + (size_t)(live ? o : 0) * a.C * a.KH * a.KW + kh * a.KW;      // w[o][0][kh][:]
    const int cstride = a.KH * a.KW;
    float v[8];
    if (c < a.C) {
      const float sc = a.in_scale[c];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (live && j < a.KW) ? wo[c * cstride + j] * sc : 0.f;
    } else {                                                  // the indicator row: sum_c w * in_shift[c], c ascending
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float t = 0.f;
        if (j < a.KW) {
          t = wo[j] * a.in_shift[0];
          for (int cc = 1; cc < a.C; ++cc) t = t + wo[cc * cstride + j] * a.in_shift[cc];
        }
        v[j] = t;
      }
    }
    Frag f[kTerms];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned t[kTerms];
      split_pair(v[2 * j], v[2 * j + 1], t);
#pragma unroll
      for (int i = 0; i < kTerms; ++i) f[i].u[j] = t[i];
    }
#pragma unroll
    for (int i = 0; i < kTerms; ++i) wl[(ms * kTerms + i) * 64 + l] = f[i].q;
  }
  if (tid < kMaxRows) {
    const int row = min(tid, krows - 1);                      // rows past the last: zero weights, the last row's pixels
    const int c = row / a.KH, kh = row - c * a.KH;
    rowoff[tid] = (c * a.IR + kh) * a.ICd;
  }
  for (int e = tid; e < a.tiles * 32; e += kThreads) {
    const int o = o0 + e;
    const bool live = o < a.O;
    epi[e] = (live && a.bias) ? a.bias[o] : 0.f;
    epi[a.tiles * 32 + e] = (live && a.post_scale) ? a.post_scale[o] : 1.f;
    epi[2 * a.tiles * 32 + e] = (live && a.post_scale) ? a.post_shift[o] : 0.f;
  }

  // ---- staging constants: a staged row is `span` bytes of memory from column ic0 on -- one channel's (NCHW: CI = 1) or all
  // channels' interleaved (channels-last: CI = C) -- walked in aligned dwords
  const int CI = a.layout ? a.C : 1;
  const int srows = a.layout ? a.IR : a.C * a.IR;
  const int span = 2 * a.ICd * CI;
  const int nd = (span + 3) / 4 + 1;                          // aligned dwords that cover span bytes at any misalignment
  const uintptr_t xbeg = reinterpret_cast<uintptr_t>(a.x);
  const uintptr_t xend = xbeg + (size_t)a.N * a.C * a.H * a.W;
  const long long img = (long long)n * a.C * a.H * a.W;
  unsigned short* const xh = reinterpret_cast<unsigned short*>(xs);
  const int ir0 = (r0 - kTop) * a.stride - a.pad_h;           // input row of patch row 0

  constexpr int kAdv = POOL == 3 ? 30 : 32;                   // conv columns a chunk advances by
  const int chunks = POOL == 3 ? (a.Wo + 14) / 15 : (a.Wc + 31) / 32;
  const int pairs = a.R / 2, runs = (pairs + a.L - 1) / a.L;
  const int units = a.tiles * runs;
  const int rowstep = a.stride * a.ICd;                       // dwords from one conv row's window to the next
  const int el = xl * a.stride;                               // the lane's first pixel inside a patch row
  const unsigned sh = (el & 1) * 2;
  const unsigned* const xlane = xs + (el >> 1);
  const float ninf = -__builtin_inff();

  for (int ck = 0; ck < chunks; ++ck) {
    const int cc0 = ck * kAdv - kTop;                         // conv column of lane 0
    const int ic0 = cc0 * a.stride - a.pad_w;                 // input column of patch column 0
    lds_barrier();                                            // the previous chunk's patch is done with (first: the tables)
    // ---- stage the patch: 32 threads per row, one aligned dword of memory per item
    for (int row = tid >> 5; row < srows; row += kThreads / 32) {
      const int cb = a.layout ? 0 : row / a.IR, rr = row - cb * a.IR;
      const int ir = ir0 + rr;
      const bool rin = ir >= 0 && ir < a.H;
      const long long off = a.layout ? ((long long)ir * a.W + ic0) * a.C : ((long long)cb * a.H + ir) * a.W + ic0;
      const uintptr_t p0 = xbeg + (uintptr_t)(img + off);     // byte of (row, column ic0); only read from where rin
      const int mis = (int)(p0 & 3);
      unsigned short* const dst = xh + ((size_t)cb * a.IR + rr) * 2 * a.ICd;
      for (int k = tid & 31; k < nd; k += 32) {
        const uintptr_t ad = p0 - mis + 4 * k;
        unsigned d = 0;
        if (rin) {
          if (ad >= xbeg && ad + 4 <= xend) {
            d = *reinterpret_cast<const unsigned*>(ad);
          } else {                                            // a dword across an end of the tensor: its bytes one by one
#pragma unroll
            for (int b = 0; b < 4; ++b)
              if (ad + b >= xbeg && ad + b < xend) d |= (unsigned)*reinterpret_cast<const uint8_t*>(ad + b) << (8 * b);
          }
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int jp = 4 * k - mis + b;                     // byte of the staged row
          if (jp < 0 || jp >= span) continue;
          const int cr = CI == 1 ? jp : CI == 2 ? jp >> 1 : (jp * 43691) >> 17;      // jp / CI
          const int ch = jp - cr * CI, col = ic0 + cr;
          const float v = (rin && col >= 0 && col < a.W) ? (float)((d >> (8 * b)) & 0xFFu) : 0.f;
          dst[(size_t)ch * 2 * plane + cr] = (unsigned short)(__float_as_uint(v) >> 16);      // exact: eight significant bits
        }
      }
    }
    if (ind) {                                                // the indicator plane: 1 inside the image; nothing is read
      for (int e = tid; e < plane; e += kThreads) {
        const int rr = e / a.ICd, col = ic0 + 2 * (e - rr * a.ICd);
        const int ir = ir0 + rr;
        const bool rin = ir >= 0 && ir < a.H;
        xs[a.C * plane + e] = ((rin && col >= 0 && col < a.W) ? kOne : 0u) | ((rin && col + 1 >= 0 && col + 1 < a.W) ? kOne << 16 : 0u);
      }
    }
    lds_barrier();

    // ---- this wave's units: (tile m, row pairs q0 .. q1 - 1 of the strip)
    for (int u = wid; u < units; u += 4) {
      const int run = u / a.tiles, m = u - run * a.tiles;
      const int q0 = run * a.L, q1 = min(q0 + a.L, pairs);
      if (r0 + 2 * q0 >= a.Hc || o0 + m * 32 >= a.O) continue;        // (wave-uniform) nothing of the unit is stored
      const uint4* wf = wl + (m * steps) * kTerms * 64 + lane;
      const float* eb = epi + m * 32;
      const int et = a.tiles * 32;
      const int cx = cc0 + xl;                                // conv column
      const bool colok = cx >= 0 && cx < a.Wc;
      float carry[16];                                        // pool 3: the finished conv row above the next pair
      if constexpr (POOL == 3) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) carry[reg] = ninf;
        if (r0 + 2 * q0 - 1 >= 0) {                           // (wave-uniform)
          f32x16 t[1];
          conv_rows<1>(wf, xlane + (2 * q0) * rowstep, rowstep, rowoff, steps, g, sh, t);
#pragma unroll
          for (int reg = 0; reg < 16; ++reg) {
            const int ol = (reg & 3) + 8 * (reg >> 2) + 4 * g;
            if (colok) carry[reg] = finish(t[0][reg], eb[ol], eb[et + ol], eb[2 * et + ol], a.relu);
          }
        }
      }
      for (int q = q0; q < q1; ++q) {
        const int rA = r0 + 2 * q;
        if (rA >= a.Hc) break;
        f32x16 t[2];
        conv_rows<2>(wf, xlane + (2 * q + kTop) * rowstep, rowstep, rowoff, steps, g, sh, t);
        // D[out-channel][pixel]: the lane holds column xl and out-channels (reg & 3) + 8 (reg >> 2) + 4 g of the tile
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int ol = (reg & 3) + 8 * (reg >> 2) + 4 * g, o = o0 + m * 32 + ol;
          const float b = eb[ol], sc = eb[et + ol], st = eb[2 * et + ol];
          float vA = finish(t[0][reg], b, sc, st, a.relu), vB = finish(t[1][reg], b, sc, st, a.relu);
          if constexpr (POOL == 1) {
            if (o < a.O && colok) {
              float* yo = a.y + (((size_t)n * a.O + o) * a.Hc + rA) * a.Wc + cx;
              yo[0] = vA;
              if (rA + 1 < a.Hc) yo[a.Wc] = vB;
            }
          } else if constexpr (POOL == 2) {
            const float v = fmaxf(vA, vB);
            const float nb = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));   // quad_perm [1, 0, 3, 2]: lane ^ 1
            const int pr = rA >> 1, pc = cx >> 1;
            if (!(xl & 1) && o < a.O && pr < a.Ho && pc < a.Wo) a.y[(((size_t)n * a.O + o) * a.Ho + pr) * a.Wo + pc] = fmaxf(v, nb);
          } else {
            // pooled row rA / 2 = max over conv rows rA - 1 (the carry), rA, rA + 1; pooled column 15 ck + j = max over the
            // lanes 2 j, 2 j + 1, 2 j + 2.  What lies outside the conv output is -inf and never wins: the centre is inside.
            if (!colok) vA = ninf;
            if (!colok || rA + 1 >= a.Hc) vB = ninf;
            const float v = fmaxf(fmaxf(carry[reg], vA), vB);
            carry[reg] = vB;
            const float nb = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));   // lane ^ 1
            const float n2 = __int_as_float(__builtin_amdgcn_ds_bpermute(((lane + 2) & 63) << 2, __float_as_int(v)));   // lane + 2
            const int pc = 15 * ck + (xl >> 1);
            if (!(xl & 1) && xl < 30 && o < a.O && pc < a.Wo)
              a.y[(((size_t)n * a.O + o) * a.Ho + (rA >> 1)) * a.Wo + pc] = fmaxf(fmaxf(v, nb), n2);
          }
        }
      }
    }
  }
}

// the work split of the header; false: not supported
bool make_plan(const lsq_conv_geom* g, int pool, int layout, Plan* p) {
  if (check_geom(g) != LSQ_OK) return false;
  if (g->groups != 1 || g->dil_h != 1 || g->dil_w != 1 || g->C > kMaxC || g->KH > kMaxKernel || g->KW > kMaxKernel ||
      g->stride_h != g->stride_w || g->stride_h > 2 || g->pad_h >= g->KH || g->pad_w >= g->KW || g->O > kMaxO ||
      pool < 1 || pool > 3 || (layout != 0 && layout != 1))
    return false;
  if (g->H + 2 * g->pad_h < g->KH || g->W + 2 * g->pad_w < g->KW) return false;
  p->Hc = out_h(g);
  p->Wc = out_w(g);
  if (p->Hc < pool || p->Wc < pool) return false;
  p->Ho = pool == 3 ? (p->Hc - 1) / 2 + 1 : p->Hc / pool;
  p->Wo = pool == 3 ? (p->Wc - 1) / 2 + 1 : p->Wc / pool;
  const long long lim = 1ll << 31;
  if ((long long)g->N * g->C * g->H * g->W >= lim || (long long)g->N * g->O * p->Hc * p->Wc >= lim) return false;
  const int s = g->stride_h, top = pool == 3 ? 1 : 0;
  p->steps = ((g->C + 1) * g->KH + 1) / 2;
  p->ICd = s == 1 ? 20 : 36;                                   // dwords 0 .. (31 s >> 1) + 4 of a row are read
  auto fits = [&](int tiles, int R) {
    const int IR = (R + top - 1) * s + g->KH;
    return lds_bytes(tiles, p->steps, (g->C + 1) * IR * p->ICd) <= (size_t)kLdsBudget;
  };
  const int mt = (g->O + 31) / 32;
  int tmax = mt < kMaxTiles ? mt : kMaxTiles;
  while (tmax > 1 && !fits(tmax, 2)) --tmax;
  if (!fits(tmax, 2)) return false;                            // (never for the sizes accepted above)
  p->groups = (mt + tmax - 1) / tmax;
  p->tiles = (mt + p->groups - 1) / p->groups;
  const int wpt = p->tiles >= 4 ? 1 : 4 / p->tiles;            // waves that share a tile
  const int hce = (p->Hc + 1) / 2 * 2;
  int R = 2 * (pool == 3 ? 2 : 1) * wpt;
  if (R > hce) R = hce;
  while (R > 2 && !fits(p->tiles, R)) R -= 2;
  while (2 * R <= kMaxStrip && 2 * R <= hce && fits(p->tiles, 2 * R) &&
         (long long)g->N * ((p->Hc + 2 * R - 1) / (2 * R)) * p->groups >= kGridTarget)
    R *= 2;
  p->R = R;
  p->L = pool == 3 ? (R / 2 + wpt - 1) / wpt : 1;
  p->IR = (R + top - 1) * s + g->KH;
  p->lds = lds_bytes(p->tiles, p->steps, (g->C + 1) * p->IR * p->ICd);
  return true;
}

}  // namespace
}  // namespace lsq

using namespace lsq;

extern "C" int lsq_stem_u8_abi_version(void) { return LSQ_STEM_U8_ABI_VERSION; }

extern "C" int lsq_stem_conv_u8_supported(const lsq_conv_geom* g, int pool, int layout) {
  Plan p;
  return g && make_plan(g, pool, layout, &p) ? 1 : 0;
}

extern "C" int lsq_stem_conv_u8(const uint8_t* x, int layout, const float* w, const float* bias, const float* in_scale,
                                const float* in_shift, const lsq_conv_geom* g, int relu, const float* post_scale,
                                const float* post_shift, int pool, float* y, void* stream) {
  if (!x || !w || !in_scale || !in_shift || !y || !g || (post_scale == nullptr) != (post_shift == nullptr)) return LSQ_E_NULL;
  const int rc = check_geom(g);
  if (rc != LSQ_OK) return rc;
  if (relu != 0 && relu != 1) return LSQ_E_SCHEME;
  Plan p;
  if (!make_plan(g, pool, layout, &p)) return LSQ_E_UNSUPPORTED;
  Args a = {};
  a.x = x; a.w = w; a.bias = bias; a.in_scale = in_scale; a.in_shift = in_shift; a.post_scale = post_scale;
  a.post_shift = post_shift; a.y = y;
  a.N = g->N; a.C = g->C; a.H = g->H; a.W = g->W; a.O = g->O; a.KH = g->KH; a.KW = g->KW;
  a.stride = g->stride_h; a.pad_h = g->pad_h; a.pad_w = g->pad_w; a.relu = relu; a.layout = layout;
  a.Hc = p.Hc; a.Wc = p.Wc; a.Ho = p.Ho; a.Wo = p.Wo;
  a.steps = p.steps; a.tiles = p.tiles; a.R = p.R; a.L = p.L; a.IR = p.IR; a.ICd = p.ICd;
  a.strips = (p.Hc + p.R - 1) / p.R;
  const long long blocks = (long long)g->N * a.strips;
  if (blocks > 0x7FFFFFFF) return LSQ_E_UNSUPPORTED;
  const dim3 grid((unsigned)blocks, (unsigned)p.groups);
  if (pool == 1) hipLaunchKernelGGL(stem_u8_kernel<1>, grid, dim3(kThreads), p.lds, (hipStream_t)stream, a);
  else if (pool == 2) hipLaunchKernelGGL(stem_u8_kernel<2>, grid, dim3(kThreads), p.lds, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(stem_u8_kernel<3>, grid, dim3(kThreads), p.lds, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
