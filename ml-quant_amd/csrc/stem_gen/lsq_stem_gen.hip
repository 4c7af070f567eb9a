// lsq_stem_conv_gen for gfx950: the full-precision front convolution of a network whose geometry is NOT the ImageNet stem's --
// 1..4 input channels, any kernel up to 7 x 7, stride 1 or 2, any 1..256 out-channels -- with bias, ReLU, a per-channel
// affine (an eval batch norm BEHIND the ReLU: LeNet) and a 2x2 / 2 max-pool in the epilogue, NCHW fp32 in and out, one launch.
// (include/lsq_hip_stem_gen.h: the contract and the work-split rule.)
//
// Arithmetic: lsq_stem.hip's SPLIT = 3 and nothing else.  x = h + m + l, each the bf16 rounding of what is left, six MFMA
// passes hh + (hm + mh) + (hl + lh + mm) on two fp32 accumulators (leading products; everything <= 2^-8 of them apart).
//
// GEMM view: D[out-channel][pixel] = A[out-channel][k] B[k][pixel] on v_mfma_f32_32x32x16_bf16.
//   M  = 32 out-channels (rows past O: zero weights, masked stores);
//   N  = 32 consecutive pixels of ONE conv row: a lane holds pixel lane % 32 and sixteen out-channels, so a store
//        instruction writes 128 consecutive bytes of an NCHW row and the 2x2 pool's horizontal max is the neighbouring lane;
//   K  = (c, kh, kw) with kw padded to 8 (the pad slots BEHIND the taps: zero weights): the eight k-values of one operand
//        register group are eight consecutive input columns of the (c, kh) input row, starting at column x stride - pad.  One
//        k-step of 16 is two (c, kh) rows (lane half g takes row 2 s + g); the step count ceil(C KH / 2) is a run-time number
//        (3x3x3: 5, 1x5x5: 3, 3x7x7: 11), a (c, kh) row past the last has zero weights and reads the last row's pixels.
//
// Data flow of one workgroup (256 threads; one image, one strip of R conv rows, T out-channel tiles):
//   once     the T tiles' weights are read, split and written to LDS as ready A fragments [tile][step][term][lane] of 16 bytes
//            (a lane's ds_read_b128, conflict-free); bias / post-scale / post-shift of the tiles and the dword offset of every
//            (c, kh) row inside the patch go to small LDS tables: the K loop has no division and no border branch;
//   chunk    (32 conv columns) the fp32 patch  C x ((R - 1) stride + KH) rows x (31 stride + 8 -> 40 | 72) columns  is
//            read with zero fill outside the image, split, and stored as three bf16 term planes.  At stride 2 every window
//            starts at an even 16-bit index.  At stride 1 the odd pixels' windows start at odd indices: a SECOND copy of each
//            term row, shifted by one element (position i holds column i + 1), serves them -- every operand read is four aligned
//            dwords, no unaligned LDS access anywhere;
//   unit     wave w takes the units w, w + 4, ... of (tile, row pair): per k-step three A fragments, three B fragments for each
//            of the two rows, twelve MFMAs; the A fragments are shared by the pair;
//   epilogue in registers: + bias, ReLU, fmaf(v, s, t); pool 2: max of the pair's two rows (same lane, same register), max with
//            lane ^ 1 (one DPP quad_perm), the even lanes store.  R is even, so no pooling window crosses a strip or a chunk.
// Barriers are LDS-only (lds_barrier): the stores of a chunk stay in flight while the next patch is staged.

#include "../lsq_common.h"
#include "lsq_hip_stem_gen.h"

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

constexpr int kTerms = 3;
constexpr int kThreads = 256;
constexpr int kMaxKernel = 7, kMaxC = 4, kMaxO = 256;
constexpr int kMaxRows = 32;                 // (c, kh) rows of K rounded up to even: 4 * 7 = 28
constexpr int kLdsBudget = 64 * 1024;
constexpr int kMaxTiles = 4;                 // out-channel tiles per workgroup
constexpr int kMaxStrip = 16;
constexpr long long kGridTarget = 512;       // two workgroups per CU of an MI355X

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

struct Plan {
  int steps;      // k-steps of 16
  int tiles;      // out-channel tiles per workgroup (T)
  int groups;     // workgroups along O
  int R;          // conv rows per strip (even)
  int IR;         // patch rows
  int ICd;        // patch row length in dwords (bf16 pairs)
  int copies;     // 1 (stride 2) or 2 (stride 1: the shifted copy)
  int plane;      // dwords of one (term, copy) plane: C * IR * ICd
  int Hc, Wc;
  size_t lds;     // bytes
};

struct Args {
  const float* x;
  const float* w;
  const float* bias;
  const float* post_scale;
  const float* post_shift;
  float* y;
  int N, C, H, W, O, KH, KW, stride, pad_h, pad_w, relu;
  int Hc, Wc, Ho, Wo;
  int steps, tiles, R, IR, ICd, copies, plane, strips;
};

// LDS: [A fragments: tiles * steps * 3 * 64 uint4][term planes: 3 * copies * plane dwords][rowoff: kMaxRows ints]
//      [bias, scale, shift: 3 * tiles * 32 floats]
__host__ __device__ inline size_t lds_bytes(int tiles, int steps, int copies, int plane) {
  return (size_t)tiles * steps * kTerms * 64 * 16 + (size_t)kTerms * copies * plane * 4 + kMaxRows * 4 + (size_t)3 * tiles * 32 * 4;
}

template <int POOL>
__global__ __launch_bounds__(kThreads, 2) void stem_conv_gen_kernel(Args a) {
  extern __shared__ uint4 smem[];
  uint4* const wl = smem;
  unsigned* const xs = reinterpret_cast<unsigned*>(wl + a.tiles * a.steps * kTerms * 64);
  int* const rowoff = reinterpret_cast<int*>(xs + kTerms * a.copies * a.plane);
  float* const epi = reinterpret_cast<float*>(rowoff + kMaxRows);

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int xl = lane & 31, g = lane >> 5;
  const int n = blockIdx.x / a.strips;
  const int r0 = (blockIdx.x - n * a.strips) * a.R;          // first conv row of the strip
  const int o0 = blockIdx.y * a.tiles * 32;                   // first out-channel of the workgroup
  const int krows = a.C * a.KH;

  // ---- once: A fragments, tables
  for (int e = tid; e < a.tiles * a.steps * 64; e += kThreads) {
    const int l = e & 63, ms = e >> 6;                        // ms = tile * steps + step
    const int m = ms / a.steps, s = ms - m * a.steps;
    const int o = o0 + m * 32 + (l & 31), row = 2 * s + (l >> 5);
    const bool live = o < a.O && row < krows;
    const float* wr = a.w + ((size_t)(live ? o : 0) * krows + (live ? row : 0)) * a.KW;      // w[o][c][kh][:]: (c, kh) = row
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (live && j < a.KW) ? wr[j] : 0.f;
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

  const float* __restrict__ xn = a.x + (size_t)n * a.C * a.H * a.W;
  const int ir0 = r0 * a.stride - a.pad_h;                    // input row of patch row 0
  const int chunks = (a.Wc + 31) / 32;
  const int units = a.tiles * (a.R / 2);
  const int rowlen = a.IR * a.ICd;                            // dwords of one channel of the patch
  // this lane's window inside a patch row: element xl * stride; an odd start reads the shifted copy at the even index below it
  const int el = xl * a.stride;
  const int lane_off = (el & 1) * a.plane + (el >> 1);

  for (int ck = 0; ck < chunks; ++ck) {
    lds_barrier();                                            // the previous chunk's patch is done with (first: nothing)
    // ---- stage the patch: item = (c, patch row, column pair); zero outside the image
    const int ic0 = 32 * ck * a.stride - a.pad_w;             // input column of patch column 0
    for (int e = tid; e < a.plane; e += kThreads) {
      const int c = e / rowlen, rem = e - c * rowlen;
      const int rr = rem / a.ICd, p = rem - rr * a.ICd;
      const int ir = ir0 + rr, ic = ic0 + 2 * p;
      const bool rin = ir >= 0 && ir < a.H;
      const float* xr = xn + ((size_t)c * a.H + (rin ? ir : 0)) * a.W;
      const float v0 = (rin && ic >= 0 && ic < a.W) ? xr[ic] : 0.f;
      const float v1 = (rin && ic + 1 >= 0 && ic + 1 < a.W) ? xr[ic + 1] : 0.f;
      unsigned t[kTerms];
      split_pair(v0, v1, t);
#pragma unroll
      for (int i = 0; i < kTerms; ++i) xs[(i * a.copies) * a.plane + e] = t[i];
      if (a.copies == 2) {                                    // (uniform) the copy shifted by one element
        const float v2 = (rin && ic + 2 >= 0 && ic + 2 < a.W) ? xr[ic + 2] : 0.f;
        split_pair(v1, v2, t);
#pragma unroll
        for (int i = 0; i < kTerms; ++i) xs[(i * 2 + 1) * a.plane + e] = t[i];
      }
    }
    lds_barrier();

    // ---- this wave's units: (tile m, conv rows 2 q and 2 q + 1 of the strip)
    for (int u = wid; u < units; u += 4) {
      const int q = u / a.tiles, m = u - q * a.tiles;
      const int rA = r0 + 2 * q;
      if (rA >= a.Hc || o0 + m * 32 >= a.O) continue;         // (wave-uniform) nothing of the unit is stored
      f32x16 acc0A = {}, acc1A = {}, acc0B = {}, acc1B = {};
      const uint4* wf = wl + (m * a.steps) * kTerms * 64 + lane;
      const unsigned* xa = xs + lane_off + (2 * q) * a.stride * a.ICd;      // row A; row B is stride * ICd dwords on
      const int rowB = a.stride * a.ICd;
      const int tplane = a.copies * a.plane;
      for (int s = 0; s < a.steps; ++s) {
        Frag af[kTerms], ba[kTerms], bb[kTerms];
        const unsigned* xr = xa + rowoff[2 * s + g];
#pragma unroll
        for (int i = 0; i < kTerms; ++i) {
          af[i].q = wf[(s * kTerms + i) * 64];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            ba[i].u[j] = xr[i * tplane + j];
            bb[i].u[j] = xr[i * tplane + rowB + j];
          }
        }
        // (MFMAs on the same accumulator are kept apart: two back to back wait for each other)
        acc1A = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1].v, ba[0].v, acc1A, 0, 0, 0);
        acc0A = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0].v, ba[0].v, acc0A, 0, 0, 0);
        acc1B = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1].v, bb[0].v, acc1B, 0, 0, 0);
        acc0B = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0].v, bb[0].v, acc0B, 0, 0, 0);
        acc1A = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0].v, ba[1].v, acc1A, 0, 0, 0);
        acc1B = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0].v, bb[1].v, acc1B, 0, 0, 0);
        acc1A = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0].v, ba[2].v, acc1A, 0, 0, 0);
        acc1B = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0].v, bb[2].v, acc1B, 0, 0, 0);
        acc1A = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[2].v, ba[0].v, acc1A, 0, 0, 0);
        acc1B = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[2].v, bb[0].v, acc1B, 0, 0, 0);
        acc1A = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1].v, ba[1].v, acc1A, 0, 0, 0);
        acc1B = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1].v, bb[1].v, acc1B, 0, 0, 0);
      }
      // ---- epilogue: D[out-channel][pixel]; the lane holds pixel xl and out-channels (reg & 3) + 8 (reg >> 2) + 4 g of the tile
      const int cx = 32 * ck + xl;                            // conv column
      const float* eb = epi + m * 32;
      const int et = a.tiles * 32;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int ol = (reg & 3) + 8 * (reg >> 2) + 4 * g, o = o0 + m * 32 + ol;
        const float b = eb[ol], sc = eb[et + ol], sh = eb[2 * et + ol];
        float vA = acc1A[reg] + acc0A[reg] + b, vB = acc1B[reg] + acc0B[reg] + b;
        if (a.relu) {
          vA = fmaxf(vA, 0.f);
          vB = fmaxf(vB, 0.f);
        }
        vA = fmaf(vA, sc, sh);                                // (without post: scale 1, shift 0 -- exact)
        vB = fmaf(vB, sc, sh);
        if constexpr (POOL == 1) {
          if (o < a.O && cx < a.Wc) {
            float* yo = a.y + (((size_t)n * a.O + o) * a.Hc + rA) * a.Wc + cx;
            yo[0] = vA;
            if (rA + 1 < a.Hc) yo[a.Wc] = vB;
          }
        } else {
          const float v = fmaxf(vA, vB);
          const float nb = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));   // quad_perm [1, 0, 3, 2]: lane ^ 1
          const int pr = rA >> 1, pc = cx >> 1;
          if (!(xl & 1) && o < a.O && pr < a.Ho && pc < a.Wo) a.y[(((size_t)n * a.O + o) * a.Ho + pr) * a.Wo + pc] = fmaxf(v, nb);
        }
      }
    }
  }
}

// the work split of the header; false: not supported
bool make_plan(const lsq_conv_geom* g, int pool, Plan* p) {
  if (check_geom(g) != LSQ_OK) return false;
  if (g->groups != 1 || g->dil_h != 1 || g->dil_w != 1 || g->C > kMaxC || g->KH > kMaxKernel || g->KW > kMaxKernel ||
      g->stride_h != g->stride_w || g->stride_h > 2 || g->pad_h >= g->KH || g->pad_w >= g->KW || g->O > kMaxO ||
      (pool != 1 && pool != 2))
    return false;
  if (g->H + 2 * g->pad_h < g->KH || g->W + 2 * g->pad_w < g->KW) return false;
  p->Hc = out_h(g);
  p->Wc = out_w(g);
  if (p->Hc < pool || p->Wc < pool) return false;
  const long long lim = 1ll << 31;
  if ((long long)g->N * g->C * g->H * g->W >= lim || (long long)g->N * g->O * p->Hc * p->Wc >= lim) return false;
  const int s = g->stride_h;
  p->steps = (g->C * g->KH + 1) / 2;
  p->copies = s == 1 ? 2 : 1;
  p->ICd = s == 1 ? 20 : 36;                                   // 31 s + 8 columns -> 40 | 72, in pairs
  auto fits = [&](int tiles, int R) {
    const int IR = (R - 1) * s + g->KH;
    return lds_bytes(tiles, p->steps, p->copies, g->C * IR * p->ICd) <= (size_t)kLdsBudget;
  };
  const int mt = (g->O + 31) / 32;
  int tmax = mt < kMaxTiles ? mt : kMaxTiles;
  while (tmax > 1 && !fits(tmax, 2)) --tmax;
  if (!fits(tmax, 2)) return false;                            // (never for the sizes accepted above)
  p->groups = (mt + tmax - 1) / tmax;
  p->tiles = (mt + p->groups - 1) / p->groups;
  const int hce = (p->Hc + 1) / 2 * 2;
  int R = 2 * ((4 + p->tiles - 1) / p->tiles);
  if (R > hce) R = hce;
  while (R > 2 && !fits(p->tiles, R)) R -= 2;
  while (2 * R <= kMaxStrip && 2 * R <= hce && fits(p->tiles, 2 * R) &&
         (long long)g->N * ((p->Hc + 2 * R - 1) / (2 * R)) * p->groups >= kGridTarget)
    R *= 2;
  p->R = R;
  p->IR = (R - 1) * s + g->KH;
  p->plane = g->C * p->IR * p->ICd;
  p->lds = lds_bytes(p->tiles, p->steps, p->copies, p->plane);
  return true;
}

}  // namespace
}  // namespace lsq

using namespace lsq;

extern "C" int lsq_stem_gen_abi_version(void) { return LSQ_STEM_GEN_ABI_VERSION; }

extern "C" int lsq_stem_conv_gen_supported(const lsq_conv_geom* g, int pool) {
  Plan p;
  return g && make_plan(g, pool, &p) ? 1 : 0;
}

extern "C" int lsq_stem_conv_gen(const float* x, const float* w, const float* bias, const lsq_conv_geom* g, int relu,
                                 const float* post_scale, const float* post_shift, int pool, float* y, void* stream) {
  if (!x || !w || !y || !g || (post_scale == nullptr) != (post_shift == nullptr)) return LSQ_E_NULL;
  const int rc = check_geom(g);
  if (rc != LSQ_OK) return rc;
  if (relu != 0 && relu != 1) return LSQ_E_SCHEME;
  Plan p;
  if (!make_plan(g, pool, &p)) return LSQ_E_UNSUPPORTED;
  Args a = {};
  a.x = x; a.w = w; a.bias = bias; a.post_scale = post_scale; a.post_shift = post_shift; a.y = y;
  a.N = g->N; a.C = g->C; a.H = g->H; a.W = g->W; a.O = g->O; a.KH = g->KH; a.KW = g->KW;
  a.stride = g->stride_h; a.pad_h = g->pad_h; a.pad_w = g->pad_w; a.relu = relu;
  a.Hc = p.Hc; a.Wc = p.Wc; a.Ho = p.Hc / pool; a.Wo = p.Wc / pool;
  a.steps = p.steps; a.tiles = p.tiles; a.R = p.R; a.IR = p.IR; a.ICd = p.ICd; a.copies = p.copies; a.plane = p.plane;
  a.strips = (p.Hc + p.R - 1) / p.R;
  const long long blocks = (long long)g->N * a.strips;
  if (blocks > 0x7FFFFFFF) return LSQ_E_UNSUPPORTED;
  const dim3 grid((unsigned)blocks, (unsigned)p.groups);
  if (pool == 1) hipLaunchKernelGGL(stem_conv_gen_kernel<1>, grid, dim3(kThreads), p.lds, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(stem_conv_gen_kernel<2>, grid, dim3(kThreads), p.lds, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
