// lsq_linear_signw_dgrad: fp32 gradient rows x sign-weight planes with the sum over the OUTPUT features, on the bf16 matrix
// cores of gfx950 (v_mfma_f32_32x32x16_bf16) -- the input gradient of QuantLinear, lsq_linear_signw transposed.
//
// As a GEMM:  gx[m][f] = sum_q sum_o (gy[m][o] ws[q][o]) s_q[o][f],  M = rows, K = O output features (per plane), N = F.
// Gradient rows are operand A (rows m), weights operand B (columns f): a lane of D holds ONE column f (lane & 31) and 16
// rows, so a store instruction writes 32 consecutive floats of a row of gx per half-wave.  Lane (r = lane & 31,
// h = lane >> 5) holds A[row r][k = 8 h + j] and B[k = 8 h + j][col r] in element j = 0..7 of its fragments.
//   * WEIGHT: the forward's planes hold the bits of 64 FEATURES in a word; here k runs over o, so a first kernel
//     (transpose_planes) writes the transposed image T[q][ceil(O / 64)][ceil16(F)] into the caller's workspace: one wave
//     per 64 x 64 bit block, lane j reads the word of output feature 64 w + j, ballot i collects bit i of all lanes =
//     the word of input feature i.  After it a lane's B fragment is 8 consecutive bits of one word of its column and
//     becomes 8 bf16 +-1.0 in registers (expand8, as the forward): one bit per weight in memory throughout.
//   * GRADIENT: a = fl32(gy ws[q][o]) -- the scale is per (plane, k) here, so it goes into A and all planes add into ONE
//     accumulator --, split into hi = bf16(a) and lo = bf16(a - hi); two MFMAs per k-step (hi, then lo).  Output features
//     past O are staged as 0: the padded slots of a plane are zero words and would read as -1.
//   * Rows past M and columns past F read a valid row / column and are never stored.
// Two kernels behind the one entry point (selected from M and F, see lsq_linear_signw_dgrad):
//   dgrad_tiled  M x F tiles of 128 x 128 or 64 x 64, four waves (2 x 2), over the kw * ceil(O / 64) stages (plane-major);
//                per stage the workgroup scales and splits its rows' gradients ONCE into LDS (hi and lo rows of 144 bytes:
//                16-byte pad, conflict-free ds_read_b128 fragments); the next stage's gradients, scales and weight words
//                are loaded into registers while the MFMAs of this one run.
//   dgrad_split  few tiles (LeNet fc1, the ResNet head): one 32 x 32 tile of gx per workgroup, the stages split over 8
//                waves, each reading, scaling, splitting and multiplying its own range straight from global memory; the
//                partial sums meet in LDS and are added in wave order.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lsq_hip_linear_train.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) unsigned short u16x2;

union Frag {
  unsigned u[4];
  bf16x8 v;
};

struct Args {
  const float* gy;                    // [M][O]
  const unsigned long long* tbits;    // transposed planes [kw][nwo][fpad]
  const float* wscales;               // [kw][O]
  float* gx;                          // [M][F]
  long long M;
  int F, O, fpad, nwo, stages;        // fpad = ceil16(F); nwo = ceil(O / 64); stages = kw * nwo
};

constexpr int kPitch = 144;           // LDS bytes per staged row of dgrad_tiled: 64 bf16 + 16 bytes of pad
constexpr int kSplitWaves = 8;        // waves of dgrad_split, one range of stages each

// v = hi + lo in bf16: hi = bf16(v) (round to nearest even), lo = bf16(v - hi); v - hi is exact in fp32, so
// |v - hi - lo| <= 2^-8 |v - hi| <= 2^-16 |v|
__device__ __forceinline__ void split_pair(float v0, float v1, unsigned& hi, unsigned& lo) {
  const f32x2 v = {v0, v1};
  const bf16x2 h = __builtin_convertvector(v, bf16x2);
  const f32x2 r = v - __builtin_convertvector(h, f32x2);
  const bf16x2 l = __builtin_convertvector(r, bf16x2);
  hi = __builtin_bit_cast(unsigned, h);
  lo = __builtin_bit_cast(unsigned, l);
}

// 8 sign bits (bit j set = +1) -> B fragment: element j = +-1.0 in bf16, half (j & 1) of dword j >> 1.  The inverted bits
// in both 16-bit halves, one packed shift brings bit 2d / 2d + 1 to the sign position of the low / high half.
__device__ __forceinline__ Frag expand8(unsigned bits) {
  const unsigned short m = (unsigned short)(~bits & 0xFFu);
  const u16x2 rep = {m, m};
  Frag f;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const u16x2 sh = {(unsigned short)(15 - 2 * d), (unsigned short)(14 - 2 * d)};
    const u16x2 s = rep << sh;
    f.u[d] = (__builtin_bit_cast(unsigned, s) & 0x80008000u) | 0x3F803F80u;
  }
  return f;
}

// ---------------------------------------------------------------------------------------------------------------------
// T[q][w][f] bit j = wbits[q][f / 64][64 w + j] bit f % 64: one wave per 64 x 64 bit block (grid-stride over the blocks).
// Output features past ceil16(O) read as zero words (their A operand is 0 in the GEMM); columns f < ceil16(F) are written.
__global__ __launch_bounds__(256) void transpose_planes(const unsigned long long* __restrict__ wbits,
                                                        unsigned long long* __restrict__ tbits, int nwf, int opad, int nwo,
                                                        int fpad, long long blocks) {
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * 4;
  for (long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); b < blocks; b += stride) {
    const int fw = (int)(b % nwf);
    const long long t = b / nwf;
    const int ow = (int)(t % nwo);
    const long long q = t / nwo;
    const int o = ow * 64 + lane;
    const unsigned long long w = o < opad ? wbits[(q * nwf + fw) * opad + o] : 0ull;
    unsigned long long out = 0;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      const unsigned long long m = __ballot((int)((w >> i) & 1ull));
      if (lane == i) out = m;
    }
    const int f = fw * 64 + lane;
    if (f < fpad) tbits[(q * nwo + ow) * fpad + f] = out;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
template <int RB, int CB, bool VEC>
__global__ __launch_bounds__(256, 2) void dgrad_tiled(Args a) {
  constexpr int BM = 64 * RB;
  constexpr int kRows = BM / 16;                      // staged rows per thread and stage (16 threads x 4 values a row)
  __shared__ __attribute__((aligned(16))) unsigned char s_a[2 * BM * kPitch];    // hi rows [BM], then lo rows [BM]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int col = lane & 31, hh = lane >> 5;
  const int wr = wid >> 1, wc = wid & 1;              // the wave's block of rows / columns in the tile
  const long long m0 = (long long)blockIdx.x * BM;
  const int f0 = blockIdx.y * 64 * CB;
  const int sf = (tid & 15) * 4, sr = tid >> 4;       // staging role: output features sf .. sf + 3 of rows sr + 16 i

  float gr[kRows][4], sc[4];
  unsigned long long wn[CB], wcur[CB];
  auto load = [&](int it) {
    const int q = it / a.nwo, st = it - q * a.nwo;
    const int o = st * 64 + sf;
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      const long long mi = m0 + sr + 16 * i;
      const float* p = a.gy + (mi < a.M ? mi : a.M - 1) * a.O;
      if constexpr (VEC) {
        const float4 v = *reinterpret_cast<const float4*>(p + min(o, a.O - 4));
        gr[i][0] = v.x; gr[i][1] = v.y; gr[i][2] = v.z; gr[i][3] = v.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) gr[i][j] = p[min(o + j, a.O - 1)];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) sc[j] = a.wscales[(long long)q * a.O + min(o + j, a.O - 1)];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
      const int f = min(f0 + wc * 32 * CB + cb * 32 + col, a.fpad - 1);
      wn[cb] = a.tbits[(long long)it * a.fpad + f];
    }
  };
  auto stash = [&](int it) {
    const int q = it / a.nwo, st = it - q * a.nwo;
    const int o = st * 64 + sf;
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      float c[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) c[j] = o + j < a.O ? __fmul_rn(gr[i][j], sc[j]) : 0.f;
      unsigned h0, l0, h1, l1;
      split_pair(c[0], c[1], h0, l0);
      split_pair(c[2], c[3], h1, l1);
      unsigned char* d = s_a + (sr + 16 * i) * kPitch + sf * 2;
      *reinterpret_cast<uint2*>(d) = make_uint2(h0, h1);
      *reinterpret_cast<uint2*>(d + BM * kPitch) = make_uint2(l0, l1);
    }
  };

  f32x16 acc[RB][CB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[rb][cb][i] = 0.f;

  load(0);
  for (int it = 0; it < a.stages; ++it) {
    __syncthreads();                                  // every wave is done reading the previous stage
    stash(it);
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) wcur[cb] = wn[cb];
    __syncthreads();
    if (it + 1 < a.stages) load(it + 1);              // in flight during the MFMAs below
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      Frag ah[RB], al[RB], bw[CB];
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        const unsigned char* r = s_a + (wr * 32 * RB + rb * 32 + col) * kPitch + 32 * s + 16 * hh;
        const uint4 vh = *reinterpret_cast<const uint4*>(r);
        const uint4 vl = *reinterpret_cast<const uint4*>(r + BM * kPitch);
        ah[rb].u[0] = vh.x; ah[rb].u[1] = vh.y; ah[rb].u[2] = vh.z; ah[rb].u[3] = vh.w;
        al[rb].u[0] = vl.x; al[rb].u[1] = vl.y; al[rb].u[2] = vl.z; al[rb].u[3] = vl.w;
      }
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) bw[cb] = expand8((unsigned)(wcur[cb] >> (16 * s + 8 * hh)));
      // hi products of every tile first, then lo: dependent MFMAs on one accumulator are RB * CB apart
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
          acc[rb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[rb].v, bw[cb].v, acc[rb][cb], 0, 0, 0);
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
          acc[rb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[rb].v, bw[cb].v, acc[rb][cb], 0, 0, 0);
    }
  }

#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
    const int f = f0 + wc * 32 * CB + cb * 32 + col;
    if (f >= a.F) continue;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const long long m = m0 + wr * 32 * RB + rb * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh;
        if (m >= a.M) continue;
        a.gx[m * a.F + f] = acc[rb][cb][i];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(64 * kSplitWaves) void dgrad_split(Args a) {
  __shared__ float s_red[kSplitWaves][16][64];        // every wave's partial sums, [register][lane]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int col = lane & 31, hh = lane >> 5;
  const int f0 = blockIdx.x * 32;
  const long long m0 = (long long)blockIdx.y * 32;
  const int per = (a.stages + kSplitWaves - 1) / kSplitWaves;
  const int i0 = wid * per, i1 = min(a.stages, i0 + per);        // this wave's stages (64 output features of one plane each)
  const long long mr = m0 + col < a.M ? m0 + col : a.M - 1;      // the lane's A row
  const float* grow = a.gy + mr * a.O;
  const int fw = min(f0 + col, a.fpad - 1);                      // the lane's B column

  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;

  float gn[32], sn[32];
  unsigned long long wn;
  auto load = [&](int it) {
    const int q = it / a.nwo, st = it - q * a.nwo;
    const float* ws = a.wscales + (long long)q * a.O;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int o = st * 64 + 16 * s + 8 * hh;
      if constexpr (VEC) {
        const float4 v0 = *reinterpret_cast<const float4*>(grow + min(o, a.O - 4));
        const float4 v1 = *reinterpret_cast<const float4*>(grow + min(o + 4, a.O - 4));
        gn[8 * s + 0] = v0.x; gn[8 * s + 1] = v0.y; gn[8 * s + 2] = v0.z; gn[8 * s + 3] = v0.w;
        gn[8 * s + 4] = v1.x; gn[8 * s + 5] = v1.y; gn[8 * s + 6] = v1.z; gn[8 * s + 7] = v1.w;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) gn[8 * s + j] = grow[min(o + j, a.O - 1)];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) sn[8 * s + j] = ws[min(o + j, a.O - 1)];
    }
    wn = a.tbits[(long long)it * a.fpad + fw];
  };

  if (i0 < i1) load(i0);
  for (int it = i0; it < i1; ++it) {
    float gv[32], sv[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) { gv[j] = gn[j]; sv[j] = sn[j]; }
    const unsigned long long wv = wn;
    const int st = it % a.nwo;
    if (it + 1 < i1) load(it + 1);                    // in flight during the MFMAs below
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int o = st * 64 + 16 * s + 8 * hh;
      float c[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) c[j] = o + j < a.O ? __fmul_rn(gv[8 * s + j], sv[8 * s + j]) : 0.f;
      Frag hi, lo;
#pragma unroll
      for (int d = 0; d < 4; ++d) split_pair(c[2 * d], c[2 * d + 1], hi.u[d], lo.u[d]);
      const Frag bw = expand8((unsigned)(wv >> (16 * s + 8 * hh)));
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hi.v, bw.v, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lo.v, bw.v, acc, 0, 0, 0);
    }
  }

#pragma unroll
  for (int i = 0; i < 16; ++i) s_red[wid][i][lane] = acc[i];
  __syncthreads();

  // wave g finishes registers 2 g and 2 g + 1 of the tile: the partial sums added in wave order
  const int f = f0 + col;
  if (f >= a.F) return;
#pragma unroll
  for (int ii = 0; ii < 2; ++ii) {
    const int i = 2 * wid + ii;
    const long long m = m0 + (i & 3) + 8 * (i >> 2) + 4 * hh;
    if (m >= a.M) continue;
    float sum = s_red[0][i][lane];
#pragma unroll
    for (int w = 1; w < kSplitWaves; ++w) sum += s_red[w][i][lane];
    a.gx[m * a.F + f] = sum;
  }
}

int launch(const Args& a, bool split, bool big, bool vec, hipStream_t st) {
  if (split) {
    const dim3 grid((unsigned)((a.F + 31) / 32), (unsigned)((a.M + 31) / 32));
    if (vec) hipLaunchKernelGGL((dgrad_split<true>), grid, dim3(64 * kSplitWaves), 0, st, a);
    else hipLaunchKernelGGL((dgrad_split<false>), grid, dim3(64 * kSplitWaves), 0, st, a);
  } else if (big) {
    const dim3 grid((unsigned)((a.M + 127) / 128), (unsigned)((a.F + 127) / 128));
    if (vec) hipLaunchKernelGGL((dgrad_tiled<2, 2, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((dgrad_tiled<2, 2, false>), grid, dim3(256), 0, st, a);
  } else {
    const dim3 grid((unsigned)((a.M + 63) / 64), (unsigned)((a.F + 63) / 64));
    if (vec) hipLaunchKernelGGL((dgrad_tiled<1, 1, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((dgrad_tiled<1, 1, false>), grid, dim3(256), 0, st, a);
  }
  return (int)hipGetLastError();
}

bool in_limits(int kw_planes, int64_t F, int64_t O) {
  return kw_planes >= 1 && kw_planes <= LSQ_MAX_PLANES && F > 0 && O > 0 && F < (1ll << 22) && O < (1ll << 21);
}

}  // namespace

extern "C" int lsq_linear_train_abi_version(void) { return LSQ_LINEAR_TRAIN_ABI_VERSION; }

extern "C" size_t lsq_linear_signw_dgrad_workspace_bytes(int kw_planes, int64_t F, int64_t O) {
  if (!in_limits(kw_planes, F, O)) return 0;
  return (size_t)kw_planes * (size_t)((O + 63) / 64) * (size_t)((F + 15) / 16 * 16) * sizeof(unsigned long long);
}

extern "C" int lsq_linear_signw_dgrad(const float* gy, const uint64_t* wbits, int kw_planes, const float* wscales,
                                      int64_t M, int64_t F, int64_t O, float* gx, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  if (!gy || !wbits || !wscales || !gx) return LSQ_E_NULL;
  if (M <= 0 || F <= 0 || O <= 0) return LSQ_E_SHAPE;
  if (!in_limits(kw_planes, F, O) || M >= (1ll << 31)) return LSQ_E_UNSUPPORTED;
  if (!workspace || ((uintptr_t)workspace & 7) ||
      workspace_bytes < lsq_linear_signw_dgrad_workspace_bytes(kw_planes, F, O))
    return LSQ_E_WORKSPACE;
  Args a = {};
  a.gy = gy;
  a.tbits = (const unsigned long long*)workspace;
  a.wscales = wscales;
  a.gx = gx;
  a.M = M;
  a.F = (int)F;
  a.O = (int)O;
  a.fpad = (int)((F + 15) / 16 * 16);
  a.nwo = (int)((O + 63) / 64);
  a.stages = kw_planes * a.nwo;
  hipStream_t st = (hipStream_t)stream;

  const int nwf = (int)((F + 63) / 64), opad = (int)((O + 15) / 16 * 16);
  const long long blocks = (long long)a.stages * nwf;             // 64 x 64 bit blocks, one wave each
  const long long tgrid = (blocks + 3) / 4;
  hipLaunchKernelGGL(transpose_planes, dim3((unsigned)(tgrid < (1ll << 20) ? tgrid : (1ll << 20))), dim3(256), 0, st,
                     (const unsigned long long*)wbits, (unsigned long long*)workspace, nwf, opad, a.nwo, a.fpad, blocks);
  int e = (int)hipGetLastError();
  if (e) return e;

  // 16-byte gradient loads where every row starts on 16 bytes (same values, same bits as the 4-byte loads)
  const bool vec = ((uintptr_t)gy & 15) == 0 && O % 4 == 0;
  // the tile rule of lsq_linear_signw with F in the place of O: fewer 64 x 64 tiles than CUs -> the summed dimension of
  // each 32 x 32 tile split over 8 waves; 128 x 128 tiles where there are at least 256 of them, 64 x 64 otherwise
  const bool split = ((M + 63) / 64) * ((F + 63) / 64) < 256;
  const bool big = ((M + 127) / 128) * ((F + 127) / 128) >= 256;
  return launch(a, split, big, vec, st);
}
