// The bf16 x sign-bit matrix-core core shared by the QuantLinear kernels of csrc/linear_fp (lsq_linear_signw), csrc/linear_train
// (lsq_linear_signw_dgrad) and csrc/linear_wgrad (lsq_linear_signx_wgrad).  Internal: not part of the C ABI under include/.
//
// All three are D[row][col] = sum_k A[row][k] B[k][col] on v_mfma_f32_32x32x16_bf16 with an fp32 operand A and a +-1 operand B
// that stays at one bit per element in memory.
//   * FRAGMENTS: lane (r = lane & 31, h = lane >> 5) holds A[row r][k = 8 h + j] and B[k = 8 h + j][col r] in element
//     j = 0..7 of its fragments; a lane of D holds ONE column (lane & 31) and, in register i, row
//     (i & 3) + 8 (i >> 2) + 4 h (d_row), so a store instruction writes 32 consecutive floats of a row of D per half-wave.
//   * A: v = hi + lo with hi = bf16(v), lo = bf16(v - hi) (split_pair); two MFMAs per k-step, hi then lo, into the same fp32
//     accumulator.  The tiled kernels stage hi and lo rows of 64 k in LDS, kPitch bytes apart (mma_stage reads them).
//   * B: the 8 sign bits of a lane's fragment are 8 consecutive bits (16 s + 8 h .. + 7 for k-step s) of one 64-bit word of
//     its column and become 8 bf16 +-1.0 in registers (expand8).
//   * 16-BIT A (csrc/linear_half, lsq_linear_signw_half): rows that already are bf16 or fp16 have no lo term: mma_stage1 reads
//     one staged row set and issues one MFMA per k-step (mfma16; expand8_f16 for +-1.0 in fp16).
//   * TILES: tile_rule picks one 32 x 32 tile per workgroup with the summed dimension split over kSplitWaves waves
//     (split_reduce / split_sum add the partial sums in wave order), or 128 x 128 / 64 x 64 tiles of four waves.

#ifndef LSQ_SIGNW_MMA_H
#define LSQ_SIGNW_MMA_H

#include <hip/hip_runtime.h>
#include <stdint.h>

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

constexpr int kPitch = 144;           // LDS bytes per staged row of a tiled kernel: 64 bf16 + 16 bytes of pad (conflict-free
                                      // ds_read_b128 fragments)
constexpr int kSplitWaves = 8;        // waves of a split kernel, one range of the summed dimension each

// v = hi + lo in bf16: hi = bf16(v) (round to nearest even), lo = bf16(v - hi); v - hi is exact in fp32, so
// |v - hi - lo| <= 2^-8 |v - hi| <= 2^-16 |v| (bf16 rounds to within 2^-8 of its operand; typically 2^-18 |v|: half an ulp each)
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

// Row of D that register i of a D fragment holds in half-wave hh, for the 32 x 32 block whose first row is `first`: the tiled
// epilogues, where i is a constant of the unrolled loop.  (The split kernels' tails, where i = 2 wave + 0 / 1 is a run-time
// value, write the same sum out: through a function the compiler picks other shift and mask instructions for it)
template <class T>
__device__ __forceinline__ T d_row(T first, int i, int hh) {
  return first + (i & 3) + 8 * (i >> 2) + 4 * hh;
}

// Four values k .. k + 3 of each of ROWS rows (row + 16 i, clamped to M - 1) of the row-major fp32 [M][K] matrix `base`:
// one 16-byte load a row (VEC: every row starts on 16 bytes), or four 4-byte loads; indices clamped into the row.
template <bool VEC, int ROWS>
__device__ __forceinline__ void load_rows4(const float* base, long long row, long long M, int K, int k,
                                           float (&v)[ROWS][4]) {
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const long long mi = row + 16 * i;
    const float* p = base + (mi < M ? mi : M - 1) * K;
    if constexpr (VEC) {
      const float4 t = *reinterpret_cast<const float4*>(p + min(k, K - 4));
      v[i][0] = t.x; v[i][1] = t.y; v[i][2] = t.z; v[i][3] = t.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[i][j] = p[min(k + j, K - 1)];
    }
  }
}

// Four consecutive values of a staged row, split and stored as bf16 pairs: the hi terms at d (row * kPitch + 2 * column
// bytes into the hi rows), the lo terms lo_offset bytes behind them.
__device__ __forceinline__ void stash_hi_lo(unsigned char* d, int lo_offset, const float (&c)[4]) {
  unsigned h0, l0, h1, l1;
  split_pair(c[0], c[1], h0, l0);
  split_pair(c[2], c[3], h1, l1);
  *reinterpret_cast<uint2*>(d) = make_uint2(h0, h1);
  *reinterpret_cast<uint2*>(d + lo_offset) = make_uint2(l0, l1);
}

// One stage of 64 k (four k-steps) of a wave's RB x CB blocks of 32 x 32, NQ accumulator sets (one per word set w[q]): A from
// the staged rows row0 + 32 rb + col of s_a (lo rows lo_offset bytes behind the hi rows), B from the words' bits.
// The hi products of every block first, then lo: dependent MFMAs on one accumulator are NQ * RB * CB apart.
template <int NQ, int RB, int CB>
__device__ __forceinline__ void mma_stage(const unsigned char* s_a, int lo_offset, int row0, int col, int hh,
                                          const unsigned long long (&w)[NQ][CB], f32x16 (&acc)[NQ][RB][CB]) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    Frag ah[RB], al[RB], bw[NQ][CB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const unsigned char* r = s_a + (row0 + rb * 32 + col) * kPitch + 32 * s + 16 * hh;
      const uint4 vh = *reinterpret_cast<const uint4*>(r);
      const uint4 vl = *reinterpret_cast<const uint4*>(r + lo_offset);
      ah[rb].u[0] = vh.x; ah[rb].u[1] = vh.y; ah[rb].u[2] = vh.z; ah[rb].u[3] = vh.w;
      al[rb].u[0] = vl.x; al[rb].u[1] = vl.y; al[rb].u[2] = vl.z; al[rb].u[3] = vl.w;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) bw[q][cb] = expand8((unsigned)(w[q][cb] >> (16 * s + 8 * hh)));
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
          acc[q][rb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[rb].v, bw[q][cb].v, acc[q][rb][cb], 0, 0, 0);
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
          acc[q][rb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[rb].v, bw[q][cb].v, acc[q][rb][cb], 0, 0, 0);
  }
}

// ---- the single-term stage: an A operand that already IS 16-bit (bf16 or fp16 rows, csrc/linear_half) has no lo term
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

// expand8 for an fp16 A operand: element j = +-1.0 in fp16
__device__ __forceinline__ Frag expand8_f16(unsigned bits) {
  Frag f = expand8(bits);
#pragma unroll
  for (int d = 0; d < 4; ++d) f.u[d] = (f.u[d] & 0x80008000u) | 0x3C003C00u;
  return f;
}

template <bool F16>
__device__ __forceinline__ Frag expand8_as(unsigned bits) {
  if constexpr (F16) return expand8_f16(bits);
  else return expand8(bits);
}

// one k-step of 16 on fragments of 16-bit values: v_mfma_f32_32x32x16_f16 (F16) or v_mfma_f32_32x32x16_bf16
template <bool F16>
__device__ __forceinline__ f32x16 mfma16(const Frag& a, const Frag& b, f32x16 acc) {
  if constexpr (F16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a.u), __builtin_bit_cast(f16x8, b.u), acc, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, b.v, acc, 0, 0, 0);
}

// mma_stage for a single-term A operand: the staged rows hold the 16-bit values themselves (one row set of kPitch bytes a
// row, no lo rows), one MFMA per k-step and accumulator, in the order of mma_stage's hi products.
template <bool F16, int NQ, int RB, int CB>
__device__ __forceinline__ void mma_stage1(const unsigned char* s_a, int row0, int col, int hh,
                                           const unsigned long long (&w)[NQ][CB], f32x16 (&acc)[NQ][RB][CB]) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    Frag a[RB], bw[NQ][CB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const uint4 v = *reinterpret_cast<const uint4*>(s_a + (row0 + rb * 32 + col) * kPitch + 32 * s + 16 * hh);
      a[rb].u[0] = v.x; a[rb].u[1] = v.y; a[rb].u[2] = v.z; a[rb].u[3] = v.w;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) bw[q][cb] = expand8_as<F16>((unsigned)(w[q][cb] >> (16 * s + 8 * hh)));
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) acc[q][rb][cb] = mfma16<F16>(a[rb], bw[q][cb], acc[q][rb][cb]);
  }
}

// Tail of a split kernel: every wave's partial sums to s_red ([wave][q][register][lane]) and the barrier.  After it wave g
// finishes registers 2 g and 2 g + 1 of the tile with split_sum (the callers skip rows and columns past the edge first, so
// the sums are read only where they are stored).
template <int NQ>
__device__ __forceinline__ void split_reduce(float (&s_red)[kSplitWaves][NQ][16][64], const f32x16 (&acc)[NQ], int wid,
                                             int lane) {
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int i = 0; i < 16; ++i) s_red[wid][q][i][lane] = acc[q][i];
  __syncthreads();
}

// register i of accumulator q of the tile: the partial sums added in wave order 0 .. kSplitWaves - 1
template <int NQ>
__device__ __forceinline__ float split_sum(const float (&s_red)[kSplitWaves][NQ][16][64], int q, int i, int lane) {
  float sum = s_red[0][q][i][lane];
#pragma unroll
  for (int w = 1; w < kSplitWaves; ++w) sum += s_red[w][q][i][lane];
  return sum;
}

// ---- host side
// Fewer 64 x 64 tiles of D than CUs (256): the stream of the summed dimension bounds the call, so each 32 x 32 tile gets a
// workgroup and its summed dimension is split over kSplitWaves waves; 128 x 128 tiles where there are at least 256 of them
// (one per CU), 64 x 64 otherwise.
struct TileRule {
  bool split, big;
};

inline TileRule tile_rule(long long rows, long long cols) {
  return {((rows + 63) / 64) * ((cols + 63) / 64) < 256, ((rows + 127) / 128) * ((cols + 127) / 128) >= 256};
}

// The kernels of one entry point, [0]: 4-byte loads, [1]: 16-byte loads.
template <class Args>
struct TileKernels {
  void (*split[2])(Args);
  void (*big[2])(Args);
  void (*small[2])(Args);
};

// Launches the kernel tile_rule chose; grid(tile) is the caller's grid for tiles of 32 (split), 128 or 64.
template <class Args, class Grid>
int launch_tiles(const TileKernels<Args>& k, const Args& a, TileRule rule, bool vec, Grid grid, hipStream_t st) {
  if (rule.split) hipLaunchKernelGGL(k.split[vec], grid(32), dim3(64 * kSplitWaves), 0, st, a);
  else if (rule.big) hipLaunchKernelGGL(k.big[vec], grid(128), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k.small[vec], grid(64), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace

#endif
