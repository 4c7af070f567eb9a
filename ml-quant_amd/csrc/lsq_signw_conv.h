// Shared declarations of the sign-weight convolution kernels (lsq_signw_conv_core.h: the general kernels, instantiated by
// lsq_signw_conv.hip and conv_half/lsq_conv_half.hip; lsq_signw_lean.hip: the 3x3 fast path with weights expanded once per
// eval session).
#pragma once

#include "lsq_common.h"

namespace lsq {
namespace signw {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

struct SwArgs {
  const float* x;                      // [N][C][H][W]
  const unsigned long long* wbits;     // [taps][Gg][Opad]  (one weight plane)
  const float* wscale;                 // [O]
  const float* bias;                   // [O] or null
  const float* pre_scale;              // [C] or null (folded eval batch norm)
  const float* pre_shift;
  float* y;                            // [N][O][Ho][Wo]
  float alpha;
  int N, C, H, W, O, KH, KW, sh, sw, ph, pw, dh, dw;
  int Gg, Ho, Wo, cg, og, og_pad, opad_total, tiles_per_group;
  int accumulate;
  int final_pass;
  int relu;                            // epilogue: y = act(conv + bias + res_pre) + res_post; LSQ_ACT_*
  const float* slope;                  // PReLU slope(s): [1] or [O]
  const float* res_pre;                // [N][O][Ho][Wo] or null
  const float* res_post;
};

union Frag {
  unsigned u[4];
  bf16x8 v;
};

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) unsigned short u16x2;

// x = hi + lo in bf16: hi = bf16(x) (v_cvt_pk_bf16_f32, round to nearest even), lo = bf16(x - hi).
// x - hi is exact in fp32, so |x - hi - lo| <= 2^-18 |x|.
__device__ __forceinline__ void split_pair(float x0, float x1, unsigned& hi, unsigned& lo) {
  const f32x2 v = {x0, x1};
  const bf16x2 h = __builtin_convertvector(v, bf16x2);
  const f32x2 r = v - __builtin_convertvector(h, f32x2);
  const bf16x2 l = __builtin_convertvector(r, bf16x2);
  hi = __builtin_bit_cast(unsigned, h);
  lo = __builtin_bit_cast(unsigned, l);
}

constexpr int kPC = 16;                          // channels per chunk (one MFMA k-step)
constexpr int kPRow = 32;                        // bytes per LDS row (16 bf16)

// LDS rows of 32 bytes without padding: the two 16-byte halves of row r are swapped when bit 3 of r is set, which
// makes the ds_read_b128 lane groups (16 lanes on consecutive rows) hit 16 distinct 4-bank groups.
__device__ __forceinline__ int swz(int row, int half) { return row * kPRow + ((half ^ ((row >> 3) & 1)) << 4); }

// lsq_signw_lean.hip
// bytes of the expanded weight operand of `planes` weight planes, 0 when the geometry is outside the fast path
long long lean_weight_bytes(const lsq_conv_geom* g, int planes);
int lean_prepare(const uint64_t* wbits, int planes, const lsq_conv_geom* g, void* wprep, hipStream_t st);
// LSQ_E_UNSUPPORTED when the call is outside the fast path (the caller then takes the general kernels)
int lean_launch(const SwArgs& a, const void* wprep, int plane, const lsq_conv_geom* g, hipStream_t st);

}  // namespace signw
}  // namespace lsq
