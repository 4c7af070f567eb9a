// Reading bf16 / fp16 rows in GROUPS of 8 elements (byte g of a row's plane words = its elements 8 g .. 8 g + 7), shared by
// the three 16-bit activation quantizers (linear_act_half/lsq_linear_act_half.hip, linear_act_solve/lsq_linear_act_solve.hip,
// conv_act_half/lsq_conv_act_half.hip; the last two also through linear_act_solve/lsq_half_table.h): the exact conversion
// to fp32, the symmetric clamp, the group load on either alignment and the wave sum whose order is the same in every lane.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lsq_half {

template <bool F16>
__device__ __forceinline__ float to_f32(unsigned h) {  // h: 16 bits
  if constexpr (F16) return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
  else return __uint_as_float(h << 16);
}

__device__ __forceinline__ float clamp_sym(float x, float alpha) {
  return alpha >= 0.f ? fminf(fmaxf(x, -alpha), alpha) : x;
}

// group g of the row (g inside the row's groups): the raw 16 bytes; what lies past L is unspecified (masked by the caller)
template <bool VEC>
__device__ __forceinline__ uint4 load_group(const unsigned short* xrow, long long L, int g) {
  const long long e = 8ll * g;
  if constexpr (VEC) {                                // L % 8 == 0: a group is inside the row or past it
    return *reinterpret_cast<const uint4*>(xrow + (e < L ? e : L - 8));
  } else {
    unsigned h[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = xrow[e + j < L ? e + j : L - 1];
    return make_uint4(h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16);
  }
}

__device__ __forceinline__ double wave_sum(double v) {  // xor butterfly: every lane ends with the same bits
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

}  // namespace lsq_half
