// ste_one of lsq_ste.hip, restated once for the libraries beside liblsq_hip.so that run the straight-through estimator in a
// GEMM's epilogue (csrc/linear_train_half: against the step's 16-bit input; csrc/linear_wgrad_half: against the fp32 weight);
// they link none of liblsq_hip.so's objects.  Internal: not part of the C ABI under include/.  The bits depend on the order
// of these operations: build without floating-point contraction (csrc/sublib.mk does).

#ifndef LSQ_STE_ONE_H
#define LSQ_STE_ONE_H

#include <hip/hip_runtime.h>
#include <math.h>

#include "lsq_hip.h"

namespace {

constexpr int kMaxK = LSQ_MAX_PLANES;

// The gradient of the quantizer chain's value through the straight-through estimator of every sign and the clamp in front:
//   r_0 = 0, d_i = clamp(xv) - r_i, r_{i+1} = r_i + v_i sign(d_i)   (sign(+-0) = +1), then with G_k = gv:
//   t_i = G_{i+1} v_i [|d_i| <= 1],  G_i = G_{i+1} - t_i,  result = [|xv| <= alpha] sum_i t_i     (k = 0: [|xv| <= alpha] gv)
__device__ __forceinline__ float ste_one(float xv, float gv, const float (&v)[kMaxK], int k, float alpha) {
  const bool inside = alpha < 0.f || (xv >= -alpha && xv <= alpha);        // clamp backward: min <= x <= max
  const float xc = alpha >= 0.f ? fminf(fmaxf(xv, -alpha), alpha) : xv;
  float r = 0.f;
  float d[kMaxK];
#pragma unroll
  for (int i = 0; i < kMaxK; ++i) {
    if (i < k) {
      d[i] = xc - r;
      r = r + v[i] * (d[i] >= 0.f ? 1.f : -1.f);       // sign(+-0) = +1
    }
  }
  float G = gv, acc = 0.f;
#pragma unroll
  for (int i = kMaxK - 1; i >= 0; --i) {
    if (i < k) {
      const float t = (fabsf(d[i]) <= 1.f) ? G * v[i] : 0.f;
      acc += t;
      G -= t;
    }
  }
  if (k == 0) acc = gv;
  return inside ? acc : 0.f;
}

}  // namespace

#endif
