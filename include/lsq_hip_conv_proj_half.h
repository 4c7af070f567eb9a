/*
 * lsq_hip_conv_proj_half.h -- C ABI of the projection shortcut on 16-bit tensors (liblsq_hip_conv_proj_half.so):
 * lsq_pointwise_conv_half, the strided 1x1 convolution lsq_pointwise_conv on a bf16 / fp16 input, and
 * lsq_xnor_conv2d_proj_half, lsq_xnor_conv2d_proj with a 16-bit projection input, 16-bit residuals and a 16-bit output.
 * Both compute in fp32 exactly as their fp32 counterparts do and round once, at the store.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller, `stream` is a hipStream_t passed as void*
 * (NULL = default stream), every function returns 0, a negative LSQ_E_* code for an argument error (returned before any
 * launch, nothing written), or a positive hipError_t if a launch failed.
 *
 * The entry points are a library of their own because the function list of lsq_hip.h is fixed at ABI version 12; the
 * kernels are those of liblsq_hip.so (csrc/lsq_pointwise.hip and the PROJ instantiations of csrc/lsq_xnor_mfma.hip, their
 * __bf16 / _Float16 instantiations), which this library links: both must come from the same build and sit in the same
 * directory.  The test hooks of lsq_hip_debug.h act on lsq_xnor_conv2d_proj_half as they do on lsq_xnor_conv2d_proj.
 *
 * Fused and unfused are NOT bit-equal in 16 bits.  lsq_xnor_conv2d_proj_half keeps the shortcut in fp32 registers and rounds
 * once, the final y.  The two-launch composition lsq_pointwise_conv_half + lsq_xnor_conv2d_half rounds the shortcut to 16 bits
 * first (it is a tensor of `dtype` in between) and y again.  In fp32 the two routes give the same bits; here each is bit-equal
 * to its OWN fp32 composition, stated at the two functions below, and they differ from each other by that one rounding.
 */
#ifndef LSQ_HIP_CONV_PROJ_HALF_H_
#define LSQ_HIP_CONV_PROJ_HALF_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"
#include "lsq_hip_linear_half.h" /* LSQ_DTYPE_* */

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_CONV_PROJ_HALF_ABI_VERSION 1

int lsq_conv_proj_half_abi_version(void);

/*
 * y[n][o][ho][wo] = sum_c w[o][c] * x[n][c][ho * stride][wo * stride] + bias[o] as lsq_pointwise_conv computes it, where
 *   x      [N][C][H][W] of `dtype`, contiguous: widened to fp32 as it is staged (exact);
 *   dtype  LSQ_DTYPE_BF16 or LSQ_DTYPE_F16: the type of x and y;
 *   w      [O][C] fp32, bias [O] fp32 or NULL: as in lsq_pointwise_conv;
 *   y      out, [N][O][Ho][Wo] of `dtype`, Ho = (H - 1) / stride + 1: the fp32 accumulator plus bias rounded ONCE, to nearest
 *          even, as Tensor.to(dtype) rounds (fp16 overflow gives +-inf); nothing outside it is written.
 * x and y are aligned to 2 bytes; nothing more is required of them (a view that starts one element into a storage is served:
 * the kernels' 8-byte accesses are taken only where the pointers allow them).
 *
 * Contract: y is bit for bit lsq_pointwise_conv(x.float(), ...).to(dtype).
 *
 * Refusals, before any launch (a refused call writes nothing): those of lsq_pointwise_conv with the same codes -- LSQ_E_NULL
 * (x, w or y), LSQ_E_SHAPE (a non-positive size or stride), LSQ_E_UNSUPPORTED (C or O not a multiple of 64, 2^30 or more
 * elements in x or y) --; LSQ_E_UNSUPPORTED for another dtype.
 */
int lsq_pointwise_conv_half(const void* x, int dtype, int N, int C, int H, int W, const float* w, const float* bias, int O,
                            int stride, void* y, void* stream);

/* The projection operand of lsq_xnor_conv2d_proj_half: lsq_proj (lsq_hip_conv_proj.h) with x of the call's `dtype`. */
typedef struct lsq_proj_half {
  const void* x;     /* [N][C][H][W] of `dtype`, contiguous, 2-byte aligned */
  const float* w;    /* [O][C] fp32, 16-byte aligned */
  const float* bias; /* [O] fp32 or NULL */
  int32_t C, H, W;   /* N and O are the convolution's */
  int32_t stride;
  int32_t post;      /* 0: the value plays res_pre (added before the non-linearity), 1: res_post (added after it) */
} lsq_proj_half;

/*
 * y = act(conv + bias + res_pre) + res_post as lsq_xnor_conv2d_proj computes it, one of the two residuals being the
 * projection `proj`, where proj->x, the residual tensor in the other slot (or NULL) and y are of `dtype` (LSQ_DTYPE_BF16 or
 * LSQ_DTYPE_F16).  16-bit values are widened exactly as they are read; the projection is computed in fp32 in the
 * epilogue's residual registers and never rounded; y is the fp32 result rounded ONCE, to nearest even.  The other arguments
 * are lsq_xnor_conv2d_half's; there is no workspace because the call is always one launch (kx = 2, kw_planes = 1).
 *
 * Contract: y is bit for bit
 *   lsq_xnor_conv2d_proj(same operands, proj with x.float(), res_pre.float(), res_post.float()).to(dtype).
 *
 * Refusals, before any launch (a refused call writes nothing): everything lsq_xnor_conv2d_proj refuses, with the same codes
 * (lsq_hip_conv_proj.h); LSQ_E_UNSUPPORTED for another dtype.  After LSQ_E_UNSUPPORTED the caller runs
 * lsq_pointwise_conv_half + lsq_xnor_conv2d_half, which rounds the shortcut first: see the note on top.
 */
int lsq_xnor_conv2d_proj_half(const uint64_t* xplanes, int kx, const float* xscales, const uint64_t* wbits,
                              const int32_t* wsum, int kw_planes, const float* wscales, const float* bias,
                              const lsq_conv_geom* g, int act, const float* act_slope, const void* res_pre,
                              const void* res_post, const lsq_proj_half* proj, int dtype, void* y, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_CONV_PROJ_HALF_H_ */
