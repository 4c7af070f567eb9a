/*
 * lsq_hip_conv_proj.h -- C ABI of lsq_xnor_conv2d_proj (liblsq_hip_conv_proj.so): lsq_xnor_conv2d with the projection
 * shortcut of a down-sampling residual block computed inside the convolution that adds it.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller, `stream` is a hipStream_t passed as void*
 * (NULL = default stream), every function returns 0, a negative LSQ_E_* code for an argument error (returned before any
 * launch, nothing written), or a positive hipError_t if a launch failed.
 *
 * The entry point is a library of its own because the function list of lsq_hip.h is fixed at ABI version 12; the kernel is
 * the XNOR matrix-core kernel of liblsq_hip.so (csrc/lsq_xnor_mfma.hip, its PROJ instantiations), which this library links:
 * both must come from the same build and sit in the same directory.  The test hooks of lsq_hip_debug.h act on this call too.
 */
#ifndef LSQ_HIP_CONV_PROJ_H_
#define LSQ_HIP_CONV_PROJ_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_CONV_PROJ_ABI_VERSION 1

int lsq_conv_proj_abi_version(void);

/*
 * The projection operand: the strided 1x1 convolution (batch norm folded into w, bias) that lsq_pointwise_conv computes,
 *   sc[n][o][ho][wo] = sum_c w[o][c] * x[n][c][ho * stride][wo * stride] + bias[o],
 * read by output pixel (n, ho, wo) of the XNOR convolution whatever that convolution's own stride is.
 */
typedef struct lsq_proj {
  const float* x;    /* [N][C][H][W] fp32, contiguous */
  const float* w;    /* [O][C] fp32, 16-byte aligned */
  const float* bias; /* [O] or NULL */
  int32_t C, H, W;   /* N and O are the convolution's */
  int32_t stride;
  int32_t post;      /* 0: the value plays res_pre (added before the non-linearity), 1: res_post (added after it) */
} lsq_proj;

/*
 * y = act(conv + bias + res_pre) + res_post as lsq_xnor_conv2d computes it, with one of the two residuals being the
 * projection `proj`, computed per tile of 32 pixels x 32 out-channels on v_mfma_f32_32x32x2_f32 in lsq_pointwise_conv's
 * k order: the result equals lsq_pointwise_conv followed by lsq_xnor_conv2d bit for bit, without the launch, the write
 * of sc and its read.  All other arguments are lsq_xnor_conv2d's.
 *
 * LSQ_E_NULL: proj, proj->x or proj->w is NULL (or what lsq_xnor_conv2d refuses as such).
 * LSQ_E_SHAPE: a non-positive C, H, W or stride; (H - 1) / stride + 1 != Ho or (W - 1) / stride + 1 != Wo.
 * LSQ_E_SCHEME: a residual tensor in the slot the projection takes (res_pre with post = 0, res_post with post = 1).
 * LSQ_E_UNSUPPORTED: C not a multiple of 64 or above 512; 2^30 or more elements in proj->x; proj->w not 16-byte aligned; a geometry outside the fp4
 *   matrix-core kernel (3x3 taps, groups 1, 64 / 128 / 256 / 512 input channels, O a multiple of 32, fewer than 2^30
 *   outputs); anything but two activation planes against one weight plane (kx = 2, kw_planes = 1: one launch);
 *   post = 1 together with a res_pre tensor (one residual array in registers); the popcount or int8 implementation
 *   selected through lsq_debug_xnor_impl.  The caller then runs lsq_pointwise_conv + lsq_xnor_conv2d: same bits.
 * A refused call launches nothing and writes nothing.
 */
int lsq_xnor_conv2d_proj(const uint64_t* xplanes, int kx, const float* xscales, const uint64_t* wbits,
                         const int32_t* wsum, int kw_planes, const float* wscales, const float* bias,
                         const lsq_conv_geom* g, int act, const float* act_slope, const float* res_pre,
                         const float* res_post, const lsq_proj* proj, float* y, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_CONV_PROJ_H_ */
