/*
 * lsq_hip_conv_xnor_gen_half.h -- C ABI of lsq_xnor_conv2d_gen_half (liblsq_hip_conv_xnor_gen_half.so): the general fp4
 * matrix-core XNOR convolution of lsq_hip_conv_xnor_gen.h for 16-bit networks.  The residual operands are read and the output
 * is written as bf16 / fp16, and every plane pass -- kw_planes * ceil(kx / 2) of them -- runs inside ONE launch with the fp32
 * running value in registers: no workspace, nothing written or read back between passes.  The kernel
 * (csrc/conv_xnor_gen_half/lsq_conv_xnor_gen_half.hip) keeps the arithmetic and the pass order of lsq_xnor_conv2d, so the
 * result is lsq_xnor_conv2d_half's bit for bit.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller, `stream` is a hipStream_t passed as void*
 * (NULL = default stream), every function returns 0, a negative LSQ_E_* code for an argument error (returned before any
 * launch, nothing written), or a positive hipError_t if the launch failed.
 *
 * The library links liblsq_hip.so for the plane layouts (lsq_act_plane_words, lsq_weight_plane_words): both must come from
 * the same build and sit in the same directory.
 */
#ifndef LSQ_HIP_CONV_XNOR_GEN_HALF_H_
#define LSQ_HIP_CONV_XNOR_GEN_HALF_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"
#include "lsq_hip_linear_half.h" /* LSQ_DTYPE_* */

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_CONV_XNOR_GEN_HALF_ABI_VERSION 1

int lsq_conv_xnor_gen_half_abi_version(void);

/*
 * Host only, no launch: 1 where lsq_xnor_conv2d_gen_half takes (g, kx, kw_planes, dtype), else 0.  It takes exactly what
 * lsq_xnor_conv2d_gen_supported takes --
 *   groups == 1;  C a multiple of 64;  O a multiple of 32;  KH, KW <= 8 with at most 64 taps;
 *   any stride, dilation and padding;  kx and kw_planes in 1..LSQ_MAX_PLANES;
 *   fewer than 2^30 outputs and fewer than 2^30 words in the kx activation planes (32-bit offsets);
 *   C * KH * KW < 2^23 (the fp32 accumulator holds the integer exactly)
 * -- with dtype LSQ_DTYPE_BF16 or LSQ_DTYPE_F16.  The kernel adds no limit of its own: its LDS (at most 54272 bytes per
 * workgroup) does not depend on the geometry.
 */
int lsq_xnor_conv2d_gen_half_supported(const lsq_conv_geom* g, int kx, int kw_planes, int dtype);

/*
 * y = act(conv + bias + res_pre) + res_post with the operands and layouts of lsq_xnor_conv2d_half, without its workspace:
 *   res_pre, res_post  [N][O][Ho][Wo] of `dtype` or NULL: widened to fp32 as they are read (exact);
 *   dtype              LSQ_DTYPE_BF16 or LSQ_DTYPE_F16: the type of y and of both residuals;
 *   y                  out, [N][O][Ho][Wo] of `dtype`: the fp32 result rounded ONCE, to nearest even, as Tensor.to(dtype)
 *                      rounds (fp16 overflow gives +-inf, results in the type's subnormal range stay subnormals); nothing
 *                      outside it is written.
 * y and the residuals are aligned to 2 bytes; nothing more is required of them.
 *
 * Contract: for every argument set it accepts, y is bit for bit what lsq_xnor_conv2d_half writes for the same arguments,
 *   lsq_xnor_conv2d(same operands, res_pre.float(), res_post.float()).to(dtype).
 *
 * LSQ_E_NULL: xplanes, xscales, wbits, wsum, wscales, y or g is NULL.  LSQ_E_SHAPE: what lsq_xnor_conv2d refuses as a shape.
 * LSQ_E_SCHEME: kx or kw_planes outside 1..LSQ_MAX_PLANES; an unknown act; a PReLU without act_slope.
 * LSQ_E_UNSUPPORTED: whatever lsq_xnor_conv2d_gen_half_supported answers 0 for otherwise (groups, other C or O, a kernel over
 *   8 x 8, the index limits, another dtype): the caller takes lsq_xnor_conv2d_half.
 * A refused call launches nothing and writes nothing.
 */
int lsq_xnor_conv2d_gen_half(const uint64_t* xplanes, int kx, const float* xscales, const uint64_t* wbits,
                             const int32_t* wsum, int kw_planes, const float* wscales, const float* bias,
                             const lsq_conv_geom* g, int act, const float* act_slope, const void* res_pre,
                             const void* res_post, int dtype, void* y, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_CONV_XNOR_GEN_HALF_H_ */
