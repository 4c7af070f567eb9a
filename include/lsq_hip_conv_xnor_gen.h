/*
 * lsq_hip_conv_xnor_gen.h -- C ABI of lsq_xnor_conv2d_gen (liblsq_hip_conv_xnor_gen.so): lsq_xnor_conv2d on the fp4 matrix
 * cores for the geometries its tuned matrix-core kernel does not take -- 1x1, 5x5, 7x7 and asymmetric kernels, dilation, any
 * stride and padding, any multiple of 64 input channels.  The kernel (csrc/conv_xnor_gen/lsq_conv_xnor_gen.hip) is an
 * implicit GEMM with a run-time K loop over (tap, channel word) steps whose weight fragments are streamed through LDS; its
 * integers are exact and its epilogue is lsq_xnor_conv2d's, so the result is lsq_xnor_conv2d's bit for bit.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller, `stream` is a hipStream_t passed as void*
 * (NULL = default stream), every function returns 0, a negative LSQ_E_* code for an argument error (returned before any
 * launch, nothing written), or a positive hipError_t if a launch failed.
 *
 * The library links liblsq_hip.so for the plane layouts (lsq_act_plane_words, lsq_weight_plane_words): both must come from
 * the same build and sit in the same directory.
 */
#ifndef LSQ_HIP_CONV_XNOR_GEN_H_
#define LSQ_HIP_CONV_XNOR_GEN_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_CONV_XNOR_GEN_ABI_VERSION 1

int lsq_conv_xnor_gen_abi_version(void);

/*
 * Host only, no launch: 1 where lsq_xnor_conv2d_gen takes (g, kx, kw_planes), else 0.  It takes
 *   groups == 1;  C a multiple of 64;  O a multiple of 32;  KH, KW <= 8 with at most 64 taps;
 *   any stride, dilation and padding;  kx and kw_planes in 1..LSQ_MAX_PLANES;
 *   fewer than 2^30 outputs and fewer than 2^30 words in the kx activation planes (32-bit offsets);
 *   C * KH * KW < 2^23 (the fp32 accumulator holds the integer exactly).
 */
int lsq_xnor_conv2d_gen_supported(const lsq_conv_geom* g, int kx, int kw_planes);

/*
 * The arguments of lsq_xnor_conv2d, the same operands in the same layouts, the same result:
 *   y = act(conv + bias + res_pre) + res_post.
 *
 * LSQ_E_NULL: xplanes, xscales, wbits, wsum, wscales, y or g is NULL.  LSQ_E_SHAPE: what lsq_xnor_conv2d refuses as a shape.
 * LSQ_E_SCHEME: kx or kw_planes outside 1..LSQ_MAX_PLANES; an unknown act; a PReLU without act_slope.
 * LSQ_E_UNSUPPORTED: whatever lsq_xnor_conv2d_gen_supported answers 0 for otherwise (groups, other C or O, a kernel over
 *   8 x 8, the index limits): the caller takes lsq_xnor_conv2d.
 * A refused call launches nothing and writes nothing.
 */
int lsq_xnor_conv2d_gen(const uint64_t* xplanes, int kx, const float* xscales, const uint64_t* wbits,
                        const int32_t* wsum, int kw_planes, const float* wscales, const float* bias,
                        const lsq_conv_geom* g, int act, const float* act_slope, const float* res_pre,
                        const float* res_post, float* y, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_CONV_XNOR_GEN_H_ */
