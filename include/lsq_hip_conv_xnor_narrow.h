/*
 * lsq_hip_conv_xnor_narrow.h -- C ABI of lsq_xnor_conv2d_narrow (liblsq_hip_conv_xnor_narrow.so): lsq_xnor_conv2d on the fp4
 * matrix cores for ANY channel count -- input channels that are no multiple of 64 and out-channels that are no multiple of 32,
 * which lsq_xnor_conv2d and lsq_xnor_conv2d_gen leave to the popcount kernel -- with an optional 2 x 2 / stride-2 max-pool
 * behind the activation.  The kernel (csrc/conv_xnor_narrow/lsq_conv_xnor_narrow.hip) is an implicit GEMM whose K loop runs
 * over 32-channel dwords with every weight fragment of a workgroup resident in LDS and every plane pass inside one launch; its
 * integers are exact and its epilogue is lsq_xnor_conv2d's, so the result is lsq_xnor_conv2d's bit for bit (followed, with
 * pool 2, by the maximum over each window).
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller, `stream` is a hipStream_t passed as void*
 * (NULL = default stream), every function returns 0, a negative LSQ_E_* code for an argument error (returned before any
 * launch, nothing written), or a positive hipError_t if a launch failed.
 *
 * The library links liblsq_hip.so for the plane layouts (lsq_act_plane_words, lsq_weight_plane_words): both must come from
 * the same build and sit in the same directory.
 */
#ifndef LSQ_HIP_CONV_XNOR_NARROW_H_
#define LSQ_HIP_CONV_XNOR_NARROW_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_CONV_XNOR_NARROW_ABI_VERSION 1

int lsq_conv_xnor_narrow_abi_version(void);

/*
 * Host only, no launch: 1 where lsq_xnor_conv2d_narrow takes (g, kx, kw_planes, pool), else 0.  It takes
 *   groups == 1;  any C >= 1 and any O >= 1;  KH, KW <= 8;  any stride, dilation and padding;
 *   KH * KW * ceil(C / 32) <= 128 (the weight fragments of a workgroup stay in LDS);
 *   kx and kw_planes in 1..LSQ_MAX_PLANES;  pool 1 (none) or 2 (then an output of at least 2 x 2);
 *   fewer than 2^30 outputs and fewer than 2^30 words in the kx activation planes (32-bit offsets);
 *   C * KH * KW < 2^23 (the fp32 accumulator holds the integer exactly).
 */
int lsq_xnor_conv2d_narrow_supported(const lsq_conv_geom* g, int kx, int kw_planes, int pool);

/*
 * The arguments of lsq_xnor_conv2d, the same operands in the same layouts, and `pool`:
 *   pool 1:  y = act(conv + bias + res_pre) + res_post,  y is [N][O][Ho][Wo];
 *   pool 2:  y = max over 2 x 2 windows, stride 2, of act(conv + bias),  y is [N][O][Ho / 2][Wo / 2] -- floor mode: an odd last
 *            row or column is dropped, as F.max_pool2d(., 2, 2) drops it.  res_pre and res_post must be NULL.
 *
 * LSQ_E_NULL: xplanes, xscales, wbits, wsum, wscales, y or g is NULL.  LSQ_E_SHAPE: what lsq_xnor_conv2d refuses as a shape; an
 * output under 2 x 2 with pool 2.  LSQ_E_SCHEME: kx or kw_planes outside 1..LSQ_MAX_PLANES; an unknown act; a PReLU without
 * act_slope.
 * LSQ_E_UNSUPPORTED: whatever lsq_xnor_conv2d_narrow_supported answers 0 for otherwise (groups, a kernel over 8 x 8, the
 *   fragment budget, another pool, the index limits), and a residual beside pool 2: the caller takes lsq_xnor_conv2d.
 * A refused call launches nothing and writes nothing.
 */
int lsq_xnor_conv2d_narrow(const uint64_t* xplanes, int kx, const float* xscales, const uint64_t* wbits,
                           const int32_t* wsum, int kw_planes, const float* wscales, const float* bias,
                           const lsq_conv_geom* g, int act, const float* act_slope, const float* res_pre,
                           const float* res_post, int pool, float* y, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_CONV_XNOR_NARROW_H_ */
