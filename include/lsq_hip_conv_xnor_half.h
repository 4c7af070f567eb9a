/*
 * lsq_hip_conv_xnor_half.h -- C ABI of lsq_xnor_conv2d_half (liblsq_hip_conv_xnor_half.so): lsq_xnor_conv2d with a 16-bit
 * epilogue.  The residual operands are read and the output is written as bf16 / fp16; everything in between is the fp32
 * arithmetic of lsq_xnor_conv2d, rounded once at the store.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller, `stream` is a hipStream_t passed as void*
 * (NULL = default stream), every function returns 0, a negative LSQ_E_* code for an argument error (returned before any
 * launch, nothing written), or a positive hipError_t if a launch failed.
 *
 * The entry points are a library of their own because the function list of lsq_hip.h is fixed at ABI version 12; the
 * kernels are the XNOR kernels of liblsq_hip.so (csrc/lsq_xnor_mfma.hip and csrc/lsq_xnor_conv.hip, their 16-bit
 * instantiations), which this library links: both must come from the same build and sit in the same directory.  The test
 * hook lsq_debug_xnor_impl of lsq_hip_debug.h acts on this call too: 1 forces the popcount kernel, 2 (the int8 matrix-core
 * comparator, which has no 16-bit epilogue) takes the fp4 kernel here.
 */
#ifndef LSQ_HIP_CONV_XNOR_HALF_H_
#define LSQ_HIP_CONV_XNOR_HALF_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"
#include "lsq_hip_linear_half.h" /* LSQ_DTYPE_* */

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_CONV_XNOR_HALF_ABI_VERSION 1

int lsq_conv_xnor_half_abi_version(void);

/*
 * Bytes of the workspace a call with these plane counts needs: a call is kw_planes * ceil(kx / 2) launches; one launch
 * needs none (0), several keep their fp32 running sum [N][O][Ho][Wo] there (4 N O Ho Wo).  0 also for arguments the call
 * refuses.  Host code: no device call.
 */
size_t lsq_xnor_conv2d_half_workspace_bytes(const lsq_conv_geom* g, int kx, int kw_planes);

/*
 * y = act(conv + bias + res_pre) + res_post with the operands, the arithmetic and the kernels of lsq_xnor_conv2d, where
 *   res_pre, res_post  [N][O][Ho][Wo] of `dtype` or NULL: widened to fp32 as they are read (exact);
 *   dtype              LSQ_DTYPE_BF16 or LSQ_DTYPE_F16: the type of y and of both residuals;
 *   y                  out, [N][O][Ho][Wo] of `dtype`: the fp32 result rounded ONCE, to nearest even, as Tensor.to(dtype)
 *                      rounds (fp16 overflow gives +-inf, results in the type's subnormal range stay subnormals); nothing
 *                      outside it is written;
 *   workspace          lsq_xnor_conv2d_half_workspace_bytes(g, kx, kw_planes) bytes, 4-byte aligned, any content, rewritten
 *                      by the call; where that is 0 it may be NULL.  Every launch but the last is lsq_xnor_conv2d's fp32
 *                      kernel accumulating there; only the last reads the residuals and writes y.
 * y and the residuals are aligned to 2 bytes; nothing more is required of them.
 *
 * Contract: for every argument set lsq_xnor_conv2d accepts, y is bit for bit
 *   lsq_xnor_conv2d(same operands, res_pre.float(), res_post.float()).to(dtype).
 *
 * Refusals, before any launch (a refused call writes nothing): everything lsq_xnor_conv2d refuses, with the same codes;
 * LSQ_E_UNSUPPORTED for another dtype; LSQ_E_WORKSPACE for a workspace that is NULL, misaligned or too small where one is
 * needed.
 */
int lsq_xnor_conv2d_half(const uint64_t* xplanes, int kx, const float* xscales, const uint64_t* wbits,
                         const int32_t* wsum, int kw_planes, const float* wscales, const float* bias,
                         const lsq_conv_geom* g, int act, const float* act_slope, const void* res_pre,
                         const void* res_post, int dtype, void* y, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_CONV_XNOR_HALF_H_ */
