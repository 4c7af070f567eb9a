/*
 * lsq_hip_conv_train_half.h -- C ABI of the 16-bit (bf16 / fp16) train-step kernels of the convolution layer
 * (liblsq_hip_conv_train_half.so), a library of its own beside liblsq_hip.so and the other liblsq_hip_*.so.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller (the library allocates nothing; the workspace
 * is the caller's), `stream` is a hipStream_t passed as void* (NULL = default stream), every function returns 0, a
 * negative LSQ_E_* code for an argument error (returned before any launch, nothing written), or a positive hipError_t if
 * a launch failed.  The library links the objects of no other library; its kernels are the ones of
 * liblsq_hip_conv_train.so, instantiated from the same source on a 16-bit gradient and an epilogue.
 */
#ifndef LSQ_HIP_CONV_TRAIN_HALF_H_
#define LSQ_HIP_CONV_TRAIN_HALF_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"
#include "lsq_hip_conv_train.h"  /* lsq_conv_dgrad_plan, LSQ_CONV_DGRAD_* */
#include "lsq_hip_linear_half.h" /* LSQ_DTYPE_* */

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_CONV_TRAIN_HALF_ABI_VERSION 1

int lsq_conv_train_half_abi_version(void);

/* The plan and the workspace size of lsq_signw_conv2d_dgrad_half: for every geometry (and plane count) what
 * lsq_signw_conv2d_dgrad_plan and lsq_signw_conv2d_dgrad_workspace_bytes of lsq_hip_conv_train.h return -- the same
 * kernels, tiles and transposed plane image.  Host code only: no device call. */
int lsq_signw_conv2d_dgrad_half_plan(const lsq_conv_geom* g, lsq_conv_dgrad_plan* plan);

size_t lsq_signw_conv2d_dgrad_half_workspace_bytes(const lsq_conv_geom* g, int kw_planes);

/*
 * Input gradient of the convolution's 16-bit train step in ONE pass: 16-bit output gradients x sign-weight planes (the sum
 * over the output channels and the taps, lsq_signw_conv2d_dgrad of lsq_hip_conv_train.h), then the straight-through
 * estimator of the activation quantizer against the step's 16-bit input, then one rounding into the type.
 *   grad_y       [N][O][Ho][Wo] of gy_dtype (LSQ_DTYPE_BF16 or LSQ_DTYPE_F16), contiguous, any 2-byte-aligned address
 *   wbits, kw_planes, wscales, g, workspace, workspace_bytes
 *                as in lsq_signw_conv2d_dgrad: the forward's own planes and fp32 scales [kw_planes][O], the FORWARD
 *                geometry, a workspace of at least lsq_signw_conv2d_dgrad_half_workspace_bytes(g, kw_planes) bytes, 8-byte
 *                aligned, rewritten by every call
 *   x            NULL (no epilogue: the convolution's gradient alone), or [N][C][H][W] of gy_dtype, contiguous, any
 *                2-byte-aligned address: the step's input
 *   kx, xscales  with x: the activation quantizer's planes and their per-sample scales [kx][N] fp32; kx = 0 (xscales may be
 *                NULL) = fp activations, the clamp alone.  Ignored without x (kx is still checked)
 *   clamp_alpha  with x: the symmetric clamp bound ALREADY ROUNDED into the type by the caller (as Tensor.clamp rounds it);
 *                negative = identity
 *   grad_x       out, [N][C][H][W] of gx_dtype: LSQ_DTYPE_F32 (4-byte aligned) or gy_dtype (2-byte aligned).  EVERY element
 *                is written and nothing outside it; an element store is one 2-byte (4-byte for F32) store, never a wider
 *                read-modify-write, so the bytes in front of and behind a view are left alone
 * Arithmetic.  Each 16-bit gradient is converted exactly to fp32.  From there the computation is lsq_signw_conv2d_dgrad's,
 * operation for operation: a = fl32(gy * ws[q][o]), the same hi + lo bf16 split, the same plan and tiles, the same order of
 * summation into one fp32 accumulator acc.  With x, in fp32,
 *   r_0 = 0, d_i = clamp(float(x)) - r_i, r_{i+1} = r_i + v_i[n] sign(d_i)   (sign(+-0) = +1), then with G_kx = acc:
 *   t_i = G_{i+1} v_i[n] [|d_i| <= 1],  G_i = G_{i+1} - t_i,  result = [|x| <= alpha] sum_i t_i     (kx = 0: [|x| <= alpha] acc)
 * -- lsq_ste_backward of lsq_hip.h on float(x), without contraction.  The result is stored as fp32, or rounded once to
 * nearest even into the type.  Bit for bit, therefore:
 *   (A) x = NULL, gx_dtype = F32:       lsq_signw_conv2d_dgrad(float(grad_y))
 *   (B) x = NULL, gx_dtype = gy_dtype:  (A) rounded into the type
 *   (C) x given:                        lsq_ste_backward(float(x), (A), kx, xscales, clamp_alpha), rounded into gx_dtype
 * Every geometry takes the instantiation its plan names (none is routed elsewhere); accuracy, summation order and
 * determinism are those stated in lsq_hip_conv_train.h.
 * LSQ_E_NULL: grad_y, wbits, wscales, g or grad_x is NULL; x given with kx > 0 and xscales NULL.  LSQ_E_SHAPE,
 * LSQ_E_WORKSPACE: as lsq_signw_conv2d_dgrad.  LSQ_E_UNSUPPORTED: what lsq_signw_conv2d_dgrad refuses; gy_dtype other than
 * BF16 / F16; gx_dtype neither F32 nor gy_dtype; kx outside 0 .. LSQ_MAX_PLANES; N > 65535 with x given (the limit of
 * lsq_ste_backward); grad_y, x or grad_x not aligned to its element.
 */
int lsq_signw_conv2d_dgrad_half(const void* grad_y, int gy_dtype, const uint64_t* wbits, int kw_planes, const float* wscales,
                                const lsq_conv_geom* g, const void* x, int kx, const float* xscales, float clamp_alpha,
                                void* grad_x, int gx_dtype, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_CONV_TRAIN_HALF_H_ */
