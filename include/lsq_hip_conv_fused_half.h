/*
 * lsq_hip_conv_fused_half.h -- C ABI of the 16-bit-activation (bf16 / fp16) x sign-weight convolution with the eval batch
 * norm in front of it folded into the read and the block epilogue (ReLU / PReLU, 16-bit residuals) in the launch
 * (liblsq_hip_conv_fused_half.so), a library of its own beside liblsq_hip_conv_half.so, whose kernels it shares at the
 * source (csrc/lsq_signw_conv_core.h).
 *
 * Conventions are those of lsq_hip.h and lsq_hip_conv_half.h: device pointers owned by the caller (the library allocates
 * nothing; the workspace is the caller's), `stream` is a hipStream_t passed as void* (NULL = default stream), every function
 * returns 0, a negative LSQ_E_* code for an argument error (returned before any launch, nothing written), or a positive
 * hipError_t if a launch failed.  The library links no object of another library of the project; its weight operand is what
 * lsq_pack_weight of liblsq_hip.so writes.
 */
#ifndef LSQ_HIP_CONV_FUSED_HALF_H_
#define LSQ_HIP_CONV_FUSED_HALF_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"
#include "lsq_hip_conv_half.h"   /* LSQ_CONV_HALF_* plan bits */
#include "lsq_hip_linear_half.h" /* LSQ_DTYPE_* */

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_CONV_FUSED_HALF_ABI_VERSION 1

int lsq_conv_fused_half_abi_version(void);

/*
 * Which kernel a call with geometry g takes: the LSQ_CONV_HALF_* bits of lsq_hip_conv_half.h, or a negative LSQ_E_* code.
 * Equal to lsq_signw_conv2d_half_plan on the same g, for every g: the folded batch norm is read per staged chunk and holds
 * no table in LDS, so it cannot move a geometry to another kernel (lsq_signw_conv2d's fp32 patch kernel leaves past 512 / 256 channels
 * a group with a fold; this one does not).  Each value names one kernel instantiation per element type.
 */
int lsq_signw_conv2d_fused_half_plan(const lsq_conv_geom* g);

/* What lsq_signw_conv2d_half_workspace_bytes returns: 4 N O Ho Wo for a 16-bit y_dtype and kw_planes >= 2, else 0. */
int64_t lsq_signw_conv2d_fused_half_workspace_bytes(const lsq_conv_geom* g, int kw_planes, int y_dtype);

/*
 * One residual-block half on a 16-bit tensor, one launch per weight plane, ONE rounding:
 *   y = act( conv(c(t), w_q) + bias + res_pre ) + res_post
 * Every argument lsq_signw_conv2d_half has keeps its meaning (x, x_dtype, clamp_alpha, wbits, kw_planes, wscales, bias, g,
 * y, y_dtype, workspace, workspace_bytes, stream); new are
 *   pre_scale    [C] fp32, device, or NULL: the folded batch norm's scale of every input channel (with groups: the global
 *                channel index)
 *   pre_shift    [C] fp32, device: its shift; both or neither
 *   act          LSQ_ACT_NONE / LSQ_ACT_RELU / LSQ_ACT_PRELU (act_slope[0]) / LSQ_ACT_PRELU_CHANNEL (act_slope[o])
 *   act_slope    fp32, device; NULL unless a PReLU
 *   res_pre      [N][O][Ho][Wo] of x_dtype, or NULL: added before the non-linearity
 *   res_post     the same, added after it
 *
 * CONTRACT.  Let
 *     t[n][c][h][w] = round_to_x_dtype( fl32( fl32( float(x[n][c][h][w]) * pre_scale[c] ) + pre_shift[c] ) )
 * -- two separately rounded fp32 operations, never one fused multiply-add, then one rounding to nearest even into x_dtype as
 * Tensor.to(dtype) rounds (fp16 overflow gives +-inf): the rule of lsq_act_quant_bn_half, lsq_hip_conv_act_bn_half.h; t = x
 * without a batch norm.  In torch: t = (x.float() * s.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)).to(dtype).  t is clamped in
 * its own type exactly as lsq_signw_conv2d_half clamps x (an fp16 overflow under a finite bound enters as +-bound).  The
 * padding is of t, not of x: an out-of-image position, a padded channel and a pixel past the end contribute exact zeros,
 * not pre_shift[c].
 * Let y32 be what lsq_signw_conv2d_half writes for t with y_dtype = LSQ_DTYPE_F32.  The result has the VALUES of
 *     v = y32 + float(res_pre);   v = act(v);   v = v + float(res_post)
 * evaluated in fp32 with a separate operation each (ReLU: max(v, 0); PReLU: v > 0 ? v : slope * v; an absent operand is no
 * operation), rounded ONCE, to nearest even, into y_dtype -- for every kw_planes: the planes before the last accumulate in
 * fp32 in the workspace (or in an fp32 y) exactly as in lsq_signw_conv2d_half, with the same fold in their read, and only
 * the last launch applies the epilogue.  Values, not bit patterns, as there: a -0 may come out as +0.  A NaN activation
 * under a finite bound stays outside the contract, as there.
 * With pre_scale = pre_shift = res_pre = res_post = NULL and LSQ_ACT_NONE the call is lsq_signw_conv2d_half bit for bit.
 * Alignment: x, res_pre, res_post and a 16-bit y are aligned to 2 bytes and no more (one element per load and store);
 * nothing outside y is written.  The summation order and the kernel are those lsq_hip_conv_half.h states for g.
 *
 * Refused before any launch, nothing written: everything lsq_signw_conv2d_half refuses, with its codes (LSQ_E_NULL,
 * LSQ_E_SHAPE, LSQ_E_UNSUPPORTED, LSQ_E_WORKSPACE); LSQ_E_NULL for exactly one of pre_scale / pre_shift, or a PReLU without
 * act_slope; LSQ_E_UNSUPPORTED for act outside 0 .. 3.
 */
int lsq_signw_conv2d_fused_half(const void* x, int x_dtype, float clamp_alpha, const float* pre_scale, const float* pre_shift,
                                const uint64_t* wbits, int kw_planes, const float* wscales, const float* bias,
                                const lsq_conv_geom* g, int act, const float* act_slope, const void* res_pre,
                                const void* res_post, void* y, int y_dtype, void* workspace, size_t workspace_bytes,
                                void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_CONV_FUSED_HALF_H_ */
