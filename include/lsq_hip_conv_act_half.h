/*
 * lsq_hip_conv_act_half.h -- C ABI of the activation quantizer of QuantConv2d for bf16 / fp16 inputs
 * (liblsq_hip_conv_act_half.so), a library of its own beside liblsq_hip.so and the liblsq_hip_linear*.so.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller (the library allocates nothing and needs no
 * workspace), `stream` is a hipStream_t passed as void* (NULL = default stream), every function returns 0, a negative
 * LSQ_E_* code for an argument error (returned before any launch, nothing written), or a positive hipError_t if a launch
 * failed.  The library does not link the objects of liblsq_hip.so; what it writes is what lsq_act_quant of that library
 * writes for the same geometry on the input converted to fp32.
 */
#ifndef LSQ_HIP_CONV_ACT_HALF_H_
#define LSQ_HIP_CONV_ACT_HALF_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"
#include "lsq_hip_linear_half.h" /* LSQ_DTYPE_* */

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_CONV_ACT_HALF_ABI_VERSION 1

int lsq_conv_act_half_abi_version(void);

/*
 * Clamp -> per-sample scales -> packed sign planes of a 16-bit NCHW batch: lsq_act_quant for bf16 / fp16 inputs, every
 * scheme, in ONE launch.  The planes are the activation operand of lsq_xnor_conv2d.
 *
 *   x            [N][C][H][W] of x_dtype (LSQ_DTYPE_BF16 or LSQ_DTYPE_F16), contiguous, any 2-byte-aligned address (16-,
 *                8- and 4-byte loads only where the address and H W allow; the same bits either way)
 *   g            the convolution's geometry, checked as lsq_act_quant checks it; N, C, H, W, pad_h, pad_w and groups are used
 *   scheme, k    LS1: k = 1;  LS2, LST: k = 2;  GF: k = 1 .. LSQ_MAX_PLANES
 *   skip         free-running LS2 / LST: the solve reads the sub-sample row[::skip] of the flattened sample, n = ceil(M / skip)
 *   clamp_alpha  the symmetric clamp bound a, USED AS GIVEN: the caller rounds it into x_dtype first (as Tensor.clamp does),
 *                so that every clamped value is a value of the type; a negative value means no clamp
 *   forced       NULL, or [k][N] fp32 scales to use instead of computing them (copied to `scales` bit for bit)
 *   planes       out, k activation planes [p][N][Gt][Hp][Wp] in the layout of lsq_hip.h; groups are honoured, bits of
 *                channels past C / groups are 0.  EVERY interior word is written in full; halo words are never written
 *                (the caller zero-fills the buffer once, exactly as for lsq_act_quant)
 *   scales       out, [k][N] fp32 (LST: row 1 repeats v1)
 *   status       out, [N] int32 or NULL: free-running LS2 / LST: 1 where the row had a candidate (the ternary extra candidate
 *                counts), 0 where it had none or where the whole sub-sample is +-0 (then v1 = 0); every other call writes 1
 * There is no pre_scale / pre_shift here: a batch norm on a 16-bit tensor rounds its output into the type.  The fold that
 * applies that rounding inside the read is lsq_hip_conv_act_bn_half.h's, a library of its own.
 *
 * Values.  A row is a sample, flattened NCHW, M = C H W elements.  Every element is converted to fp32 exactly (subnormals
 * kept) and clamped to +-a, then runs the chain of lsq_act_quant operation for operation: result_0 = 0, res_0 = c,
 * bit_q = (c - result_q) >= 0, result_{q+1} = result_q +- v_q, res_{q+1} = res_q -+ v_q.  With the same scales the planes
 * are lsq_act_quant's on the input converted to fp32, word for word.
 * Free-running LS1 / GF: v_q = fl32(S_q / M), S_q = the sum of |res_q| over the sample by this SUMMATION RULE: fp32 inside a
 * group of at most 8 elements (8 consecutive channels of one pixel), fp64 across groups, in an order that (C, H, W, groups)
 * alone fix -- not N, the sample's position in the batch, the address of x or the call.  Hence |v_q - mean| <= 2^-21 mean
 * against the exact mean of the fp32 magnitudes (7 roundings of 2^-24 and the final one), and the same bits on every call.
 * Free-running LS2 / LST: v1 is the optimal first scale of quant/binary/optimal.py on the sub-sample, solved on a table of
 * one count per 15-bit magnitude key in LDS with the arithmetic of csrc/lsq_solver_math.h: the same bits as lsq_act_quant on
 * the input converted to fp32 and as lsq_linear_act_quant_solve_half on the view [N][M].  v2 = fl32(S_1 / M) by the rule
 * above for LS2, v1 for LST.  Inf and NaN are outside the contract (as for lsq_act_quant); no bit pattern indexes outside
 * the table.
 * Work distribution: one workgroup of 1024 threads owns a sample from its first load to its last plane word (a grid of N
 * workgroups).  No workspace, integer atomics in LDS only, no sample shared between workgroups: a single very long row
 * runs on one compute unit.
 *
 * LSQ_E_NULL: x, g, planes or scales is NULL.  LSQ_E_SHAPE: a non-positive dimension or skip, C not divisible by groups.
 * LSQ_E_SCHEME: an unknown scheme, or a wrong k for the scheme.  LSQ_E_UNSUPPORTED: x_dtype other than BF16 / F16,
 * M >= 2^31.
 */
int lsq_act_quant_half(const void* x, int x_dtype, const lsq_conv_geom* g, int scheme, int k, int skip, float clamp_alpha,
                       const float* forced, uint64_t* planes, float* scales, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_CONV_ACT_HALF_H_ */
