/*
 * lsq_hip_conv_act_bn_half.h -- C ABI of the activation quantizer of QuantConv2d for bf16 / fp16 inputs with the eval batch
 * norm in front of it folded into the read (liblsq_hip_conv_act_bn_half.so), a library of its own beside
 * liblsq_hip_conv_act_half.so, whose kernels it shares at the source (csrc/conv_act_half/lsq_conv_act_half_core.h).
 *
 * Conventions are those of lsq_hip.h and lsq_hip_conv_act_half.h: device pointers owned by the caller (the library allocates
 * nothing and needs no workspace), `stream` is a hipStream_t passed as void* (NULL = default stream), every function returns
 * 0, a negative LSQ_E_* code for an argument error (returned before any launch, nothing written), or a positive hipError_t
 * if a launch failed.  The library links no object of another library of the project.
 */
#ifndef LSQ_HIP_CONV_ACT_BN_HALF_H_
#define LSQ_HIP_CONV_ACT_BN_HALF_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"
#include "lsq_hip_linear_half.h" /* LSQ_DTYPE_* */

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_CONV_ACT_BN_HALF_ABI_VERSION 1

int lsq_conv_act_bn_half_abi_version(void);

/*
 * The quantizer of lsq_hip_conv_act_half.h on the batch-normed input, without that input in memory: ONE launch reads x and
 * writes planes, scales and status.  Every argument that the quantizer of lsq_hip_conv_act_half.h has keeps its meaning (x,
 * x_dtype, g, scheme, k, skip, clamp_alpha, forced, planes, scales, status, stream); two are new:
 *
 *   pre_scale    [C] fp32, device: the folded batch norm's scale of every input channel
 *   pre_shift    [C] fp32, device: its shift
 *
 * CONTRACT.  Let
 *     t[n][c][h][w] = round_to_dtype( fl32( fl32( float(x[n][c][h][w]) * pre_scale[c] ) + pre_shift[c] ) )
 * -- two separately rounded fp32 operations (a multiplication, then an addition: never one fused multiply-add), fp32
 * denormals not flushed, then ONE rounding to nearest even into x_dtype exactly as Tensor.to(dtype) rounds: subnormals of
 * the type kept, fp16 overflow gives +-inf.  In torch: t = (x.float() * s.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)).to(dtype).
 * planes, scales and status are WORD FOR WORD what the quantizer of lsq_hip_conv_act_half.h writes for the materialised
 * tensor t -- every scheme, given or free-running scales, every skip, every geometry, any 2-byte-aligned x.
 *
 * Why the fold is exact.  t is rounded inside the read, so every value the quantizer sees is a value of the type: the
 * count table of one count per 15-bit magnitude key of the free-running LS2 / LST solve, the clamp bound's key and the
 * summation rule hold as they stand.  What that header states follows from the contract: halo words are never written,
 * every interior word is written in full, the SUMMATION RULE of the scales, and the independence of N, of the sample's
 * position in the batch and of the address of x.
 * The clamp applies to t: an fp16 overflow to +-inf under a clamp bound >= 0 is defined and clamps to +-a.  Without a clamp,
 * Inf and NaN stay outside the contract (as a product 0 * inf does with one); no bit pattern indexes outside the table.
 * t need not equal torch's batch_norm(x) bit for bit: both round one fp32 evaluation of the same affine map, associated
 * differently (the recorded deviation: DESIGN 4.30).  The caller that wants this contract's bits from torch composes t as
 * above.
 *
 * pre_scale and pre_shift both NULL: the call is the quantizer of lsq_hip_conv_act_half.h on x, bit for bit (no map is
 * applied).  Exactly one of them NULL: LSQ_E_NULL.  Every other refusal and code is that quantizer's: LSQ_E_NULL: x, g,
 * planes or scales is NULL.  LSQ_E_SHAPE: a non-positive dimension or skip, C not divisible by groups.  LSQ_E_SCHEME: an
 * unknown scheme, or a wrong k for the scheme.  LSQ_E_UNSUPPORTED: x_dtype other than BF16 / F16, M >= 2^31.
 */
int lsq_act_quant_bn_half(const void* x, int x_dtype, const lsq_conv_geom* g, int scheme, int k, int skip, float clamp_alpha,
                          const float* pre_scale, const float* pre_shift, const float* forced, uint64_t* planes,
                          float* scales, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_CONV_ACT_BN_HALF_H_ */
