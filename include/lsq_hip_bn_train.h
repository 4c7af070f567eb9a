/*
 * lsq_hip_bn_train.h -- C ABI of the train-mode batch norm in front of a quantized convolution (liblsq_hip_bn_train.so), a
 * library of its own beside liblsq_hip.so.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller (the library allocates nothing), `stream` is a
 * hipStream_t passed as void* (NULL = default stream), every function returns 0, a negative LSQ_E_* code for an argument
 * error (returned before any launch), or a positive hipError_t if a launch failed.  The library does not link the objects
 * of liblsq_hip.so; it shares the LSQ_E_* codes and LSQ_MAX_PLANES with it.
 *
 * Every tensor is fp32, dense NCHW: x [N][C][H][W], per-channel vectors [C], plane scales [k][N].  Operand rules, in this
 * order, for every entry point: a required pointer that is NULL: LSQ_E_NULL; N, C, H or W < 1 or H * W >= 2^31:
 * LSQ_E_SHAPE; k outside 0..LSQ_MAX_PLANES: LSQ_E_SCHEME; N or C > 65535, or a pointer that is not 4-byte aligned:
 * LSQ_E_UNSUPPORTED; a workspace that is NULL, too small or not 16-byte aligned: LSQ_E_WORKSPACE.  A refused call writes
 * nothing.  16-byte accesses are used where H * W % 4 == 0 and the call's tensors of x's shape are 16-byte aligned, 4-byte
 * accesses otherwise: the results are the same bits either way.
 *
 * With m = N * H * W values per channel and u = 2^-53:
 *
 *   y      = fmaf(x, scale[c], shift[c])               one rounding: the expression of lsq_act_quant's pre_scale / pre_shift
 *   x^     = (x - mean[c]) * invstd[c]
 *   g      = the straight-through gradient of lsq_ste_backward at the input y for the output gradient grad_q
 *   grad_x = scale[c] * (g - sum(g) / m - x^ * sum(g x^) / m)          (sums over the channel)
 */
#ifndef LSQ_HIP_BN_TRAIN_H_
#define LSQ_HIP_BN_TRAIN_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_BN_TRAIN_ABI_VERSION 1

int lsq_bn_train_abi_version(void);

/*
 * Batch statistics of x and the affine map they give, as nn.BatchNorm2d computes them in train mode; x is read once.
 *   gamma, beta      [C] or NULL (1 / 0)
 *   momentum         >= 0: running = (1 - momentum) running + momentum batch;  < 0: the cumulative average,
 *                    running += (batch - running) / batch_count, with the caller's batch_count >= 1 (this batch included)
 *   running_mean/var [C] updated in place, or both NULL; the variance that enters is the unbiased one, var m / (m - 1)
 *   mean, var        out [C]: batch mean and biased variance
 *   invstd           out [C]: 1 / sqrt(var + eps)
 *   scale, shift     out [C]: gamma invstd and beta - mean scale
 *   workspace        lsq_bn_train_workspace_bytes(N, C, H, W) bytes, 16-byte aligned, any content
 * m < 2: LSQ_E_SHAPE (torch raises there).
 *
 * Two launches.  The first has one workgroup per (channel, slab of samples): every lane adds x and x * x (exact in fp64)
 * into fp64 accumulators, the wave and then the workgroup reduce them in a fixed order and one fp64 pair per (channel, slab)
 * goes to the workspace.  The second adds a channel's slabs in slab order and writes every output.  No atomics and no
 * hand-off inside a launch: for a given shape the bits do not depend on which workgroup runs first, nor on the run.
 *
 * Accuracy.  S = sum x and Q = sum x^2 are sums of m exact fp64 terms, each through at most m - 1 additions, so
 * |S^ - S| <= (m - 1) u sum|x| and |Q^ - Q| <= (m - 1) u Q to first order.  mean = fl32(S^ / m) adds the division's u |mean|
 * <= u mean|x| and the conversion's 2^-24 |mean|:
 *     |mean - mean*| <= 2^-24 |mean*| + m u mean|x|.
 * The variance is fma(-S^, S^ / m, Q^) / m, clamped at 0: the fused step rounds Q^ - S^ (S^ / m) once, so beside the
 * summation term (m - 1) u mean(x^2) of Q^ there remain the terms of S^ (twice its relative error, times mean^2 <= mean(x^2))
 * and three single roundings.  The additions a value really passes through are the d = ceil(values per lane) + 6 + 4 + slabs
 * of its lane, its wave, its workgroup and its channel, far fewer than m - 1 for all but the smallest m, which is why
 *     |var - var*| <= 2^-24 var* + m u mean(x^2)
 * is the figure the tests hold the kernel to; the guaranteed first-order worst case is that with 3 min(d, m - 1) + 3 for m.
 * invstd, scale and shift are the fp64 formulas evaluated on the fp32 mean and var that were written, rounded once: within
 * one fp32 ulp of them.  The running statistics are the fp64 update evaluated on the fp64 batch values, rounded once.
 */
size_t lsq_bn_train_workspace_bytes(int N, int C, int H, int W);
int lsq_bn_train_stats(const float* x, int N, int C, int H, int W, const float* gamma, const float* beta, float eps,
                       float momentum, int64_t batch_count, float* running_mean, float* running_var, float* mean, float* var,
                       float* invstd, float* scale, float* shift, void* workspace, size_t workspace_bytes, void* stream);

/*
 * y = fmaf(x, scale[c], shift[c]): what the quantizers see behind their pre_scale / pre_shift, materialised -- the operand
 * of a consumer that is not one of the kernels.  y may be x.
 */
int lsq_bn_apply(const float* x, int N, int C, int H, int W, const float* scale, const float* shift, float* y, void* stream);

/*
 * lsq_quant_values of the rows fmaf(x, scale[c], shift[c]) without writing them: x_q = sum_i v_i b_i of the quantizer chain
 * under the clamp [-clamp_alpha, clamp_alpha] (negative: none), rows = samples, xscales [k][N] (k = 0: the clamp alone, xscales
 * may be NULL).  Bit for bit lsq_quant_values(lsq_bn_apply(x)).
 */
int lsq_quant_values_bn(const float* x, int N, int C, int H, int W, const float* scale, const float* shift, int k,
                        const float* xscales, float clamp_alpha, float* x_q, void* stream);

/*
 * Backward of quantizer(bn(x)) for the gradient grad_q with respect to the quantizer's value: g as lsq_ste_backward gives it
 * at fmaf(x, scale, shift) (the same bits; never stored), then the batch norm's backward.
 *   grad_x      out [N][C][H][W]
 *   grad_gamma  out [C]: sum g x^        grad_beta  out [C]: sum g
 *   workspace   lsq_bn_ste_backward_workspace_bytes(N, C, H, W) bytes, 16-byte aligned, any content
 * x and grad_q are read twice and grad_x written once.  Launch one, one workgroup per (channel, slab of samples): g and
 * g * x^ (x^ in fp64 from the fp32 mean and invstd) into fp64 accumulators, reduced as in lsq_bn_train_stats; a launch of C
 * threads adds the slabs in slab order, writes grad_beta and grad_gamma (one rounding each) and the fp32 coefficients
 * a = fl32(grad_beta / m), b = fl32(grad_gamma / m); launch two recomputes g and writes, in fp32 and this order,
 *     x^ = (x - mean) * invstd;   grad_x = scale * ((g - a) - x^ * b).
 * Accuracy.  grad_beta and grad_gamma: as the mean above, |error| <= 2^-24 |sum| + m u mean|g| (mean|g x^|; the three
 * roundings of g x^ in fp64 are below the summation term for m > 4).  grad_x against the same expression in fp64 on
 * the written grad_beta and grad_gamma: eight fp32 roundings (a, b, x - mean, * invstd, x^ * b, g - a, the difference, * scale),
 * each at most 2^-24 of |scale| (|g| + |a| + |x^| |b|) to first order:
 *     |grad_x - grad_x*| <= 9 * 2^-24 |scale| (|g| + |grad_beta| / m + |x^| |grad_gamma| / m),
 * the ninth for the second-order terms.  Where g, grad_beta and x^ grad_gamma are all 0, grad_x is exactly 0.
 */
size_t lsq_bn_ste_backward_workspace_bytes(int N, int C, int H, int W);
int lsq_bn_ste_backward(const float* x, const float* grad_q, int N, int C, int H, int W, const float* scale, const float* shift,
                        const float* mean, const float* invstd, int k, const float* xscales, float clamp_alpha, float* grad_x,
                        float* grad_gamma, float* grad_beta, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_BN_TRAIN_H_ */
