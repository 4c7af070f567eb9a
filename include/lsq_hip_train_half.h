/*
 * lsq_hip_train_half.h -- C ABI of lsq_train_wgrad_half (liblsq_hip_train_half.so): the weight and bias gradient of a
 * binary-activation convolution from the activation sign planes and a 16-bit (bf16 / fp16) output gradient, the 16-bit
 * counterpart of lsq_train_wgrad (lsq_hip_train.h).  A library of its own: liblsq_hip_train.so is not touched.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller (the library allocates nothing), `stream` is a
 * hipStream_t passed as void* (NULL = default stream), every function returns 0, a negative LSQ_E_* code for an argument
 * error (returned before any launch, nothing written), or a positive hipError_t if a launch failed.  The library does not
 * link the objects of liblsq_hip.so; it shares lsq_conv_geom, the LSQ_E_* codes and the activation plane layout with it.
 */
#ifndef LSQ_HIP_TRAIN_HALF_H_
#define LSQ_HIP_TRAIN_HALF_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"
#include "lsq_hip_linear_half.h" /* LSQ_DTYPE_* */

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_TRAIN_HALF_ABI_VERSION 1

int lsq_train_half_abi_version(void);

/*
 * Bytes of the workspace of a call.  The reduction k = (n, ho, wo) is cut into S slices; S, like every slice boundary,
 * depends on the geometry alone.  S = 1: 0 (with or without the bias).  S > 1: S slabs of
 *   ceil(O / 64) * ceil(C / 64) * ceil(KH KW / TT) * 4 * TT * 1024 floats     (TT = 1 for a 1 x 1 kernel, else 9)
 * -- lsq_train_wgrad_workspace_bytes for the same S -- and with `with_bias` S * 64 ceil(O / 64) more floats, the bias
 * partials of the slices, behind them.  0 also for arguments the call refuses.  Host code: no device call.
 */
size_t lsq_train_wgrad_half_workspace_bytes(const lsq_conv_geom* g, int kx, int with_bias);

/*
 * grad_wq and grad_b of a convolution with binary activations:
 *   grad_wq[o][c][i][j] = sum_n sum_(ho,wo) grad_y[n][o][ho][wo] * x_q[n][c][ho*s + i - pad_h][wo*s + j - pad_w],
 *   x_q[n][c][h][w]     = sum_{p<kx} xscales[p][n] * (2 bit_p - 1), and 0 outside the image,
 *   grad_b[o]           = sum_n sum_(ho,wo) grad_y[n][o][ho][wo]
 * -- lsq_train_wgrad of lsq_hip_train.h with grad_y widened exactly to fp32, and the bias gradient from the same pass.
 *   xplanes      [kx] activation planes in the layout of lsq_hip.h (what the quantizer wrote for this step; the halo words
 *                are zero and contribute nothing, nor do the bits of channels >= C)
 *   xscales      [kx][N] fp32 plane scales
 *   grad_y       [N][O][Ho][Wo] of `dtype`, aligned to 2 bytes; nothing more is required of its address (a 16-byte-aligned
 *                run of 8 values is read with one load, any other element by element: the same bits either way)
 *   dtype        LSQ_DTYPE_BF16 or LSQ_DTYPE_F16
 *   grad_wq      out, [O][C][KH][KW] fp32, aligned to 4 bytes; nothing outside it is written
 *   grad_b       out, [O] fp32, aligned to 4 bytes, or NULL (then no bias gradient is computed and nothing is written for it)
 *   workspace    lsq_train_wgrad_half_workspace_bytes(g, kx, grad_b != NULL) bytes, 16-byte aligned, any content (NULL when
 *                that is 0): the partial sums of the K split, reduced in slice order
 * Geometry, as lsq_train_wgrad: groups 1, dilation 1, stride_h == stride_w in {1, 2}, pad <= kernel - 1, KH, KW <= 8,
 * 1 <= kx <= LSQ_MAX_PLANES, N * Ho * Wo < 2^31, O, C <= 65535; LSQ_E_UNSUPPORTED otherwise.
 *
 * Arithmetic.  Every sample's Ho Wo positions are padded to whole steps of 16 with zero operands, so a matrix instruction
 * never mixes two samples.  Per plane p and sample n the sums t = sum grad_y * (2 bit_p - 1) run on the matrix cores with
 * grad_y as it is (v_mfma_f32_32x32x16_bf16 / _f16: the products with +-1 are exact, fp32 accumulation), over at most 64
 * positions of the sample at a time; xscales[p][n] * t is then added to the fp32 result with one fused multiply-add.
 * Planes 2m, 2m + 1 whose scales are equal for a sample (ls-T) are one operand in {-2, 0, +2} for that sample, so that
 * x_q = 0 contributes an exact 0.  Per element the result is within a few fp32 roundings of sum |grad_y| |x_q|
 * (of sum |grad_y| for grad_b), and bitwise the same from call to call, on any stream and for any address of grad_y.
 *
 * Refusals, before any launch: everything lsq_train_wgrad refuses, with its codes (LSQ_E_NULL for a NULL geometry, xplanes,
 * xscales, grad_y or grad_wq; LSQ_E_SCHEME for kx; LSQ_E_SHAPE; LSQ_E_UNSUPPORTED); LSQ_E_UNSUPPORTED for another dtype,
 * for a grad_y not aligned to 2 bytes and for a grad_wq / grad_b not aligned to 4 bytes; LSQ_E_NULL for a NULL workspace
 * where one is needed; LSQ_E_WORKSPACE for one that is too small or not 16-byte aligned.
 */
int lsq_train_wgrad_half(const uint64_t* xplanes, int kx, const float* xscales, const void* grad_y, int dtype,
                         const lsq_conv_geom* g, float* grad_wq, float* grad_b, void* workspace, size_t workspace_bytes,
                         void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_TRAIN_HALF_H_ */
