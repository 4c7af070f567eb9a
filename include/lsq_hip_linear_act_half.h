/*
 * lsq_hip_linear_act_half.h -- C ABI of the activation quantizer for bf16 / fp16 rows (liblsq_hip_linear_act_half.so), a
 * library of its own beside liblsq_hip.so and the liblsq_hip_linear*.so.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller (the library allocates nothing and needs no
 * workspace), `stream` is a hipStream_t passed as void* (NULL = default stream), every function returns 0, a negative
 * LSQ_E_* code for an argument error (returned before any launch, nothing written), or a positive hipError_t if a launch
 * failed.  The library does not link the objects of liblsq_hip.so; what it writes is what lsq_act_quant of that library
 * writes for the geometry (N, C = L, 1, 1) -- the activation operand of lsq_linear_xnor.
 */
#ifndef LSQ_HIP_LINEAR_ACT_HALF_H_
#define LSQ_HIP_LINEAR_ACT_HALF_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"
#include "lsq_hip_linear_half.h" /* LSQ_DTYPE_* */

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_LINEAR_ACT_HALF_ABI_VERSION 1

int lsq_linear_act_half_abi_version(void);

/*
 * Sign planes and per-sample scales of N rows of L 16-bit activations, for the schemes that need no scale SOLVE:
 *   LSQ_SCHEME_LS1 (k = 1) and LSQ_SCHEME_GF (k = 1 .. LSQ_MAX_PLANES), with or without `forced`;
 *   LSQ_SCHEME_LS2 / LSQ_SCHEME_LST (k = 2) only WITH `forced` (moving-average inference).
 *
 *   x            [N][L] of x_dtype (LSQ_DTYPE_BF16 or LSQ_DTYPE_F16), rows contiguous, any 2-byte-aligned address, any L
 *                (16-byte loads only where x is 16-byte aligned and L % 8 == 0, so that every row starts on 16 bytes; the
 *                planes and the scales are the same bits either way)
 *   clamp_alpha  the symmetric clamp bound a, USED AS GIVEN: the caller rounds it into x_dtype first (Tensor.clamp rounds
 *                its bound into the tensor's type: bf16(1.3) = 1.296875), so that every clamped value is a value of the
 *                type; a negative value means no clamp
 *   forced       NULL, or [k][N] fp32 scales to use instead of computing them (copied to `scales`)
 *   planes       out, [k][N][ceil(L / 64)] words: bit i of word w of a row is element 64 w + i, bits past L are 0.  EVERY
 *                word is written in full (the buffer needs no zero-filling), nothing outside it is written
 *   scales       out, [k][N] fp32
 *
 * Values.  Every element is converted to fp32 exactly (subnormals included: nothing is flushed), clamped to +-a, and put
 * through the chain of lsq_act_quant (chain_eval of csrc/lsq_act_quant.hip), operation for operation in fp32:
 *   result_0 = 0, res_0 = c;   bit_q = (c - result_q) >= 0;   result_(q+1) = result_q +- v_q (+ where bit_q);
 *   res_(q+1) = res_q -+ v_q (- where res_q >= 0)
 * so -0.0 has bit 1 and a negative subnormal bit 0: with the same scales the planes are lsq_act_quant's on x converted to
 * fp32, bit for bit.
 * Scales without `forced`: v_q = fl32(S_q / L), S_q = the sum over the row of |res_q|.  The fp32 magnitudes of 8 consecutive
 * elements (8 g .. 8 g + 7) are added in fp32, in element order; these group sums are added in fp64, in an order that L
 * alone fixes: a row's scale is the same bits whatever N, whichever row of the batch it is, wherever x lies, on every call.
 * |v_q - mean| <= 2^-21 mean against the exact mean of the fp32 magnitudes (7 roundings of 2^-24 in a group sum, one in the
 * final conversion; the fp64 additions are far below that).
 * Work distribution: rows of up to 4096 elements take one wave each (four rows a workgroup), longer rows one workgroup of
 * 256 threads each.  gf-k without `forced` makes k passes over the row (plane q needs v_0 .. v_(q-1)): the row is kept in
 * LDS between them where it fits (up to 16384 elements) and read again (from L2) where it does not.  No workspace, no
 * atomics, no row shared between workgroups: a single very long row runs on one compute unit.
 *
 * LSQ_E_NULL: x, planes or scales is NULL.  LSQ_E_SHAPE: N or L is not positive.  LSQ_E_SCHEME: unknown scheme, k outside
 * 1 .. LSQ_MAX_PLANES, LS1 with k != 1, LS2 / LST with k != 2.  LSQ_E_UNSUPPORTED: x_dtype other than BF16 / F16, L >= 2^31,
 * N >= 2^31, LS2 / LST without `forced`.
 */
int lsq_linear_act_quant_half(const void* x, int x_dtype, int64_t N, int64_t L, int scheme, int k, float clamp_alpha,
                              const float* forced, uint64_t* planes, float* scales, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_LINEAR_ACT_HALF_H_ */
