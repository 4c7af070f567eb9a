/*
 * lsq_hip_linear_act_solve.h -- C ABI of the free-running ls-2 / ls-T activation quantizer for bf16 / fp16 rows
 * (liblsq_hip_linear_act_solve.so), a library of its own beside liblsq_hip.so and the liblsq_hip_linear*.so.
 *
 * Conventions are those of lsq_hip_linear_act_half.h: device pointers owned by the caller (the library allocates nothing
 * and needs no workspace), `stream` is a hipStream_t passed as void* (NULL = default stream), every function returns 0, a
 * negative LSQ_E_* code for an argument error (returned before any launch, nothing written), or a positive hipError_t if a
 * launch failed.  The library does not link the objects of liblsq_hip.so; what it writes is what lsq_act_quant of that
 * library writes, free-running, for the geometry (N, C = L, 1, 1) on the rows converted to fp32.
 */
#ifndef LSQ_HIP_LINEAR_ACT_SOLVE_H_
#define LSQ_HIP_LINEAR_ACT_SOLVE_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"
#include "lsq_hip_linear_half.h" /* LSQ_DTYPE_* */

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_LINEAR_ACT_SOLVE_ABI_VERSION 1

int lsq_linear_act_solve_abi_version(void);

/*
 * The optimal first scale v1 (quant/binary/optimal.py), the second scale and both sign planes of N rows of L 16-bit
 * activations, for LSQ_SCHEME_LS2 and LSQ_SCHEME_LST without given scales, in ONE launch.
 *
 *   x            [N][L] of x_dtype (LSQ_DTYPE_BF16 or LSQ_DTYPE_F16), rows contiguous, any 2-byte-aligned address, any L >= 1
 *                (16-byte loads only where x is 16-byte aligned and L % 8 == 0; the same bits either way)
 *   skip         the solve reads the sub-sample row[::skip], n = ceil(L / skip) keys
 *   clamp_alpha  the symmetric clamp bound a, USED AS GIVEN: the caller rounds it into x_dtype first (as Tensor.clamp does),
 *                so that every clamped value is a value of the type; a negative value means no clamp
 *   planes       out, [2][N][ceil(L / 64)] words: bit i of word w of a row is element 64 w + i, bits past L are 0.  EVERY
 *                word is written in full, nothing outside it is written
 *   scales       out, [2][N] fp32: v1 then v2
 *   status       out, [N] int32 or NULL: 1 where the row had a candidate (the ternary extra candidate counts), 0 where it
 *                had none (then v1 = 0)
 *
 * Values.  Every element is converted to fp32 exactly (subnormals kept) and clamped to +-a.  The magnitude of a clamped
 * value is a 15-bit key; the solve runs on a table of one count per key in LDS (a key's sum is count x value): candidates
 * at the inner sorted positions 1 .. n - 2, the m2 test always and the m1 test for LS2, for LST the extra candidate
 * fl32(mean) / 2 where min > mean / 2, the closed-form cost minimised, ties to the smallest sorted position, a row without
 * a candidate gives v1 = 0 -- the arithmetic of csrc/lsq_solver_math.h, which lsq_act_quant shares: v1 is an element of the
 * row (or the extra candidate) and the same bits as lsq_act_quant's on x converted to fp32 with the same bound.
 * Planes: the chain of lsq_linear_act_quant_half, operation for operation, with v_0 = v1: bit_0 = c >= 0,
 * result_1 = +-v1, bit_1 = (c - result_1) >= 0, res_1 = c -+ v1.
 * v2: LST: v1.  LS2: fl32(S_1 / L), S_1 = the sum of |res_1| over the WHOLE row by the summation rule of
 * lsq_hip_linear_act_half.h (fp32 inside a group of 8 elements in element order, fp64 across groups in an order that L alone
 * fixes): |v2 - mean| <= 2^-21 mean, the same bits whatever N, whichever row of the batch it is, wherever x lies, on every
 * call.  Inf and NaN are outside the contract (as for lsq_act_quant); no bit pattern indexes outside the table.
 * Work distribution: one workgroup of 512 threads owns a row from its first load to its last plane word (a grid of N
 * workgroups).  No workspace, integer atomics in LDS only, no row shared between
 * workgroups: a single very long row runs on one compute unit.
 *
 * LSQ_E_NULL: x, planes or scales is NULL.  LSQ_E_SHAPE: N, L or skip is not positive.  LSQ_E_SCHEME: scheme other than
 * LS2 / LST.  LSQ_E_UNSUPPORTED: x_dtype other than BF16 / F16, L >= 2^31, N >= 2^31.
 */
int lsq_linear_act_quant_solve_half(const void* x, int x_dtype, int64_t N, int64_t L, int scheme, int skip, float clamp_alpha,
                                    uint64_t* planes, float* scales, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_LINEAR_ACT_SOLVE_H_ */
