/*
 * lsq_hip_linear_half.h -- C ABI of the 16-bit-activation (bf16 / fp16) x sign-weight linear layer
 * (liblsq_hip_linear_half.so), a library of its own beside liblsq_hip.so and the other liblsq_hip_linear*.so.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller (the library allocates nothing; the workspace
 * is the caller's), `stream` is a hipStream_t passed as void* (NULL = default stream), every function returns 0, a
 * negative LSQ_E_* code for an argument error (returned before any launch, nothing written), or a positive hipError_t if
 * a launch failed.  The library does not link the objects of liblsq_hip.so; its weight operand is what lsq_pack_weight
 * of that library writes -- the very planes lsq_linear_signw reads.
 */
#ifndef LSQ_HIP_LINEAR_HALF_H_
#define LSQ_HIP_LINEAR_HALF_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_LINEAR_HALF_ABI_VERSION 1

/* element types of x and y */
enum { LSQ_DTYPE_F32 = 0, LSQ_DTYPE_BF16 = 1, LSQ_DTYPE_F16 = 2 };

int lsq_linear_half_abi_version(void);

/*
 * 16-bit activations x sign-weight planes on the 16-bit matrix cores, for M rows of F features and O outputs:
 *   y[m][o] = bias[o] + sum_q ws[q][o] * I_q[m][o],   I_q[m][o] = sum_f c(x[m][f]) * s_q[o][f],
 *   c(v) = clamp(v, -a, a) with a = clamp_alpha ROUNDED TO NEAREST (even) IN x_dtype if clamp_alpha >= 0, else v
 * with s_q the +-1 signs of weight plane q, i.e. F.linear(x.clamp(-alpha, alpha), w_q, bias) for w_q = sum_q ws_q s_q
 * and a 16-bit tensor x: Tensor.clamp rounds its bound into the tensor's type as well (bf16(1.3) = 1.296875,
 * fp16(0.7) = 0.7001953125).  A bound that overflows the type (fp16: above 65504) is +inf, the identity.
 *   x           [M][F] of x_dtype (LSQ_DTYPE_BF16 or LSQ_DTYPE_F16), row-major, any 2-byte-aligned address and any F
 *               (16-byte loads only where x is 16-byte aligned and F % 8 == 0, so that every row starts on 16 bytes; the
 *               result is the same bits either way)
 *   wbits       the weight planes lsq_pack_weight writes for (O, C = F, KH = KW = 1): words [q][ceil(F / 64)][ceil16(O)]
 *   wscales     [kw_planes][O] fp32
 *   bias        [O] fp32 or NULL
 *   y           out, [M][O] of y_dtype: LSQ_DTYPE_F32 or x_dtype, aligned to its element; nothing outside it is written
 *               (16-bit elements are stored one by one: with odd O two outputs of different rows share a dword)
 *   workspace   at least lsq_linear_signw_half_workspace_bytes(M, O, kw_planes, y_dtype) bytes, 4-byte aligned, any
 *               content, rewritten by the call; where that is 0 it may be NULL (LSQ_E_WORKSPACE if it is NULL, misaligned
 *               or too small where one is needed)
 * Accuracy: every clamped activation is a value of x_dtype, the weights are exact +-1 in that type, so every product is
 * exact, and the products are summed in fp32 by v_mfma_f32_32x32x16_bf16 / v_mfma_f32_32x32x16_f16: ONE matrix
 * instruction per 16 features and plane (lsq_linear_signw issues two, for the hi and the lo half of an fp32 value), no
 * split arithmetic.  What is left against the exact sum is the fp32 rounding of the accumulation.
 * Summation order (fixed for given M, F, O: results are bitwise deterministic, no atomics): lsq_linear_signw's -- the same
 * choice of kernel, I_q accumulates 16 features per MFMA step in feature order; the small-M kernel adds the partial I_q of
 * its 8 waves' feature ranges in wave order, ((I^0 + I^1) + I^2) + ...; the epilogue is
 *   y = fma(I_(kw-1), ws[kw-1][o], ... fma(I_1, ws[1][o], fma(I_0, ws[0][o], b)) ...),  b = bias[o] (0 without bias)
 * in fp32.  For bf16 rows the fp32 result therefore has the values of lsq_linear_signw on the same rows converted to fp32
 * whenever clamp_alpha is a bf16 value (or negative): the lo products that kernel adds are all zero.  (Values, not bit
 * patterns: adding +0 turns a -0 sum into +0.)
 * 16-bit y: the fp32 result above rounded ONCE, to nearest even, for every kw_planes.  A launch holds two planes; with
 * three or more planes and a 16-bit y the running fp32 sum lives in `workspace` ([M][O] fp32) between launches and only the
 * last launch stores y, so no intermediate is ever rounded to 16 bits.  With an fp32 y the running sum lives in y itself,
 * as in lsq_linear_signw, and no workspace is needed.
 * Subnormals: bf16 and fp16 subnormal activations are NOT flushed by the matrix instruction: 64 fp16 subnormals against
 * an all +1 plane of scale 1 give their exact sum (measured on an MI355X, tests/test_gpu_linear_half.py; the kernels are
 * compiled with hipcc's default denormal mode, which the clamp's v_pk_min_f16 / v_pk_max_f16 and v_med3_f32 honour).
 * Kernels: fewer than 256 tiles of 64 x 64 in M x O -> one 32 x 32 output tile per workgroup with its F split over 8
 * waves; otherwise 128 x 128 tiles (where there are at least 256 of them) or 64 x 64 tiles, each over the whole F.
 * LSQ_E_NULL: x, wbits, wscales or y is NULL.  LSQ_E_SHAPE: M, F or O is not positive.  LSQ_E_UNSUPPORTED: x_dtype other
 * than BF16 / F16; y_dtype other than F32 / x_dtype; kw_planes outside 1 .. LSQ_MAX_PLANES; F >= 2^22, M >= 2^31 or
 * O >= 2^21.
 */
int64_t lsq_linear_signw_half_workspace_bytes(int64_t M, int64_t O, int kw_planes, int y_dtype);

int lsq_linear_signw_half(const void* x, int x_dtype, float clamp_alpha, const uint64_t* wbits, int kw_planes,
                          const float* wscales, const float* bias, int64_t M, int64_t F, int64_t O, void* y, int y_dtype,
                          void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_LINEAR_HALF_H_ */
