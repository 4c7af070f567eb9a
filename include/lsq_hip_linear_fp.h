/*
 * lsq_hip_linear_fp.h -- C ABI of the full-precision-activation x sign-weight linear layer (liblsq_hip_linear_fp.so), a
 * library of its own beside liblsq_hip.so and liblsq_hip_linear.so.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller (the library allocates nothing and needs no
 * workspace), `stream` is a hipStream_t passed as void* (NULL = default stream), every function returns 0, a negative
 * LSQ_E_* code for an argument error (returned before any launch), or a positive hipError_t if a launch failed.  The
 * library does not link the objects of liblsq_hip.so; its weight operand is what lsq_pack_weight of that library writes.
 */
#ifndef LSQ_HIP_LINEAR_FP_H_
#define LSQ_HIP_LINEAR_FP_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_LINEAR_FP_ABI_VERSION 1

int lsq_linear_fp_abi_version(void);

/*
 * fp32 activations x sign-weight planes on the bf16 matrix cores, for M rows of F features and O outputs:
 *   y[m][o] = bias[o] + sum_q ws[q][o] * I_q[m][o],   I_q[m][o] = sum_f c(x[m][f]) * s_q[o][f],
 *   c(v) = clamp(v, -clamp_alpha, clamp_alpha) if clamp_alpha >= 0, else v
 * with s_q the +-1 signs of weight plane q, i.e. F.linear(c(x), w_q, bias) for w_q = sum_q ws_q s_q.
 *   x           [M][F] fp32, row-major, any 4-byte-aligned address and any F (16-byte loads only where x is 16-byte
 *               aligned and F % 4 == 0; the result is the same bits either way)
 *   wbits       the weight planes lsq_pack_weight writes for (O, C = F, KH = KW = 1): words [q][ceil(F / 64)][ceil16(O)]
 *   wscales     [kw_planes][O] fp32
 *   bias        [O] fp32 or NULL
 *   y           out, [M][O] fp32; nothing outside it is written
 * Accuracy: each clamped activation v is split into hi = bf16(v) and lo = bf16(v - hi) (v - hi is exact in fp32, so
 * |v - hi - lo| <= 2^-16 |v|, typically 2^-18 |v|); the weights are exact +-1 in bf16, every product hi * s and lo * s is
 * exact, and the products are summed in fp32 by v_mfma_f32_32x32x16_bf16.  I_q therefore differs from the exact sum by at
 * most 2^-16 sum_f |c(x[m][f])| (typically 2^-18) plus the fp32 rounding of the accumulation -- a single bf16 operand
 * (2^-8 per product at most, typically 2^-9) would be 2^8 times coarser.
 * Summation order (fixed for given M, F, O: results are bitwise deterministic, no atomics): I_q accumulates 16 features
 * per MFMA step in feature order, the hi products of a step before its lo products; the small-M kernel adds the partial
 * I_q of its 8 waves' feature ranges in wave order, ((I^0 + I^1) + I^2) + ...; the epilogue is
 *   y = fma(I_(kw-1), ws[kw-1][o], ... fma(I_1, ws[1][o], fma(I_0, ws[0][o], b)) ...),  b = bias[o] (0 without bias).
 * Kernels: fewer than 256 tiles of 64 x 64 in M x O -> one 32 x 32 output tile per workgroup with its F split over 8
 * waves (weight-streaming shapes: decode, small batches); otherwise 128 x 128 tiles (where there are at least 256 of
 * them) or 64 x 64 tiles, each over the whole F.
 * Limits: 1 <= kw_planes <= LSQ_MAX_PLANES, F < 2^22, M < 2^31, O < 2^21; LSQ_E_UNSUPPORTED otherwise.
 */
int lsq_linear_signw(const float* x, float clamp_alpha, const uint64_t* wbits, int kw_planes, const float* wscales,
                     const float* bias, int64_t M, int64_t F, int64_t O, float* y, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_LINEAR_FP_H_ */
