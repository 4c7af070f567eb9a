/*
 * lsq_hip_linear.h -- C ABI of the binary linear layer (liblsq_hip_linear.so), a library of its own beside liblsq_hip.so.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller (the library allocates nothing), `stream` is a
 * hipStream_t passed as void* (NULL = default stream), every function returns 0, a negative LSQ_E_* code for an argument
 * error (returned before any launch), or a positive hipError_t if a launch failed.  The library does not link the objects
 * of liblsq_hip.so; its operands are what lsq_act_quant and lsq_pack_weight of that library write.
 */
#ifndef LSQ_HIP_LINEAR_H_
#define LSQ_HIP_LINEAR_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_LINEAR_ABI_VERSION 1

int lsq_linear_abi_version(void);

/*
 * Binary x binary linear layer on the fp4 matrix cores, for M rows of F features and O outputs, T = rows_per_scale rows per
 * sample (N = M / T samples):
 *   y[m][o] = bias[o] + sum_q ws[q][o] * sum_p xs[p][m / T] * I_pq[m][o],   I_pq = sum_f a_p[m][f] * w_q[o][f] in [-F, F]
 * with a, w the +-1 signs of the planes, i.e. F.linear(x_q, w_q, bias) for x_q = sum_p xs_p b_p, w_q = sum_q ws_q s_q.
 *   xplanes     [kx] activation planes as lsq_act_quant writes them for the geometry (N, C = T*F, H = 1, W = 1): words
 *               [p][M][ceil(F / 64)] (T > 1 needs F % 64 == 0)
 *   xscales     [kx][N] fp32 plane scales
 *   wbits, wsum the weight planes and tap sums lsq_pack_weight writes for (O, C = F, KH = KW = 1): words
 *               [q][ceil(F / 64)][ceil16(O)], wsum [q][O]
 *   wscales     [kw_planes][O] fp32
 *   bias        [O] fp32 or NULL
 *   y           out, [M][O] fp32
 * The integers I_pq are exact; the epilogue is the fp32 arithmetic of lsq_xnor_conv2d in the same order, so y is bit for bit
 * what lsq_xnor_conv2d returns for the 1x1 convolution (M, F, 1, 1) with the scales of sample m / T at row m.
 * Limits: 1 <= kx, kw_planes <= LSQ_MAX_PLANES, F < 2^22, M < 2^31, O < 2^21; LSQ_E_UNSUPPORTED otherwise.
 */
int lsq_linear_xnor(const uint64_t* xplanes, int kx, const float* xscales, int64_t rows_per_scale,
                    const uint64_t* wbits, const int32_t* wsum, int kw_planes, const float* wscales, const float* bias,
                    int64_t M, int64_t F, int64_t O, float* y, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_LINEAR_H_ */
