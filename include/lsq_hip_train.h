/*
 * lsq_hip_train.h -- C ABI of the training kernels (liblsq_hip_train.so), a library of its own beside liblsq_hip.so.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller (the library allocates nothing), `stream` is a
 * hipStream_t passed as void* (NULL = default stream), every function returns 0, a negative LSQ_E_* code for an argument
 * error (returned before any launch), or a positive hipError_t if a launch failed.  The library does not link the objects
 * of liblsq_hip.so; it shares lsq_conv_geom, the LSQ_E_* codes and the activation plane layout with it.
 */
#ifndef LSQ_HIP_TRAIN_H_
#define LSQ_HIP_TRAIN_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_TRAIN_ABI_VERSION 1

int lsq_train_abi_version(void);

/*
 * Weight gradient of a convolution with binary activations, from the activation sign planes:
 *   grad_wq[o][c][i][j] = sum_n sum_(ho,wo) grad_y[n][o][ho][wo] * x_q[n][c][ho*s + i - pad_h][wo*s + j - pad_w],
 *   x_q[n][c][h][w]     = sum_{p<kx} xscales[p][n] * (2 bit_p - 1), and 0 outside the image,
 * i.e. what torch.nn.grad.conv2d_weight returns for the quantizer's value x_q (QuantConv2d's weight gradient before the
 * straight-through estimator over the weight rows).
 *   xplanes      [kx] activation planes in the layout of lsq_hip.h (what lsq_act_quant wrote for this step; the halo words
 *                are zero and contribute nothing here, nor do the bits of channels >= C)
 *   xscales      [kx][N] fp32 plane scales
 *   grad_y       [N][O][Ho][Wo] fp32
 *   grad_wq      out, [O][C][KH][KW] fp32; nothing outside it is written
 *   workspace    lsq_train_wgrad_workspace_bytes(g, kx) bytes, 16-byte aligned, any content (NULL when that is 0): the
 *                partial sums of the K split, reduced in a fixed order -- the result is bitwise the same from call to call
 * Geometry: groups 1, dilation 1, stride_h == stride_w in {1, 2}, pad <= kernel - 1, KH, KW <= 8, 1 <= kx <= LSQ_MAX_PLANES,
 * N * Ho * Wo < 2^31; LSQ_E_UNSUPPORTED otherwise.
 * Accuracy: per element within a few fp32 roundings of sum |grad_y| |x_q| (bf16 three-term split of the fp32 products,
 * exact +-1 signs, fp32 accumulation).
 */
size_t lsq_train_wgrad_workspace_bytes(const lsq_conv_geom* g, int kx);
int lsq_train_wgrad(const uint64_t* xplanes, int kx, const float* xscales, const float* grad_y, const lsq_conv_geom* g,
                    float* grad_wq, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_TRAIN_H_ */
