/*
 * lsq_hip_linear_wgrad.h -- C ABI of the weight-gradient kernel of the linear layer (liblsq_hip_linear_wgrad.so), a library
 * of its own beside liblsq_hip.so, liblsq_hip_train.so, liblsq_hip_linear.so, liblsq_hip_linear_fp.so,
 * liblsq_hip_linear_train.so and liblsq_hip_linear_wgrad_half.so (lsq_hip_linear_wgrad_half.h: the same kernels, compiled from
 * the same source, on bf16 / fp16 operands).
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller (the library allocates nothing; the workspace
 * is the caller's), `stream` is a hipStream_t passed as void* (NULL = default stream), every function returns 0, a
 * negative LSQ_E_* code for an argument error (returned before any launch, nothing written), or a positive hipError_t if
 * a launch failed.  The library links no other library's objects.
 */
#ifndef LSQ_HIP_LINEAR_WGRAD_H_
#define LSQ_HIP_LINEAR_WGRAD_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_LINEAR_WGRAD_ABI_VERSION 1

int lsq_linear_wgrad_abi_version(void);

/*
 * Weight gradient of the linear layer with binary activations: fp32 gradient rows transposed x the sign planes of the
 * quantized input, the sum running over the ROWS (grad_wq = grad_y^T . x_q for x_q = sum_p xs_p b_p), on the bf16 matrix
 * cores:
 *   gwq[o][f] = sum_{p < kx} sum_{m < M} a_p[m][o] * b_p[m][f],   a_p[m][o] = fl32(gy[m][o] * xs[p][m / T]),   M = N * T
 * with b_p the +-1 signs of activation plane p.
 *   gy          [M][O] fp32, row-major, any 4-byte-aligned address and any O (16-byte loads only where gy is 16-byte
 *               aligned and O % 4 == 0; the result is the same bits either way)
 *   x           [M][F] fp32, row-major: the layer's input BEFORE the clamp
 *   xscales     [kx][N] fp32: the per-(plane, sample) scales; row m belongs to sample m / T
 *   clamp_alpha the symmetric clamp in front of the quantizer; < 0: no clamp
 *   gwq         out, [O][F] fp32; nothing outside it is written
 *   workspace   at least lsq_linear_signx_wgrad_workspace_bytes(kx, N, T, F, O) bytes, 8-byte aligned, any content; it is
 *               rewritten by every call (LSQ_E_WORKSPACE if it is NULL, unaligned or too small)
 * Signs: those of the quantizer chain exactly as lsq_quant_values / lsq_ste_backward form them, in fp32:
 *   xc = clamp(x), r_0 = 0, d_i = xc - r_i, b_i = (d_i >= 0 ? +1 : -1), r_{i+1} = r_i + v_i b_i,   v_i = xs[i][m / T]
 * (sign(+-0) = +1) -- the bits lsq_act_quant packed in the forward.
 * Sign image: a first kernel of the call writes X[p][ceil(M / 64)][ceil16(F)] (64-bit words) into `workspace`: bit j of word
 * [p][w][f] is 1 where b_p = +1 at row 64 w + j, feature f.  One wave per block of 64 rows x 64 features, a lane owns one
 * feature and walks the rows (256-byte coalesced reads of x), ORing the kx chain bits into its kx words.  Rows >= M and
 * features >= F leave zero bits; the A operand of rows >= M is staged as 0 and columns >= F are never stored.
 *   workspace bytes = kx * ceil(M / 64) * ceil16(F) * 8
 * This replaces the M x F fp32 image lsq_quant_values writes by kx bits per activation.
 * GEMM: D rows = output features o (operand A = the scaled gradient, transposed through LDS), D columns = input features f
 * (operand B: 8 consecutive bits of one image word per lane, expanded to bf16 +-1), v_mfma_f32_32x32x16_bf16.
 * Accuracy: the per-(plane, sample) scale sits on the summed index, so it is multiplied INTO the A operand: a = fl32(gy * xs)
 * is split into hi = bf16(a) and lo = bf16(a - hi).  bf16 keeps 8 significant bits, so round-to-nearest gives
 * |a - hi| <= 2^-8 |a| (a - hi is exact in fp32) and |a - hi - lo| <= 2^-8 |a - hi| <= 2^-16 |a|; the signs are exact +-1 in
 * bf16, every product hi * b and lo * b is exact, and the products of ALL planes are summed into one fp32 accumulator.
 * With the rounding of the product a (2^-24 |gy xs|),
 *   |gwq - exact| <= (2^-16 + 2^-24) sum_p sum_m |gy[m][o] xs[p][m / T]|  plus the fp32 rounding of the accumulation
 * in the worst case; what the prescribed arithmetic gives against fp64 is 3-4e-6 of max |gwq| for 330 outputs and more
 * (tests/test_linear_wgrad_host.py emulates it on the CPU, tests/test_gpu_linear_wgrad.py holds the kernel to 1e-5 of
 * max |gwq|).  A single bf16 operand is 2^8 times coarser.
 * Summation order (fixed for given kx, N, T, F, O: results are bitwise deterministic, no atomics): the 64-row words in order
 * w = 0 .. ceil(M / 64) - 1, within a word the planes p = 0 .. kx - 1, within a plane four MFMA steps of 16 rows in order
 * of m, the hi products of a step before its lo products, everything into one accumulator.  The small-shape kernel cuts
 * that sequence of (word, plane, step) units into 8 consecutive ranges, one per wave, and adds the partial sums in wave
 * order, ((S^0 + S^1) + S^2) + ...
 * Kernels: fewer than 256 tiles of 64 x 64 in O x F -> one 32 x 32 tile of gwq per workgroup with the summed dimension
 * split over 8 waves; otherwise 128 x 128 tiles (where there are at least 256 of them) or 64 x 64 tiles, four waves each,
 * the scaled and split gradient tile staged once per (word, plane) in LDS.
 * Limits: 1 <= kx <= LSQ_MAX_PLANES, N <= 65535 (the limit of lsq_quant_values), M = N * T < 2^31, F < 2^22, O < 2^21;
 * LSQ_E_UNSUPPORTED otherwise, before anything is written (the workspace size of such a call is 0).
 */
size_t lsq_linear_signx_wgrad_workspace_bytes(int kx, int64_t N, int64_t T, int64_t F, int64_t O);

int lsq_linear_signx_wgrad(const float* gy, const float* x, int kx, const float* xscales, float clamp_alpha, int64_t N,
                           int64_t T, int64_t F, int64_t O, float* gwq, void* workspace, size_t workspace_bytes,
                           void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_LINEAR_WGRAD_H_ */
