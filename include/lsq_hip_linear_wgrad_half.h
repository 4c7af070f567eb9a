/*
 * lsq_hip_linear_wgrad_half.h -- C ABI of the 16-bit (bf16 / fp16) weight-gradient kernel of the linear layer
 * (liblsq_hip_linear_wgrad_half.so), a library of its own beside liblsq_hip.so and the other liblsq_hip_*.so.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller (the library allocates nothing; the workspace
 * is the caller's), `stream` is a hipStream_t passed as void* (NULL = default stream), every function returns 0, a
 * negative LSQ_E_* code for an argument error (returned before any launch, nothing written), or a positive hipError_t if
 * a launch failed.  The library links the objects of no other library; its kernels are the ones of
 * liblsq_hip_linear_wgrad.so, instantiated from the same source on a 16-bit element type and an epilogue.
 */
#ifndef LSQ_HIP_LINEAR_WGRAD_HALF_H_
#define LSQ_HIP_LINEAR_WGRAD_HALF_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"
#include "lsq_hip_linear_half.h" /* LSQ_DTYPE_* */

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_LINEAR_WGRAD_HALF_ABI_VERSION 1

int lsq_linear_wgrad_half_abi_version(void);

/* The workspace size of lsq_linear_signx_wgrad_half: for every (kx, N, T, F, O) what
 * lsq_linear_signx_wgrad_workspace_bytes of lsq_hip_linear_wgrad.h returns -- the same sign image; 0 for arguments the call
 * refuses.  Host code only: no device call. */
size_t lsq_linear_signx_wgrad_half_workspace_bytes(int kx, int64_t N, int64_t T, int64_t F, int64_t O);

/*
 * Weight gradient of the linear layer's 16-bit train step with binary activations in ONE call: 16-bit gradient rows
 * transposed x the sign planes of the quantized 16-bit input, the sum over the rows (lsq_linear_signx_wgrad of
 * lsq_hip_linear_wgrad.h), then -- with w -- the straight-through estimator of the WEIGHT quantizer in the GEMM's epilogue.
 *   gy, x        [M][O] and [M][F] of `dtype` (LSQ_DTYPE_BF16 or LSQ_DTYPE_F16), M = N * T, row-major, any 2-byte-aligned
 *                address, any O and F.  Wider loads (8 bytes of gy) are used only where the address and the row length put
 *                every row on that size (gy 8-byte aligned, O % 4 == 0); the result is the same bits either way.  x is the
 *                layer's input BEFORE the clamp
 *   kx, xscales  the activation quantizer's planes and their per-sample scales [kx][N] fp32; row m belongs to sample m / T
 *   clamp_alpha  the symmetric clamp bound ALREADY ROUNDED into the type by the caller (as Tensor.clamp rounds it);
 *                negative = no clamp
 *   w            NULL, or the layer's fp32 weight [O][F] (4-byte aligned)
 *   kw, wscales  with w: the weight quantizer's planes, 1 .. LSQ_MAX_PLANES, and their per-output scales [kw][O] fp32.
 *                Ignored without w
 *   out          [O][F] fp32, 4-byte aligned.  EVERY element is written and nothing outside it
 *   workspace    the sign image of lsq_linear_signx_wgrad: at least
 *                lsq_linear_signx_wgrad_half_workspace_bytes(kx, N, T, F, O) bytes, 8-byte aligned, any content, rewritten
 *                by every call
 * Arithmetic.  Each 16-bit value is converted exactly to fp32 as it is read.  From there the computation is
 * lsq_linear_signx_wgrad's, operation for operation: the sign chain on clamp(float(x)) with sign(+-0) = +1,
 * a = fl32(float(gy) * xs[p][m / T]), the same bf16 hi + lo split, the same sign image, tile rule (on (O, F)) and stage
 * order, the same 8-range split reduction, into one fp32 accumulator acc.  With w, in fp32 and without contraction, for
 * element (o, f) with v_i = wscales[i][o]:
 *   r_0 = 0, d_i = w[o F + f] - r_i, r_{i+1} = r_i + v_i sign(d_i)   (sign(+-0) = +1), then with G_kw = acc:
 *   t_i = G_{i+1} v_i [|d_i| <= 1],  G_i = G_{i+1} - t_i,  out = sum_i t_i
 * Bit for bit, therefore:
 *   (A) w == NULL:  out = lsq_linear_signx_wgrad(float(gy), float(x), kx, xscales, clamp_alpha, N, T, F, O)
 *   (B) w given:    out = lsq_ste_backward(w viewed [O][F], (A), kw, wscales, -1.0) of lsq_hip.h
 * In (B) the fp32 product never goes to memory: the step's grad_w is this one call.
 * Accuracy, summation order and determinism (no atomics: the same bits from call to call and on any stream) are those stated
 * in lsq_hip_linear_wgrad.h.
 * LSQ_E_NULL: gy, x, xscales or out is NULL; w given with wscales NULL.  LSQ_E_SHAPE, LSQ_E_UNSUPPORTED, LSQ_E_WORKSPACE: as
 * lsq_linear_signx_wgrad returns them (kx outside 1 .. LSQ_MAX_PLANES, N > 65535, M >= 2^31, F >= 2^22, O >= 2^21).
 * LSQ_E_UNSUPPORTED also: dtype other than BF16 / F16; kw outside 1 .. LSQ_MAX_PLANES with w given; gy or x not 2-byte
 * aligned; w, wscales or out not 4-byte aligned.
 */
int lsq_linear_signx_wgrad_half(const void* gy, const void* x, int dtype, int kx, const float* xscales, float clamp_alpha,
                                int64_t N, int64_t T, int64_t F, int64_t O, const float* w, int kw, const float* wscales,
                                float* out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_LINEAR_WGRAD_HALF_H_ */
