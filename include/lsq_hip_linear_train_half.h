/*
 * lsq_hip_linear_train_half.h -- C ABI of the 16-bit (bf16 / fp16) train-step kernels of the linear layer
 * (liblsq_hip_linear_train_half.so), a library of its own beside liblsq_hip.so and the other liblsq_hip_*.so.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller (the library allocates nothing; the workspace
 * is the caller's), `stream` is a hipStream_t passed as void* (NULL = default stream), every function returns 0, a
 * negative LSQ_E_* code for an argument error (returned before any launch, nothing written), or a positive hipError_t if
 * a launch failed.  The library links the objects of no other library; its kernels are the ones of
 * liblsq_hip_linear_train.so, instantiated from the same source on a 16-bit gradient and an epilogue.
 */
#ifndef LSQ_HIP_LINEAR_TRAIN_HALF_H_
#define LSQ_HIP_LINEAR_TRAIN_HALF_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"
#include "lsq_hip_linear_half.h" /* LSQ_DTYPE_* */

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_LINEAR_TRAIN_HALF_ABI_VERSION 1

int lsq_linear_train_half_abi_version(void);

/* The workspace size of lsq_linear_signw_dgrad_half: for every (kw_planes, F, O) what
 * lsq_linear_signw_dgrad_workspace_bytes of lsq_hip_linear_train.h returns -- the same transposed plane image.  Host code
 * only: no device call. */
size_t lsq_linear_signw_dgrad_half_workspace_bytes(int kw_planes, int64_t F, int64_t O);

/*
 * Input gradient of the linear layer's 16-bit train step in ONE pass: 16-bit gradient rows x sign-weight planes (the sum
 * over the output features, lsq_linear_signw_dgrad of lsq_hip_linear_train.h), then the straight-through estimator of the
 * activation quantizer against the step's 16-bit input, then one rounding into the type.
 *   gy           [M][O] of gy_dtype (LSQ_DTYPE_BF16 or LSQ_DTYPE_F16), row-major, any 2-byte-aligned address and any O (a
 *                staging role's values in one 8- or 16-byte load only where gy and O put every row on that size; the result
 *                is the same bits either way)
 *   wbits, kw_planes, wscales, M, F, O, workspace, workspace_bytes
 *                as in lsq_linear_signw_dgrad: the forward's own planes and fp32 scales [kw_planes][O], a workspace of at
 *                least lsq_linear_signw_dgrad_half_workspace_bytes(kw_planes, F, O) bytes, 8-byte aligned, rewritten by
 *                every call
 *   x            NULL (no epilogue: the product alone), or [M][F] of gy_dtype, row-major, any 2-byte-aligned address: the
 *                step's input.  Sample n owns rows n T .. n T + T - 1 (M % T == 0)
 *   T            with x: rows per sample.  Ignored without x
 *   kx, xscales  with x: the activation quantizer's planes and their per-sample scales [kx][M / T] fp32; kx = 0 (xscales may
 *                be NULL) = fp activations, the clamp alone.  Ignored without x (kx is still checked)
 *   clamp_alpha  with x: the symmetric clamp bound ALREADY ROUNDED into the type by the caller (as Tensor.clamp rounds it);
 *                negative = identity
 *   gx           out, [M][F] of gx_dtype: LSQ_DTYPE_F32 (4-byte aligned) or gy_dtype (2-byte aligned).  EVERY element is
 *                written and nothing outside it; an element store is one 2-byte (4-byte for F32) store, never a wider
 *                read-modify-write, so the bytes in front of and behind a view are left alone
 * Arithmetic.  Each 16-bit gradient is converted exactly to fp32.  From there the computation is lsq_linear_signw_dgrad's,
 * operation for operation: a = fl32(gy * ws[q][o]), the same hi + lo bf16 split, the same transposed plane image, the same
 * tile rule, stage order and split-kernel reduction order into one fp32 accumulator acc.  With x, in fp32, for row m of
 * sample n = m / T,
 *   r_0 = 0, d_i = clamp(float(x)) - r_i, r_{i+1} = r_i + v_i[n] sign(d_i)   (sign(+-0) = +1), then with G_kx = acc:
 *   t_i = G_{i+1} v_i[n] [|d_i| <= 1],  G_i = G_{i+1} - t_i,  result = [|x| <= alpha] sum_i t_i     (kx = 0: [|x| <= alpha] acc)
 * -- lsq_ste_backward of lsq_hip.h on float(x) viewed [M / T][T F], without contraction.  The result is stored as fp32, or
 * rounded once to nearest even into the type.  Bit for bit, therefore:
 *   (A) x = NULL, gx_dtype = F32:       lsq_linear_signw_dgrad(float(gy))
 *   (B) x = NULL, gx_dtype = gy_dtype:  (A) rounded into the type
 *   (C) x given:                        lsq_ste_backward(float(x) viewed [M / T][T F], (A), kx, xscales, clamp_alpha), rounded
 *                                       into gx_dtype
 * Accuracy, summation order and determinism are those stated in lsq_hip_linear_train.h.
 * LSQ_E_NULL: gy, wbits, wscales or gx is NULL; x given with kx > 0 and xscales NULL.  LSQ_E_SHAPE, LSQ_E_WORKSPACE: as
 * lsq_linear_signw_dgrad; LSQ_E_SHAPE also for T <= 0 or M % T != 0 with x given.  LSQ_E_UNSUPPORTED: what
 * lsq_linear_signw_dgrad refuses; gy_dtype other than BF16 / F16; gx_dtype neither F32 nor gy_dtype; kx outside
 * 0 .. LSQ_MAX_PLANES; M / T > 65535 with x given (the limit of lsq_ste_backward); gy, x or gx not aligned to its element.
 */
int lsq_linear_signw_dgrad_half(const void* gy, int gy_dtype, const uint64_t* wbits, int kw_planes, const float* wscales,
                                int64_t M, int64_t F, int64_t O, const void* x, int64_t T, int kx, const float* xscales,
                                float clamp_alpha, void* gx, int gx_dtype, void* workspace, size_t workspace_bytes,
                                void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_LINEAR_TRAIN_HALF_H_ */
