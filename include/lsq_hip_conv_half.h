/*
 * lsq_hip_conv_half.h -- C ABI of the 16-bit-activation (bf16 / fp16) x sign-weight convolution
 * (liblsq_hip_conv_half.so), a library of its own beside liblsq_hip.so and the other liblsq_hip_*.so.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller (the library allocates nothing; the workspace
 * is the caller's), `stream` is a hipStream_t passed as void* (NULL = default stream), every function returns 0, a
 * negative LSQ_E_* code for an argument error (returned before any launch, nothing written), or a positive hipError_t if
 * a launch failed.  The library does not link the objects of liblsq_hip.so; its weight operand is what lsq_pack_weight
 * of that library writes -- the very planes lsq_signw_conv2d reads.  There is no prepared weight image and no prepare
 * entry point: the bits are expanded in the kernel.
 */
#ifndef LSQ_HIP_CONV_HALF_H_
#define LSQ_HIP_CONV_HALF_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"
#include "lsq_hip_linear_half.h" /* LSQ_DTYPE_* */

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_CONV_HALF_ABI_VERSION 1

int lsq_conv_half_abi_version(void);

/*
 * Which kernel a call with geometry g takes: a combination of the bits below, or a negative LSQ_E_* code for a geometry
 * the convolution refuses (LSQ_E_NULL, LSQ_E_SHAPE, LSQ_E_UNSUPPORTED, as there).  Host code only: no device call.
 *   PATCH        the patch kernel (the input patch of a workgroup's output pixels fits its LDS plane); clear: the general
 *                (im2col) kernel
 *   WIDE         O / groups > 64: tiles of 128 out-channels; clear: 64
 *   UNIT_STRIDE  (with PATCH only) stride 1 x 1: 128 (wide) or 256 pixels per workgroup, a patch of at most 512 entries;
 *                clear: 64 (wide) or 128 pixels, at most 640 entries
 *   MANY_TAPS    (with PATCH only) more than 9 taps: the weights of later groups of 9 taps are staged in place
 * Each value names one kernel instantiation per element type.  The patch rule is the one of lsq_signw_conv2d (same tiles,
 * same patch lengths), so both libraries take a patch kernel for the same geometries.
 */
enum {
  LSQ_CONV_HALF_PATCH = 1,
  LSQ_CONV_HALF_WIDE = 2,
  LSQ_CONV_HALF_UNIT_STRIDE = 4,
  LSQ_CONV_HALF_MANY_TAPS = 8
};

int lsq_signw_conv2d_half_plan(const lsq_conv_geom* g);

/*
 * 16-bit activations x sign-weight planes on the 16-bit matrix cores:
 *   y[n][o] = bias[o] + sum_q ws[q][o] * conv(c(x), s_q)[n][o],   c(v) = clamp(v, -a, a)
 * with s_q the +-1 signs of weight plane q, i.e. F.conv2d(x.clamp(-a, a), w_q, bias, stride, padding, dilation, groups)
 * for w_q = sum_q ws_q s_q and a 16-bit tensor x.
 *   x            [N][C][H][W] of x_dtype (LSQ_DTYPE_BF16 or LSQ_DTYPE_F16), contiguous, any 2-byte-aligned address.  The
 *                elements are loaded one by one (2-byte loads, a wave on consecutive addresses), never wider: the result is
 *                the same bits at every address.  (Wider loads where the address allows would be bitwise safe too; they are
 *                not implemented, and what they would gain has not been measured)
 *   clamp_alpha  the symmetric clamp bound a, USED AS GIVEN: the caller rounds it into x_dtype first (as Tensor.clamp does
 *                and as lsq_act_quant_half specifies), so that every clamped value is a value of the type.  Negative: no
 *                clamp.  A bound above fp16's range arrives as +inf and is the identity.  Without a bound the values pass
 *                untouched, NaN and +-inf included, as Tensor.clamp leaves them.  Under a finite bound a NaN activation is
 *                OUTSIDE the contract: the min / max instructions return their non-NaN operand, so it enters the sum as
 *                -a where Tensor.clamp would propagate the NaN
 *   wbits        the weight planes lsq_pack_weight writes for g: words [q][tap][ceil(C / groups / 64)][groups * ceil16(O / groups)]
 *   wscales      [kw_planes][O] fp32
 *   bias         [O] fp32 or NULL
 *   g            every geometry check_geom of lsq_hip.h accepts is computed: any kernel size, stride, padding (zero padding
 *                is exact), dilation, groups, and channel counts that are not multiples of 16 or 64
 *   y            out, [N][O][Ho][Wo] of y_dtype: LSQ_DTYPE_F32 or x_dtype, aligned to its element; nothing outside it is
 *                written (16-bit elements are stored one by one: two outputs of different workgroups can share a dword)
 *   workspace    at least lsq_signw_conv2d_half_workspace_bytes(g, kw_planes, y_dtype) bytes, 4-byte aligned, any content,
 *                rewritten by the call; where that is 0 it may be NULL (LSQ_E_WORKSPACE if it is NULL, misaligned or too
 *                small where one is needed)
 * No fused epilogue: no folded batch norm, ReLU / PReLU or residual operands -- on a 16-bit tensor torch rounds after each
 * of them, so they cannot be fused without changing bits.  The call that fuses them and rounds once, with other bits than
 * the composition in torch, is lsq_signw_conv2d_fused_half of lsq_hip_conv_fused_half.h; this one stays as it is.
 * Accuracy: every clamped activation is a value of x_dtype and the weights are exact +-1 in that type, so every product is
 * exact, and the products are summed in fp32 by v_mfma_f32_32x32x16_bf16 / v_mfma_f32_32x32x16_f16: ONE matrix instruction
 * per (16 channels, tap) and tile (lsq_signw_conv2d issues two, for the hi and the lo half of an fp32 value), one LDS plane,
 * no split arithmetic.  What is left against the exact sum is the fp32 rounding of the accumulation.  The weight scales
 * stay fp32.
 * Subnormals: bf16 and fp16 subnormal activations are NOT flushed (the instruction and denormal mode of
 * lsq_linear_signw_half): 64 channels of the smallest fp16 subnormal against an all +1 plane of scale 1 give 64 * 2^-24.
 * Summation order (fixed by g alone: results are bitwise deterministic, no atomics).  I_q = conv(c(x), s_q) of one output
 * accumulates in one fp32 MFMA accumulator,
 *   patch kernel:    channel chunks of 16 in order; within a chunk the taps in (kh, kw) order, one MFMA each;
 *   general kernel:  taps in (kh, kw) order; within a tap channel chunks of 16 in order, one MFMA each
 * (channels past C / groups and input positions in the padding contribute exact zeros), and the epilogue is, with a separate
 * multiply and add in fp32,
 *   t_0 = b + I_0 * ws[0][o],  t_q = t_(q-1) + I_q * ws[q][o],  b = bias[o] (0 without bias).
 * This is the order and expression of lsq_signw_conv2d's patch kernel and 3x3 fast path: for bf16 x and a clamp_alpha that
 * is a bf16 value (or negative), the fp32 result of a PATCH plan has the values of lsq_signw_conv2d on x converted to fp32
 * wherever that call takes one of those two paths -- the lo products it adds are all zero.  (Values, not bit patterns:
 * adding +0 turns a -0 sum into +0.)
 * 16-bit y: t_(kw_planes-1) rounded ONCE, to nearest even, for every kw_planes.  A launch holds ONE plane, as in
 * lsq_signw_conv2d (64 accumulator registers a lane on the 128 x 128 and 64 x 256 tiles, 136 vector registers in all: a
 * second accumulator set would halve the two waves a SIMD the kernels run at); with two or more planes and a 16-bit y
 * the running fp32 sum lives in `workspace` ([N][O][Ho][Wo] fp32) between launches and only the last launch stores y, so
 * no intermediate is ever rounded to 16 bits.  With an fp32 y the running sum lives in y itself, as in
 * lsq_signw_conv2d, and no workspace is needed: lsq_signw_conv2d_half_workspace_bytes is 4 N O Ho Wo for a 16-bit y_dtype
 * and kw_planes >= 2, and 0 otherwise (also for a geometry the call refuses).
 * LSQ_E_NULL: x, wbits, wscales, y or g is NULL.  LSQ_E_SHAPE: what check_geom refuses, or an empty output (Ho or Wo < 1).
 * LSQ_E_UNSUPPORTED: x_dtype other than BF16 / F16; y_dtype other than F32 / x_dtype; kw_planes outside
 * 1 .. LSQ_MAX_PLANES; sizes past the 32-bit index limits: N C H W, N O Ho Wo or N (H + 2 pad_h) (W + 2 pad_w) >= 2^31,
 * 2^28 or more words in a weight plane, more than 65535 out-channel tiles (groups * ceil(O / groups / 128), or / 64 where
 * O / groups <= 64).
 */
int64_t lsq_signw_conv2d_half_workspace_bytes(const lsq_conv_geom* g, int kw_planes, int y_dtype);

int lsq_signw_conv2d_half(const void* x, int x_dtype, float clamp_alpha, const uint64_t* wbits, int kw_planes,
                          const float* wscales, const float* bias, const lsq_conv_geom* g, void* y, int y_dtype,
                          void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_CONV_HALF_H_ */
