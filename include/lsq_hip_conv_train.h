/*
 * lsq_hip_conv_train.h -- C ABI of the train-step kernels of the convolution layer (liblsq_hip_conv_train.so), a library
 * of its own beside liblsq_hip.so and the other liblsq_hip_*.so.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller (the library allocates nothing; the workspace
 * is the caller's), `stream` is a hipStream_t passed as void* (NULL = default stream), every function returns 0, a
 * negative LSQ_E_* code for an argument error (returned before any launch, nothing written), or a positive hipError_t if
 * a launch failed.  The library does not link the objects of liblsq_hip.so; its weight operand is what lsq_pack_weight of
 * that library writes for the FORWARD geometry -- the very planes lsq_xnor_conv2d and lsq_signw_conv2d read.
 */
#ifndef LSQ_HIP_CONV_TRAIN_H_
#define LSQ_HIP_CONV_TRAIN_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_CONV_TRAIN_ABI_VERSION 1

int lsq_conv_train_abi_version(void);

/*
 * What a call with the forward geometry g does.
 *   kernel        LSQ_CONV_DGRAD_NARROW (C / groups <= 64: tiles of 128 pixels x 64 channels) or LSQ_CONV_DGRAD_WIDE (tiles
 *                 of 128 pixels x 128 channels), with LSQ_CONV_DGRAD_PATCH where the patch kernel runs: a tile of
 *                 NS samples x TH x TW pixels of a class (powers of two, 128 in all) whose taps read at most 222 positions
 *                 NS (TH + dH)(TW + dW) of grad_y, dH / dW = the spread of the taps' shifts in the class with the most taps;
 *                 the patch is scaled, split and staged once per (64 out-channels, plane) for all taps.  Without the bit
 *                 (large or widely dilated kernels) the gather kernel runs: 128 consecutive pixels of a class, staged once
 *                 per (tap, 64 out-channels, plane).  Each of the four values names one kernel instantiation
 *   classes       stride_h * stride_w residue classes of input pixels: class (rh, rw) holds the pixels with
 *                 (h + pad_h) % stride_h == rh and (w + pad_w) % stride_w == rw, and is reached only by the taps with
 *                 (i * dil_h) % stride_h == rh and (j * dil_w) % stride_w == rw
 *   dead_classes  classes no tap reaches: their pixels are stored as +0 without a matrix instruction
 *   tap_steps     sum over the classes of the taps a class walks; every tap belongs to exactly one class, so this is KH * KW
 */
enum {
  LSQ_CONV_DGRAD_NARROW = 1,
  LSQ_CONV_DGRAD_WIDE = 2,
  LSQ_CONV_DGRAD_PATCH = 4
};

typedef struct lsq_conv_dgrad_plan {
  int32_t kernel;
  int32_t classes;
  int32_t dead_classes;
  int32_t tap_steps;
} lsq_conv_dgrad_plan;

/* Host code only: no device call.  0 and *plan filled, or the negative code lsq_signw_conv2d_dgrad returns for g
 * (LSQ_E_NULL: g or plan is NULL). */
int lsq_signw_conv2d_dgrad_plan(const lsq_conv_geom* g, lsq_conv_dgrad_plan* plan);

/*
 * Input gradient of the convolution: fp32 output gradients x sign-weight planes, the sum running over the OUTPUT channels
 * and the taps (grad_xq = conv2d_input(x.shape, w_q, grad_y, stride, padding, dilation, groups) for w_q = sum_q ws_q s_q),
 * on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16):
 *   grad_xq[n][c][h][w] = sum_q sum_{o in group(c)} sum_{(i,j)} fl32(grad_y[n][o][ho][wo] * ws[q][o]) * s_q[o][c'][i][j]
 * over the taps with h + pad_h - i dil_h = ho stride_h, 0 <= ho < Ho (and likewise for the columns), s_q the +-1 signs of
 * weight plane q and c' = c - group(c) C / groups.
 *   grad_y      [N][O][Ho][Wo] fp32, contiguous, any 4-byte-aligned address
 *   wbits       the planes lsq_pack_weight writes for g: words [q][tap][ceil(C / groups / 64)][groups * ceil16(O / groups)]
 *   wscales     [kw_planes][O] fp32
 *   g           the FORWARD geometry
 *   grad_xq     out, [N][C][H][W] fp32; EVERY element is written (those no tap reaches get +0) and nothing outside it
 *   workspace   at least lsq_signw_conv2d_dgrad_workspace_bytes(g, kw_planes) bytes, 8-byte aligned, any content; rewritten
 *               by every call (LSQ_E_WORKSPACE if it is NULL, misaligned or too small)
 * Where the sign bits come from: a word of the forward's planes holds 64 CHANNELS of one out-channel, while k runs over
 * the out-channels here.  A first kernel of the call writes the transposed image
 *   T[q][tap][group][ceil(O / groups / 64)][ceil16(C / groups)],  bit j of word (q, tap, grp, w, c') = sign of
 *   weight (o = grp O / groups + 64 w + j, c', tap)
 * into `workspace` (one wave per 64 x 64 bit block, 64 ballots, no LDS); lsq_signw_conv2d_dgrad_workspace_bytes is its size
 * (0 for a geometry or plane count the call refuses).  After it a lane's sign fragment is 8 consecutive bits of ONE word,
 * as in the forward kernels.  The weight stream stays at one bit per weight.
 * Stride without zero insertion: the input pixels are split into the stride_h * stride_w classes of the plan.  A workgroup
 * owns 128 pixels of ONE class and walks only that class's taps, so over all classes every (pixel tile, tap) pair is
 * walked once; a class without a tap stores zeros.  In class coordinates (h = h0 + stride_h ah) tap i is the pure shift
 * ho = ah + (h0 + pad_h - i dil_h) / stride_h, which is what lets the patch kernel stage one patch for all taps.
 * Accuracy: the per-(plane, o) scale sits on the summed index, so it is multiplied INTO the gradient, a = fl32(gy * ws),
 * which is split a = hi + lo with hi = bf16(a), lo = bf16(a - hi): |a - hi - lo| <= 2^-18 |a| under round-to-nearest
 * (half an ulp of 8 significant bits, twice).  The signs are exact +-1, every product hi * s and lo * s is exact, and the
 * products of ALL planes and taps are summed into one fp32 accumulator.  With the rounding of a itself,
 *   |grad_xq - exact| <= (2^-18 + 2^-24) sum |gy ws|  plus the fp32 rounding of the accumulation.
 * Out-channel slots o >= O / groups (zero words in the planes, which would read as -1) enter as a = 0; taps that fall
 * outside grad_y enter as a = 0; channels c' >= C / groups are computed and never stored.
 * Summation order (fixed by g and kw_planes alone: bitwise deterministic, no atomics): one fp32 MFMA accumulator per
 * output element, four steps of 16 out-channels per (tap, word of 64 out-channels, plane), the hi products of a step before
 * its lo products;
 *   patch kernel:   words of 64 out-channels in order; within a word the planes q = 0 .. kw_planes - 1; within a plane the
 *                   class's taps in (i, j) order;
 *   gather kernel:  the class's taps in (i, j) order; within a tap the words in order; within a word the planes in order.
 * LSQ_E_NULL: a NULL operand or g.  LSQ_E_SHAPE: what check_geom of lsq_hip.h refuses, or an empty output (Ho or Wo < 1).
 * LSQ_E_UNSUPPORTED: kw_planes outside 1 .. LSQ_MAX_PLANES; N C H W or N O Ho Wo >= 2^31; more than 65535 classes; more
 * than 65535 channel tiles (groups * ceil(C / groups / 64), or / 128 on the wide kernel); 2^28 or more words in the
 * transposed image of one plane.
 */
size_t lsq_signw_conv2d_dgrad_workspace_bytes(const lsq_conv_geom* g, int kw_planes);

int lsq_signw_conv2d_dgrad(const float* grad_y, const uint64_t* wbits, int kw_planes, const float* wscales,
                           const lsq_conv_geom* g, float* grad_xq, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_CONV_TRAIN_H_ */
