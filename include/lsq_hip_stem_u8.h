/*
 * lsq_hip_stem_u8.h -- C ABI of lsq_stem_conv_u8 (liblsq_hip_stem_u8.so): the front convolution of a network on the uint8
 * pixels an image pipeline delivers, planar or interleaved, with the input normalisation inside:
 *
 *   y = pool( post( relu( conv2d( x_u8 * in_scale[c] + in_shift[c], w, stride, pad ) + bias ) ) ),   fp32 NCHW out, ONE launch.
 *
 * Zero padding applies to the NORMALISED image: a padded pixel contributes 0, not in_shift.
 *
 * The kernel (csrc/stem_u8/lsq_stem_u8.hip) is an implicit GEMM on the bf16 matrix cores.  A byte is exact in one bf16, so
 * the activation side is ONE term; in_scale is folded into the weights (one fp32 product) and the scaled weights are split
 * into three bf16 terms (all 24 bits: any finite weight, no overflow flag): three MFMA passes, fp32 accumulation, every
 * product exact.  in_shift is served by a synthetic input channel that is 1 inside the image and 0 in the padding, with the
 * weights sum_c w[o][c][kh][kw] * in_shift[c] (fp32, c ascending); with in_shift == 0 for every c it is left out.
 *
 * Work split (the rule lsq_stem_conv_u8 launches by):
 *   * out-channels go in tiles of 32 (the last one padded with zero weight rows, its stores masked); a workgroup holds
 *     T of the ceil(O / 32) tiles: the tiles are spread evenly over the fewest groups of at most 4 tiles whose split
 *     weights (T * ceil((C + 1) KH / 2) * 3 KB) leave room for the smallest input patch in 64 KB of LDS;
 *   * a workgroup (256 threads) owns one image, one strip of R conv rows (R even) and its group of tiles, and walks the
 *     strip in chunks of 32 conv columns -- 30 for pool 3, whose windows overlap: lane 0 holds the column left of the
 *     chunk, fifteen pooled columns come out of a chunk and two of 32 conv columns are computed twice (6.7 %);
 *   * a wave's unit of work is (one tile, L consecutive pairs of conv rows).  Pool 1 and 2: L = 1.  Pool 3: the pooled row p
 *     is the max over the conv rows 2 p - 1, 2 p, 2 p + 1, so a unit first computes the conv row above its first pair
 *     alone and carries it in registers from pair to pair: 2 L + 1 conv rows for L pooled rows; L = ceil(R / 2 / waves per
 *     tile), waves per tile = max(1, 4 / T) (the ImageNet stem: R = 14, L = 2, five conv rows per four owned: 25 %);
 *   * R starts at the smallest height that gives the four waves a unit each (2 max(1, 4 / T); twice that for pool 3), is cut
 *     down to what fits LDS and to the conv height rounded up to even, and is then doubled (up to 32) for as long as the
 *     grid N * ceil(Hc / R) * groups keeps at least 512 workgroups (two per CU) and the patch still fits.
 * LDS: [A fragments T * steps * 3 KB][patch (C + 1) * IR * ICd * 4 B, IR = (R + (pool == 3) - 1) stride + KH, ICd = 20 dwords at
 * stride 1, 36 at stride 2][row offsets 128 B][bias, post scale, post shift 384 T B].  Bias, ReLU, the affine and every pooling
 * maximum stay in registers and cross-lane operations.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller, `stream` is a hipStream_t passed as void*
 * (NULL = default stream), every function returns 0, a negative LSQ_E_* code for an argument error (returned before any
 * launch, nothing written), or a positive hipError_t if the launch failed.  The library allocates nothing, keeps no state
 * and uses no atomics: a call can be captured in a HIP graph.  It links nothing of liblsq_hip.so.
 */
#ifndef LSQ_HIP_STEM_U8_H_
#define LSQ_HIP_STEM_U8_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_STEM_U8_ABI_VERSION 1

int lsq_stem_u8_abi_version(void);

/*
 * Host only, no launch: 1 where lsq_stem_conv_u8 takes (g, pool, layout), else 0.  It takes
 *   groups == 1, dilation 1;  1 <= C <= 3;  KH, KW <= 7;  stride_h == stride_w in {1, 2};  pad < kernel per axis;
 *   1 <= O <= 256 (any O);  pool 1 (none), 2 (2x2 / 2 max-pool, pad 0, floor mode) or 3 (3x3 / 2, pad 1, floor mode: a
 *   padded position never wins the max);  a conv output of at least pool x pool;  x and the conv output below 2^31
 *   elements each;  layout 0 (x is [N][C][H][W]) or 1 (channels-last: [N][H][W][C] in memory).
 */
int lsq_stem_conv_u8_supported(const lsq_conv_geom* g, int pool, int layout);

/*
 * x: uint8, logical shape [N][C][H][W] in the memory order `layout` names (any byte alignment).  w [O][C][KH][KW] fp32.
 * in_scale, in_shift: fp32 [C] (ImageNet: 1 / (255 std_c) and -mean_c / std_c).  bias: NULL or [O].  relu: 0 / 1.
 * post_scale, post_shift: both NULL or both [O]: v -> fmaf(v, post_scale[o], post_shift[o]) behind the ReLU and in front
 * of the max (a negative scale is handled correctly).  y: fp32 [N][O][Ho][Wo]; with (Hc, Wc) the convolution's output size,
 * (Ho, Wo) = (Hc, Wc) / pool for pool 1 and 2 and ((Hc - 1) / 2 + 1, (Wc - 1) / 2 + 1) for pool 3.
 *
 * LSQ_E_NULL: x, w, in_scale, in_shift, y or g is NULL; one of post_scale / post_shift without the other.  LSQ_E_SHAPE: what
 * check_geom refuses (a non-positive size, channels not divisible by groups).  LSQ_E_SCHEME: relu other than 0 / 1.
 * LSQ_E_UNSUPPORTED: whatever lsq_stem_conv_u8_supported answers 0 for otherwise, an unknown layout among it.  A refused
 * call launches nothing and writes nothing.
 */
int lsq_stem_conv_u8(const uint8_t* x, int layout, const float* w, const float* bias, const float* in_scale,
                     const float* in_shift, const lsq_conv_geom* g, int relu, const float* post_scale,
                     const float* post_shift, int pool, float* y, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_STEM_U8_H_ */
