/*
 * lsq_hip_stem_gen.h -- C ABI of lsq_stem_conv_gen (liblsq_hip_stem_gen.so): the full-precision front convolution of a
 * network for the geometries lsq_stem_conv_pool (7x7 / 2 from 3 to 64 channels + 3x3 / 2 pool) does not take -- the
 * CIFAR stem (3x3 / 1, no pool), LeNet's conv1 (1 -> 20 channels, 5x5, ReLU, batch norm, 2x2 pool) and their kin:
 *
 *   y = pool( post( relu( conv2d(x, w, stride, pad) + bias ) ) ),   NCHW fp32 in and out, ONE launch.
 *
 * The kernel (csrc/stem_gen/lsq_stem_gen.hip) is an implicit GEMM on the bf16 matrix cores with every fp32 operand split
 * into three bf16 terms (six passes hh + (hm + mh) + (hl + lh + mm), fp32 accumulation: fp32-class accuracy for any finite
 * operand; there is no other mode and no overflow flag).
 *
 * Work split (the rule lsq_stem_conv_gen launches by):
 *   * out-channels go in tiles of 32 (the last one padded with zero weight rows, its stores masked); a workgroup holds
 *     T of the ceil(O / 32) tiles: the tiles are spread evenly over the fewest groups of at most 4 tiles whose split
 *     weights (T * ceil(C KH / 2) * 3 KB) leave room for the smallest input patch in 64 KB of LDS;
 *   * a workgroup (256 threads) owns one image, one strip of R conv rows (R even) and its group of tiles, and walks the
 *     strip in chunks of 32 conv columns; a wave's unit of work is (one tile, two conv rows of the strip);
 *   * R starts at the smallest even height that gives the four waves a unit each (2 ceil(4 / T)), is cut down to what fits
 *     LDS and to the conv height rounded up to even, and is then doubled (up to 16) for as long as the grid
 *     N * ceil(Hc / R) * groups keeps at least 512 workgroups (two per CU) and the patch still fits.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller, `stream` is a hipStream_t passed as void*
 * (NULL = default stream), every function returns 0, a negative LSQ_E_* code for an argument error (returned before any
 * launch, nothing written), or a positive hipError_t if the launch failed.  The library allocates nothing and keeps no
 * state: a call can be captured in a HIP graph.  It links nothing of liblsq_hip.so.
 */
#ifndef LSQ_HIP_STEM_GEN_H_
#define LSQ_HIP_STEM_GEN_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_STEM_GEN_ABI_VERSION 1

int lsq_stem_gen_abi_version(void);

/*
 * Host only, no launch: 1 where lsq_stem_conv_gen takes (g, pool), else 0.  It takes
 *   groups == 1, dilation 1;  1 <= C <= 4;  KH, KW <= 7;  stride_h == stride_w in {1, 2};  pad < kernel per axis;
 *   1 <= O <= 256 (any O: 20 is fine);  pool 1 (none) or 2 (2x2 / 2 max-pool, pad 0, floor mode);
 *   a conv output of at least pool x pool;  x, w and the conv output below 2^31 elements each.
 */
int lsq_stem_conv_gen_supported(const lsq_conv_geom* g, int pool);

/*
 * x [N][C][H][W], w [O][C][KH][KW], y [N][O][Hc / pool][Wc / pool] with (Hc, Wc) the convolution's output size.
 * bias: NULL or [O].  relu: 0 / 1.  post_scale, post_shift: both NULL or both [O]: v -> fmaf(v, post_scale[o],
 * post_shift[o]) behind the ReLU and in front of the max (an eval-mode batch norm folded by the caller; a negative scale
 * is handled correctly).
 *
 * LSQ_E_NULL: x, w, y or g is NULL; one of post_scale / post_shift without the other.  LSQ_E_SHAPE: what check_geom
 * refuses (a non-positive size, channels not divisible by groups).  LSQ_E_SCHEME: relu other than 0 / 1.
 * LSQ_E_UNSUPPORTED: whatever lsq_stem_conv_gen_supported answers 0 for otherwise.  A refused call launches nothing and
 * writes nothing.
 */
int lsq_stem_conv_gen(const float* x, const float* w, const float* bias, const lsq_conv_geom* g, int relu,
                      const float* post_scale, const float* post_shift, int pool, float* y, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_STEM_GEN_H_ */
