/*
 * lsq_hip_conv_chain.h -- C ABI of lsq_xnor_conv2d_chain_fixed (liblsq_hip_conv_chain.so): lsq_xnor_conv2d with the NEXT
 * layer's activation quantizer in its epilogue, for consumers whose scales are GIVEN (moving-average inference: what
 * lsq_act_quant takes as `forced`).  With given scales a quantizer is an element-wise function of the tensor the convolution
 * has in registers -- sign bits of a chain of compares and adds --, so the lsq_act_quant launch between two quantized
 * convolutions and its read of y disappear; there is no sum, no atomic and nothing the caller must zero but the halo.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller, `stream` is a hipStream_t passed as void*
 * (NULL = default stream), every function returns 0, a negative LSQ_E_* code for an argument error (returned before any
 * launch, nothing written), or a positive hipError_t if a launch failed.
 *
 * The entry point is a library of its own because the function list of lsq_hip.h is fixed at ABI version 12; the kernel is
 * the XNOR matrix-core kernel of liblsq_hip.so (csrc/lsq_xnor_mfma.hip, its NQF instantiations), which this library links:
 * both must come from the same build and sit in the same directory.
 */
#ifndef LSQ_HIP_CONV_CHAIN_H_
#define LSQ_HIP_CONV_CHAIN_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_CONV_CHAIN_ABI_VERSION 1

int lsq_conv_chain_abi_version(void);

/*
 * Where the convolution leaves the next layer's input and how it quantizes it.  With t = clamp(fmaf(y, pre_scale[o],
 * pre_shift[o])) (no fmaf without pre_scale, no clamp with a negative clamp_alpha), plane p holds the bits
 *   bit_p = (t - result_p) >= 0     (-0.0 gives 1),     result_0 = 0,  result_{p+1} = result_p + (bit_p ? v_p : -v_p),
 * all in fp32 with v_p = scales[p * N + n]: the result chain of lsq_act_quant, whose planes these are bit for bit
 * (lsq_act_quant(y, scheme, k, forced = scales, pre_scale, pre_shift, clamp_alpha) for LS1 at k = 1, LS2 / LST at k = 2 and
 * GF at any k: with given scales the planes depend on k alone).
 */
typedef struct lsq_next_fixed {
  uint64_t* planes;       /* [k] planes of the NEXT layer, [N][O/64][Ho+2pad_h][Wo+2pad_w] each; halo zeroed by the caller */
  int32_t k;              /* 1..LSQ_MAX_PLANES */
  const float* scales;    /* [k][N] fp32, device */
  const float* pre_scale; /* [O] or NULL (both or neither): folded batch norm in front of the next quantizer */
  const float* pre_shift;
  float clamp_alpha;      /* > 0, or negative for clamp identity */
  int32_t pad_h, pad_w;   /* the next layer's padding */
} lsq_next_fixed;

/*
 * y = act(conv + bias + res_pre) + res_post exactly as lsq_xnor_conv2d computes it on the same operands (xplanes [kx] planes,
 * xscales [kx][N], ...), and every interior word of next->planes written in the same launch; the halo is left alone.
 *
 * LSQ_E_NULL: next, next->planes or next->scales is NULL; only one of pre_scale / pre_shift (or what lsq_xnor_conv2d refuses).
 * LSQ_E_SCHEME: next->k outside 1..LSQ_MAX_PLANES; kx outside 1..2.
 * LSQ_E_UNSUPPORTED: a geometry outside the fp4 matrix-core kernel (3x3 taps, groups 1, 64 / 128 / 256 / 512 input channels,
 *   fewer than 2^30 outputs); O not a multiple of 64; a negative pad; 2^30 or more dwords in one of the next planes.  The
 *   caller then runs lsq_xnor_conv2d + lsq_act_quant: same bits.
 * A refused call launches nothing and writes nothing.
 */
int lsq_xnor_conv2d_chain_fixed(const uint64_t* xplanes, int kx, const float* xscales, const uint64_t* wbits,
                                const int32_t* wsum, int kw_planes, const float* wscales, const float* bias,
                                const lsq_conv_geom* g, int act, const float* act_slope, const float* res_pre,
                                const float* res_post, const lsq_next_fixed* next, float* y, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_CONV_CHAIN_H_ */
