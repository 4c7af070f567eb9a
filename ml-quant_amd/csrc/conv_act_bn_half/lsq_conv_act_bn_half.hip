// lsq_act_quant_bn_half: lsq_act_quant_half on t = round_to_dtype(x * pre_scale[c] + pre_shift[c]) without t in memory -- the
// eval batch norm in front of a 16-bit quantizer folded into the quantizer's read.  The kernels are
// conv_act_half/lsq_conv_act_half_core.h's: BN = true with the two arrays, BN = false (the statements of lsq_act_quant_half)
// when both are NULL.

#include "lsq_hip_conv_act_bn_half.h"
#include "../conv_act_half/lsq_conv_act_half_core.h"

extern "C" int lsq_conv_act_bn_half_abi_version(void) { return LSQ_CONV_ACT_BN_HALF_ABI_VERSION; }

extern "C" int lsq_act_quant_bn_half(const void* x, int x_dtype, const lsq_conv_geom* g, int scheme, int k, int skip,
                                     float clamp_alpha, const float* pre_scale, const float* pre_shift, const float* forced,
                                     uint64_t* planes, float* scales, int32_t* status, void* stream) {
  if ((pre_scale == nullptr) != (pre_shift == nullptr)) return LSQ_E_NULL;
  if (!pre_scale)
    return act_quant_rows<false>(x, x_dtype, g, scheme, k, skip, clamp_alpha, nullptr, nullptr, forced, planes, scales, status,
                                 stream);
  return act_quant_rows<true>(x, x_dtype, g, scheme, k, skip, clamp_alpha, pre_scale, pre_shift, forced, planes, scales, status,
                              stream);
}
