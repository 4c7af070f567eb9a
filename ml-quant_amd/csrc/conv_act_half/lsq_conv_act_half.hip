// lsq_act_quant_half: sign planes and per-sample scales of a bf16 / fp16 NCHW batch in the convolution's plane layout -- the
// activation operand of lsq_xnor_conv2d from a 16-bit input, every scheme of lsq_act_quant, in ONE launch.  The kernels are
// lsq_conv_act_half_core.h's with BN = false (described there); conv_act_bn_half/lsq_conv_act_bn_half.hip instantiates the
// same source with the folded batch norm in the read.

#include "lsq_hip_conv_act_half.h"
#include "lsq_conv_act_half_core.h"

extern "C" int lsq_conv_act_half_abi_version(void) { return LSQ_CONV_ACT_HALF_ABI_VERSION; }

extern "C" int lsq_act_quant_half(const void* x, int x_dtype, const lsq_conv_geom* g, int scheme, int k, int skip,
                                  float clamp_alpha, const float* forced, uint64_t* planes, float* scales, int32_t* status,
                                  void* stream) {
  return act_quant_rows<false>(x, x_dtype, g, scheme, k, skip, clamp_alpha, nullptr, nullptr, forced, planes, scales, status,
                               stream);
}
