// liblsq_hip_conv_proj.so: the C entry point of the XNOR convolution with the projection shortcut folded in
// (include/lsq_hip_conv_proj.h).  No kernel of its own: the PROJ instantiations of csrc/lsq_xnor_mfma.hip and the argument
// checks of csrc/lsq_xnor_conv.hip live in liblsq_hip.so, whose header's function list is fixed; this library links it and
// forwards.

#include "lsq_hip_conv_proj.h"

namespace lsq {
int xnor_conv2d_proj(const uint64_t* xplanes, int kx, const float* xscales, const uint64_t* wbits, const int32_t* wsum,
                     int kw_planes, const float* wscales, const float* bias, const lsq_conv_geom* g, int act,
                     const float* act_slope, const float* res_pre, const float* res_post, const lsq_proj* proj, float* y,
                     void* stream);
}

extern "C" int lsq_conv_proj_abi_version(void) { return LSQ_CONV_PROJ_ABI_VERSION; }

extern "C" int lsq_xnor_conv2d_proj(const uint64_t* xplanes, int kx, const float* xscales, const uint64_t* wbits,
                                    const int32_t* wsum, int kw_planes, const float* wscales, const float* bias,
                                    const lsq_conv_geom* g, int act, const float* act_slope, const float* res_pre,
                                    const float* res_post, const lsq_proj* proj, float* y, void* stream) {
  return lsq::xnor_conv2d_proj(xplanes, kx, xscales, wbits, wsum, kw_planes, wscales, bias, g, act, act_slope, res_pre,
                               res_post, proj, y, stream);
}
