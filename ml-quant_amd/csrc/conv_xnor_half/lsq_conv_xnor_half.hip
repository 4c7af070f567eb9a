// liblsq_hip_conv_xnor_half.so: the C entry points of the XNOR convolution with a 16-bit epilogue
// (include/lsq_hip_conv_xnor_half.h).  No kernel of its own: the __bf16 / _Float16 instantiations of csrc/lsq_xnor_mfma.hip
// and csrc/lsq_xnor_conv.hip and the argument checks of the latter live in liblsq_hip.so, whose header's function list is
// fixed; this library links it and forwards.

#include "lsq_hip_conv_xnor_half.h"

namespace lsq {
int xnor_conv2d_half(const uint64_t* xplanes, int kx, const float* xscales, const uint64_t* wbits, const int32_t* wsum,
                     int kw_planes, const float* wscales, const float* bias, const lsq_conv_geom* g, int act,
                     const float* act_slope, const void* res_pre, const void* res_post, int dtype, void* y, void* workspace,
                     size_t workspace_bytes, void* stream);
size_t xnor_conv2d_half_workspace_bytes(const lsq_conv_geom* g, int kx, int kw_planes);
}

extern "C" int lsq_conv_xnor_half_abi_version(void) { return LSQ_CONV_XNOR_HALF_ABI_VERSION; }

extern "C" size_t lsq_xnor_conv2d_half_workspace_bytes(const lsq_conv_geom* g, int kx, int kw_planes) {
  return lsq::xnor_conv2d_half_workspace_bytes(g, kx, kw_planes);
}

extern "C" int lsq_xnor_conv2d_half(const uint64_t* xplanes, int kx, const float* xscales, const uint64_t* wbits,
                                    const int32_t* wsum, int kw_planes, const float* wscales, const float* bias,
                                    const lsq_conv_geom* g, int act, const float* act_slope, const void* res_pre,
                                    const void* res_post, int dtype, void* y, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  return lsq::xnor_conv2d_half(xplanes, kx, xscales, wbits, wsum, kw_planes, wscales, bias, g, act, act_slope, res_pre,
                               res_post, dtype, y, workspace, workspace_bytes, stream);
}
