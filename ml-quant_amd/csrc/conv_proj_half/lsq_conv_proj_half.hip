// liblsq_hip_conv_proj_half.so: the C entry points of the projection shortcut on 16-bit tensors
// (include/lsq_hip_conv_proj_half.h).  No kernel of its own: the __bf16 / _Float16 instantiations of csrc/lsq_pointwise.hip and
// of the PROJ kernels of csrc/lsq_xnor_mfma.hip and the argument checks of csrc/lsq_xnor_conv.hip live in liblsq_hip.so, whose
// header's function list is fixed; this library links it and forwards.

#include "lsq_hip_conv_proj_half.h"

namespace lsq {
int pointwise_conv_half(const void* x, int dtype, int N, int C, int H, int W, const float* w, const float* bias, int O,
                        int stride, void* y, void* stream);
int xnor_conv2d_proj_half(const uint64_t* xplanes, int kx, const float* xscales, const uint64_t* wbits, const int32_t* wsum,
                          int kw_planes, const float* wscales, const float* bias, const lsq_conv_geom* g, int act,
                          const float* act_slope, const void* res_pre, const void* res_post, const lsq_proj_half* proj, int dtype,
                          void* y, void* stream);
}

extern "C" int lsq_conv_proj_half_abi_version(void) { return LSQ_CONV_PROJ_HALF_ABI_VERSION; }

extern "C" int lsq_pointwise_conv_half(const void* x, int dtype, int N, int C, int H, int W, const float* w, const float* bias,
                                       int O, int stride, void* y, void* stream) {
  return lsq::pointwise_conv_half(x, dtype, N, C, H, W, w, bias, O, stride, y, stream);
}

extern "C" int lsq_xnor_conv2d_proj_half(const uint64_t* xplanes, int kx, const float* xscales, const uint64_t* wbits,
                                         const int32_t* wsum, int kw_planes, const float* wscales, const float* bias,
                                         const lsq_conv_geom* g, int act, const float* act_slope, const void* res_pre,
                                         const void* res_post, const lsq_proj_half* proj, int dtype, void* y, void* stream) {
  return lsq::xnor_conv2d_proj_half(xplanes, kx, xscales, wbits, wsum, kw_planes, wscales, bias, g, act, act_slope, res_pre,
                                    res_post, proj, dtype, y, stream);
}
