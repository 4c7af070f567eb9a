// liblsq_hip_conv_train.so: lsq_signw_conv2d_dgrad, the fp32 instantiation of the input-gradient kernels of lsq_conv_dgrad.h
// (fp32 gradients, the accumulators stored as they are).  Kernels, plan and tile choice: that header.

#include "lsq_conv_dgrad.h"

extern "C" int lsq_conv_train_abi_version(void) { return LSQ_CONV_TRAIN_ABI_VERSION; }

extern "C" int lsq_signw_conv2d_dgrad_plan(const lsq_conv_geom* g, lsq_conv_dgrad_plan* plan) { return plan_of(g, plan); }

extern "C" size_t lsq_signw_conv2d_dgrad_workspace_bytes(const lsq_conv_geom* g, int kw_planes) {
  return workspace_bytes_of(g, kw_planes);
}

extern "C" int lsq_signw_conv2d_dgrad(const float* grad_y, const uint64_t* wbits, int kw_planes, const float* wscales,
                                      const lsq_conv_geom* g, float* grad_xq, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  if (!grad_y || !wbits || !wscales || !g || !grad_xq) return LSQ_E_NULL;
  Shape s;
  if (int e = check_call(g, kw_planes, workspace, workspace_bytes, &s)) return e;
  return launch_dgrad(grad_y, wbits, kw_planes, wscales, g, s, EpiStore{grad_xq}, workspace, (hipStream_t)stream);
}
