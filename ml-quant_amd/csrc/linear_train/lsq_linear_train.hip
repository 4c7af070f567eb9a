// liblsq_hip_linear_train.so: lsq_linear_signw_dgrad, the input gradient of QuantLinear -- the kernels of lsq_linear_dgrad.h
// (there: the GEMM, the transposed plane image, the two kernels) instantiated on fp32 gradients with plain fp32 stores.

#include "lsq_hip_linear_train.h"
#include "lsq_linear_dgrad.h"

extern "C" int lsq_linear_train_abi_version(void) { return LSQ_LINEAR_TRAIN_ABI_VERSION; }

extern "C" size_t lsq_linear_signw_dgrad_workspace_bytes(int kw_planes, int64_t F, int64_t O) {
  return workspace_bytes_of(kw_planes, F, O);
}

extern "C" int lsq_linear_signw_dgrad(const float* gy, const uint64_t* wbits, int kw_planes, const float* wscales,
                                      int64_t M, int64_t F, int64_t O, float* gx, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  if (!gy || !wbits || !wscales || !gx) return LSQ_E_NULL;
  if (int e = check_call(kw_planes, M, F, O, workspace, workspace_bytes)) return e;
  return launch_dgrad(gy, wbits, kw_planes, wscales, M, F, O, EpiStore{gx}, workspace, (hipStream_t)stream);
}
