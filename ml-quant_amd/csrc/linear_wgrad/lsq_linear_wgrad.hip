// liblsq_hip_linear_wgrad.so: lsq_linear_signx_wgrad, fp32 gradient rows (transposed) x the sign planes of the quantized input
// with the sum over the ROWS, on the bf16 matrix cores of gfx950 (v_mfma_f32_32x32x16_bf16) -- the weight gradient of
// QuantLinear with binary activations.
// The kernels and the host logic live in lsq_linear_wgrad_core.h, shared with liblsq_hip_linear_wgrad_half.so; this library
// instantiates them on fp32 operands with the plain fp32 store.

#include "lsq_hip_linear_wgrad.h"
#include "lsq_linear_wgrad_core.h"

extern "C" int lsq_linear_wgrad_abi_version(void) { return LSQ_LINEAR_WGRAD_ABI_VERSION; }

extern "C" size_t lsq_linear_signx_wgrad_workspace_bytes(int kx, int64_t N, int64_t T, int64_t F, int64_t O) {
  return workspace_bytes_of(kx, N, T, F, O);
}

extern "C" int lsq_linear_signx_wgrad(const float* gy, const float* x, int kx, const float* xscales, float clamp_alpha,
                                      int64_t N, int64_t T, int64_t F, int64_t O, float* gwq, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  if (!gy || !x || !xscales || !gwq) return LSQ_E_NULL;
  if (int e = check_call(kx, N, T, F, O, workspace, workspace_bytes)) return e;
  const EpiStore epi = {gwq};
  return launch_wgrad(gy, x, kx, xscales, clamp_alpha, N, T, F, O, epi, workspace, (hipStream_t)stream);
}
