// liblsq_hip_linear_wgrad_half.so: lsq_linear_signx_wgrad_half, the weight gradient of QuantLinear's 16-bit train step in one
// call -- the kernels of ../linear_wgrad/lsq_linear_wgrad_core.h instantiated on bf16 / fp16 gradients and inputs (each
// converted exactly to fp32 as it is read; from there sign image, tile rule, stages, the hi + lo split and the order of
// summation are lsq_linear_signx_wgrad's) with the plain fp32 store, or with an epilogue that takes the fp32 accumulator
// through the straight-through estimator of the weight quantizer against the layer's fp32 weight.  A lane of the epilogue holds
// one column f and 16 rows o of a 32 x 32 block: it reads w[o F + f] and stores out[o F + f] as single 4-byte elements (a
// half-wave's 32 lanes are 128 consecutive bytes of a row); the kw scales of row o are fetched once per row.

#include "lsq_hip_linear_wgrad_half.h"
#include "../linear_wgrad/lsq_linear_wgrad_core.h"
#include "../lsq_ste_one.h"           // ste_one, kMaxK: the straight-through estimator of ../lsq_ste.hip

namespace {

// The straight-through store: out[i] = ste_one(w[i], acc, wscales[.][o], kw, no clamp).
struct EpiSte {
  float* out;                         // [O][F]
  const float* w;                     // [O][F]
  const float* ws;                    // [kw][O]
  int kw, O;
  struct Row {
    float v[kMaxK];
  };
  __device__ __forceinline__ void row(int o, Row& r) const {
#pragma unroll
    for (int i = 0; i < kMaxK; ++i) r.v[i] = i < kw ? ws[(long long)i * O + o] : 0.f;
  }
  __device__ __forceinline__ float operand(long long i) const { return w[i]; }
  __device__ __forceinline__ void store(long long i, const Row& r, float acc, float wv) const {
    out[i] = ste_one(wv, acc, r.v, kw, -1.f);
  }
};

template <class T>
int run(const void* gy, const void* x, int kx, const float* xscales, float clamp_alpha, int64_t N, int64_t Tt, int64_t F,
        int64_t O, const float* w, int kw, const float* wscales, float* out, void* workspace, hipStream_t st) {
  const T* g = static_cast<const T*>(gy);
  const T* xv = static_cast<const T*>(x);
  if (!w) {
    const EpiStore epi = {out};
    return launch_wgrad(g, xv, kx, xscales, clamp_alpha, N, Tt, F, O, epi, workspace, st);
  }
  const EpiSte epi = {out, w, wscales, kw, (int)O};
  return launch_wgrad(g, xv, kx, xscales, clamp_alpha, N, Tt, F, O, epi, workspace, st);
}

}  // namespace

extern "C" int lsq_linear_wgrad_half_abi_version(void) { return LSQ_LINEAR_WGRAD_HALF_ABI_VERSION; }

extern "C" size_t lsq_linear_signx_wgrad_half_workspace_bytes(int kx, int64_t N, int64_t T, int64_t F, int64_t O) {
  return workspace_bytes_of(kx, N, T, F, O);
}

extern "C" int lsq_linear_signx_wgrad_half(const void* gy, const void* x, int dtype, int kx, const float* xscales,
                                           float clamp_alpha, int64_t N, int64_t T, int64_t F, int64_t O, const float* w, int kw,
                                           const float* wscales, float* out, void* workspace, size_t workspace_bytes,
                                           void* stream) {
  if (!gy || !x || !xscales || !out) return LSQ_E_NULL;
  if (w && !wscales) return LSQ_E_NULL;
  if (N <= 0 || T <= 0 || F <= 0 || O <= 0) return LSQ_E_SHAPE;
  if (dtype != LSQ_DTYPE_BF16 && dtype != LSQ_DTYPE_F16) return LSQ_E_UNSUPPORTED;
  if (w && (kw < 1 || kw > LSQ_MAX_PLANES)) return LSQ_E_UNSUPPORTED;
  if (int e = check_call(kx, N, T, F, O, workspace, workspace_bytes)) return e;
  if (((uintptr_t)gy & 1) || ((uintptr_t)x & 1) || ((uintptr_t)out & 3)) return LSQ_E_UNSUPPORTED;
  if (w && (((uintptr_t)w & 3) || ((uintptr_t)wscales & 3))) return LSQ_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == LSQ_DTYPE_BF16)
    return run<__bf16>(gy, x, kx, xscales, clamp_alpha, N, T, F, O, w, kw, wscales, out, workspace, st);
  return run<_Float16>(gy, x, kx, xscales, clamp_alpha, N, T, F, O, w, kw, wscales, out, workspace, st);
}
