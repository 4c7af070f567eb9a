// liblsq_hip_linear_train_half.so: lsq_linear_signw_dgrad_half, the input gradient of QuantLinear's 16-bit train step in one
// pass -- the kernels of ../linear_train/lsq_linear_dgrad.h instantiated on bf16 / fp16 gradients (each converted exactly to
// fp32 as it is read; from there tile rule, stages, the hi + lo split and the order of summation are lsq_linear_signw_dgrad's)
// with an epilogue that takes the fp32 accumulator through the straight-through estimator against the 16-bit input of the
// step and rounds the result once into the type.  A lane of the epilogue holds one column f and 16 rows of a 32 x 32 block:
// it reads x[m F + f] and stores gx[m F + f] as single elements (with odd F two rows share a dword), so any 2-byte-aligned
// address serves; the kx scales of sample m / T are fetched again only where the lane's rows reach another sample.

#include "lsq_hip_linear_train_half.h"
#include "../linear_train/lsq_linear_dgrad.h"
#include "../lsq_ste_one.h"           // ste_one, kMaxK: the straight-through estimator of ../lsq_ste.hip

namespace {

// The epilogue: x given -> ste_one against the step's input with the sample's scales; then fp32 or one rounding into T.
template <class T>
struct EpiSte {
  void* gx;                           // [M][F] of T, or of float (f32out)
  const T* x;                         // [M][F], or null: the accumulators as they are
  const float* xs;                    // [kx][N]
  int kx, N, rows;                    // rows = rows per sample
  float alpha;                        // the clamp bound in T's values, < 0: none
  int f32out;
  struct Row {
    float v[kMaxK];
  };
  __device__ __forceinline__ int sample(long long m) const { return x ? (int)((unsigned)m / (unsigned)rows) : 0; }
  __device__ __forceinline__ void row(int n, Row& r) const {
#pragma unroll
    for (int i = 0; i < kMaxK; ++i) r.v[i] = (x && i < kx) ? xs[(long long)i * N + n] : 0.f;
  }
  __device__ __forceinline__ void store(long long i, const Row& r, float acc) const {
    const float o = x ? ste_one((float)x[i], acc, r.v, kx, alpha) : acc;
    if (f32out) static_cast<float*>(gx)[i] = o;
    else static_cast<T*>(gx)[i] = (T)o;             // round to nearest even, one 2-byte store
  }
};

template <class T>
int run(const void* gy, const uint64_t* wbits, int kw_planes, const float* wscales, int64_t M, int64_t F, int64_t O,
        const void* x, int64_t rows, int kx, const float* xscales, float clamp_alpha, void* gx, int f32out, void* workspace,
        hipStream_t st) {
  EpiSte<T> epi = {gx, static_cast<const T*>(x), xscales, kx, x ? (int)(M / rows) : 1, x ? (int)rows : 1, clamp_alpha, f32out};
  return launch_dgrad(static_cast<const T*>(gy), wbits, kw_planes, wscales, M, F, O, epi, workspace, st);
}

}  // namespace

extern "C" int lsq_linear_train_half_abi_version(void) { return LSQ_LINEAR_TRAIN_HALF_ABI_VERSION; }

extern "C" size_t lsq_linear_signw_dgrad_half_workspace_bytes(int kw_planes, int64_t F, int64_t O) {
  return workspace_bytes_of(kw_planes, F, O);
}

extern "C" int lsq_linear_signw_dgrad_half(const void* gy, int gy_dtype, const uint64_t* wbits, int kw_planes,
                                           const float* wscales, int64_t M, int64_t F, int64_t O, const void* x, int64_t T,
                                           int kx, const float* xscales, float clamp_alpha, void* gx, int gx_dtype,
                                           void* workspace, size_t workspace_bytes, void* stream) {
  if (!gy || !wbits || !wscales || !gx) return LSQ_E_NULL;
  if (x && kx > 0 && !xscales) return LSQ_E_NULL;
  if (M <= 0 || F <= 0 || O <= 0) return LSQ_E_SHAPE;
  if (x && (T <= 0 || M % T != 0)) return LSQ_E_SHAPE;
  if (gy_dtype != LSQ_DTYPE_BF16 && gy_dtype != LSQ_DTYPE_F16) return LSQ_E_UNSUPPORTED;
  if (gx_dtype != LSQ_DTYPE_F32 && gx_dtype != gy_dtype) return LSQ_E_UNSUPPORTED;
  if (kx < 0 || kx > LSQ_MAX_PLANES) return LSQ_E_UNSUPPORTED;
  if (int e = check_call(kw_planes, M, F, O, workspace, workspace_bytes)) return e;
  if (x && M / T > 65535) return LSQ_E_UNSUPPORTED;   // (the limit of lsq_ste_backward, whose result this call states)
  if (((uintptr_t)gy & 1) || ((uintptr_t)x & 1) || ((uintptr_t)gx & (gx_dtype == LSQ_DTYPE_F32 ? 3 : 1)))
    return LSQ_E_UNSUPPORTED;
  const int f32out = gx_dtype == LSQ_DTYPE_F32;
  hipStream_t st = (hipStream_t)stream;
  if (gy_dtype == LSQ_DTYPE_BF16)
    return run<__bf16>(gy, wbits, kw_planes, wscales, M, F, O, x, T, kx, xscales, clamp_alpha, gx, f32out, workspace, st);
  return run<_Float16>(gy, wbits, kw_planes, wscales, M, F, O, x, T, kx, xscales, clamp_alpha, gx, f32out, workspace, st);
}
