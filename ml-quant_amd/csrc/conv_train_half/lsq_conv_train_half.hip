// liblsq_hip_conv_train_half.so: lsq_signw_conv2d_dgrad_half, the input gradient of QuantConv2d's 16-bit train step in one
// pass -- the kernels of ../conv_train/lsq_conv_dgrad.h instantiated on bf16 / fp16 gradients (each converted exactly to fp32
// as it is read; from there plan, tiles, the hi + lo split and the order of summation are lsq_signw_conv2d_dgrad's) with an
// epilogue that takes the fp32 accumulator through the straight-through estimator against the 16-bit input of the step and
// rounds the result once into the type.  Element loads of x and element stores of grad_x are single 2-byte accesses (the
// class-strided pixels of a lane are not neighbours in memory), so any 2-byte-aligned address serves.

#include "lsq_hip_conv_train_half.h"
#include "../conv_train/lsq_conv_dgrad.h"

namespace {

constexpr int kMaxK = LSQ_MAX_PLANES;

// ste_one of ../lsq_ste.hip, restated (this library links none of liblsq_hip.so's objects): the gradient of the quantizer
// chain's value through the straight-through estimator of every sign and the clamp in front.
__device__ __forceinline__ float ste_one(float xv, float gv, const float (&v)[kMaxK], int k, float alpha, bool backward) {
  const bool inside = alpha < 0.f || (xv >= -alpha && xv <= alpha);        // clamp backward: min <= x <= max
  const float xc = lsq::clamp_sym(xv, alpha);
  float r = 0.f;
  float d[kMaxK];
#pragma unroll
  for (int i = 0; i < kMaxK; ++i) {
    if (i < k) {
      d[i] = xc - r;
      r = r + v[i] * (d[i] >= 0.f ? 1.f : -1.f);       // sign(+-0) = +1
    }
  }
  if (!backward) return k == 0 ? xc : r;
  float G = gv, acc = 0.f;
#pragma unroll
  for (int i = kMaxK - 1; i >= 0; --i) {
    if (i < k) {
      const float t = (fabsf(d[i]) <= 1.f) ? G * v[i] : 0.f;
      acc += t;
      G -= t;
    }
  }
  if (k == 0) acc = gv;
  return inside ? acc : 0.f;
}

// The epilogue: x given -> ste_one against the step's input with the sample's scales; then fp32 or one rounding into T.
template <class T>
struct EpiSte {
  void* gx;                           // [N][C][H][W] of T, or of float (f32out)
  const T* x;                         // [N][C][H][W], or null: the accumulators as they are
  const float* xs;                    // [kx][N]
  int kx, N;
  float alpha;                        // the clamp bound in T's values, < 0: none
  int f32out;
  struct Row {
    float v[kMaxK];
  };
  __device__ __forceinline__ void row(int n, Row& r) const {
#pragma unroll
    for (int i = 0; i < kMaxK; ++i) r.v[i] = (x && i < kx) ? xs[(long long)i * N + n] : 0.f;
  }
  __device__ __forceinline__ void store(long long i, const Row& r, float acc) const {
    const float o = x ? ste_one((float)x[i], acc, r.v, kx, alpha, true) : acc;
    if (f32out) static_cast<float*>(gx)[i] = o;
    else static_cast<T*>(gx)[i] = (T)o;             // round to nearest even, one 2-byte store
  }
};

template <class T>
int run(const void* grad_y, const uint64_t* wbits, int kw_planes, const float* wscales, const lsq_conv_geom* g, const Shape& s,
        const void* x, int kx, const float* xscales, float clamp_alpha, void* grad_x, int f32out, void* workspace,
        hipStream_t st) {
  EpiSte<T> epi = {grad_x, static_cast<const T*>(x), xscales, kx, (int)g->N, clamp_alpha, f32out};
  return launch_dgrad(static_cast<const T*>(grad_y), wbits, kw_planes, wscales, g, s, epi, workspace, st);
}

}  // namespace

extern "C" int lsq_conv_train_half_abi_version(void) { return LSQ_CONV_TRAIN_HALF_ABI_VERSION; }

extern "C" int lsq_signw_conv2d_dgrad_half_plan(const lsq_conv_geom* g, lsq_conv_dgrad_plan* plan) { return plan_of(g, plan); }

extern "C" size_t lsq_signw_conv2d_dgrad_half_workspace_bytes(const lsq_conv_geom* g, int kw_planes) {
  return workspace_bytes_of(g, kw_planes);
}

extern "C" int lsq_signw_conv2d_dgrad_half(const void* grad_y, int gy_dtype, const uint64_t* wbits, int kw_planes,
                                           const float* wscales, const lsq_conv_geom* g, const void* x, int kx,
                                           const float* xscales, float clamp_alpha, void* grad_x, int gx_dtype, void* workspace,
                                           size_t workspace_bytes, void* stream) {
  if (!grad_y || !wbits || !wscales || !g || !grad_x) return LSQ_E_NULL;
  if (gy_dtype != LSQ_DTYPE_BF16 && gy_dtype != LSQ_DTYPE_F16) return LSQ_E_UNSUPPORTED;
  if (gx_dtype != LSQ_DTYPE_F32 && gx_dtype != gy_dtype) return LSQ_E_UNSUPPORTED;
  if (kx < 0 || kx > LSQ_MAX_PLANES) return LSQ_E_UNSUPPORTED;
  if (x && kx > 0 && !xscales) return LSQ_E_NULL;
  Shape s;
  if (int e = check_call(g, kw_planes, workspace, workspace_bytes, &s)) return e;
  if (x && g->N > 65535) return LSQ_E_UNSUPPORTED;    // (the limit of lsq_ste_backward, whose result this call states)
  if (((uintptr_t)grad_y & 1) || ((uintptr_t)x & 1) || ((uintptr_t)grad_x & (gx_dtype == LSQ_DTYPE_F32 ? 3 : 1)))
    return LSQ_E_UNSUPPORTED;
  const int f32out = gx_dtype == LSQ_DTYPE_F32;
  hipStream_t st = (hipStream_t)stream;
  if (gy_dtype == LSQ_DTYPE_BF16)
    return run<__bf16>(grad_y, wbits, kw_planes, wscales, g, s, x, kx, xscales, clamp_alpha, grad_x, f32out, workspace, st);
  return run<_Float16>(grad_y, wbits, kw_planes, wscales, g, s, x, kx, xscales, clamp_alpha, grad_x, f32out, workspace, st);
}
