// liblsq_hip_bn_train.so (include/lsq_hip_bn_train.h): the train-mode batch norm in front of a quantized convolution, folded
// into the quantizer's read (forward) and into the straight-through estimator's pass (backward).  Four memory-bound kernels
// and two one-thread-per-channel reducers:
//
//   stats_partial     grid (slab, channel): sum x, sum x^2 in fp64 -> one pair per (channel, slab)
//   stats_finish      adds a channel's slabs in slab order; mean, var, invstd, scale, shift, running statistics
//   rows_kernel       y = fmaf(x, scale, shift) (APPLY), the quantizer chain's value of it (VALUES), or the input gradient
//                     scale ((g - a) - x^ b) with g recomputed (GRAD)
//   grad_partial      grid (slab, channel): sum g, sum g x^ in fp64 -> one pair per (channel, slab)
//   grad_finish       adds the slabs in order; grad_beta, grad_gamma and the coefficients a, b of rows_kernel<GRAD>
//
// A channel's values are N runs of H * W floats, C * H * W apart.  A workgroup of 256 lanes covers `rows` runs at a time with
// `tpr` = 2^t lanes each (t the smallest with 2^t >= the run's accesses, at most 256): shifts and masks, no division per
// access, consecutive lanes on consecutive addresses.  Built without floating-point contraction (csrc/sublib.mk): the bits of
// g depend on the order of ste_one's operations.

#include <initializer_list>

#include "lsq_hip_bn_train.h"
#include "../lsq_common.h"            // wave_sum(double)
#include "../lsq_ste_one.h"           // ste_one, kMaxK: the straight-through estimator of ../lsq_ste.hip

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kGridTarget = 2048;      // workgroups a launch aims at: eight per CU
constexpr int kSlabValues = 1024;      // a slab holds at least this many values of its channel (or all samples)

struct Shape {
  int N, C, HW;
  int sps, slabs;        // samples per slab, slabs per channel
};

// slabs per channel: enough for kGridTarget workgroups over all channels, none below kSlabValues values
Shape shape_of(int N, int C, int H, int W) {
  Shape s;
  s.N = N, s.C = C, s.HW = H * W;
  const int want = (kGridTarget + C - 1) / C;
  int sps = (N + want - 1) / want;
  const int least = (kSlabValues + s.HW - 1) / s.HW;
  if (sps < least) sps = least;
  if (sps > N) sps = N;
  s.sps = sps;
  s.slabs = (N + sps - 1) / sps;
  return s;
}

struct Lanes {
  int shift;             // log2 of the lanes per run
  __host__ __device__ int tpr() const { return 1 << shift; }
  __host__ __device__ int rows() const { return kThreads >> shift; }
};

Lanes lanes_of(int accesses) {
  Lanes l = {0};
  while (l.shift < 8 && (1 << l.shift) < accesses) ++l.shift;
  return l;
}

// the workgroup's sum of (a, b), added in a fixed order: butterfly inside each wave, then the waves in wave order
__device__ __forceinline__ void block_sum2(double& a, double& b) {
  __shared__ double red[2][kWaves];
  a = lsq::wave_sum(a);
  b = lsq::wave_sum(b);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][wave] = a;
    red[1][wave] = b;
  }
  __syncthreads();
  a = red[0][0], b = red[1][0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) {
    a += red[0][w];
    b += red[1][w];
  }
}

// ------------------------------------------------------------------------------------------------------------ statistics
template <int VEC>
__global__ __launch_bounds__(kThreads) void stats_partial(const float* __restrict__ x, Shape s, Lanes l, double* __restrict__ ws) {
  const int slab = blockIdx.x, c = blockIdx.y;
  const int n1 = min(s.N, (slab + 1) * s.sps);
  const int accesses = s.HW / VEC, tpr = l.tpr(), rows = l.rows();
  const int v0 = threadIdx.x & (tpr - 1);
  double sum = 0.0, sq = 0.0;
  for (int n = slab * s.sps + (threadIdx.x >> l.shift); n < n1; n += rows) {
    const float* __restrict__ run = x + ((long long)n * s.C + c) * s.HW;
#pragma unroll 2
    for (int v = v0; v < accesses; v += tpr) {
      if constexpr (VEC == 4) {
        const float4 q = reinterpret_cast<const float4*>(run)[v];
        const double a = q.x, b = q.y, cc = q.z, d = q.w;
        sum += a, sq += a * a;
        sum += b, sq += b * b;
        sum += cc, sq += cc * cc;
        sum += d, sq += d * d;
      } else {
        const double a = run[v];
        sum += a, sq += a * a;
      }
    }
  }
  block_sum2(sum, sq);
  if (threadIdx.x == 0) {
    ws[2 * ((long long)c * s.slabs + slab)] = sum;
    ws[2 * ((long long)c * s.slabs + slab) + 1] = sq;
  }
}

struct StatsOut {
  const float *gamma, *beta;
  float *running_mean, *running_var, *mean, *var, *invstd, *scale, *shift;
  double eps, factor;      // factor: the weight of this batch in the running statistics
};

__global__ __launch_bounds__(64) void stats_finish(const double* __restrict__ ws, Shape s, StatsOut o) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= s.C) return;
  double sum = 0.0, sq = 0.0;
  for (int i = 0; i < s.slabs; ++i) {
    sum += ws[2 * ((long long)c * s.slabs + i)];
    sq += ws[2 * ((long long)c * s.slabs + i) + 1];
  }
  const double m = (double)s.N * (double)s.HW;
  const double mean = sum / m;
  const double var = fmax(fma(-sum, mean, sq) / m, 0.0);
  const float mean32 = (float)mean, var32 = (float)var;
  // the affine map from the values that are written: the caller's formulas on mean[] and var[] reproduce it to one rounding
  const double inv = 1.0 / sqrt((double)var32 + o.eps);
  const double sc = (o.gamma ? (double)o.gamma[c] : 1.0) * inv;
  o.mean[c] = mean32;
  o.var[c] = var32;
  o.invstd[c] = (float)inv;
  o.scale[c] = (float)sc;
  o.shift[c] = (float)((o.beta ? (double)o.beta[c] : 0.0) - (double)mean32 * sc);
  if (o.running_mean) {
    const double rm = o.running_mean[c], rv = o.running_var[c];
    o.running_mean[c] = (float)(rm + o.factor * (mean - rm));
    o.running_var[c] = (float)(rv + o.factor * (var * (m / (m - 1.0)) - rv));
  }
}

// -------------------------------------------------------------------------------------------------- the quantizer chain
// lsq_quant_values' value (ste_kernel<.., false> of ../lsq_ste.hip): r_k of the chain, the clamped input when k = 0
__device__ __forceinline__ float chain_value(float xv, const float (&v)[kMaxK], int k, float alpha) {
  const float xc = alpha >= 0.f ? fminf(fmaxf(xv, -alpha), alpha) : xv;
  float r = 0.f;
#pragma unroll
  for (int i = 0; i < kMaxK; ++i) {
    if (i < k) {
      const float d = xc - r;
      r = r + v[i] * (d >= 0.f ? 1.f : -1.f);
    }
  }
  return k == 0 ? xc : r;
}

__device__ __forceinline__ void load_scales(float (&v)[kMaxK], const float* __restrict__ xscales, int k, int N, int n) {
#pragma unroll
  for (int i = 0; i < kMaxK; ++i) v[i] = i < k ? xscales[(long long)i * N + n] : 0.f;
}

struct RowArgs {
  const float *x, *gq;                       // gq: GRAD only
  float* out;
  const float *scale, *shift, *mean, *invstd;
  const float* coef;                         // GRAD: a[C] then b[C]
  const float* xscales;
  int N, C, HW, k;
  float alpha;
  long long row_groups;
};

enum { APPLY = 0, VALUES = 1, GRAD = 2 };

template <int MODE>
__device__ __forceinline__ float row_one(float xv, float gv, float sc, float sh, float mu, float inv, float a, float b,
                                         const float (&v)[kMaxK], int k, float alpha) {
  const float y = fmaf(xv, sc, sh);
  if constexpr (MODE == APPLY) return y;
  if constexpr (MODE == VALUES) return chain_value(y, v, k, alpha);
  const float g = ste_one(y, gv, v, k, alpha);
  const float xh = (xv - mu) * inv;
  return sc * ((g - a) - xh * b);
}

template <int VEC, int MODE>
__global__ __launch_bounds__(kThreads) void rows_kernel(RowArgs p, Lanes l) {
  const int accesses = p.HW / VEC, tpr = l.tpr(), rows = l.rows();
  const int v0 = threadIdx.x & (tpr - 1), r0 = threadIdx.x >> l.shift;
  const long long R = (long long)p.N * p.C;
  for (long long rg = blockIdx.x; rg < p.row_groups; rg += gridDim.x) {
    const long long row = rg * rows + r0;
    if (row >= R) continue;
    const int n = (int)((unsigned)row / (unsigned)p.C), c = (int)((unsigned)row - (unsigned)n * (unsigned)p.C);     // N C < 2^32
    const float sc = p.scale[c], sh = p.shift[c];
    float mu = 0.f, inv = 0.f, a = 0.f, b = 0.f;
    float v[kMaxK];
    if constexpr (MODE != APPLY) load_scales(v, p.xscales, p.k, p.N, n);
    if constexpr (MODE == GRAD) mu = p.mean[c], inv = p.invstd[c], a = p.coef[c], b = p.coef[p.C + c];
    const float* xr = p.x + row * p.HW;
    const float* gr = MODE == GRAD ? p.gq + row * p.HW : nullptr;
    float* outr = p.out + row * p.HW;
    for (int i = v0; i < accesses; i += tpr) {
      if constexpr (VEC == 4) {
        const float4 xv = reinterpret_cast<const float4*>(xr)[i];
        float4 gv = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (MODE == GRAD) gv = reinterpret_cast<const float4*>(gr)[i];
        float4 o;
        o.x = row_one<MODE>(xv.x, gv.x, sc, sh, mu, inv, a, b, v, p.k, p.alpha);
        o.y = row_one<MODE>(xv.y, gv.y, sc, sh, mu, inv, a, b, v, p.k, p.alpha);
        o.z = row_one<MODE>(xv.z, gv.z, sc, sh, mu, inv, a, b, v, p.k, p.alpha);
        o.w = row_one<MODE>(xv.w, gv.w, sc, sh, mu, inv, a, b, v, p.k, p.alpha);
        reinterpret_cast<float4*>(outr)[i] = o;
      } else {
        outr[i] = row_one<MODE>(xr[i], MODE == GRAD ? gr[i] : 0.f, sc, sh, mu, inv, a, b, v, p.k, p.alpha);
      }
    }
  }
}

// -------------------------------------------------------------------------------------------------------------- backward
template <int VEC>
__global__ __launch_bounds__(kThreads) void grad_partial(RowArgs p, Shape s, Lanes l, double* __restrict__ ws) {
  const int slab = blockIdx.x, c = blockIdx.y;
  const int n1 = min(s.N, (slab + 1) * s.sps);
  const int accesses = s.HW / VEC, tpr = l.tpr(), rows = l.rows();
  const int v0 = threadIdx.x & (tpr - 1);
  const float sc = p.scale[c], sh = p.shift[c];
  const double mu = p.mean[c], inv = p.invstd[c];
  double sg = 0.0, sgx = 0.0;
  for (int n = slab * s.sps + (threadIdx.x >> l.shift); n < n1; n += rows) {
    float v[kMaxK];
    load_scales(v, p.xscales, p.k, p.N, n);
    const long long off = ((long long)n * s.C + c) * s.HW;
    const float* __restrict__ xr = p.x + off;
    const float* __restrict__ gr = p.gq + off;
    for (int i = v0; i < accesses; i += tpr) {
      float xs[VEC], gs[VEC];
      if constexpr (VEC == 4) {
        const float4 xv = reinterpret_cast<const float4*>(xr)[i], gv = reinterpret_cast<const float4*>(gr)[i];
        xs[0] = xv.x, xs[1] = xv.y, xs[2] = xv.z, xs[3] = xv.w;
        gs[0] = gv.x, gs[1] = gv.y, gs[2] = gv.z, gs[3] = gv.w;
      } else {
        xs[0] = xr[i], gs[0] = gr[i];
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const double g = ste_one(fmaf(xs[j], sc, sh), gs[j], v, p.k, p.alpha);
        sg += g;
        sgx += g * (((double)xs[j] - mu) * inv);
      }
    }
  }
  block_sum2(sg, sgx);
  if (threadIdx.x == 0) {
    ws[2 * ((long long)c * s.slabs + slab)] = sg;
    ws[2 * ((long long)c * s.slabs + slab) + 1] = sgx;
  }
}

__global__ __launch_bounds__(64) void grad_finish(const double* __restrict__ ws, Shape s, float* __restrict__ grad_gamma,
                                                  float* __restrict__ grad_beta, float* __restrict__ coef) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= s.C) return;
  double sg = 0.0, sgx = 0.0;
  for (int i = 0; i < s.slabs; ++i) {
    sg += ws[2 * ((long long)c * s.slabs + i)];
    sgx += ws[2 * ((long long)c * s.slabs + i) + 1];
  }
  const double m = (double)s.N * (double)s.HW;
  const float gb = (float)sg, gg = (float)sgx;
  grad_beta[c] = gb;
  grad_gamma[c] = gg;
  coef[c] = (float)((double)gb / m);             // from the values that are written: one rounding away from the caller's
  coef[s.C + c] = (float)((double)gg / m);
}

// ------------------------------------------------------------------------------------------------------------------ host
size_t slab_bytes(const Shape& s) { return (size_t)s.C * (size_t)s.slabs * 2 * sizeof(double); }
size_t coef_bytes(const Shape& s) { return ((size_t)s.C * 2 * sizeof(float) + 15) / 16 * 16; }

bool misaligned(const void* p, int to) { return ((uintptr_t)p & (uintptr_t)(to - 1)) != 0; }

int check_shape(int N, int C, int H, int W) {
  if (N < 1 || C < 1 || H < 1 || W < 1 || (long long)H * W >= (1ll << 31)) return LSQ_E_SHAPE;
  return LSQ_OK;
}

int check_limits(int N, int C, std::initializer_list<const void*> tensors) {
  if (N > 65535 || C > 65535) return LSQ_E_UNSUPPORTED;
  for (const void* t : tensors)
    if (t && misaligned(t, 4)) return LSQ_E_UNSUPPORTED;
  return LSQ_OK;
}

int check_workspace(size_t need, const void* workspace, size_t workspace_bytes) {
  if (!workspace || workspace_bytes < need || misaligned(workspace, 16)) return LSQ_E_WORKSPACE;
  return LSQ_OK;
}

bool vec4(int HW, std::initializer_list<const void*> tensors) {
  if (HW % 4) return false;
  for (const void* t : tensors)
    if (misaligned(t, 16)) return false;
  return true;
}

template <int MODE>
int launch_rows(RowArgs p, bool vec, hipStream_t st) {
  const Lanes l = lanes_of(vec ? p.HW / 4 : p.HW);
  const long long R = (long long)p.N * p.C;
  p.row_groups = (R + l.rows() - 1) / l.rows();
  const unsigned grid = (unsigned)(p.row_groups < 4 * kGridTarget ? p.row_groups : 4 * kGridTarget);
  if (vec) hipLaunchKernelGGL((rows_kernel<4, MODE>), dim3(grid), dim3(kThreads), 0, st, p, l);
  else hipLaunchKernelGGL((rows_kernel<1, MODE>), dim3(grid), dim3(kThreads), 0, st, p, l);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int lsq_bn_train_abi_version(void) { return LSQ_BN_TRAIN_ABI_VERSION; }

extern "C" size_t lsq_bn_train_workspace_bytes(int N, int C, int H, int W) {
  if (check_shape(N, C, H, W) != LSQ_OK) return 0;
  return slab_bytes(shape_of(N, C, H, W));
}

extern "C" int lsq_bn_train_stats(const float* x, int N, int C, int H, int W, const float* gamma, const float* beta, float eps,
                                  float momentum, int64_t batch_count, float* running_mean, float* running_var, float* mean,
                                  float* var, float* invstd, float* scale, float* shift, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  if (!x || !mean || !var || !invstd || !scale || !shift || (!running_mean != !running_var)) return LSQ_E_NULL;
  if (const int e = check_shape(N, C, H, W)) return e;
  if ((long long)N * H * W < 2 || (momentum < 0.f && running_mean && batch_count < 1)) return LSQ_E_SHAPE;
  if (const int e = check_limits(N, C, {x, gamma, beta, running_mean, running_var, mean, var, invstd, scale, shift})) return e;
  const Shape s = shape_of(N, C, H, W);
  if (const int e = check_workspace(slab_bytes(s), workspace, workspace_bytes)) return e;
  hipStream_t st = (hipStream_t)stream;
  double* ws = (double*)workspace;
  const bool vec = vec4(s.HW, {x});
  const Lanes l = lanes_of(vec ? s.HW / 4 : s.HW);
  const dim3 grid((unsigned)s.slabs, (unsigned)C);
  if (vec) hipLaunchKernelGGL(stats_partial<4>, grid, dim3(kThreads), 0, st, x, s, l, ws);
  else hipLaunchKernelGGL(stats_partial<1>, grid, dim3(kThreads), 0, st, x, s, l, ws);
  if (const int e = (int)hipGetLastError()) return e;
  StatsOut o = {gamma, beta, running_mean, running_var, mean, var, invstd, scale, shift, (double)eps,
                momentum < 0.f ? 1.0 / (double)(batch_count < 1 ? 1 : batch_count) : (double)momentum};
  hipLaunchKernelGGL(stats_finish, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, st, ws, s, o);
  return (int)hipGetLastError();
}

extern "C" int lsq_bn_apply(const float* x, int N, int C, int H, int W, const float* scale, const float* shift, float* y,
                            void* stream) {
  if (!x || !scale || !shift || !y) return LSQ_E_NULL;
  if (const int e = check_shape(N, C, H, W)) return e;
  if (const int e = check_limits(N, C, {x, scale, shift, y})) return e;
  RowArgs p = {x, nullptr, y, scale, shift, nullptr, nullptr, nullptr, nullptr, N, C, H * W, 0, -1.f, 0};
  return launch_rows<APPLY>(p, vec4(p.HW, {x, y}), (hipStream_t)stream);
}

extern "C" int lsq_quant_values_bn(const float* x, int N, int C, int H, int W, const float* scale, const float* shift, int k,
                                   const float* xscales, float clamp_alpha, float* x_q, void* stream) {
  if (!x || !scale || !shift || !x_q || (k > 0 && !xscales)) return LSQ_E_NULL;
  if (const int e = check_shape(N, C, H, W)) return e;
  if (k < 0 || k > kMaxK) return LSQ_E_SCHEME;
  if (const int e = check_limits(N, C, {x, scale, shift, xscales, x_q})) return e;
  RowArgs p = {x, nullptr, x_q, scale, shift, nullptr, nullptr, nullptr, xscales, N, C, H * W, k, clamp_alpha, 0};
  return launch_rows<VALUES>(p, vec4(p.HW, {x, x_q}), (hipStream_t)stream);
}

extern "C" size_t lsq_bn_ste_backward_workspace_bytes(int N, int C, int H, int W) {
  if (check_shape(N, C, H, W) != LSQ_OK) return 0;
  const Shape s = shape_of(N, C, H, W);
  return slab_bytes(s) + coef_bytes(s);
}

extern "C" int lsq_bn_ste_backward(const float* x, const float* grad_q, int N, int C, int H, int W, const float* scale,
                                   const float* shift, const float* mean, const float* invstd, int k, const float* xscales,
                                   float clamp_alpha, float* grad_x, float* grad_gamma, float* grad_beta, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  if (!x || !grad_q || !scale || !shift || !mean || !invstd || !grad_x || !grad_gamma || !grad_beta || (k > 0 && !xscales))
    return LSQ_E_NULL;
  if (const int e = check_shape(N, C, H, W)) return e;
  if (k < 0 || k > kMaxK) return LSQ_E_SCHEME;
  if (const int e = check_limits(N, C, {x, grad_q, scale, shift, mean, invstd, xscales, grad_x, grad_gamma, grad_beta})) return e;
  const Shape s = shape_of(N, C, H, W);
  if (const int e = check_workspace(slab_bytes(s) + coef_bytes(s), workspace, workspace_bytes)) return e;
  hipStream_t st = (hipStream_t)stream;
  double* ws = (double*)workspace;
  float* coef = (float*)((char*)workspace + slab_bytes(s));
  RowArgs p = {x, grad_q, grad_x, scale, shift, mean, invstd, coef, xscales, N, C, s.HW, k, clamp_alpha, 0};
  const bool vec = vec4(s.HW, {x, grad_q, grad_x});
  const Lanes l = lanes_of(vec ? s.HW / 4 : s.HW);
  const dim3 grid((unsigned)s.slabs, (unsigned)C);
  if (vec) hipLaunchKernelGGL(grad_partial<4>, grid, dim3(kThreads), 0, st, p, s, l, ws);
  else hipLaunchKernelGGL(grad_partial<1>, grid, dim3(kThreads), 0, st, p, s, l, ws);
  if (const int e = (int)hipGetLastError()) return e;
  hipLaunchKernelGGL(grad_finish, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, st, ws, s, grad_gamma, grad_beta, coef);
  if (const int e = (int)hipGetLastError()) return e;
  return launch_rows<GRAD>(p, vec, (hipStream_t)stream);
}
