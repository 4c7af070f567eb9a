// lsq_signw_conv2d: full-precision activation x sign-weight convolution on the gfx950 matrix cores.
//
// Replaces F.conv2d(x, w_q, ...) of quant/binary/binary_conv.py:165-173 when x_quant == 'fp' and the
// weights are sums of scaled sign planes:  y[n,o] = bias[o] + sum_q u_q[o] * conv(clamp(x), s_q)[n,o].
//
// The kernels, the patch-or-tiled rule and the launch table are lsq_signw_conv_core.h; this file supplies what fp32
// activations need.  v_mfma_f32_32x32x16_bf16: fp32 activations are split x = hi + lo with hi = bf16(x) and
// lo = bf16(x - hi): two LDS planes and two MFMAs per tile, relative error <= 2^-18 per product, fp32 accumulation --
// inside the 1e-4 bound where single bf16 (2^-9) is not.  The folded eval batch norm and the clamp are applied before the
// split; the epilogue adds the residuals and the activation on the last weight plane.

#include <type_traits>

#include "lsq_signw_conv_core.h"

namespace lsq {
namespace signw {
namespace {

// fp32 in memory, bf16 hi and lo planes in LDS, the folded batch norm before the clamp, the fused epilogue.
struct XF32 {
  typedef SwArgs Args;
  typedef float T;                     // an element of x in memory
  typedef float Raw;                   // ... in a register right after its load
  static constexpr bool kFp32 = true, kF16 = false;
  static constexpr bool kFused = false;
  static constexpr int kPlanes = 2, kPerReg = 1;
  template <bool PATCH>
  using Off = std::conditional_t<PATCH, unsigned, size_t>;
};

}  // namespace
}  // namespace signw
}  // namespace lsq

using namespace lsq;
using namespace lsq::signw;

extern "C" int64_t lsq_signw_weight_bytes(const lsq_conv_geom* g, int kw_planes) {
  if (check_geom(g) || kw_planes < 1 || kw_planes > LSQ_MAX_PLANES) return 0;
  return lean_weight_bytes(g, kw_planes);
}

extern "C" int lsq_signw_prepare_weight(const uint64_t* wbits, int kw_planes, const lsq_conv_geom* g, void* wprep, void* stream) {
  if (!wbits || !wprep) return LSQ_E_NULL;
  if (int e = check_geom(g)) return e;
  if (kw_planes < 1 || kw_planes > LSQ_MAX_PLANES) return LSQ_E_SCHEME;
  return lean_prepare(wbits, kw_planes, g, wprep, (hipStream_t)stream);
}

extern "C" int lsq_signw_conv2d(const float* x, float clamp_alpha, const float* pre_scale, const float* pre_shift,
                                const uint64_t* wbits, const void* wprep, int kw_planes, const float* wscales, const float* bias,
                                const lsq_conv_geom* g, int relu, const float* act_slope, const float* res_pre,
                                const float* res_post,
                                float* y, void* stream) {
  if (!x || !wbits || !wscales || !y) return LSQ_E_NULL;
  if (int e = check_geom(g)) return e;
  if (kw_planes < 1 || kw_planes > LSQ_MAX_PLANES) return LSQ_E_SCHEME;
  const int Ho = out_h(g), Wo = out_w(g);
  if (Ho <= 0 || Wo <= 0) return LSQ_E_SHAPE;
  SwArgs a = {};
  if ((pre_scale == nullptr) != (pre_shift == nullptr)) return LSQ_E_NULL;
  a.x = x; a.bias = bias; a.y = y; a.alpha = clamp_alpha;
  a.pre_scale = pre_scale; a.pre_shift = pre_shift;
  if (relu < LSQ_ACT_NONE || relu > LSQ_ACT_PRELU_CHANNEL || (relu >= LSQ_ACT_PRELU && !act_slope)) return LSQ_E_SCHEME;
  a.relu = relu; a.slope = act_slope; a.res_pre = res_pre; a.res_post = res_post;
  fill_geom(a, g, Ho, Wo);
  const long long wplane_words = lsq_weight_plane_words(g);
  hipStream_t st = (hipStream_t)stream;
  PatchPlan plan = patch_plan(g, Ho, Wo, pre_scale != nullptr);
#ifdef LSQ_TUNE
  if (getenv("LSQ_SIGNW_NOPATCH")) plan.patch = false;
#endif
  for (int q = 0; q < kw_planes; ++q) {
    a.wbits = (const unsigned long long*)wbits + (long long)q * wplane_words;
    a.wscale = wscales + (long long)q * g->O;
    a.accumulate = q ? 1 : 0;
    a.final_pass = q == kw_planes - 1 ? 1 : 0;
    // 3x3 fast path on the weights expanded by lsq_signw_prepare_weight (lsq_signw_lean.hip)
    const int fast = lean_launch(a, wprep, q, g, st);
    if (fast != LSQ_E_UNSUPPORTED) {
      if (fast) return fast;
      continue;
    }
    if (int e = launch<XF32>(a, plan, st)) return e;
  }
  return LSQ_OK;
}
