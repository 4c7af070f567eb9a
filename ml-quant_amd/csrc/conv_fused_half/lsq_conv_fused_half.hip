// lsq_signw_conv2d_fused_half: lsq_signw_conv2d_half (../conv_half/lsq_conv_half.hip) with the eval batch norm in front of
// it folded into the read and act(. + res_pre) + res_post on 16-bit residuals in the epilogue -- one launch per weight plane,
// one rounding into the 16-bit y.
//
// The kernels are ../lsq_signw_conv_core.h instantiated with X16F, whose kFused branches differ from X16's in two places:
//   read      a loaded element v of channel c becomes round_to_type(fl32(fl32(v * pre_scale[c]) + pre_shift[c])) (fold2) in
//             front of the clamp; the scales and shifts of the 16 (patch: 8 an item) channels being staged are read at
//             wave-uniform addresses, never held in LDS, so the kernel patch_plan names does not depend on the fold;
//   epilogue  on the last plane, in fp32 with a separate operation each: out += res_pre; out = act(out); out += res_post,
//             the residuals one 16-bit element per load at the output's own index, issued with the batch's other loads.
// Everything else -- tiles, staging, the summation order, the fp32 sum between launches -- is the unfused call's.

#include <math.h>
#include <string.h>

#include "lsq_hip_conv_fused_half.h"
#include "../lsq_signw_conv_core.h"
#include "../conv_half/lsq_conv_half_plan.h"      // host side: Plan, plan_of, workspace_bytes_of, fill_clamp

namespace lsq {
namespace signw {
namespace {

struct HFArgs {
  const unsigned short* x;             // [N][C][H][W], bf16 or fp16 bits
  const unsigned long long* wbits;     // [taps][Gg][Opad]  (the weight plane of this launch)
  const float* wscale;                 // [O], the plane of this launch
  const float* bias;                   // [O] or null
  const float* pre_scale;              // [C] or null (folded eval batch norm)
  const float* pre_shift;
  const float* prev;                   // [N][O][Ho][Wo] fp32 sum of the launches before this one, or null (base = bias or 0)
  void* out;                           // [N][O][Ho][Wo] of odt
  int odt;                             // LSQ_DTYPE_* of out
  float lim;                           // clamp bound, a value of the activations' type (+inf: identity)
  unsigned lim2;                       // fp16: its bits in both halves
  int clamp;                           // 0: no bound
  int N, C, H, W, O, KH, KW, sh, sw, ph, pw, dh, dw;
  int Gg, Ho, Wo, cg, og, og_pad, opad_total, tiles_per_group;
  int final_pass;                      // the last plane: the epilogue below applies
  int act;                             // y = act(conv + bias + res_pre) + res_post; LSQ_ACT_*
  const float* slope;                  // PReLU slope(s): [1] or [O]
  const unsigned short* res_pre;       // [N][O][Ho][Wo] of x's type, or null
  const unsigned short* res_post;

  __device__ __forceinline__ void store(long long i, float v) const {
    if (odt == LSQ_DTYPE_F32) static_cast<float*>(out)[i] = v;
    else if (odt == LSQ_DTYPE_BF16) static_cast<__bf16*>(out)[i] = (__bf16)v;
    else static_cast<_Float16*>(out)[i] = (_Float16)v;
  }
};

// X16 of ../conv_half/lsq_conv_half.hip with the fused read and epilogue.
template <bool F16>
struct X16F {
  typedef HFArgs Args;
  typedef unsigned short T;
  typedef unsigned Raw;
  static constexpr bool kFp32 = false, kF16 = F16;
  static constexpr bool kFused = true;
  static constexpr int kPlanes = 1, kPerReg = 2;
  template <bool PATCH>
  using Off = long long;
};

}  // namespace
}  // namespace signw
}  // namespace lsq

using namespace lsq;
using namespace lsq::signw;

extern "C" int lsq_conv_fused_half_abi_version(void) { return LSQ_CONV_FUSED_HALF_ABI_VERSION; }

extern "C" int lsq_signw_conv2d_fused_half_plan(const lsq_conv_geom* g) {
  Plan p;
  if (int e = plan_of(g, &p)) return e;
  return p.kind;
}

extern "C" int64_t lsq_signw_conv2d_fused_half_workspace_bytes(const lsq_conv_geom* g, int kw_planes, int y_dtype) {
  return workspace_bytes_of(g, kw_planes, y_dtype);
}

extern "C" int lsq_signw_conv2d_fused_half(const void* x, int x_dtype, float clamp_alpha, const float* pre_scale,
                                           const float* pre_shift, const uint64_t* wbits, int kw_planes, const float* wscales,
                                           const float* bias, const lsq_conv_geom* g, int act, const float* act_slope,
                                           const void* res_pre, const void* res_post, void* y, int y_dtype, void* workspace,
                                           size_t workspace_bytes, void* stream) {
  if (!x || !wbits || !wscales || !y) return LSQ_E_NULL;
  if (int e = check_geom(g)) return e;
  if (!half_type(x_dtype) || (y_dtype != LSQ_DTYPE_F32 && y_dtype != x_dtype)) return LSQ_E_UNSUPPORTED;
  if (kw_planes < 1 || kw_planes > LSQ_MAX_PLANES) return LSQ_E_UNSUPPORTED;
  Plan p;
  if (int e = plan_of(g, &p)) return e;
  if (!pre_scale != !pre_shift) return LSQ_E_NULL;
  if (act < LSQ_ACT_NONE || act > LSQ_ACT_PRELU_CHANNEL) return LSQ_E_UNSUPPORTED;
  if (act >= LSQ_ACT_PRELU && !act_slope) return LSQ_E_NULL;
  const size_t need = (size_t)workspace_bytes_of(g, kw_planes, y_dtype);
  if (need && (!workspace || ((uintptr_t)workspace & 3) || workspace_bytes < need)) return LSQ_E_WORKSPACE;
  const bool f16 = x_dtype == LSQ_DTYPE_F16;
  HFArgs a = {};
  a.x = static_cast<const unsigned short*>(x);
  a.bias = bias;
  a.pre_scale = pre_scale;
  a.pre_shift = pre_shift;
  a.act = act;
  a.slope = act_slope;
  a.res_pre = static_cast<const unsigned short*>(res_pre);
  a.res_post = static_cast<const unsigned short*>(res_post);
  fill_clamp(a, clamp_alpha);
  fill_geom(a, g, p.Ho, p.Wo);
  const long long wplane_words = (long long)g->KH * g->KW * a.Gg * a.opad_total;
  float* const sum = need ? static_cast<float*>(workspace) : static_cast<float*>(y);   // the fp32 sum between launches
  hipStream_t st = (hipStream_t)stream;
  for (int q = 0; q < kw_planes; ++q) {
    const bool last = q == kw_planes - 1;
    a.wbits = (const unsigned long long*)wbits + (long long)q * wplane_words;
    a.wscale = wscales + (long long)q * g->O;
    a.prev = q ? sum : nullptr;
    a.out = last ? y : sum;
    a.odt = last ? y_dtype : LSQ_DTYPE_F32;
    a.final_pass = last;
    if (int e = f16 ? launch<X16F<true>>(a, p.pp, st) : launch<X16F<false>>(a, p.pp, st)) return e;
  }
  return LSQ_OK;
}
