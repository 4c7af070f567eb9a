// Host side of the 16-bit sign-weight convolutions, shared at the source by liblsq_hip_conv_half.so (lsq_conv_half.hip) and
// liblsq_hip_conv_fused_half.so (../conv_fused_half/lsq_conv_fused_half.hip): the geometry checks and the plan, so that both
// libraries refuse the same geometries with the same codes and name the same kernel for every other one; and the clamp
// bound's fields, which both operand structs have.  Host code only; include after ../lsq_signw_conv_core.h.
#pragma once

#include <math.h>
#include <string.h>

#include "lsq_hip_conv_half.h"

namespace lsq {
namespace signw {
namespace {

struct Plan {
  int kind;                            // LSQ_CONV_HALF_* bits
  int Ho, Wo;
  PatchPlan pp;
};

bool half_type(int t) { return t == LSQ_DTYPE_BF16 || t == LSQ_DTYPE_F16; }

// 0 and *p filled, or a negative LSQ_E_* code.  The patch rule is patch_plan, lsq_signw_conv2d's own, so that both libraries
// take a patch kernel for the same geometries -- always without a pre-scale table: the fused library reads the folded batch
// norm of the chunk being staged and holds none in LDS.
int plan_of(const lsq_conv_geom* g, Plan* p) {
  if (int e = check_geom(g)) return e;
  const long long Hp = (long long)g->H + 2ll * g->pad_h, Wp = (long long)g->W + 2ll * g->pad_w;
  const long long Ho64 = (Hp - (long long)g->dil_h * (g->KH - 1) - 1) / g->stride_h + 1;
  const long long Wo64 = (Wp - (long long)g->dil_w * (g->KW - 1) - 1) / g->stride_w + 1;
  if (Hp - (long long)g->dil_h * (g->KH - 1) - 1 < 0 || Wp - (long long)g->dil_w * (g->KW - 1) - 1 < 0) return LSQ_E_SHAPE;
  const long long lim = 1ll << 31;
  if (Hp >= lim || Wp >= lim || Ho64 >= lim || Wo64 >= lim) return LSQ_E_UNSUPPORTED;
  // (products of at most three factors below 2^31 each: checked step by step)
  auto prod_fits = [&](long long a, long long b, long long c, long long d) {
    long long v = a;
    for (long long f : {b, c, d}) {
      if (v >= lim) return false;
      v *= f;
    }
    return v < lim;
  };
  const int cg = g->C / g->groups, og = g->O / g->groups;
  const long long Gg = (cg + 63) / 64, og_pad = (og + 15) / 16 * 16;
  if (!prod_fits(g->N, g->C, g->H, g->W) || !prod_fits(g->N, g->O, Ho64, Wo64) || !prod_fits(g->N, Hp, Wp, 1)) return LSQ_E_UNSUPPORTED;
  if (!prod_fits(g->KH, g->KW, Gg, (long long)g->groups * og_pad) ||
      (long long)g->KH * g->KW * Gg * g->groups * og_pad >= (1ll << 28))
    return LSQ_E_UNSUPPORTED;
  const int og_tiles = (og + tile_bm(og > 64) - 1) / tile_bm(og > 64);
  if ((long long)g->groups * og_tiles > 65535) return LSQ_E_UNSUPPORTED;
  p->Ho = (int)Ho64; p->Wo = (int)Wo64;
  p->pp = patch_plan(g, Ho64, Wo64, false);
  p->kind = p->pp.wide ? LSQ_CONV_HALF_WIDE : 0;
  if (p->pp.patch)
    p->kind |= LSQ_CONV_HALF_PATCH | (p->pp.unit ? LSQ_CONV_HALF_UNIT_STRIDE : 0) | (p->pp.many ? LSQ_CONV_HALF_MANY_TAPS : 0);
  return LSQ_OK;
}

// A launch holds one plane: the fp32 running sum of a 16-bit y of more than one plane lives in the workspace.
int64_t workspace_bytes_of(const lsq_conv_geom* g, int kw_planes, int y_dtype) {
  Plan p;
  if (!half_type(y_dtype) || kw_planes <= 1 || plan_of(g, &p)) return 0;
  return 4ll * g->N * g->O * p.Ho * p.Wo;
}

// lim / lim2 / clamp of an operand struct.  The bound is used as given: the caller has rounded it into the activations'
// type (a NaN or negative one: identity)
template <class A>
void fill_clamp(A& a, float clamp_alpha) {
  a.lim = clamp_alpha >= 0.f ? clamp_alpha : INFINITY;
  a.clamp = !isinf(a.lim);
  const _Float16 h = (_Float16)a.lim;
  uint16_t hb;
  memcpy(&hb, &h, 2);
  a.lim2 = (uint32_t)hb << 16 | hb;
}

}  // namespace
}  // namespace signw
}  // namespace lsq
