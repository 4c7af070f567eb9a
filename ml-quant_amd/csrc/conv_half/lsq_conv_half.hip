// lsq_signw_conv2d_half: bf16 / fp16 activations x sign-weight planes, the convolution, on the 16-bit matrix cores of gfx950
// (v_mfma_f32_32x32x16_bf16 / v_mfma_f32_32x32x16_f16).
//
// lsq_signw_conv2d (csrc/lsq_signw_conv.hip) with a B operand that already is 16-bit.  The kernels, the patch-or-tiled rule
// and the launch table are the same code, ../lsq_signw_conv_core.h; this file supplies what 16-bit activations need: they
// are read as they are (half the bytes), clamped in their own type and staged as ONE LDS plane -- no hi / lo split, one MFMA
// per (16 channels, tap) and tile where the fp32 instantiation issues two.  The weights stay at one bit each in memory and
// are expanded to +-1.0 of the activations' type in the kernel (0x3F80 / 0x3C00 with the sign bit merged in).
// Activations are loaded element by element (2-byte loads, lanes on consecutive addresses of one channel), so any
// 2-byte-aligned x gives the same bits.  Out-of-image entries, padded channels and pixels past the end read a valid address
// and are zeroed: zero padding is exact.
// Epilogue: out = base + I * ws[o] with a separate multiply and add, base = bias[o] (or 0) at the first plane and the fp32
// sum of the planes before it afterwards; a launch holds one plane.  The sum is stored as fp32 (into y, or into the
// workspace while launches of a 16-bit y remain) or rounded once into the 16-bit y by the last launch, one element per store.

#include <math.h>
#include <string.h>

#include "lsq_hip_conv_half.h"
#include "../lsq_signw_conv_core.h"
#include "lsq_conv_half_plan.h"      // host side: Plan, plan_of, workspace_bytes_of, fill_clamp

namespace lsq {
namespace signw {
namespace {

struct HArgs {
  const unsigned short* x;             // [N][C][H][W], bf16 or fp16 bits
  const unsigned long long* wbits;     // [taps][Gg][Opad]  (the weight plane of this launch)
  const float* wscale;                 // [O], the plane of this launch
  const float* bias;                   // [O] or null
  const float* prev;                   // [N][O][Ho][Wo] fp32 sum of the launches before this one, or null (base = bias or 0)
  void* out;                           // [N][O][Ho][Wo] of odt
  int odt;                             // LSQ_DTYPE_* of out
  float lim;                           // clamp bound, a value of the activations' type (+inf: identity)
  unsigned lim2;                       // fp16: its bits in both halves
  int clamp;                           // 0: no bound (negative or +inf): the values pass as they are, NaN and inf included
  int N, C, H, W, O, KH, KW, sh, sw, ph, pw, dh, dw;
  int Gg, Ho, Wo, cg, og, og_pad, opad_total, tiles_per_group;

  // the epilogue's store: fp32, or rounded to nearest even into the 16-bit type (one element: nothing beside it is written)
  __device__ __forceinline__ void store(long long i, float v) const {
    if (odt == LSQ_DTYPE_F32) static_cast<float*>(out)[i] = v;
    else if (odt == LSQ_DTYPE_BF16) static_cast<__bf16*>(out)[i] = (__bf16)v;
    else static_cast<_Float16*>(out)[i] = (_Float16)v;
  }
};

// 16-bit words in memory, one LDS plane of the same words, clamped in their own type.
template <bool F16>
struct X16 {
  typedef HArgs Args;
  typedef unsigned short T;            // an element of x in memory
  typedef unsigned Raw;                // ... in a register right after its load
  static constexpr bool kFp32 = false, kF16 = F16;
  static constexpr bool kFused = false;
  static constexpr int kPlanes = 1, kPerReg = 2;
  template <bool PATCH>
  using Off = long long;
};

}  // namespace
}  // namespace signw
}  // namespace lsq

using namespace lsq;
using namespace lsq::signw;

extern "C" int lsq_conv_half_abi_version(void) { return LSQ_CONV_HALF_ABI_VERSION; }

extern "C" int lsq_signw_conv2d_half_plan(const lsq_conv_geom* g) {
  Plan p;
  if (int e = plan_of(g, &p)) return e;
  return p.kind;
}

extern "C" int64_t lsq_signw_conv2d_half_workspace_bytes(const lsq_conv_geom* g, int kw_planes, int y_dtype) {
  return workspace_bytes_of(g, kw_planes, y_dtype);
}

extern "C" int lsq_signw_conv2d_half(const void* x, int x_dtype, float clamp_alpha, const uint64_t* wbits, int kw_planes,
                                     const float* wscales, const float* bias, const lsq_conv_geom* g, void* y, int y_dtype,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !wbits || !wscales || !y) return LSQ_E_NULL;
  if (int e = check_geom(g)) return e;
  if (!half_type(x_dtype) || (y_dtype != LSQ_DTYPE_F32 && y_dtype != x_dtype)) return LSQ_E_UNSUPPORTED;
  if (kw_planes < 1 || kw_planes > LSQ_MAX_PLANES) return LSQ_E_UNSUPPORTED;
  Plan p;
  if (int e = plan_of(g, &p)) return e;
  const size_t need = (size_t)lsq_signw_conv2d_half_workspace_bytes(g, kw_planes, y_dtype);
  if (need && (!workspace || ((uintptr_t)workspace & 3) || workspace_bytes < need)) return LSQ_E_WORKSPACE;
  const bool f16 = x_dtype == LSQ_DTYPE_F16;
  HArgs a = {};
  a.x = static_cast<const unsigned short*>(x);
  a.bias = bias;
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
    if (int e = f16 ? launch<X16<true>>(a, p.pp, st) : launch<X16<false>>(a, p.pp, st)) return e;
  }
  return LSQ_OK;
}
