// Shared between the two implementations of lsq_xnor_conv2d: the popcount kernel (lsq_xnor_conv.hip, every
// geometry) and the integer-MFMA kernel (lsq_xnor_mfma.hip, 3x3 taps over 64 channels).
#ifndef LSQ_XNOR_CONV_H_
#define LSQ_XNOR_CONV_H_

#include <type_traits>

#include "lsq_common.h"
#include "lsq_hip_linear_half.h"       // LSQ_DTYPE_*

namespace lsq {

struct ConvArgs {
  const unsigned long long* xplanes;   // [KX][N][Gt][Hp][Wp]
  const float* xscales;                // [KX][N]
  const unsigned long long* wbits;     // [taps][Gg][Opad]  (one weight plane)
  const int* wsum;                     // [O][taps]
  const float* wscale;                 // [O]
  const float* bias;                   // [O] or null
  float* y;                            // [N][O][Ho][Wo]
  long long xplane_words;
  int N, H, W, O, KH, KW, sh, sw, ph, pw, dh, dw;
  int Gg, Gt, Hp, Wp, Ho, Wo, cg, og, og_pad, opad_total, tiles_per_group;
  int accumulate;
  int final_pass;                      // last launch of a multi-plane sequence: apply the epilogue
  int relu;                            // epilogue: y = act(conv + bias + res_pre) + res_post; LSQ_ACT_*
  const float* slope;                  // PReLU slope(s): [1] (LSQ_ACT_PRELU) or [O] (LSQ_ACT_PRELU_CHANNEL)
  const float* res_pre;                // [N][O][Ho][Wo] or null
  const float* res_post;
  int res_stream;                      // the residual operand is read with the non-temporal hint: it and the output together exceed the
                                       // Infinity Cache and this is its last use (set by the entry point, kStreamBytes)
  int dbg_no_corr;                     // tuning builds only
  int int8_mfma;                       // test hook: the int8 matrix-core kernel instead of the fp4 one (two-plane, unchained launches)
  // ---- chained 1-bit layers (lsq_xnor_conv2d_chain): the NEXT layer's ls-1 quantizer in this layer's epilogue, and this
  // layer's activation scale from the exact row sum the PREVIOUS layer's epilogue left
  const long long* xunits;             // [N] or null: row sum of |clamp(x)| in units of 2^e; xscale = float(units * xunit / xM)
  double xunit, xM;
  unsigned* nq_planes32;               // or null: next layer's plane [N][O/64][nq_Hp][nq_Wp] as dwords
  unsigned long long* nq_units;        // [N]: += this launch's part of the next layer's row sums (zeroed by the caller)
  const float* nq_scale;               // [O] or null: folded batch norm in front of the next quantizer
  const float* nq_shift;
  float nq_alpha;                      // next layer's clamp (> 0)
  double nq_magic, nq_inv_unit;        // 1.5 * 2^(52 + e) and 2^-e
  int nq_Hp, nq_Wp, nq_ph, nq_pw;
  int tap_xoff[64];                    // (kh*dil_h)*Wp + kw*dil_w per tap
  // ---- projection shortcut computed in the epilogue's residual registers (lsq_xnor_conv2d_proj; the PROJ instantiations of
  // lsq_xnor_mfma.hip only): residual[n, o, ho, wo] = sum_c proj_w[o, c] * proj_x[n, c, ho * s, wo * s] + proj_bias[o]
  const float* proj_x;                 // [N][proj_c][proj_h][proj_w_in] or null (no projection): fp32, in a 16-bit launch of io_dtype
  const float* proj_w;                 // [O][proj_c]
  const float* proj_bias;              // [O] or null
  int proj_c, proj_h, proj_w_in, proj_stride;
  int proj_post;                       // 0: the value plays res_pre, 1: res_post
  // ---- 16-bit epilogue I/O (lsq_xnor_conv2d_half): the final launch of a call reads res_pre / res_post and writes y in
  // io_dtype (the three fields above keep their float types and are cast in the 16-bit instantiations); the fp32 running
  // sum of a multi-launch call lives in `sum`, which the launches before the last write as their fp32 y
  const float* sum;                    // [N][O][Ho][Wo] fp32: the accumulate read of a 16-bit launch (fp32 launches read y)
  int io_dtype;                        // LSQ_DTYPE_F32 (0, every other entry point) | LSQ_DTYPE_BF16 | LSQ_DTYPE_F16: THIS launch's
};

// The epilogue's memory accesses in the I/O type T of a kernel instantiation: float (as ever), __bf16 or _Float16.  A 16-bit
// load widens exactly; a 16-bit store is ONE round-to-nearest-even of the final fp32 value, the conversion Tensor.to(dtype)
// makes (fp16 overflow -> +-inf, results in the subnormal range stay subnormals).
template <typename T>
__device__ __forceinline__ float epi_load(const T* p) {
  if constexpr (std::is_same<T, __bf16>::value) return __uint_as_float((unsigned)*reinterpret_cast<const unsigned short*>(p) << 16);
  else return (float)*p;
}
template <typename T>
__device__ __forceinline__ float epi_load_nt(const T* p) {
  if constexpr (std::is_same<T, __bf16>::value)
    return __uint_as_float((unsigned)__builtin_nontemporal_load(reinterpret_cast<const unsigned short*>(p)) << 16);
  else return (float)__builtin_nontemporal_load(p);
}
template <typename T>
__device__ __forceinline__ void epi_store(T* p, float v) {
  *p = (T)v;
}
// A value that stays in registers as it was loaded (a gather issued ahead of its use) and is widened where it is used: the
// exact widening of epi_load, the identity for float.
template <typename T>
__device__ __forceinline__ float epi_widen(T v) {
  if constexpr (std::is_same<T, __bf16>::value) return __uint_as_float((unsigned)__builtin_bit_cast(unsigned short, v) << 16);
  else return (float)v;
}

// The projection operand of lsq_xnor_conv2d_proj's kernel: channels a multiple of 64 (the k order of lsq_pointwise.hip, in
// chunks of 64), at most kProjMaxChannels (32 x (C + 4) floats of LDS next to the weight fragments).
constexpr int kProjMaxChannels = 512;

// A block's tensors go from kernel to kernel through the 256 MiB Infinity Cache.  Where a launch reads a tensor for the last time
// while it writes one of the same size and the two do not fit together (the 56 x 56 layers at batch 256: 205 MB each), the dead
// tensor's loads carry the non-temporal hint so that the new lines push out consumed ones instead of lines the launch (or the
// next quantizer) still needs: measured on the ResNet-18 step, xnor conv 88 -> 86 us and the quantizer BEHIND it 93 -> 89 us per
// 56 x 56 layer; on tensors that do fit the hint costs 2-5 us per launch (28 x 28: 61 -> 67 us), hence the threshold.
constexpr long long kInfinityCacheBytes = 256ll << 20;

constexpr int kXnorMfmaNotEligible = 1;
// One launch (one weight plane x kx <= 2 activation planes) on the matrix cores; kXnorMfmaNotEligible when the
// geometry is not covered (the caller then takes the popcount kernel), else hipGetLastError().
int xnor_conv_mfma(const ConvArgs& a, int kx, int groups, hipStream_t st);
// Whether xnor_conv_mfma takes the geometry (no launch): what lsq_xnor_conv2d_proj must know before it launches anything.
bool xnor_conv_mfma_eligible(const ConvArgs& a, int kx, int groups);

}  // namespace lsq
#endif  // LSQ_XNOR_CONV_H_
