// Single-launch activation quantizer (lsq_act_fused.hip), called by lsq_act_quant for the LS-2 / LS-T
// solver schemes when the row's sub-sample fits the register file of one workgroup.
#pragma once

#include "lsq_common.h"

namespace lsq {

struct FusedArgs {
  const float* x;
  long long row_elems;      // M = C*H*W
  int C, H, W, cg, Gg, Gt, Hp, Wp, pad_h, pad_w;
  float alpha;
  const float* pre_scale;   // [C] or null (folded eval batch norm)
  const float* pre_shift;
  unsigned long long* planes;
  long long plane_words;    // words of one plane (all rows)
  long long row_words;      // words of one row of one plane
  float* scales;            // [2][N]
  int N;
  int ternary;
  int debug;                // developer / test switches: 1 every flagged bin through the block path, 2 a 2048-key list,
                            // 4 no windowed level-1 histogram (the round-2..4 solve only), 8 windowed histogram built, then dropped
  unsigned win_k0;          // windowed level-1 histogram (set by fused_act_quant): fine bin of key k >= win_k0 is
  int win_sh;               // (k - win_k0) >> win_sh, 8192 bins up to the top of the clamp value's binade; 0: off
  const float* forced;      // [2][N] scales given by the caller (moving-average inference): no solve, planes only
  int* trace;               // test hook: chosen sorted position per row (lsq_debug_solver_trace), or null
  int reserved[2];          // unused.  The block keeps its size and `greedy` its offset: the solving kernels copy it to LDS and hold
                            // it in scalar registers, and without these 8 bytes all 24 of them come out with other LDS addresses,
                            // other scalar-register spills and another scratch size than the ones that were tuned and measured
  int greedy;               // gf-2 (quantization.py:118-148 with k = 2): v1 = mean |x| instead of the solve; planes and
                            // v2 = mean |x - v1 b1| are the 2-bit least-squares scheme's
};

constexpr int kFusedNotEligible = 1;   // the shape is left to the streaming three-kernel path

// LSQ_OK, an hipError_t, or kFusedNotEligible (nothing launched).  skip is the reference's 3.
int fused_act_quant(const FusedArgs& a, hipStream_t st);

}  // namespace lsq
