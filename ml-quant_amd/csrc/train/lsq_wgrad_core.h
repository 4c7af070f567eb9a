// What lsq_train_wgrad (lsq_wgrad.hip) and lsq_train_wgrad_half (../train_half/lsq_wgrad_half.hip) share: the
// constants, the geometry and tile fields of the kernels' arguments, the LDS layout of the staged sign words, the reduce
// kernel and the whole host side -- what is refused, the tile and split rule, the workspace check and the launch.  Internal:
// not part of the C ABI under include/; it is compiled into each of the two libraries.
//
// Both are D[o][(c, tap)] = sum_k A[o][k] B_p[k][(c, tap)] over the positions k = (n, ho, wo) and the planes p, with
//   B_p[k][(c, i, j)] = 2 bit_p - 1 of channel c at padded pixel (ho s + i, wo s + j): exactly +-1 in A's 16-bit type, or 0 on a
//                       halo word and where k is no position.
// Tiles: a workgroup (4 waves) owns 64 output channels x 64 input channels (one plane word) x up to TT taps, every wave a
// 32 x 32 block of (o, c) for each of the tile's taps (TT accumulators of 16 registers).  Per chunk of 64 k and plane the
// workgroup stages the sign words of its taps (complemented, 0 on the halo) in LDS (SignSmem).
// Split-K: the chunks are cut into S slices of whole chunks (S from the geometry alone: about kTargetGroups workgroups,
// tile_plan).  With S > 1 every workgroup stores its accumulators as a slab in MFMA order (coalesced) and a second launch
// sums the S slabs of each output element in slice order (wgrad_reduce_kernel) -- bitwise deterministic, no atomics, no
// inter-workgroup hand-off.  S = 1 writes grad_wq directly.
// What a file keeps: its A operand and with it what a chunk is (the runs of 64 k across samples of the fp32 kernel, the
// per-sample padded k-steps of the 16-bit one), its entry points, and its main kernel IN ONE TEXT.  The steps of that text
// which read the same in both files -- position -> sign word, the fold decision, the staging of a tap's sign words, the
// expansion of a staged word into a B fragment, the epilogue stores -- are NOT functions of this header: as __forceinline__
// functions (struct or scalar parameters, values returned or written through references) each of them changed the
// instruction streams of the main kernels, and all of them together measured 0.5 - 3 % slower on the MI355X with bit-equal
// results.  A change to one of those steps belongs in both files; tests/test_gpu_wgrad_cases.py compares
// the two kernels on the same operands.

#ifndef LSQ_WGRAD_CORE_H
#define LSQ_WGRAD_CORE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsq_hip.h"
#include "../linear/lsq_signw_mma.h"     // Frag, f32x16, d_row, mfma16

namespace {

constexpr int kThreads = 256;
constexpr int kKC = 64;               // k per chunk: four k-steps
constexpr int kOT = 64;               // output channels per workgroup
constexpr int kApitch = kKC + 8;      // 16-bit values per staged A row (16-byte pad: the row reads of a wave fall on distinct banks)
constexpr int kTargetGroups = 512;    // workgroups the K split aims at (2 per CU)
constexpr int kTapTile = 9;           // taps per workgroup for kernels larger than 1x1

// The geometry, and the planes, tiles and K split, as the kernels read them: members g and t of each file's Args.
struct WgradGeom {
  long long plane_words;
  int N, C, H, W, O, KH, KW, s, ph, pw, Ho, Wo, Hp, Wp, Gt;
  unsigned HoWo;
};

struct WgradTiles {
  int kx, ntc, tiles, chunks_per_split, S;
};

// The staged sign words of a (chunk, plane): a member of each file's Smem<TT>, behind its A rows.
template <int TT>
struct SignSmem {
  unsigned p[TT][2][kKC];             // ~(word half) of tap tl at chunk position k; 0 on the halo / where k is no position
  unsigned z[TT][2][kKC];             // channels whose value is 0 (a folded pair of planes with opposite signs)
  unsigned short b0[TT][kKC];         // +1 (0x3F80 bf16, 0x3C00 fp16) or +2 (0x4000 in both, a folded pair) where the sign is real, else 0
};

// Sum of the S partial sums of every output element, in slice order.  Thread = one slab position (MFMA order); BIAS (Args
// with bias_part [S][OB], grad_b or NULL): behind the slab one element of the bias rows.
template <int TT, bool BIAS, class Args>
__global__ __launch_bounds__(kThreads) void wgrad_reduce_kernel(Args a) {
  const size_t slab = (size_t)a.t.tiles * 4 * TT * 16 * 64;
  const size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= slab) {
    if constexpr (BIAS) {
      const size_t o = idx - slab;
      if (a.grad_b == nullptr || o >= (size_t)a.g.O) return;
      float sum = a.bias_part[o];
      for (int s = 1; s < a.t.S; ++s) sum += a.bias_part[(size_t)s * a.OB + o];
      a.grad_b[o] = sum;
    }
    return;
  }
  const int lane = (int)(idx & 63), reg = (int)((idx >> 6) & 15);
  const size_t rest = idx >> 10;
  const int tl = (int)(rest % TT), w = (int)((rest / TT) % 4), tile = (int)(rest / (TT * 4));
  const int tc = tile % a.t.ntc, g = (tile / a.t.ntc) % a.g.Gt, ot = tile / (a.t.ntc * a.g.Gt);
  const int KK = a.g.KH * a.g.KW, tap = tc * TT + tl;
  const int c = g * 64 + 32 * (w >> 1) + (lane & 31);
  const int o = d_row(ot * kOT + 32 * (w & 1), reg, lane >> 5);
  if (tap >= KK || c >= a.g.C || o >= a.g.O) return;
  float sum = a.out[idx];
  for (int s = 1; s < a.t.S; ++s) sum += a.out[(size_t)s * slab + idx];
  a.grad_wq[((size_t)o * a.g.C + c) * KK + tap] = sum;
}

// ---- host side

// What both entry points refuse, and with which code.
inline int check_geom(const lsq_conv_geom* g, int kx) {
  if (!g) return LSQ_E_NULL;
  if (kx < 1 || kx > LSQ_MAX_PLANES) return LSQ_E_SCHEME;
  if (g->N < 1 || g->C < 1 || g->H < 1 || g->W < 1 || g->O < 1 || g->KH < 1 || g->KW < 1 || g->stride_h < 1 ||
      g->stride_w < 1 || g->pad_h < 0 || g->pad_w < 0 || g->dil_h < 1 || g->dil_w < 1 || g->groups < 1)
    return LSQ_E_SHAPE;
  if (g->C % g->groups || g->O % g->groups) return LSQ_E_SHAPE;
  const long long ho = ((long long)g->H + 2 * g->pad_h - (long long)g->dil_h * (g->KH - 1) - 1) / g->stride_h + 1;
  const long long wo = ((long long)g->W + 2 * g->pad_w - (long long)g->dil_w * (g->KW - 1) - 1) / g->stride_w + 1;
  if (g->H + 2 * g->pad_h < g->dil_h * (g->KH - 1) + 1 || g->W + 2 * g->pad_w < g->dil_w * (g->KW - 1) + 1 || ho < 1 || wo < 1)
    return LSQ_E_SHAPE;
  if (g->groups != 1 || g->dil_h != 1 || g->dil_w != 1 || g->stride_h != g->stride_w || g->stride_h > 2)
    return LSQ_E_UNSUPPORTED;
  if (g->KH > 8 || g->KW > 8 || g->pad_h > g->KH - 1 || g->pad_w > g->KW - 1) return LSQ_E_UNSUPPORTED;
  if ((long long)g->N * ho * wo >= (1ll << 31) || g->O > 65535 || g->C > 65535) return LSQ_E_UNSUPPORTED;
  return LSQ_OK;
}

// The geometry fields of a checked geometry.
inline WgradGeom fill_geom(const lsq_conv_geom* g) {
  WgradGeom a;
  a.N = g->N; a.C = g->C; a.H = g->H; a.W = g->W; a.O = g->O; a.KH = g->KH; a.KW = g->KW;
  a.s = g->stride_h; a.ph = g->pad_h; a.pw = g->pad_w;
  a.Ho = (g->H + 2 * g->pad_h - g->KH) / g->stride_h + 1;
  a.Wo = (g->W + 2 * g->pad_w - g->KW) / g->stride_w + 1;
  a.Hp = g->H + 2 * g->pad_h;
  a.Wp = g->W + 2 * g->pad_w;
  a.Gt = (g->C + 63) / 64;
  a.HoWo = (unsigned)a.Ho * (unsigned)a.Wo;
  a.plane_words = (long long)g->N * a.Gt * a.Hp * a.Wp;
  return a;
}

// THE tile and split rule, given how many chunks the caller's reduction has: tiles of kOT output channels x one channel word
// x TT taps, S slices of chunks_per_split whole chunks (about kTargetGroups workgroups), slabs of slab_floats each.
struct TilePlan {
  WgradTiles t;
  int TT;
  size_t slab_floats;
};

inline TilePlan tile_plan(const WgradGeom& g, int kx, long long chunks) {
  TilePlan p;
  const int KK = g.KH * g.KW;
  p.TT = KK == 1 ? 1 : kTapTile;
  p.t.kx = kx;
  p.t.ntc = (KK + p.TT - 1) / p.TT;
  p.t.tiles = ((g.O + kOT - 1) / kOT) * g.Gt * p.t.ntc;
  long long S = (kTargetGroups + p.t.tiles - 1) / p.t.tiles;
  if (S > chunks) S = chunks;
  if (S < 1) S = 1;
  p.t.chunks_per_split = (int)((chunks + S - 1) / S);
  p.t.S = (int)((chunks + p.t.chunks_per_split - 1) / p.t.chunks_per_split);
  p.slab_floats = (size_t)p.t.tiles * 4 * p.TT * 16 * 64;
  return p;
}

// A workspace of `need` bytes: LSQ_E_NULL where it is needed and missing, LSQ_E_WORKSPACE where short or not 16-byte-aligned.
inline int check_workspace(size_t need, const void* workspace, size_t workspace_bytes) {
  if (need > 0 && !workspace) return LSQ_E_NULL;
  if (workspace_bytes < need || ((uintptr_t)workspace & 15)) return LSQ_E_WORKSPACE;
  return LSQ_OK;
}

// The kernels of one entry point (and operand type): main[TT == kTapTile][fold], reduce[TT == kTapTile].
template <class Args>
struct WgradKernels {
  void (*main[2][2])(Args);
  void (*reduce[2])(Args);
};

// The main kernel of (TT, fold) over tiles x S workgroups and, with S > 1, the reduce kernel: a thread per slab position and
// `behind` more (the 16-bit entry's bias row).
template <class Args>
int launch_wgrad(const WgradKernels<Args>& k, const Args& a, const TilePlan& p, bool fold, size_t behind, hipStream_t st) {
  const dim3 grid((unsigned)(p.t.tiles * p.t.S)), block(kThreads);
  const dim3 rgrid((unsigned)((p.slab_floats + behind + kThreads - 1) / kThreads));
  hipLaunchKernelGGL(k.main[p.TT != 1][fold], grid, block, 0, st, a);
  if (p.t.S > 1) hipLaunchKernelGGL(k.reduce[p.TT != 1], rgrid, block, 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace

#endif
