/*
 * lsq_hip_linear_train.h -- C ABI of the train-step kernels of the linear layer (liblsq_hip_linear_train.so), a library of
 * its own beside liblsq_hip.so, liblsq_hip_train.so, liblsq_hip_linear.so and liblsq_hip_linear_fp.so.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller (the library allocates nothing; the workspace
 * is the caller's), `stream` is a hipStream_t passed as void* (NULL = default stream), every function returns 0, a
 * negative LSQ_E_* code for an argument error (returned before any launch), or a positive hipError_t if a launch failed.
 * The library does not link the objects of liblsq_hip.so; its weight operand is what lsq_pack_weight of that library
 * writes -- the very planes the forward (lsq_linear_xnor, lsq_linear_signw) reads.
 */
#ifndef LSQ_HIP_LINEAR_TRAIN_H_
#define LSQ_HIP_LINEAR_TRAIN_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_LINEAR_TRAIN_ABI_VERSION 1

int lsq_linear_train_abi_version(void);

/*
 * Input gradient of the linear layer: fp32 gradient rows x sign-weight planes, the sum running over the OUTPUT features
 * (grad_xq = grad_y . w_q for w_q = sum_q ws_q s_q), on the bf16 matrix cores:
 *   gx[m][f] = sum_q sum_o a_q[m][o] * s_q[o][f],   a_q[m][o] = fl32(gy[m][o] * ws[q][o])
 * with s_q the +-1 signs of weight plane q.
 *   gy          [M][O] fp32, row-major, any 4-byte-aligned address and any O (16-byte loads only where gy is 16-byte
 *               aligned and O % 4 == 0; the result is the same bits either way)
 *   wbits       the weight planes lsq_pack_weight writes for (O, C = F, KH = KW = 1): words [q][ceil(F / 64)][ceil16(O)]
 *   wscales     [kw_planes][O] fp32
 *   gx          out, [M][F] fp32; nothing outside it is written
 *   workspace   at least lsq_linear_signw_dgrad_workspace_bytes(kw_planes, F, O) bytes, 8-byte aligned, any content; it is
 *               rewritten by every call (LSQ_E_WORKSPACE if it is NULL or too small)
 * Where the sign bits come from: a TRANSPOSED plane image T[q][ceil(O / 64)][ceil16(F)] (bit j of word [q][w][f] = the sign
 * of weight (o = 64 w + j, f)) is built in `workspace` by a first kernel of the call -- a 64 x 64 bit transpose of the
 * forward's planes, one wave per block of 64 words, 64 ballots --, after which a B fragment of the GEMM is 8 consecutive
 * bits of ONE word per lane, exactly as in lsq_linear_signw.  Reading the forward's planes in place would make every
 * fragment a gather of one bit out of each of 8 words; the transpose moves 2 bits per weight once per call (1/32 of the
 * traffic of an fp32 weight image, 1/16 of a bf16 one) and keeps the main loop that of the forward.  The weight stream
 * stays at one bit per weight: no fp32 or bf16 weight image is ever written.
 * Accuracy: the per-(plane, o) scale sits on the summed index, so it is multiplied INTO the A operand: a = fl32(gy * ws) is
 * split into hi = bf16(a) and lo = bf16(a - hi).  bf16 keeps 8 significant bits, so round-to-nearest gives
 * |a - hi| <= 2^-8 |a| (a - hi is exact in fp32) and |a - hi - lo| <= 2^-8 |a - hi| <= 2^-16 |a|; the signs are exact +-1 in
 * bf16, every product hi * s and lo * s is exact, and the products of ALL planes are summed into one fp32 accumulator by
 * v_mfma_f32_32x32x16_bf16.  With the rounding of the product a (2^-24 |gy ws|),
 *   |gx - exact| <= (2^-16 + 2^-24) sum_q sum_o |gy[m][o] ws[q][o]|  plus the fp32 rounding of the accumulation
 * in the worst case (every a at the bottom of a binade with both roundings at half an ulp); the dropped terms are
 * independent of each other, and what is measured against fp64 is 2-4e-6 of max |gx| (tests/test_gpu_linear_train.py
 * holds every case to 1e-5 of it).  A single bf16 operand (2^-8 per product) is 2^8 times coarser and measures 2e-3.
 * Summation order (fixed for given M, F, O, kw_planes: results are bitwise deterministic, no atomics): planes in order
 * q = 0 .. kw - 1, within a plane 16 output features per MFMA step in order of o, the hi products of a step before its lo
 * products, everything into one accumulator.  The small-shape kernel splits that sequence of (plane, 64-feature word)
 * stages into 8 consecutive ranges, one per wave, and adds the partial sums in wave order, ((S^0 + S^1) + S^2) + ...
 * Output features o >= O (the zero words lsq_pack_weight leaves in the padded slots) enter the A operand as 0; bits of
 * input features >= F are never stored as columns.
 * Kernels: fewer than 256 tiles of 64 x 64 in M x F -> one 32 x 32 tile of gx per workgroup with the summed dimension
 * split over 8 waves; otherwise 128 x 128 tiles (where there are at least 256 of them) or 64 x 64 tiles -- the rule of
 * lsq_linear_signw with F in the place of O.
 * Limits: 1 <= kw_planes <= LSQ_MAX_PLANES, F < 2^22, M < 2^31, O < 2^21; LSQ_E_UNSUPPORTED otherwise, before anything
 * is written.
 */
size_t lsq_linear_signw_dgrad_workspace_bytes(int kw_planes, int64_t F, int64_t O);

int lsq_linear_signw_dgrad(const float* gy, const uint64_t* wbits, int kw_planes, const float* wscales, int64_t M,
                           int64_t F, int64_t O, float* gx, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_LINEAR_TRAIN_H_ */
