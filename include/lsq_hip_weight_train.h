/*
 * lsq_hip_weight_train.h -- C ABI of lsq_weight_quant_pack (liblsq_hip_weight_train.so): the weight side of one train step
 * in one launch.  From the fp32 weight of a quantized layer it computes the scales the torch weight quantizer's train-mode
 * forward leaves in the module's buffers (quant/binary/weight_quantization.py) and packs the sign planes and tap sums
 * lsq_pack_weight would pack for those scales, with every out-channel row resident in LDS from its one read to its last use.
 *
 * Conventions are those of lsq_hip.h: device pointers owned by the caller, `stream` is a hipStream_t passed as void*
 * (NULL = default stream), every function returns 0, a negative LSQ_E_* code for an argument error (returned before any
 * launch, nothing written), or a positive hipError_t if a launch failed.
 */
#ifndef LSQ_HIP_WEIGHT_TRAIN_H_
#define LSQ_HIP_WEIGHT_TRAIN_H_

#include <stddef.h>
#include <stdint.h>

#include "lsq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSQ_WEIGHT_TRAIN_ABI_VERSION 1

/* The longest out-channel row, (C / groups) * KH * KW floats, the kernel takes: the row and the sorted copy of its
 * sub-sample (skip >= 1) stay in the 160 KB of LDS of one workgroup. */
#define LSQ_WEIGHT_TRAIN_MAX_ROW 16384

int lsq_weight_train_abi_version(void);

/*
 * 1 where lsq_weight_quant_pack takes (geometry, scheme, k, skip), 0 where the caller must keep the present route
 * (the torch weight quantizer, then lsq_pack_weight): a row over LSQ_WEIGHT_TRAIN_MAX_ROW, 2^31 or more weights or plane
 * words, and whatever the call below answers with an argument error.
 */
int lsq_weight_quant_pack_supported(const lsq_conv_geom* g, int scheme, int k, int skip);

/*
 * w [O][C/groups][KH][KW] fp32  ->  scales [k][O] fp32, wbits [k][lsq_weight_plane_words(g)] and wsum [k][O][KH*KW] in
 * exactly lsq_pack_weight's layout (padded out-channel slots zero), in one launch: no workspace, no host synchronisation,
 * capturable in a HIP graph, bitwise repeatable (every sum in a fixed order, no atomics).
 *
 * Per out-channel row of M = (C/groups) * KH * KW weights, with sign(+-0) = +1:
 *   LS1 (k = 1), GF (k planes):  v_q = mean |r_q| over the row, r_0 = w, r_{q+1} = r_q - v_q sign(r_q) in fp32; the sum is
 *     carried in fp64 and rounded once to fp32.
 *   LS2, LST (k = 2):  v_1 is the optimal first scale over |row[::skip]| (quant/binary/optimal.py) as lsq_solve_rows
 *     chooses it: same candidates, same fp64 closed-form costs, ties to the smallest sorted position, the ternary scheme's
 *     extra candidate mean / 2, and 0 for a row without a candidate.  LS2: v_2 = mean | |w| - v_1 | over the full row (fp64
 *     sum rounded once).  LST: v_1 is written twice.
 *   Planes and wsum: bit for bit lsq_pack_weight(w, g, k, scales) for the scales this call wrote.
 *
 * LSQ_E_NULL: w, g, scales, wbits or wsum is NULL.  LSQ_E_SHAPE: what check_geom refuses.  LSQ_E_SCHEME: an unknown scheme;
 * k other than 1 for LS1, 2 for LS2 / LST, 1..LSQ_MAX_PLANES for GF; skip < 1.  LSQ_E_UNSUPPORTED: whatever
 * lsq_weight_quant_pack_supported answers 0 for.  A refused call launches nothing and writes nothing.
 */
int lsq_weight_quant_pack(const float* w, const lsq_conv_geom* g, int scheme, int k, int skip, float* scales,
                          uint64_t* wbits, int32_t* wsum, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LSQ_HIP_WEIGHT_TRAIN_H_ */
