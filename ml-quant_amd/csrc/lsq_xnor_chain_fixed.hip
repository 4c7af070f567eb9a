// The NQF instantiations of the fp4 matrix-core XNOR kernel -- lsq_xnor_conv2d_chain_fixed's final launch, the next layer's
// given-scale quantizer in the epilogue -- as a translation unit of their own: the kernel template of lsq_xnor_mfma.hip,
// instantiated here for NQF = 2 and LSQ_MAX_PLANES alone (lsq::xnor_conv_mfma_fixed), and compiled without packed fp32 VALU
// instructions (csrc/Makefile), which the object of lsq_xnor_mfma.hip itself keeps as it always had them.
#define LSQ_XNOR_NQF_TU 1
#include "lsq_xnor_mfma.hip"
