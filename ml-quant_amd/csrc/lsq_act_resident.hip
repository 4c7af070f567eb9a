// The row-resident instantiations of the single-launch ls-2 / ls-T quantizer (Impl::run_resident, lsq::resident_act_quant) as
// a translation unit of their own: the device functions of lsq_act_fused.hip, compiled a second time without packed fp32 VALU
// instructions (csrc/Makefile); the object of lsq_act_fused.hip itself keeps the flags its kernels were tuned with.
#define LSQ_RESIDENT_TU 1
#undef LSQ_PHASE_CLOCKS
#include "lsq_act_fused.hip"
