// One instantiation of the register-resident forward (mlp_rr_body.inc) per object, so that they compile in parallel:
// the Makefile compiles this file once per stem of RR_INST, mlp_rr_i_<element>_<NS>_<SAVE>_<EMB>.o, with
// -DRR_INST_NS / _SAVE / _EMB (and -DRR_BF16 for bf16 elements) taken from the stem.  mlp_fwd_route.h lists the rows.
// With -DRR_INST_CNT (stems of RR_CNT_INST, mlp_rr_c_<element>_<NS>_<SAVE>.o): the row's counted variant.
#include "mlp_rr_body.inc"
#include "mlp_fwd_route.h"

namespace plnerf {
namespace impl {
#ifdef RR_INST_CNT
int PLNERF_RR_CNT_LAUNCHER(PLNERF_RR_ELEM, RR_INST_NS, RR_INST_SAVE)(const RrFwdArgs& a, hipStream_t st) {
    return RR_NS::launch<RR_INST_NS, bool(RR_INST_SAVE), false, true>(a, st);
}
#else
static_assert(route::rr_exists(route::PLNERF_RR_PASTE(ELEM_, PLNERF_RR_ELEM), RR_INST_NS, RR_INST_SAVE, RR_INST_EMB),
              "not a row of PLNERF_RR_INSTANCES");
int PLNERF_RR_LAUNCHER(PLNERF_RR_ELEM, RR_INST_NS, RR_INST_SAVE, RR_INST_EMB)(const RrFwdArgs& a, hipStream_t st) {
    return RR_NS::launch<RR_INST_NS, bool(RR_INST_SAVE), bool(RR_INST_EMB)>(a, st);
}
#endif
}  // namespace impl
}  // namespace plnerf
