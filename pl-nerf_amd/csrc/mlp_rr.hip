// Register-resident forward kernel of the 16-bit-operand MFMA MLP: packing, dispatch and the C++ entry points.  The
// kernel itself is mlp_rr_body.inc; its instantiations (PLNERF_RR_INSTANCES, mlp_fwd_route.h) are compiled one per object
// from mlp_rr_inst.hip so that they compile in parallel (-DRR_SINGLE_TU puts an element's all here: the trace builds of
// tools/build_variant.sh).  This file is compiled once per element type -- mlp_rr.o (IEEE half) and, with -DRR_BF16,
// mlp_rr_bf16.o -- for that element's weight packing; what does not depend on the element is in the half object alone.
#include "mlp_rr_body.inc"
#include "mlp_fwd_route.h"

namespace plnerf {
namespace impl {

// kernel<NS, SAVE, EMB> behind a plain function each
#define RR_DECLARE(E, NS, SAVE, EMB) int PLNERF_RR_LAUNCHER(E, NS, SAVE, EMB)(const RrFwdArgs& a, hipStream_t st);
PLNERF_RR_INSTANCES(RR_DECLARE)
#undef RR_DECLARE
// ... and the counted variants (PLNERF_RR_CNT_INSTANCES)
#define RR_DECLARE(E, NS, SAVE) int PLNERF_RR_CNT_LAUNCHER(E, NS, SAVE)(const RrFwdArgs& a, hipStream_t st);
PLNERF_RR_CNT_INSTANCES(RR_DECLARE)
#undef RR_DECLARE
#ifdef RR_SINGLE_TU
#define RR_DEFINE(E, NS, SAVE, EMB) \
    int PLNERF_RR_LAUNCHER(E, NS, SAVE, EMB)(const RrFwdArgs& a, hipStream_t st) { return RR_NS::launch<NS, bool(SAVE), bool(EMB)>(a, st); }
PLNERF_RR_PASTE(PLNERF_RR_INSTANCES_, PLNERF_RR_ELEM)(RR_DEFINE)
#undef RR_DEFINE
#define RR_DEFINE(E, NS, SAVE) \
    int PLNERF_RR_CNT_LAUNCHER(E, NS, SAVE)(const RrFwdArgs& a, hipStream_t st) { return RR_NS::launch<NS, bool(SAVE), false, true>(a, st); }
PLNERF_RR_PASTE(PLNERF_RR_CNT_INSTANCES_, PLNERF_RR_ELEM)(RR_DEFINE)
#undef RR_DEFINE
#endif

// rr_pack_f16 | rr_pack_bf16
int PLNERF_RR_PASTE(rr_pack_, PLNERF_RR_ELEM)(const float* const* params, int xyz_ch, int dir_ch, int ns, const float* cb,
                                              void* section, hipStream_t st) {
    ParamPtrs P;
    P.xyz_ch = xyz_ch; P.dir_ch = dir_ch; P.cb = cb;
    for (int i = 0; i < PLNERF_N_PARAM_TENSORS; ++i) P.p[i] = params[i];
    const int groups = lay::FWDC_FLOATS / 8, threads = 256, blocks = (groups + threads - 1) / threads;
    if (ns == 1) hipLaunchKernelGGL(RR_NS::rr_pack_kernel<1>, dim3(blocks), dim3(threads), 0, st, P, (unsigned char*)section);
    else hipLaunchKernelGGL(RR_NS::rr_pack_kernel<2>, dim3(blocks), dim3(threads), 0, st, P, (unsigned char*)section);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}

#ifndef RR_BF16
size_t rr_packed_bytes(int ns) { return (size_t)lay::FWDC_FLOATS * ns * 2; }

// (elem: route::ELEM_*; a combination that is no row of PLNERF_RR_INSTANCES: PLNERF_EINVAL -- route::fwd_uses_rr sends none)
int rr_fwd(int elem, const void* packed, const void* section, int ns, const float* pts, const float* viewdirs,
           const float* embedded, int in_ch, int view_ch, int n_rows, int samples_per_ray, FwdOpt opt, float* raw_out,
           void* saved, unsigned* status, hipStream_t st, const unsigned* n_dev) {
    RrFwdArgs a{packed, section, pts, viewdirs, n_rows, samples_per_ray < 1 ? 1 : samples_per_ray, raw_out, saved,
                status, embedded, in_ch, view_ch, opt.pe_scale, opt.act_beta, n_dev};
    if (n_dev) {      // the counted kernels: rows of PLNERF_RR_CNT_INSTANCES, or PLNERF_EINVAL
        if (embedded) return PLNERF_EINVAL;
#define RR_DISPATCH(E, NS, SAVE) \
    if (elem == route::ELEM_##E && ns == NS && (saved != nullptr) == bool(SAVE)) return PLNERF_RR_CNT_LAUNCHER(E, NS, SAVE)(a, st);
        PLNERF_RR_CNT_INSTANCES(RR_DISPATCH)
#undef RR_DISPATCH
        return PLNERF_EINVAL;
    }
#define RR_DISPATCH(E, NS, SAVE, EMB) \
    if (elem == route::ELEM_##E && ns == NS && (saved != nullptr) == bool(SAVE) && (embedded != nullptr) == bool(EMB)) \
        return PLNERF_RR_LAUNCHER(E, NS, SAVE, EMB)(a, st);
    PLNERF_RR_INSTANCES(RR_DISPATCH)
#undef RR_DISPATCH
    return PLNERF_EINVAL;
}
#endif

}  // namespace impl
}  // namespace plnerf

#ifndef RR_BF16
extern "C" int plnerf_build_flags_rr(void) {
    int f = 0;
#ifdef RR_TRACE
    f |= 4;
#endif
    return f;
}

#ifdef RR_TRACE
extern "C" int plnerf_debug_rr_trace(unsigned long long* out8) {
    return (int)hipMemcpyFromSymbol(out8, HIP_SYMBOL(plnerf_rr::g_rr_trace), 128 * sizeof(unsigned long long));
}
#endif
#endif
