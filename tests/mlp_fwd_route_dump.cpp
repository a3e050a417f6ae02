// Prints what pl-nerf_amd/csrc/mlp_fwd_route.h decides, for tests/test_mlp_fwd_route.py: per (element, NS, training,
// embedded) whether the register-resident instantiation exists and the route under each fwd_kernel value; then the rows
// of the instantiation list as the Makefile's stems spell them.
#include <cstdio>

#include "mlp_fwd_route.h"

using namespace plnerf::route;

int main() {
    const char* names[2] = {"f16", "bf16"};
    static_assert(ELEM_f16 == 0 && ELEM_bf16 == 1, "");
    static_assert(fwd_uses_rr(ELEM_f16, 2, true, false, FWD_AUTO) && !fwd_uses_rr(ELEM_f16, 2, true, false, FWD_PP), "constexpr");
    for (int e = 0; e < 2; ++e)
        for (int ns = 1; ns <= 2; ++ns)
            for (int t = 0; t < 2; ++t)
                for (int emb = 0; emb < 2; ++emb)
                    std::printf("%s %d %d %d exists=%d auto=%d rr=%d pp=%d\n", names[e], ns, t, emb, (int)rr_exists(e, ns, t, emb),
                                (int)fwd_uses_rr(e, ns, t, emb, FWD_AUTO), (int)fwd_uses_rr(e, ns, t, emb, FWD_RR),
                                (int)fwd_uses_rr(e, ns, t, emb, FWD_PP));
#define ROW(E, NS, SAVE, EMB) std::printf("row %s_%d_%d_%d\n", #E, NS, SAVE, EMB);
    PLNERF_RR_INSTANCES(ROW)
    return 0;
}
