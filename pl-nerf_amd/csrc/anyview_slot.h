// A network slot of the experimental one-call entries (plnerf_anyview_net, include/experimental/plnerf_hip_anyview.h): which
// route it names, what its route's workspace needs, and its checks -- the shape as far as it can be judged without its
// pointers, then the pointers.  Shared by plnerf_render_view_any (render_view_any.hip) and plnerf_density_grid (mesh.hip).
#pragma once
#include "step_common.h"
#include "generic_net.h"
#include "../../include/experimental/plnerf_hip_anyview.h"

namespace {

constexpr int MAX_FREQS = 16;      // plnerf_embed_rows' limit on either encoding

// a slot's encoding: frequency bands of the positions and of the directions, columns of an embedded row
struct Encoding { int L, M, cols; };

inline bool generic(const plnerf_anyview_net& n) { return n.route == PLNERF_ANYVIEW_CHAIN16 || n.route == PLNERF_ANYVIEW_LAYERS32; }

inline size_t net_workspace_bytes(const plnerf_anyview_net& n, int rows) {
    if (n.route == PLNERF_ANYVIEW_CHAIN16) return plnerf_generic_fwd_workspace_bytes(&n.shape, rows, n.precision);
    if (n.route == PLNERF_ANYVIEW_LAYERS32) return plnerf_generic_fwd_f32_workspace_bytes(&n.shape, rows);
    return 0;
}

// a generic slot's shape as far as it can be judged without its pointers: PLNERF_OK and its encoding, or the refusal
inline int check_shape(const plnerf_anyview_net& n, int net_rows, Encoding& e) {
    const plnerf_generic_shape& s = n.shape;
    if (!s.use_viewdirs) return PLNERF_EINVAL;
    if (s.input_ch < 3 || (s.input_ch - 3) % 6 != 0 || s.view_ch < 3 || (s.view_ch - 3) % 6 != 0) return PLNERF_EINVAL;
    e = Encoding{(s.input_ch - 3) / 6, (s.view_ch - 3) / 6, s.input_ch + s.view_ch};
    if (e.L > MAX_FREQS || e.M > MAX_FREQS) return PLNERF_EINVAL;
    // the shape's (and the precision's) own refusals, in the order the entry looks: describe() (generic_net.h; the fp32 loop
    // describes under a two-plane precision, which changes nothing about a shape), then whatever else the size query refuses
    // -- an empty call of the entry, which launches nothing, says with which code
    Net net;
    int rc = describe(&s, n.route == PLNERF_ANYVIEW_CHAIN16 ? n.precision : PLNERF_PREC_BF16X3, net);
    if (rc) return rc;
    if (net_workspace_bytes(n, 1) == 0) {
        rc = n.route == PLNERF_ANYVIEW_CHAIN16
                 ? plnerf_generic_fwd(&s, nullptr, nullptr, e.cols, 0, n.precision, nullptr, 0, nullptr, 4, nullptr, nullptr)
                 : plnerf_generic_fwd_f32(&s, nullptr, nullptr, e.cols, 0, nullptr, 0, nullptr, 4, nullptr);
        return rc ? rc : PLNERF_EINVAL;      // (a size of 0 is a refusal whatever the empty call says)
    }
    // every launch's grid, before the first: plnerf_generic_fwd_f32's row limit, plnerf_generic_fwd's tiles and copies
    // (check_grids, as that entry calls it for a network with a concatenation: one with view directions has one)
    if (net_workspace_bytes(n, net_rows) == 0) return PLNERF_ERANGE;
    return n.route == PLNERF_ANYVIEW_CHAIN16 ? check_grids(net, net_rows, true) : PLNERF_OK;
}

inline int check_slot(const plnerf_anyview_net& n, int cols) {
    if (n.route == PLNERF_ANYVIEW_FUSED) return plnerf_step::check_net(&n.fused);
    // (an empty call: the entry's own checks of the table, no launch)
    return n.route == PLNERF_ANYVIEW_CHAIN16
               ? plnerf_generic_fwd(&n.shape, n.params, nullptr, cols, 0, n.precision, nullptr, 0, nullptr, 4, nullptr, nullptr)
               : plnerf_generic_fwd_f32(&n.shape, n.params, nullptr, cols, 0, nullptr, 0, nullptr, 4, nullptr);
}

}  // namespace
