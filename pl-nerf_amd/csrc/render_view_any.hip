// plnerf_render_view_any (include/experimental/plnerf_hip_anyview.h): plnerf_render_view's sequence (render_view.hip) with a
// route per network slot.  A slot on the compiled trunk runs step_common.h's network(); a slot outside it runs, per sub-block
// of at most io.max_net_rows rows, what run_network() reaches for such a network through Python (run_plnerf.py:78-92):
// plnerf_embed_rows, then the whole layer-by-layer forward as one call (plnerf_generic_fwd on 16-bit planes, or
// plnerf_generic_fwd_f32), into the pass's raw outputs; the pass's density noise follows either.  Rows are independent in
// both routes, so where a pass is cut does not show in the frame.  No kernel of the path is written here.
#include "step_common.h"
#include "anyview_slot.h"

namespace {

using namespace plnerf_step;

// The workspace: plnerf_render_view's blocks in its order (so that two FUSED slots need exactly its bytes), then the embedded
// rows and the network workspace of one sub-block.
struct Plan {
    Rays rays;
    float *o_ndc, *d_ndc;
    Samples coarse, fine;
    ViewMaps left_out;
    float* embedded;
    void* net_ws;
    size_t net_ws_bytes;
    int net_rows;
    size_t bytes;
};

Plan carve(const plnerf_step_config* c, const plnerf_anyview_io* io, int cols, void* workspace) {
    const size_t R = (size_t)c->max_rays, S = (size_t)c->n_samples, F = S + (size_t)c->n_importance;
    const bool noise = c->raw_noise_std > 0.0f;
    Carver w{(unsigned char*)workspace, 0};
    Plan p{};
    p.rays = w.rays(R);
    p.o_ndc = w.floats(c->ndc ? 3 * R : 0); p.d_ndc = w.floats(c->ndc ? 3 * R : 0);
    p.coarse = w.samples(R, S, noise);
    p.fine = w.samples(R, F, noise);
    p.left_out = w.view_maps(R);
    if (generic(io->coarse) || generic(io->fine)) {
        const size_t most = R * F;      // (check_pass: inside an int)
        p.net_rows = most < (size_t)io->max_net_rows ? (int)most : io->max_net_rows;
        p.embedded = w.floats((size_t)p.net_rows * (size_t)cols);
        const size_t bc = net_workspace_bytes(io->coarse, p.net_rows), bf = net_workspace_bytes(io->fine, p.net_rows);
        p.net_ws_bytes = bc > bf ? bc : bf;
        p.net_ws = w.take<void>(p.net_ws_bytes);
    }
    p.bytes = w.off;
    return p;
}

Pass pass_of(const plnerf_step_config* c, int R, int ray_id0, uint32_t step, const float* t_vals, const float* u_vals) {
    return make_pass(*c, c->mode, c->farcolorfix, 1.0f, 0.0f, R, ray_id0, step, t_vals, u_vals);
}

// Behind plnerf_render_view's checks of the configuration: the routes, max_net_rows, and that both slots read rows of the
// same widths.  No pointer of `io` is followed.
int check_config(const plnerf_step_config* c, const plnerf_anyview_io* io, Encoding& enc) {
    if (!c || !io) return PLNERF_EINVAL;
    const plnerf_anyview_net* slots[2] = {&io->coarse, &io->fine};
    bool fused = false;
    for (const plnerf_anyview_net* n : slots) {
        if (n->route != PLNERF_ANYVIEW_FUSED && !generic(*n)) return PLNERF_EINVAL;
        fused = fused || n->route == PLNERF_ANYVIEW_FUSED;
    }
    Pass ps = pass_of(c, c->max_rays, 0, 0, nullptr, nullptr);
    if (!fused) {      // (nothing runs in the configuration's precision, on its widths or with its forward kernel)
        ps.precision = PLNERF_PREC_FP32; ps.input_ch = 63; ps.input_ch_views = 27; ps.fwd_kernel = PLNERF_FWD_KERNEL_AUTO;
    }
    int rc = check_pass(ps, min_samples(c->mode), 1024, 0);
    if (rc) return rc;
    if (c->H < 1 || c->W < 1 || (c->ndc && !(c->ndc_focal != 0.0)) || !(c->fx != 0.0f) || !(c->fy != 0.0f)) return PLNERF_EINVAL;
    if ((uint64_t)c->H * (uint64_t)c->W > (1ull << 30)) return PLNERF_ERANGE;
    if (io->max_net_rows < 1) return PLNERF_EINVAL;
    const long long most = (long long)c->max_rays * ((long long)c->n_samples + c->n_importance);
    const int net_rows = most < io->max_net_rows ? (int)most : io->max_net_rows;
    enc = Encoding{(c->input_ch - 3) / 6, (c->input_ch_views - 3) / 6, c->input_ch + c->input_ch_views};
    bool first = !fused;
    for (const plnerf_anyview_net* n : slots) {
        if (!generic(*n)) continue;
        Encoding e{};
        if ((rc = check_shape(*n, net_rows, e))) return rc;
        if (!first && (e.L != enc.L || e.M != enc.M)) return PLNERF_EINVAL;
        enc = e;
        first = false;
    }
    return PLNERF_OK;
}

// One network outside the trunk over a pass's K samples per ray, in sub-blocks of at most p.net_rows rows, then that pass's
// density noise.  plnerf_embed_rows takes row i's direction from ray i / K of ITS rows: a sub-block that begins inside a ray
// embeds that ray's remaining rows in a call of their own (fewer than K rows, all of ray 0 of that call), the rest from a ray
// boundary on.
int network_generic(const Pass& ps, const Rays& r, const plnerf_anyview_net& n, const Encoding& e, const Plan& p, const Samples& s,
                    int K, uint32_t noise_stream, plnerf_stream_t stream) {
    int rc;
    const long long total = (long long)ps.R * K;
    for (long long r0 = 0; r0 < total; r0 += p.net_rows) {
        const int rows = total - r0 < p.net_rows ? (int)(total - r0) : p.net_rows;
        const long long ray = r0 / K;
        const int inside = (int)(r0 % K);
        const int head = inside ? (K - inside < rows ? K - inside : rows) : 0;
        if (head)
            STEP_OK(plnerf_embed_rows(s.pts + 3 * r0, r.viewdirs + 3 * ray, nullptr, head, K, e.L, e.M, 0, 1.0f, nullptr, 1.0f,
                                      p.embedded, stream));
        if (rows > head)
            STEP_OK(plnerf_embed_rows(s.pts + 3 * (r0 + head), r.viewdirs + 3 * (ray + (head ? 1 : 0)), nullptr, rows - head, K, e.L,
                                      e.M, 0, 1.0f, nullptr, 1.0f, p.embedded + (size_t)head * e.cols, stream));
        if (n.route == PLNERF_ANYVIEW_CHAIN16)
            STEP_OK(plnerf_generic_fwd(&n.shape, n.params, p.embedded, e.cols, rows, n.precision, p.net_ws, p.net_ws_bytes,
                                       s.raw + 4 * r0, 4, n.status, stream));
        else
            STEP_OK(plnerf_generic_fwd_f32(&n.shape, n.params, p.embedded, e.cols, rows, p.net_ws, p.net_ws_bytes, s.raw + 4 * r0, 4,
                                           stream));
    }
    return density_noise(ps, s, K, noise_stream, stream);
}

}  // namespace

extern "C" size_t plnerf_render_view_any_workspace_bytes(const plnerf_step_config* config, const plnerf_anyview_io* io) {
    Encoding enc{};
    if (check_config(config, io, enc) != PLNERF_OK) return 0;
    return carve(config, io, enc.cols, nullptr).bytes;
}

extern "C" int plnerf_render_view_any(const plnerf_step_config* c, const plnerf_anyview_io* io, const plnerf_view_args* a,
                                      void* workspace, size_t workspace_bytes, plnerf_stream_t stream) {
    // ---- every check first: a refused call enqueues nothing ----
    Encoding enc{};
    int rc = check_config(c, io, enc);
    if (rc) return rc;
    if (!a || !workspace || ((uintptr_t)workspace % ALIGN) != 0) return PLNERF_EINVAL;
    if (a->n_pix < 1 || a->pix0 < 0) return PLNERF_EINVAL;
    if ((uint64_t)a->pix0 + (uint64_t)a->n_pix > (uint64_t)c->H * (uint64_t)c->W) return PLNERF_ERANGE;
    if ((rc = check_slot(io->coarse, enc.cols)) || (rc = check_slot(io->fine, enc.cols))) return rc;
    if (!io->t_vals || !io->rgb || (!c->perturb && !io->u_vals) || (io->depth16 && !io->depth)) return PLNERF_EINVAL;
    const Plan p = carve(c, io, enc.cols, workspace);
    if (workspace_bytes < p.bytes) return PLNERF_EINVAL;
    const plnerf_anyview_net* slots[2] = {&io->coarse, &io->fine};
    for (const plnerf_anyview_net* n : slots)
        if (n->route == PLNERF_ANYVIEW_FUSED && (rc = check_params_aligned(n->fused.params))) return rc;

    const int F = c->n_samples + c->n_importance;
    if (a->pack_weights)
        for (const plnerf_anyview_net* n : slots)
            if (n->route == PLNERF_ANYVIEW_FUSED)
                STEP_OK(plnerf_mlp_pack_weights(n->fused.params, c->precision, c->input_ch, c->input_ch_views, n->fused.packed, stream));
    const int end = a->pix0 + a->n_pix;
    for (int p0 = a->pix0; p0 < end; p0 += c->max_rays) {      // (a ray's global id is its pixel index)
        const int R = end - p0 < c->max_rays ? end - p0 : c->max_rays;
        const Pass ps = pass_of(c, R, p0, a->step, io->t_vals, io->u_vals);
        const ViewMaps m = block_maps(io, (size_t)p0, p.left_out);

        // ---- this block's rays: origins, directions, unit view directions, near / far ----
        Rays r = p.rays;
        STEP_OK(plnerf_view_rays(c->H, c->W, c->fx, c->fy, c->cx, c->cy, a->c2w, p0, R, c->near, c->far, r.o, r.d, r.viewdirs,
                                 r.near, r.far, stream));
        if (c->ndc) {      // (the view directions stay those of the camera-space rays)
            STEP_OK(plnerf_ndc_rays(c->H, c->W, c->ndc_focal, 1.0, r.o, r.d, R, p.o_ndc, p.d_ndc, stream));
            r.o = p.o_ndc; r.d = p.d_ndc;
        }

        // ---- both passes up to the fine network's raw output, each network by its slot's route, then the last stage ----
        const auto by_route = [&](const plnerf_anyview_net& n) {
            return [&, pn = &n](const Samples& s, int K, uint32_t noise_stream) {
                if (pn->route == PLNERF_ANYVIEW_FUSED) return network(ps, r, pn->fused.packed, s, K, noise_stream, stream);
                return network_generic(ps, r, *pn, enc, p, s, K, noise_stream, stream);
            };
        };
        STEP_OK(forward_with(ps, r, by_route(io->coarse), by_route(io->fine), p.coarse, p.fine, m.coarse, stream));
        STEP_OK(plnerf_quad_fwd(p.fine.raw, p.fine.z, r.near, r.far, r.d, p.fine.noise, R, F, ps.mode, ps.color_mode, ps.white_bkgd,
                                ps.farcolorfix, m.fine.rgb, m.fine.disp, m.fine.acc, m.fine.depth, nullptr, nullptr, nullptr,
                                stream));
    }

    // ---- the call's pixels as 8-bit colour and 16-bit depth ----
    if (io->rgb8 || io->depth16) {
        const size_t at = (size_t)a->pix0;
        STEP_OK(plnerf_frame_export(io->rgb8 ? io->rgb + 3 * at : nullptr, io->rgb8 ? io->rgb8 + 3 * at : nullptr,
                                    io->depth16 ? io->depth + at : nullptr, a->depth16_scale,
                                    io->depth16 ? io->depth16 + at : nullptr, a->n_pix, stream));
    }
    return PLNERF_OK;
}
