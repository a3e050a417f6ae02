// plnerf_render_view (include/plnerf_hip_view.h): the pixels of one view as ONE library call.  Per block of at most
// config.max_rays pixels it is the forward half of plnerf_train_step (train_step.hip) with plnerf_view_rays as the ray
// source and nothing saved for a backward -- the launches render() -> batchify_rays() -> render_rays() reach through Python,
// ctypes and torch under torch.no_grad(), with the same arguments, in the same order, on the one stream -- so the two routes
// agree bit for bit.  The maps are written straight into the caller's frame planes at the block's pixel offset; one
// plnerf_frame_export over the call's pixels follows the last block.  The forward up to the fine network and the choice
// between a caller's plane and the workspace are step_common.h's.  No kernel of the path is duplicated here.
#include "step_common.h"
#include "../../include/plnerf_hip_view.h"

namespace {

using namespace plnerf_step;

// The workspace, carved for config.max_rays: one block's rays, samples and raw outputs, and a block of every plane the
// caller may leave out.
struct Plan {
    Rays rays;
    float *o_ndc, *d_ndc;
    Samples coarse, fine;
    ViewMaps left_out;
    size_t bytes;
};

Plan carve(const plnerf_step_config* c, void* workspace) {
    const size_t R = (size_t)c->max_rays, S = (size_t)c->n_samples, F = S + (size_t)c->n_importance;
    const bool noise = c->raw_noise_std > 0.0f;
    Carver w{(unsigned char*)workspace, 0};
    Plan p{};
    p.rays = w.rays(R);
    p.o_ndc = w.floats(c->ndc ? 3 * R : 0); p.d_ndc = w.floats(c->ndc ? 3 * R : 0);
    p.coarse = w.samples(R, S, noise);
    p.fine = w.samples(R, F, noise);
    p.left_out = w.view_maps(R);
    p.bytes = w.off;
    return p;
}

Pass pass_of(const plnerf_step_config* c, int R, int ray_id0, uint32_t step, const float* t_vals, const float* u_vals) {
    return make_pass(*c, c->mode, c->farcolorfix, 1.0f, 0.0f, R, ray_id0, step, t_vals, u_vals);
}

// Behind the shared checks, those of the fields only this entry reads: the view's size and intrinsics, NDC (the ray source,
// the bank and Adam are not its business)
int check_config(const plnerf_step_config* c) {
    if (!c) return PLNERF_EINVAL;
    const int rc = check_pass(pass_of(c, c->max_rays, 0, 0, nullptr, nullptr), min_samples(c->mode), 1024, 0);
    if (rc) return rc;
    if (c->H < 1 || c->W < 1 || (c->ndc && !(c->ndc_focal != 0.0)) || !(c->fx != 0.0f) || !(c->fy != 0.0f)) return PLNERF_EINVAL;
    if ((uint64_t)c->H * (uint64_t)c->W > (1ull << 30)) return PLNERF_ERANGE;
    return PLNERF_OK;
}

}  // namespace

extern "C" size_t plnerf_render_view_workspace_bytes(const plnerf_step_config* config) {
    if (check_config(config) != PLNERF_OK) return 0;
    return carve(config, nullptr).bytes;
}

extern "C" int plnerf_render_view(const plnerf_step_config* c, const plnerf_view_io* io, const plnerf_view_args* a,
                                  void* workspace, size_t workspace_bytes, plnerf_stream_t stream) {
    // ---- every check first: a refused call enqueues nothing ----
    int rc = check_config(c);
    if (rc) return rc;
    if (!io || !a || !workspace || ((uintptr_t)workspace % ALIGN) != 0) return PLNERF_EINVAL;
    if (a->n_pix < 1 || a->pix0 < 0) return PLNERF_EINVAL;
    if ((uint64_t)a->pix0 + (uint64_t)a->n_pix > (uint64_t)c->H * (uint64_t)c->W) return PLNERF_ERANGE;
    if ((rc = check_net(&io->coarse)) || (rc = check_net(&io->fine))) return rc;
    if (!io->t_vals || !io->rgb || (!c->perturb && !io->u_vals) || (io->depth16 && !io->depth)) return PLNERF_EINVAL;
    const Plan p = carve(c, workspace);
    if (workspace_bytes < p.bytes) return PLNERF_EINVAL;
    if ((rc = check_params_aligned(io->coarse.params)) || (rc = check_params_aligned(io->fine.params))) return rc;

    const int F = c->n_samples + c->n_importance;
    if (a->pack_weights) {
        STEP_OK(plnerf_mlp_pack_weights(io->coarse.params, c->precision, c->input_ch, c->input_ch_views, io->coarse.packed, stream));
        STEP_OK(plnerf_mlp_pack_weights(io->fine.params, c->precision, c->input_ch, c->input_ch_views, io->fine.packed, stream));
    }
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

        // ---- both passes up to the fine network's raw output, then the last stage ----
        STEP_OK(forward(ps, r, io->coarse.packed, io->fine.packed, p.coarse, p.fine, m.coarse, stream));
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
