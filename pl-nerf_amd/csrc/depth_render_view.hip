// plnerf_depth_render_view (include/experimental/plnerf_hip_depthview.h): the pixels of one view of the depth-supervised
// variant as ONE library call.  Per block of at most config.max_rays pixels it is the forward half of plnerf_depth_train_step
// (depth_train_step.hip) with plnerf_depth_view_rays as the ray source and nothing saved for a backward -- the launches
// depth.render() -> batchify_rays() -> render_rays() reach through Python, ctypes and torch under torch.no_grad(), with the
// same arguments, in the same order, on the one stream -- so the two routes agree bit for bit.  The maps and the hypotheses
// are written straight into the caller's frame planes at the block's pixel offset; a block's hypotheses are scored by
// plnerf_sample_error while they are there; the exports over the call's pixels follow the last block.  The forward, the
// last stage and the choice between a caller's plane and the workspace are step_common.h's.  No kernel of the path is
// duplicated here.
#include "step_common.h"
#include "../../include/experimental/plnerf_hip_depthview.h"

namespace {

using namespace plnerf_step;

// The workspace, carved for config.max_rays: one block's rays, samples and raw outputs, what the last stage has to write
// besides the maps (its weights and knots, the hypotheses' search indices), the sampling error's partial rows, and a block
// of every plane the caller may leave out.
struct Plan {
    Rays rays;
    Samples coarse, fine;
    HypPlanes hyp;
    void* err_ws;
    ViewMaps left_out;
    size_t bytes;
};

Plan carve(const plnerf_depth_view_config* c, void* workspace) {
    const size_t R = (size_t)c->max_rays, S = (size_t)c->n_samples, N = (size_t)c->n_importance, F = S + N;
    const bool noise = c->raw_noise_std > 0.0f;
    Carver w{(unsigned char*)workspace, 0};
    Plan p{};
    p.rays = w.rays(R);
    p.coarse = w.samples(R, S, noise);
    p.fine = w.samples(R, F, noise);
    // (the depth step's planes; no u_used: no backward follows, and z_std is a left-out plane)
    p.hyp.w = w.floats(R * (F + 1)); p.hyp.tau = w.floats(R * (F + 2)); p.hyp.T = w.floats(R * (F + 2));
    p.hyp.hyp = w.floats(R * N);
    p.hyp.inds = w.take<int64_t>(R * N * sizeof(int64_t));
    p.err_ws = w.take<void>(plnerf_sample_error_workspace_bytes(c->max_rays));
    p.left_out = w.view_maps(R);
    p.bytes = w.off;
    return p;
}

// (the depth script's raw2outputs ignores farcolorfix: 0 throughout)
Pass pass_of(const plnerf_depth_view_config* c, int R, int ray_id0, uint32_t step, const float* t_vals, const float* u_vals) {
    return make_pass(*c, c->mode, 0, c->input_scale, c->density_beta, R, ray_id0, step, t_vals, u_vals);
}

// Behind the shared checks (the last stage runs the quadrature over all n_samples + n_importance depths, plnerf_fine_epilogue's
// limit, on planes of two columns more; the sampling error takes up to PLNERF_SAMPLEERR_MAX_N hypotheses, which that limit
// implies), the view's size
int check_config(const plnerf_depth_view_config* c) {
    if (!c) return PLNERF_EINVAL;
    const int rc = check_pass(pass_of(c, c->max_rays, 0, 0, nullptr, nullptr), min_samples(c->mode), PLNERF_MAX_SAMPLES, 2);
    if (rc) return rc;
    if (c->H < 1 || c->W < 1) return PLNERF_EINVAL;
    if ((uint64_t)c->H * (uint64_t)c->W > (1ull << 30)) return PLNERF_ERANGE;
    return PLNERF_OK;
}

}  // namespace

extern "C" size_t plnerf_depth_render_view_workspace_bytes(const plnerf_depth_view_config* config) {
    if (check_config(config) != PLNERF_OK) return 0;
    return carve(config, nullptr).bytes;
}

extern "C" int plnerf_depth_render_view(const plnerf_depth_view_config* c, const plnerf_depth_view_io* io,
                                        const plnerf_depth_view_args* a, void* workspace, size_t workspace_bytes,
                                        plnerf_stream_t stream) {
    // ---- every check first: a refused call enqueues nothing ----
    int rc = check_config(c);
    if (rc) return rc;
    if (!io || !a || !workspace || ((uintptr_t)workspace % ALIGN) != 0) return PLNERF_EINVAL;
    if (a->n_pix < 1 || a->pix0 < 0 || !(a->fx != 0.0f) || !(a->fy != 0.0f)) return PLNERF_EINVAL;
    if ((uint64_t)a->pix0 + (uint64_t)a->n_pix > (uint64_t)c->H * (uint64_t)c->W) return PLNERF_ERANGE;
    if ((rc = check_net(&io->coarse)) || (rc = check_net(&io->fine))) return rc;
    if (!io->t_vals || !io->rgb || (!c->perturb && !io->u_vals)) return PLNERF_EINVAL;
    if ((io->valid == nullptr) != (io->error_row == nullptr)) return PLNERF_EINVAL;
    if ((io->depth16 || io->depth_mm16) && !io->depth) return PLNERF_EINVAL;
    // (neither plnerf_frame_export nor plnerf_sample_error looks at these: a misaligned pointer must not reach a kernel)
    if (((uintptr_t)io->depth16 % 2) != 0 || ((uintptr_t)io->depth_mm16 % 2) != 0 || ((uintptr_t)io->error_row % 8) != 0)
        return PLNERF_EINVAL;
    const Plan p = carve(c, workspace);
    if (workspace_bytes < p.bytes) return PLNERF_EINVAL;
    if ((rc = check_params_aligned(io->coarse.params)) || (rc = check_params_aligned(io->fine.params))) return rc;

    const int N = c->n_importance;
    const bool score = io->valid != nullptr;
    if (a->pack_weights) {
        STEP_OK(plnerf_mlp_pack_weights(io->coarse.params, c->precision, c->input_ch, c->input_ch_views, io->coarse.packed, stream));
        STEP_OK(plnerf_mlp_pack_weights(io->fine.params, c->precision, c->input_ch, c->input_ch_views, io->fine.packed, stream));
    }
    const float* u_in = c->perturb ? nullptr : io->u_vals;      // (NULL: drawn in the kernel, counter stream 4)
    const int end = a->pix0 + a->n_pix;
    for (int p0 = a->pix0; p0 < end; p0 += c->max_rays) {      // (a ray's global id is its pixel index)
        const int R = end - p0 < c->max_rays ? end - p0 : c->max_rays;
        const size_t at = (size_t)p0;
        const Pass ps = pass_of(c, R, p0, a->step, io->t_vals, io->u_vals);
        const ViewMaps m = block_maps(io, at, p.left_out);
        // (the z_std render_rays returns is the HYPOTHESES' spread: the importance samples' of the coarse epilogue stays in
        // the workspace)
        CoarseMaps maps0 = m.coarse;
        maps0.z_std = p.left_out.coarse.z_std;
        HypPlanes h = p.hyp;
        h.z_std = m.coarse.z_std;
        if (io->pred_hyp) h.hyp = io->pred_hyp + (size_t)N * at;

        // ---- this block's rays: origins, directions, unit view directions, near / far ----
        STEP_OK(plnerf_depth_view_rays(c->H, c->W, a->fx, a->fy, a->cx, a->cy, a->c2w, p0, R, c->near, c->far, p.rays.o, p.rays.d,
                                       p.rays.viewdirs, p.rays.near, p.rays.far, stream));

        // ---- both passes up to the fine network's raw output; the last stage also draws the depth hypotheses from the
        //      final weights ----
        STEP_OK(forward(ps, p.rays, io->coarse.packed, io->fine.packed, p.coarse, p.fine, maps0, stream));
        STEP_OK(depth_last_stage(ps, p.rays, p.fine, u_in, m.fine, h, stream));

        // ---- the block's term of test_samples_error, while its hypotheses are there ----
        if (score)
            STEP_OK(plnerf_sample_error(R, N, h.hyp, m.fine.depth, io->valid + at, 1, p.err_ws, io->error_row, stream));
    }

    // ---- the call's pixels as 8-bit colour, 16-bit depth / far and 16-bit millimetres ----
    const size_t at = (size_t)a->pix0;
    if (io->rgb8 || io->depth16)
        STEP_OK(plnerf_frame_export(io->rgb8 ? io->rgb + 3 * at : nullptr, io->rgb8 ? io->rgb8 + 3 * at : nullptr,
                                    io->depth16 ? io->depth + at : nullptr, a->depth16_scale,
                                    io->depth16 ? io->depth16 + at : nullptr, a->n_pix, stream));
    if (io->depth_mm16)
        STEP_OK(plnerf_frame_export_u16(io->depth + at, a->depth_mm_mult, io->depth_mm16 + at, a->n_pix, stream));
    return PLNERF_OK;
}
