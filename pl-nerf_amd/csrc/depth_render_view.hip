// plnerf_depth_render_view (include/experimental/plnerf_hip_depthview.h): the pixels of one view of the depth-supervised
// variant as ONE library call.  Per block of at most config.max_rays pixels it is the forward half of plnerf_depth_train_step
// (depth_train_step.hip) with plnerf_depth_view_rays as the ray source and nothing saved for a backward -- the launches
// depth.render() -> batchify_rays() -> render_rays() reach through Python, ctypes and torch under torch.no_grad(), with the
// same arguments, in the same order, on the one stream -- so the two routes agree bit for bit.  The maps and the hypotheses
// are written straight into the caller's frame planes at the block's pixel offset; a block's hypotheses are scored by
// plnerf_sample_error while they are there; the exports over the call's pixels follow the last block.  No kernel of the
// path is duplicated here.
#include "step_common.h"
#include "../../include/experimental/plnerf_hip_depthview.h"

namespace {

using namespace plnerf_step;      // ALIGN, NOISE_STREAM, scale2, Carver, check_params_aligned

// The workspace, carved for config.max_rays: one block's rays, samples and raw outputs, what the last stage has to write
// besides the maps (its weights and knots, the hypotheses' search indices), the sampling error's partial rows, and a block
// of every plane the caller may leave out.
struct Plan {
    float *rays_o, *rays_d, *viewdirs, *near, *far;
    float *z_c, *pts_c, *raw_c, *noise_c, *z_f, *pts_f, *raw_f, *noise_f;
    float *w, *tau, *T, *hyp;
    int64_t* inds;
    void* err_ws;
    float *disp, *acc, *depth, *rgb0, *disp0, *acc0, *depth0, *z_std;
    size_t bytes;
};

Plan carve(const plnerf_depth_view_config* c, void* workspace) {
    const size_t R = (size_t)c->max_rays, S = (size_t)c->n_samples, N = (size_t)c->n_importance, F = S + N;
    const bool noise = c->raw_noise_std > 0.0f;
    Carver w{(unsigned char*)workspace, 0};
    Plan p{};
    p.rays_o = w.floats(3 * R); p.rays_d = w.floats(3 * R); p.viewdirs = w.floats(3 * R);
    p.near = w.floats(R); p.far = w.floats(R);
    p.z_c = w.floats(R * S); p.pts_c = w.floats(3 * R * S); p.raw_c = w.floats(4 * R * S);
    p.noise_c = w.floats(noise ? R * S : 0);
    p.z_f = w.floats(R * F); p.pts_f = w.floats(3 * R * F); p.raw_f = w.floats(4 * R * F);
    p.noise_f = w.floats(noise ? R * F : 0);
    // (the depth step's planes: linear mode weights [R,F+1], tau / T [R,F+2]; constant mode weights [R,F] in the tau plane,
    // bins [R,F-1] in the T plane)
    p.w = w.floats(R * (F + 1)); p.tau = w.floats(R * (F + 2)); p.T = w.floats(R * (F + 2));
    p.hyp = w.floats(R * N);
    p.inds = w.take<int64_t>(R * N * sizeof(int64_t));
    p.err_ws = w.take<void>(plnerf_sample_error_workspace_bytes(c->max_rays));
    p.disp = w.floats(R); p.acc = w.floats(R); p.depth = w.floats(R);
    p.rgb0 = w.floats(3 * R); p.disp0 = w.floats(R); p.acc0 = w.floats(R); p.depth0 = w.floats(R); p.z_std = w.floats(R);
    p.bytes = w.off;
    return p;
}

// plnerf_depth_train_step's checks of the fields this call reads
int check_config(const plnerf_depth_view_config* c) {
    if (!c) return PLNERF_EINVAL;
    if (c->mode != PLNERF_MODE_LINEAR && c->mode != PLNERF_MODE_CONSTANT) return PLNERF_EINVAL;
    if (c->max_rays < 1 || c->n_samples < (c->mode == PLNERF_MODE_LINEAR ? 2 : 3) || c->n_importance < 1) return PLNERF_EINVAL;
    // (each count on its own first: their sum below is then far from INT_MAX)
    if (c->n_samples > PLNERF_MAX_SAMPLES || c->n_importance > PLNERF_MAX_SAMPLES) return PLNERF_ERANGE;
    if (c->color_mode != PLNERF_COLOR_MIDPOINT && c->color_mode != PLNERF_COLOR_LEFT) return PLNERF_EINVAL;
    if (c->H < 1 || c->W < 1) return PLNERF_EINVAL;
    if (c->fwd_kernel != PLNERF_FWD_KERNEL_AUTO && c->fwd_kernel != PLNERF_FWD_KERNEL_RR && c->fwd_kernel != PLNERF_FWD_KERNEL_PP)
        return PLNERF_EINVAL;
    if (!(c->raw_noise_std >= 0.0f) || !(c->density_beta >= 0.0f) || !(c->input_scale > 0.0f)) return PLNERF_EINVAL;
    // the in-kernel encoding's widths (plnerf_mlp_fwd without `embedded`)
    if (c->input_ch < 3 || c->input_ch > 63 || (c->input_ch - 3) % 6 != 0 || c->input_ch_views < 3 || c->input_ch_views > 27 ||
        (c->input_ch_views - 3) % 6 != 0)
        return PLNERF_EINVAL;
    if (plnerf_mlp_packed_bytes(c->precision) == 0) return PLNERF_ENOSYS;
    // (the last stage runs the quadrature over all n_samples + n_importance depths: plnerf_fine_epilogue's limit; the
    // sampling error takes up to PLNERF_SAMPLEERR_MAX_N hypotheses, which that limit implies)
    if (c->n_samples + c->n_importance > PLNERF_MAX_SAMPLES) return PLNERF_ERANGE;
    if ((uint64_t)c->H * (uint64_t)c->W > (1ull << 30)) return PLNERF_ERANGE;
    // (row counts are ints throughout the ABI)
    if ((uint64_t)c->max_rays * (uint64_t)(c->n_samples + c->n_importance + 2) > (uint64_t)INT32_MAX / 4) return PLNERF_ERANGE;
    return PLNERF_OK;
}

int check_net(const plnerf_view_net* n) {
    if (!n->packed) return PLNERF_EINVAL;
    for (int i = 0; i < PLNERF_N_PARAM_TENSORS; ++i)
        if (!n->params[i]) return PLNERF_EINVAL;
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

    hipStream_t st = (hipStream_t)stream;
    const int S = c->n_samples, N = c->n_importance, F = S + N;
    const int prec = c->precision, xyz = c->input_ch, dir = c->input_ch_views;
    const int white = c->white_bkgd ? 1 : 0;
    const bool noise = c->raw_noise_std > 0.0f, constant = c->mode == PLNERF_MODE_CONSTANT, score = io->valid != nullptr;
    const float beta = c->density_beta;
#define VIEW_OK(call) do { rc = (call); if (rc) return rc; } while (0)

    if (a->pack_weights) {
        VIEW_OK(plnerf_mlp_pack_weights(io->coarse.params, prec, xyz, dir, io->coarse.packed, stream));
        VIEW_OK(plnerf_mlp_pack_weights(io->fine.params, prec, xyz, dir, io->fine.packed, stream));
    }
    const int end = a->pix0 + a->n_pix;
    for (int p0 = a->pix0; p0 < end; p0 += c->max_rays) {      // (a ray's global id is its pixel index)
        const int R = end - p0 < c->max_rays ? end - p0 : c->max_rays;
        const size_t at = (size_t)p0;
        // a plane the caller left out: this block's values go to the workspace
        float* rgb = io->rgb + 3 * at;
        float* disp = io->disp ? io->disp + at : p.disp;
        float* acc = io->acc ? io->acc + at : p.acc;
        float* depth = io->depth ? io->depth + at : p.depth;
        float* rgb0 = io->rgb0 ? io->rgb0 + 3 * at : p.rgb0;
        float* disp0 = io->disp0 ? io->disp0 + at : p.disp0;
        float* acc0 = io->acc0 ? io->acc0 + at : p.acc0;
        float* depth0 = io->depth0 ? io->depth0 + at : p.depth0;
        float* z_std = io->z_std ? io->z_std + at : p.z_std;
        float* hyp = io->pred_hyp ? io->pred_hyp + (size_t)N * at : p.hyp;

        // ---- this block's rays: origins, directions, unit view directions, near / far ----
        VIEW_OK(plnerf_depth_view_rays(c->H, c->W, a->fx, a->fy, a->cx, a->cy, a->c2w, p0, R, c->near, c->far, p.rays_o, p.rays_d,
                                       p.viewdirs, p.near, p.far, stream));
        const float *o = p.rays_o, *d = p.rays_d;

        // ---- coarse pass ----
        VIEW_OK(plnerf_coarse_samples(o, d, p.near, p.far, io->t_vals, nullptr, c->seed, a->step, p0, R, S, c->lindisp ? 1 : 0,
                                      c->perturb ? 1 : 0, p.z_c, p.pts_c, stream));
        VIEW_OK(plnerf_mlp_fwd(io->coarse.packed, prec, p.pts_c, p.viewdirs, nullptr, xyz, dir, R * S, S, c->input_scale, beta,
                               p.raw_c, nullptr, c->fwd_kernel, stream));
        if (noise) {
            VIEW_OK(plnerf_normal(c->seed, NOISE_STREAM, a->step, p0, R, S, p.noise_c, stream));
            if (c->raw_noise_std != 1.0f) VIEW_OK(scale2(p.noise_c, (size_t)R * S, nullptr, 0, c->raw_noise_std, st));
        }
        // (the depth script's raw2outputs ignores farcolorfix: 0 throughout)
        if (!constant)
            VIEW_OK(plnerf_coarse_epilogue(p.raw_c, p.z_c, p.near, p.far, o, d, noise ? p.noise_c : nullptr,
                                           c->perturb ? nullptr : io->u_vals, 0, c->seed, a->step, p0, R, S, N, c->color_mode,
                                           white, 0, c->zero_tol, c->epsilon, rgb0, disp0, acc0, depth0, nullptr, nullptr,
                                           nullptr, p.z_f, p.pts_f, p.z_std, stream));
        else
            VIEW_OK(plnerf_coarse_epilogue_const(p.raw_c, p.z_c, p.near, p.far, o, d, noise ? p.noise_c : nullptr,
                                                 c->perturb ? nullptr : io->u_vals, 0, c->seed, a->step, p0, R, S, N, white, rgb0,
                                                 disp0, acc0, depth0, nullptr, p.z_f, p.pts_f, p.z_std, stream));

        // ---- fine pass; its last stage also draws the depth hypotheses from the final weights (the z_std render_rays
        //      returns is THEIR spread; the importance samples' of the coarse epilogue stayed in the workspace) ----
        VIEW_OK(plnerf_mlp_fwd(io->fine.packed, prec, p.pts_f, p.viewdirs, nullptr, xyz, dir, R * F, F, c->input_scale, beta,
                               p.raw_f, nullptr, c->fwd_kernel, stream));
        if (noise) {
            VIEW_OK(plnerf_normal(c->seed, NOISE_STREAM + 1, a->step, p0, R, F, p.noise_f, stream));
            if (c->raw_noise_std != 1.0f) VIEW_OK(scale2(p.noise_f, (size_t)R * F, nullptr, 0, c->raw_noise_std, st));
        }
        const float* u_in = c->perturb ? nullptr : io->u_vals;      // (NULL: drawn in the kernel, counter stream 4)
        if (!constant)
            VIEW_OK(plnerf_fine_epilogue(p.raw_f, p.z_f, p.near, p.far, d, noise ? p.noise_f : nullptr, u_in, 0, c->seed, a->step,
                                         p0, R, F, N, c->color_mode, white, 0, c->zero_tol, c->epsilon, rgb, disp, acc, depth, p.w,
                                         p.tau, p.T, hyp, p.inds, nullptr, z_std, stream));
        else
            VIEW_OK(plnerf_fine_epilogue_const(p.raw_f, p.z_f, p.near, p.far, d, noise ? p.noise_f : nullptr, u_in, 0, c->seed,
                                               a->step, p0, R, F, N, white, rgb, disp, acc, depth, p.tau, p.T, hyp, p.inds, nullptr,
                                               z_std, stream));

        // ---- the block's term of test_samples_error, while its hypotheses are there ----
        if (score)
            VIEW_OK(plnerf_sample_error(R, N, hyp, depth, io->valid + at, 1, p.err_ws, io->error_row, stream));
    }

    // ---- the call's pixels as 8-bit colour, 16-bit depth / far and 16-bit millimetres ----
    const size_t at = (size_t)a->pix0;
    if (io->rgb8 || io->depth16)
        VIEW_OK(plnerf_frame_export(io->rgb8 ? io->rgb + 3 * at : nullptr, io->rgb8 ? io->rgb8 + 3 * at : nullptr,
                                    io->depth16 ? io->depth + at : nullptr, a->depth16_scale,
                                    io->depth16 ? io->depth16 + at : nullptr, a->n_pix, stream));
    if (io->depth_mm16)
        VIEW_OK(plnerf_frame_export_u16(io->depth + at, a->depth_mm_mult, io->depth_mm16 + at, a->n_pix, stream));
#undef VIEW_OK
    return PLNERF_OK;
}
