// plnerf_train_step (include/plnerf_hip_step.h): one optimisation step of the reference's two-network configuration as ONE
// library call.  The step is the sequence of this library's own entry points that train.TrainStep._step reaches through
// Python, ctypes and torch.autograd on its fused route -- the same launches with the same arguments, in the same order, on
// the one stream -- so the two routes agree bit for bit; what the Python route does between those launches in torch (the
// density noise's scale, the loss scale on the two image gradients) is the small kernel of step_common.h.  No kernel of the
// path is duplicated here.
// plnerf_train_step_const (include/plnerf_hip_conststep.h) is the same sequence in piecewise-constant mode -- the route
// TrainStep._step takes for mode == "constant" and under constant_init: one function serves both, `mode` says which.
#include "step_common.h"
#include "../../include/plnerf_hip_batching.h"
#include "../../include/plnerf_hip_conststep.h"

namespace {

using namespace plnerf_step;      // ALIGN, NOISE_STREAM, scale2, Carver, check_net (shared with depth_train_step.hip)

// The workspace, carved for config.max_rays: the same addresses at every step of a run.
struct Plan {
    void* loss_ws;
    float *rays_o, *rays_d, *viewdirs, *near, *far, *target, *o_ndc, *d_ndc;
    float *z_c, *pts_c, *raw_c, *noise_c, *rgb0, *disp0, *acc0, *depth0, *z_std;
    float *z_f, *pts_f, *raw_f, *noise_f, *rgb, *disp, *acc, *depth;
    float *g_rgb, *g_rgb0, *g_raw_c, *g_raw_f;
    uint32_t *absmax_c, *absmax_f;
    void *saved_c, *saved_f, *bwd_c, *bwd_f;
    size_t bytes;
};

Plan carve(const plnerf_step_config* c, void* workspace) {
    const size_t R = (size_t)c->max_rays, S = (size_t)c->n_samples, F = S + (size_t)c->n_importance;
    const bool noise = c->raw_noise_std > 0.0f;
    Carver w{(unsigned char*)workspace, 0};
    Plan p{};
    p.loss_ws = w.take<void>(PLNERF_IMAGE_LOSS_WORKSPACE_BYTES);
    p.rays_o = w.floats(3 * R); p.rays_d = w.floats(3 * R); p.viewdirs = w.floats(3 * R);
    p.near = w.floats(R); p.far = w.floats(R); p.target = w.floats(3 * R);
    p.o_ndc = w.floats(c->ndc ? 3 * R : 0); p.d_ndc = w.floats(c->ndc ? 3 * R : 0);
    p.z_c = w.floats(R * S); p.pts_c = w.floats(3 * R * S); p.raw_c = w.floats(4 * R * S);
    p.noise_c = w.floats(noise ? R * S : 0);
    p.rgb0 = w.floats(3 * R); p.disp0 = w.floats(R); p.acc0 = w.floats(R); p.depth0 = w.floats(R); p.z_std = w.floats(R);
    p.z_f = w.floats(R * F); p.pts_f = w.floats(3 * R * F); p.raw_f = w.floats(4 * R * F);
    p.noise_f = w.floats(noise ? R * F : 0);
    p.rgb = w.floats(3 * R); p.disp = w.floats(R); p.acc = w.floats(R); p.depth = w.floats(R);
    p.g_rgb = w.floats(3 * R); p.g_rgb0 = w.floats(3 * R);
    p.g_raw_c = w.floats(4 * R * S); p.g_raw_f = w.floats(4 * R * F);
    const size_t groups = (R + PLNERF_QUAD_RAYS_PER_GROUP - 1) / PLNERF_QUAD_RAYS_PER_GROUP;
    p.absmax_c = w.take<uint32_t>(groups * sizeof(uint32_t)); p.absmax_f = w.take<uint32_t>(groups * sizeof(uint32_t));
    p.saved_c = w.take<void>(plnerf_mlp_saved_bytes((int)(R * S), c->precision));
    p.saved_f = w.take<void>(plnerf_mlp_saved_bytes((int)(R * F), c->precision));
    p.bwd_c = w.take<void>(plnerf_mlp_bwd_workspace_bytes((int)(R * S), c->precision));
    p.bwd_f = w.take<void>(plnerf_mlp_bwd_workspace_bytes((int)(R * F), c->precision));
    p.bytes = w.off;
    return p;
}

// mode: the entry's (plnerf_train_step: PLNERF_MODE_LINEAR; plnerf_train_step_const: PLNERF_MODE_CONSTANT, whose sampler
// needs one interior weight)
int check_config(const plnerf_step_config* c, const int mode) {
    if (!c) return PLNERF_EINVAL;
    if (c->max_rays < 1 || c->n_samples < (mode == PLNERF_MODE_LINEAR ? 2 : 3) || c->n_importance < 1) return PLNERF_EINVAL;
    if (c->mode != mode) return PLNERF_EINVAL;
    if (c->color_mode != PLNERF_COLOR_MIDPOINT && c->color_mode != PLNERF_COLOR_LEFT) return PLNERF_EINVAL;
    if (c->ray_source != PLNERF_STEP_RAYS_VIEW && c->ray_source != PLNERF_STEP_RAYS_BANK) return PLNERF_EINVAL;
    if (c->H < 1 || c->W < 1 || (c->ndc && !(c->ndc_focal != 0.0))) return PLNERF_EINVAL;
    if (c->ray_source == PLNERF_STEP_RAYS_BANK && c->n_views < 1) return PLNERF_EINVAL;
    if (c->fwd_kernel != PLNERF_FWD_KERNEL_AUTO && c->fwd_kernel != PLNERF_FWD_KERNEL_RR && c->fwd_kernel != PLNERF_FWD_KERNEL_PP)
        return PLNERF_EINVAL;
    if (!(c->raw_noise_std >= 0.0f)) return PLNERF_EINVAL;
    // the in-kernel encoding's widths (plnerf_mlp_fwd without `embedded`)
    if (c->input_ch < 3 || c->input_ch > 63 || (c->input_ch - 3) % 6 != 0 || c->input_ch_views < 3 || c->input_ch_views > 27 ||
        (c->input_ch_views - 3) % 6 != 0)
        return PLNERF_EINVAL;
    if (plnerf_mlp_packed_bytes(c->precision) == 0) return PLNERF_ENOSYS;
    if (c->n_samples > PLNERF_MAX_SAMPLES || c->n_samples + c->n_importance > 1024) return PLNERF_ERANGE;
    // (row counts are ints throughout the ABI)
    if ((uint64_t)c->max_rays * (uint64_t)(c->n_samples + c->n_importance) > (uint64_t)INT32_MAX / 4) return PLNERF_ERANGE;
    return PLNERF_OK;
}

int train_step(const plnerf_step_config* c, const plnerf_step_io* io, const plnerf_step_args* a, void* workspace,
               size_t workspace_bytes, plnerf_stream_t stream, const int mode) {
    // ---- every check first: a refused call enqueues nothing ----
    int rc = check_config(c, mode);
    if (rc) return rc;
    if (!io || !a || !workspace || ((uintptr_t)workspace % ALIGN) != 0) return PLNERF_EINVAL;
    if (a->rays < 1 || a->rays > c->max_rays || a->ray_id0 < 0) return PLNERF_EINVAL;
    if (a->adam_step_fine < 1 || a->adam_step_coarse < 1) return PLNERF_EINVAL;
    if ((rc = check_net(&io->coarse)) || (rc = check_net(&io->fine))) return rc;
    if (!io->t_vals || !io->loss4 || (!c->perturb && !io->u_vals)) return PLNERF_EINVAL;
    const int R = a->rays, S = c->n_samples, N = c->n_importance, F = S + N;
    if (c->ray_source == PLNERF_STEP_RAYS_VIEW) {
        if (!a->image) return PLNERF_EINVAL;
        if (a->crop_rows < 1 || a->crop_cols < 1 || a->crop_r0 < 0 || a->crop_c0 < 0 || a->crop_r0 + a->crop_rows > c->H ||
            a->crop_c0 + a->crop_cols > c->W)
            return PLNERF_EINVAL;
        const uint64_t M = (uint64_t)a->crop_rows * (uint64_t)a->crop_cols;
        if (M > (1ull << 30) || (uint64_t)a->ray_id0 + (uint64_t)R > M) return PLNERF_ERANGE;
    } else {
        if (!io->views || !io->poses || !io->images || a->pos0 < 0) return PLNERF_EINVAL;
        const uint64_t M = (uint64_t)c->n_views * (uint64_t)c->H * (uint64_t)c->W;
        if (M > (1ull << 30) || (uint64_t)a->pos0 + (uint64_t)R > M) return PLNERF_ERANGE;
    }
    const Plan p = carve(c, workspace);
    if (workspace_bytes < p.bytes) return PLNERF_EINVAL;
    const int layout = plnerf_mlp_saved_layout(c->precision, 0, c->fwd_kernel);
    if (layout < 0) return layout;
    if ((rc = check_params_aligned(io->coarse.params)) || (rc = check_params_aligned(io->fine.params))) return rc;

    hipStream_t st = (hipStream_t)stream;
    const int prec = c->precision, xyz = c->input_ch, dir = c->input_ch_views;
    const bool noise = c->raw_noise_std > 0.0f;
#define STEP_OK(call) do { rc = (call); if (rc) return rc; } while (0)

    // ---- this step's rays: origins, directions, unit view directions, near / far, target colours ----
    if (c->ray_source == PLNERF_STEP_RAYS_VIEW)
        STEP_OK(plnerf_select_rays(c->H, c->W, c->fx, c->fy, c->cx, c->cy, a->c2w, a->image, a->crop_r0, a->crop_c0, a->crop_rows,
                                   a->crop_cols, c->seed, a->step, a->ray_id0, R, c->near, c->far, p.rays_o, p.rays_d, p.viewdirs,
                                   p.near, p.far, p.target, nullptr, stream));
    else
        STEP_OK(plnerf_select_bank_rays(c->n_views, io->views, c->H, c->W, c->fx, c->fy, c->cx, c->cy, io->poses, io->images,
                                        c->bank_seed, a->epoch, a->pos0, R, c->near, c->far, p.rays_o, p.rays_d, p.viewdirs, p.near,
                                        p.far, p.target, nullptr, stream));
    const float *o = p.rays_o, *d = p.rays_d;
    if (c->ndc) {      // (the view directions stay those of the camera-space rays)
        STEP_OK(plnerf_ndc_rays(c->H, c->W, c->ndc_focal, 1.0, p.rays_o, p.rays_d, R, p.o_ndc, p.d_ndc, stream));
        o = p.o_ndc; d = p.d_ndc;
    }

    // ---- coarse pass ----
    STEP_OK(plnerf_coarse_samples(o, d, p.near, p.far, io->t_vals, nullptr, c->seed, a->step, a->ray_id0, R, S, c->lindisp ? 1 : 0,
                                  c->perturb ? 1 : 0, p.z_c, p.pts_c, stream));
    STEP_OK(plnerf_mlp_pack_weights(io->coarse.params, prec, xyz, dir, io->coarse.packed, stream));
    STEP_OK(plnerf_mlp_fwd(io->coarse.packed, prec, p.pts_c, p.viewdirs, nullptr, xyz, dir, R * S, S, 1.0f, 0.0f, p.raw_c, p.saved_c,
                           c->fwd_kernel, stream));
    if (noise) {
        STEP_OK(plnerf_normal(c->seed, NOISE_STREAM, a->step, a->ray_id0, R, S, p.noise_c, stream));
        if (c->raw_noise_std != 1.0f) STEP_OK(scale2(p.noise_c, (size_t)R * S, nullptr, 0, c->raw_noise_std, st));
    }
    if (mode == PLNERF_MODE_LINEAR)
        STEP_OK(plnerf_coarse_epilogue(p.raw_c, p.z_c, p.near, p.far, o, d, noise ? p.noise_c : nullptr,
                                       c->perturb ? nullptr : io->u_vals, 0, c->seed, a->step, a->ray_id0, R, S, N, c->color_mode,
                                       c->white_bkgd ? 1 : 0, c->farcolorfix ? 1 : 0, c->zero_tol, c->epsilon, p.rgb0, p.disp0,
                                       p.acc0, p.depth0, nullptr, nullptr, nullptr, p.z_f, p.pts_f, p.z_std, stream));
    else
        STEP_OK(plnerf_coarse_epilogue_const(p.raw_c, p.z_c, p.near, p.far, o, d, noise ? p.noise_c : nullptr,
                                             c->perturb ? nullptr : io->u_vals, 0, c->seed, a->step, a->ray_id0, R, S, N,
                                             c->white_bkgd ? 1 : 0, p.rgb0, p.disp0, p.acc0, p.depth0, nullptr, p.z_f, p.pts_f,
                                             p.z_std, stream));

    // ---- fine pass ----
    STEP_OK(plnerf_mlp_pack_weights(io->fine.params, prec, xyz, dir, io->fine.packed, stream));
    STEP_OK(plnerf_mlp_fwd(io->fine.packed, prec, p.pts_f, p.viewdirs, nullptr, xyz, dir, R * F, F, 1.0f, 0.0f, p.raw_f, p.saved_f,
                           c->fwd_kernel, stream));
    if (noise) {
        STEP_OK(plnerf_normal(c->seed, NOISE_STREAM + 1, a->step, a->ray_id0, R, F, p.noise_f, stream));
        if (c->raw_noise_std != 1.0f) STEP_OK(scale2(p.noise_f, (size_t)R * F, nullptr, 0, c->raw_noise_std, st));
    }
    STEP_OK(plnerf_quad_fwd(p.raw_f, p.z_f, p.near, p.far, d, noise ? p.noise_f : nullptr, R, F, mode, c->color_mode,
                            c->white_bkgd ? 1 : 0, c->farcolorfix ? 1 : 0, p.rgb, p.disp, p.acc, p.depth, nullptr, nullptr, nullptr,
                            stream));

    // ---- loss and its two image gradients ----
    STEP_OK(plnerf_image_loss(p.rgb, p.rgb0, p.target, R, io->loss4, p.g_rgb, p.g_rgb0, nullptr, p.loss_ws, stream));
    if (a->loss_scale != 1.0f) STEP_OK(scale2(p.g_rgb, (size_t)R * 3, p.g_rgb0, (size_t)R * 3, a->loss_scale, st));

    // ---- backward: d loss / d raw of either pass (the fine one first, as autograd orders them), then both networks at once ----
    STEP_OK(plnerf_quad_bwd(p.raw_f, p.z_f, p.near, p.far, d, noise ? p.noise_f : nullptr, R, F, mode, c->color_mode,
                            c->white_bkgd ? 1 : 0, c->farcolorfix ? 1 : 0, p.g_rgb, nullptr, nullptr, nullptr, nullptr, nullptr,
                            p.g_raw_f, p.absmax_f, stream));
    STEP_OK(plnerf_quad_bwd(p.raw_c, p.z_c, p.near, p.far, d, noise ? p.noise_c : nullptr, R, S, mode, c->color_mode,
                            c->white_bkgd ? 1 : 0, c->farcolorfix ? 1 : 0, p.g_rgb0, nullptr, nullptr, nullptr, nullptr, nullptr,
                            p.g_raw_c, p.absmax_c, stream));
    const plnerf_step_net* nets[2] = {&io->coarse, &io->fine};
    float* grads[2 * PLNERF_N_PARAM_TENSORS];
    for (int j = 0; j < 2; ++j)
        for (int i = 0; i < PLNERF_N_PARAM_TENSORS; ++i)
            grads[j * PLNERF_N_PARAM_TENSORS + i] = nets[j]->grad_flat + (nets[j]->params[i] - nets[j]->param_flat);
    const int groups = (R + PLNERF_QUAD_RAYS_PER_GROUP - 1) / PLNERF_QUAD_RAYS_PER_GROUP;
    const void* packed[2] = {io->coarse.packed, io->fine.packed};
    const float* g_raw[2] = {p.g_raw_c, p.g_raw_f};
    const uint32_t* absmax[2] = {p.absmax_c, p.absmax_f};
    const int n_absmax[2] = {groups, groups};
    const int n_rows[2] = {R * S, R * F};
    const void* saved[2] = {p.saved_c, p.saved_f};
    const int layouts[2] = {layout, layout};
    void* bwd_ws[2] = {p.bwd_c, p.bwd_f};
    float* status_out[2] = {io->coarse.grad_flat + io->coarse.n_params, io->fine.grad_flat + io->fine.n_params};
    STEP_OK(plnerf_mlp_bwd_multi(2, packed, prec, g_raw, absmax, n_absmax, xyz, dir, n_rows, saved, layouts, nullptr, 0.0f, bwd_ws,
                                 grads, status_out, stream));

    // ---- both optimizers, the fine network's first (run_plnerf.py:1302-1303) ----
    STEP_OK(plnerf_adam_step(io->fine.param_flat, io->fine.grad_flat, io->fine.exp_avg, io->fine.exp_avg_sq, io->fine.n_params,
                             a->lr_fine, c->beta1, c->beta2, c->adam_eps, a->adam_step_fine, 1.0f, 0.0f, io->fine.skip_if_set,
                             io->fine.skip_if_set2, io->fine.withheld, stream));
    STEP_OK(plnerf_adam_step(io->coarse.param_flat, io->coarse.grad_flat, io->coarse.exp_avg, io->coarse.exp_avg_sq,
                             io->coarse.n_params, a->lr_coarse, c->beta1, c->beta2, c->adam_eps, a->adam_step_coarse, 1.0f, 0.0f,
                             io->coarse.skip_if_set, io->coarse.skip_if_set2, io->coarse.withheld, stream));
#undef STEP_OK
    return PLNERF_OK;
}

}  // namespace

extern "C" size_t plnerf_train_step_workspace_bytes(const plnerf_step_config* config) {
    if (check_config(config, PLNERF_MODE_LINEAR) != PLNERF_OK) return 0;
    return carve(config, nullptr).bytes;
}

extern "C" int plnerf_train_step(const plnerf_step_config* c, const plnerf_step_io* io, const plnerf_step_args* a,
                                 void* workspace, size_t workspace_bytes, plnerf_stream_t stream) {
    return train_step(c, io, a, workspace, workspace_bytes, stream, PLNERF_MODE_LINEAR);
}

// ---- piecewise-constant mode (include/plnerf_hip_conststep.h): the same carve, so the same bytes and offsets ----
extern "C" size_t plnerf_train_step_const_workspace_bytes(const plnerf_step_config* config) {
    if (check_config(config, PLNERF_MODE_CONSTANT) != PLNERF_OK) return 0;
    return carve(config, nullptr).bytes;
}

extern "C" int plnerf_train_step_const(const plnerf_step_config* c, const plnerf_step_io* io, const plnerf_step_args* a,
                                       void* workspace, size_t workspace_bytes, plnerf_stream_t stream) {
    return train_step(c, io, a, workspace, workspace_bytes, stream, PLNERF_MODE_CONSTANT);
}
