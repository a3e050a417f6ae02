// plnerf_train_step (include/plnerf_hip_step.h): one optimisation step of the reference's two-network configuration as ONE
// library call.  The step is the sequence of this library's own entry points that train.TrainStep._step reaches through
// Python, ctypes and torch.autograd on its fused route -- the same launches with the same arguments on the one stream, in
// the same order but for one launch that no launch in between depends on: both networks' weights are packed ahead of the
// coarse samples (there: each network's just before its forward) -- so the two routes agree bit for bit; what the Python
// route does between those launches in torch (the density noise's scale, the loss scale on the two image gradients) is the
// small kernel of step_common.h.  The forward up to the fine network and the backward of both networks are step_common.h's
// too; here are the step's rays, the NVS last stage with its backward, the loss and the optimizers.  No kernel of the path
// is duplicated here.
// plnerf_train_step_const (include/plnerf_hip_conststep.h) is the same sequence in piecewise-constant mode -- the route
// TrainStep._step takes for mode == "constant" and under constant_init: one function serves both, `mode` says which.
// The sequence is written as two halves, up to the complete gradients and the optimizers: a data-parallel caller takes them
// one by one with its exchange in between (include/experimental/plnerf_hip_dpstep.h), the one-call entries back to back.
#include <math.h>

#include "step_common.h"
#include "../../include/plnerf_hip_batching.h"
#include "../../include/plnerf_hip_conststep.h"
#include "../../include/experimental/plnerf_hip_dpstep.h"

namespace {

using namespace plnerf_step;

// The workspace, carved for config.max_rays: the same addresses at every step of a run.
struct Plan {
    void* loss_ws;
    Rays rays;
    float *target, *o_ndc, *d_ndc;
    Samples coarse, fine;
    CoarseMaps maps0;
    FineMaps maps;
    float *g_rgb, *g_rgb0;
    Backward bwd;
    size_t bytes;
};

Plan carve(const plnerf_step_config* c, void* workspace) {
    const size_t R = (size_t)c->max_rays, S = (size_t)c->n_samples, F = S + (size_t)c->n_importance;
    const bool noise = c->raw_noise_std > 0.0f;
    Carver w{(unsigned char*)workspace, 0};
    Plan p{};
    p.loss_ws = w.take<void>(PLNERF_IMAGE_LOSS_WORKSPACE_BYTES);
    p.rays = w.rays(R);
    p.target = w.floats(3 * R);
    p.o_ndc = w.floats(c->ndc ? 3 * R : 0); p.d_ndc = w.floats(c->ndc ? 3 * R : 0);
    p.coarse = w.samples(R, S, noise);
    p.maps0 = w.coarse_maps(R);
    p.fine = w.samples(R, F, noise);
    p.maps = w.fine_maps(R);
    p.g_rgb = w.floats(3 * R); p.g_rgb0 = w.floats(3 * R);
    p.bwd = w.backward(R, S, F, c->precision, &p.coarse, &p.fine, true);
    p.bytes = w.off;
    return p;
}

Pass pass_of(const plnerf_step_config* c, int mode, int R, int ray_id0, uint32_t step, const float* t_vals, const float* u_vals) {
    return make_pass(*c, mode, c->farcolorfix, 1.0f, 0.0f, R, ray_id0, step, t_vals, u_vals);
}

// mode: the entry's (plnerf_train_step: PLNERF_MODE_LINEAR; plnerf_train_step_const: PLNERF_MODE_CONSTANT).  Behind the
// shared checks, those of the fields only the steps read: the mode field, the ray source and the bank.
int check_config(const plnerf_step_config* c, const int mode) {
    if (!c) return PLNERF_EINVAL;
    const int rc = check_pass(pass_of(c, mode, c->max_rays, 0, 0, nullptr, nullptr), min_samples(mode), 1024, 0);
    if (rc) return rc;
    if (c->mode != mode) return PLNERF_EINVAL;
    if (c->ray_source != PLNERF_STEP_RAYS_VIEW && c->ray_source != PLNERF_STEP_RAYS_BANK) return PLNERF_EINVAL;
    if (c->H < 1 || c->W < 1 || (c->ndc && !(c->ndc_focal != 0.0))) return PLNERF_EINVAL;
    if (c->ray_source == PLNERF_STEP_RAYS_BANK && c->n_views < 1) return PLNERF_EINVAL;
    return PLNERF_OK;
}

// The step in two halves (include/experimental/plnerf_hip_dpstep.h): `grads` ends with both networks' gradients complete,
// `apply` is the optimizers.  A data-parallel caller sums the gradients over the ranks in between; the one-call entries are
// grads + apply(1.0f).

// apply's own checks (with_config: not behind grads' checks, which have looked at the structs already)
int check_apply(const plnerf_step_config* c, const plnerf_step_io* io, const plnerf_step_args* a, const float grad_scale,
                const bool with_config) {
    int rc;
    if (with_config) {
        if (!c || !io || !a) return PLNERF_EINVAL;
        if ((rc = check_config(c, c->mode))) return rc;
    }
    if (!(grad_scale > 0.0f) || !isfinite(grad_scale)) return PLNERF_EINVAL;
    if (a->adam_step_fine < 1 || a->adam_step_coarse < 1) return PLNERF_EINVAL;
    if (with_config && ((rc = check_net(&io->coarse)) || (rc = check_net(&io->fine)))) return rc;
    return PLNERF_OK;
}

// both optimizers, the fine network's first (run_plnerf.py:1302-1303)
int enqueue_apply(const plnerf_step_config* c, const plnerf_step_io* io, const plnerf_step_args* a, const float grad_scale,
                  plnerf_stream_t stream) {
    int rc;
    STEP_OK(plnerf_adam_step(io->fine.param_flat, io->fine.grad_flat, io->fine.exp_avg, io->fine.exp_avg_sq, io->fine.n_params,
                             a->lr_fine, c->beta1, c->beta2, c->adam_eps, a->adam_step_fine, grad_scale, 0.0f, io->fine.skip_if_set,
                             io->fine.skip_if_set2, io->fine.withheld, stream));
    STEP_OK(plnerf_adam_step(io->coarse.param_flat, io->coarse.grad_flat, io->coarse.exp_avg, io->coarse.exp_avg_sq,
                             io->coarse.n_params, a->lr_coarse, c->beta1, c->beta2, c->adam_eps, a->adam_step_coarse, grad_scale,
                             0.0f, io->coarse.skip_if_set, io->coarse.skip_if_set2, io->coarse.withheld, stream));
    return PLNERF_OK;
}

// whole_step: the one-call entry, whose optimizer launches follow -- their checks stand where they always stood
int train_step_grads(const plnerf_step_config* c, const plnerf_step_io* io, const plnerf_step_args* a, void* workspace,
                     size_t workspace_bytes, plnerf_stream_t stream, const int mode, const bool whole_step) {
    // ---- every check first: a refused call enqueues nothing ----
    int rc = check_config(c, mode);
    if (rc) return rc;
    if (!io || !a || !workspace || ((uintptr_t)workspace % ALIGN) != 0) return PLNERF_EINVAL;
    if (a->rays < 1 || a->rays > c->max_rays || a->ray_id0 < 0) return PLNERF_EINVAL;
    if (whole_step && (rc = check_apply(c, io, a, 1.0f, false))) return rc;
    if ((rc = check_net(&io->coarse)) || (rc = check_net(&io->fine))) return rc;
    if (!io->t_vals || !io->loss4 || (!c->perturb && !io->u_vals)) return PLNERF_EINVAL;
    const int R = a->rays;
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
    const Pass ps = pass_of(c, mode, R, a->ray_id0, a->step, io->t_vals, io->u_vals);
    const int F = ps.S + ps.N;

    // ---- this step's rays: origins, directions, unit view directions, near / far, target colours ----
    Rays r = p.rays;
    if (c->ray_source == PLNERF_STEP_RAYS_VIEW)
        STEP_OK(plnerf_select_rays(c->H, c->W, c->fx, c->fy, c->cx, c->cy, a->c2w, a->image, a->crop_r0, a->crop_c0, a->crop_rows,
                                   a->crop_cols, c->seed, a->step, a->ray_id0, R, c->near, c->far, r.o, r.d, r.viewdirs, r.near,
                                   r.far, p.target, nullptr, stream));
    else
        STEP_OK(plnerf_select_bank_rays(c->n_views, io->views, c->H, c->W, c->fx, c->fy, c->cx, c->cy, io->poses, io->images,
                                        c->bank_seed, a->epoch, a->pos0, R, c->near, c->far, r.o, r.d, r.viewdirs, r.near, r.far,
                                        p.target, nullptr, stream));
    if (c->ndc) {      // (the view directions stay those of the camera-space rays)
        STEP_OK(plnerf_ndc_rays(c->H, c->W, c->ndc_focal, 1.0, r.o, r.d, R, p.o_ndc, p.d_ndc, stream));
        r.o = p.o_ndc; r.d = p.d_ndc;
    }

    // ---- both passes up to the fine network's raw output, then the last stage ----
    STEP_OK(plnerf_mlp_pack_weights(io->coarse.params, ps.precision, ps.input_ch, ps.input_ch_views, io->coarse.packed, stream));
    STEP_OK(plnerf_mlp_pack_weights(io->fine.params, ps.precision, ps.input_ch, ps.input_ch_views, io->fine.packed, stream));
    // (the fine pass's route, decided once for the forward and the backward's fold)
    Backward bwd = p.bwd;
    if (!unique_pass(ps, F, true, bwd.uniq_f)) bwd.uniq_f = nullptr;
    STEP_OK(forward(ps, r, io->coarse.packed, io->fine.packed, p.coarse, p.fine, p.maps0, stream, bwd.uniq_f));
    STEP_OK(plnerf_quad_fwd(p.fine.raw, p.fine.z, r.near, r.far, r.d, p.fine.noise, R, F, mode, ps.color_mode, ps.white_bkgd,
                            ps.farcolorfix, p.maps.rgb, p.maps.disp, p.maps.acc, p.maps.depth, nullptr, nullptr, nullptr, stream));

    // ---- loss and its two image gradients ----
    STEP_OK(plnerf_image_loss(p.maps.rgb, p.maps0.rgb0, p.target, R, io->loss4, p.g_rgb, p.g_rgb0, nullptr, p.loss_ws, stream));
    if (a->loss_scale != 1.0f) STEP_OK(scale2(p.g_rgb, (size_t)R * 3, p.g_rgb0, (size_t)R * 3, a->loss_scale, st));

    // ---- backward: d loss / d raw of either pass (the fine one first, as autograd orders them), then both networks at once ----
    STEP_OK(plnerf_quad_bwd(p.fine.raw, p.fine.z, r.near, r.far, r.d, p.fine.noise, R, F, mode, ps.color_mode, ps.white_bkgd,
                            ps.farcolorfix, p.g_rgb, nullptr, nullptr, nullptr, nullptr, nullptr, p.bwd.g_raw_f, p.bwd.absmax_f,
                            stream));
    return backward_nets(ps, r, p.coarse, p.fine, p.g_rgb0, bwd, layout, &io->coarse, &io->fine, stream);
}

int train_step(const plnerf_step_config* c, const plnerf_step_io* io, const plnerf_step_args* a, void* workspace,
               size_t workspace_bytes, plnerf_stream_t stream, const int mode) {
    const int rc = train_step_grads(c, io, a, workspace, workspace_bytes, stream, mode, true);
    return rc ? rc : enqueue_apply(c, io, a, 1.0f, stream);
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

// ---- the two halves on their own (include/experimental/plnerf_hip_dpstep.h) ----
extern "C" int plnerf_train_step_grads(const plnerf_step_config* c, const plnerf_step_io* io, const plnerf_step_args* a,
                                       void* workspace, size_t workspace_bytes, plnerf_stream_t stream) {
    return train_step_grads(c, io, a, workspace, workspace_bytes, stream, PLNERF_MODE_LINEAR, false);
}

extern "C" int plnerf_train_step_const_grads(const plnerf_step_config* c, const plnerf_step_io* io, const plnerf_step_args* a,
                                             void* workspace, size_t workspace_bytes, plnerf_stream_t stream) {
    return train_step_grads(c, io, a, workspace, workspace_bytes, stream, PLNERF_MODE_CONSTANT, false);
}

extern "C" int plnerf_train_step_apply(const plnerf_step_config* c, const plnerf_step_io* io, const plnerf_step_args* a,
                                       float grad_scale, plnerf_stream_t stream) {
    const int rc = check_apply(c, io, a, grad_scale, true);
    return rc ? rc : enqueue_apply(c, io, a, grad_scale, stream);
}
