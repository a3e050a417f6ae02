// plnerf_depth_train_step (include/plnerf_hip_depthstep.h): one iteration of the depth-supervised loop as ONE library call.
// Like plnerf_train_step (train_step.hip) it is the sequence of this library's own entry points that the Python route
// -- depth.DepthTrainStep.step_view on render_rays' fused branch with train.backward_merged -- reaches through Python,
// ctypes and torch.autograd: the same launches with the same arguments on the one stream, in the same order but for two
// launches that no launch in between depends on: both networks' weights are packed ahead of the coarse samples (there:
// each network's just before its forward), and so is is_joint's one row of hypothesis draws drawn (there: between the fine
// forward and the fine pass's noise).  So the two routes agree bit for bit.  The forward, the last stage and the backward of
// both networks are step_common.h's; here are the step's rays, its loss, the last stage's backward and the optimizers.
// The one kernel of its own is the depth scales' and shifts' Adam (plnerf_depth_ss_adam), which stands for the
// torch.optim.Adam over two [V, 1] tensors of that route.
#include <math.h>

#include "step_common.h"
#include "ray_bwd_dev.h"
#include "../../include/plnerf_hip_depthstep.h"
#include "../../include/plnerf_hip_conststep.h"
#include "../../include/experimental/plnerf_hip_dpstep.h"

namespace {

using namespace plnerf_step;

constexpr uint32_t HYP_STREAM = 4;      // functional.FineEpilogueFn.HYP_STREAM: the depth hypotheses' draws

// torch.optim.Adam's update (adam.hip's arithmetic) over scale[V] ++ shift[V] with grad / m / v [2, V]: one workgroup
__global__ __launch_bounds__(256) void ss_adam_kernel(float* __restrict__ scale, float* __restrict__ shift,
                                                      const float* __restrict__ g, float* __restrict__ m,
                                                      float* __restrict__ v, const int V, const float step_size, const float b1,
                                                      const float b2, const float eps, const float bc2_sqrt,
                                                      const float gscale) {
    for (int i = threadIdx.x; i < 2 * V; i += 256) {
        float* p = i < V ? scale + i : shift + (i - V);
        const float gi = g[i] * gscale;
        const float mi = m[i] + (gi - m[i]) * (1.0f - b1);
        const float vi = v[i] * b2 + (1.0f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        *p = *p - step_size * (mi / denom);
    }
}

// The workspace, carved for config.max_rays: the same addresses at every step of a run.
struct Plan {
    void *loss_ws, *ss_ws;
    Rays rays;
    float *target, *target_h, *mask, *hyp_raw;
    int* pixels;
    Samples coarse, fine;
    CoarseMaps maps0;
    float* u_row;
    FineMaps maps;
    HypPlanes hyp;
    float *g_rgb, *g_rgb0, *g_hyp, *g_tau, *g_T;
    Backward bwd;
    size_t bytes;
};

Plan carve(const plnerf_depth_step_config* c, void* workspace) {
    const size_t R = (size_t)c->max_rays, S = (size_t)c->n_samples, N = (size_t)c->n_importance, F = S + N;
    const size_t Hn = (size_t)c->n_hyp;
    const bool noise = c->raw_noise_std > 0.0f;
    Carver w{(unsigned char*)workspace, 0};
    Plan p{};
    p.loss_ws = w.take<void>(PLNERF_DEPTH_LOSS_WORKSPACE_BYTES);
    p.ss_ws = w.take<void>(PLNERF_DEPTH_SS_WORKSPACE_BYTES);
    p.rays = w.rays(R);
    p.target = w.floats(3 * R);
    p.target_h = w.floats(Hn * R); p.mask = w.floats(R); p.hyp_raw = w.floats(Hn * R);
    p.pixels = w.take<int>(2 * R * sizeof(int));
    p.coarse = w.samples(R, S, noise);
    p.maps0 = w.coarse_maps(R);
    p.fine = w.samples(R, F, noise);
    p.u_row = w.floats(c->is_joint && c->perturb ? N : 0);
    p.maps = w.fine_maps(R);
    p.hyp.w = w.floats(R * (F + 1)); p.hyp.tau = w.floats(R * (F + 2)); p.hyp.T = w.floats(R * (F + 2));
    p.hyp.hyp = w.floats(R * N); p.hyp.u_used = c->perturb ? w.floats(R * N) : nullptr; p.hyp.z_std = w.floats(R);
    p.hyp.inds = w.take<int64_t>(R * N * sizeof(int64_t));
    p.g_rgb = w.floats(3 * R); p.g_rgb0 = w.floats(3 * R); p.g_hyp = w.floats(R * N);
    p.g_tau = w.floats(R * (F + 2)); p.g_T = w.floats(R * (F + 2));
    p.bwd = w.backward(R, S, F, c->precision, &p.coarse, &p.fine);
    p.bytes = w.off;
    return p;
}

// (the depth script's raw2outputs ignores farcolorfix: 0 throughout)
Pass pass_of(const plnerf_depth_step_config* c, int mode, int R, int ray_id0, uint32_t step, const float* t_vals,
             const float* u_vals) {
    return make_pass(*c, mode, 0, c->input_scale, c->density_beta, R, ray_id0, step, t_vals, u_vals);
}

// mode: the entry's (PLNERF_MODE_CONSTANT: plnerf_depth_train_step_const).  Behind the shared checks (the last stage runs
// the quadrature over all n_samples + n_importance depths, plnerf_fine_epilogue's limit, on planes of two columns more),
// those of the fields only this step has, and the constant step's limit: its last stage's backward keeps a longer LDS row
// than any kernel of the linear step.
int check_config(const plnerf_depth_step_config* c, const int mode) {
    if (!c) return PLNERF_EINVAL;
    const int rc = check_pass(pass_of(c, mode, c->max_rays, 0, 0, nullptr, nullptr), min_samples(mode), PLNERF_MAX_SAMPLES, 2);
    if (rc) return rc;
    if (c->n_views < 1 || c->H < 1 || c->W < 1 || c->n_hyp < 1 || (c->pose_rows != 3 && c->pose_rows != 4)) return PLNERF_EINVAL;
    if ((uint64_t)c->H * (uint64_t)c->W > (1ull << 30)) return PLNERF_ERANGE;
    if ((uint64_t)c->max_rays * (uint64_t)c->n_hyp > (uint64_t)INT32_MAX / 4) return PLNERF_ERANGE;
    const size_t row_floats = plnerf::fine_const_bwd_row_floats(c->n_samples + c->n_importance, c->n_importance);
    if (mode == PLNERF_MODE_CONSTANT && (size_t)plnerf::RAY_WAVES * row_floats * sizeof(float) > 160 * 1024) return PLNERF_ERANGE;
    return PLNERF_OK;
}

size_t workspace_bytes_of(const plnerf_depth_step_config* config, const int mode) {
    if (check_config(config, mode) != PLNERF_OK) return 0;
    return carve(config, nullptr).bytes;
}

int layout_of(const plnerf_depth_step_config* config, plnerf_depth_step_views* out, const int mode) {
    const int rc = check_config(config, mode);
    if (rc) return rc;
    if (!out) return PLNERF_EINVAL;
    const Plan p = carve(config, nullptr);      // (from a null base the addresses ARE the offsets)
    const auto off = [](const void* q) { return (size_t)(uintptr_t)q; };
    out->rgb = off(p.maps.rgb); out->rgb0 = off(p.maps0.rgb0); out->depth = off(p.maps.depth); out->depth0 = off(p.maps0.depth0);
    out->acc = off(p.maps.acc); out->acc0 = off(p.maps0.acc0); out->disp = off(p.maps.disp); out->disp0 = off(p.maps0.disp0);
    out->z_std = off(p.hyp.z_std); out->pred_hyp = off(p.hyp.hyp); out->z_vals = off(p.fine.z); out->z_vals0 = off(p.coarse.z);
    out->pixels = off(p.pixels); out->target_h = off(p.target_h); out->mask = off(p.mask);
    return PLNERF_OK;
}

}  // namespace

extern "C" int plnerf_depth_ss_adam(float* scale, float* shift, const float* grad, float* exp_avg, float* exp_avg_sq,
                                    int n_views, float lr, float beta1, float beta2, float eps, int step, float grad_scale,
                                    plnerf_stream_t stream) {
    if (!scale || !shift || !grad || !exp_avg || !exp_avg_sq || n_views < 1 || step < 1) return PLNERF_EINVAL;
    if (n_views > (1 << 24)) return PLNERF_ERANGE;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    hipLaunchKernelGGL(ss_adam_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, scale, shift, grad, exp_avg, exp_avg_sq,
                       n_views, (float)((double)lr / bc1), beta1, beta2, eps, (float)sqrt(bc2), grad_scale);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}

namespace {

// The step in two halves (include/experimental/plnerf_hip_dpstep.h), as train_step.hip's: `grads` ends with both networks'
// gradients (and, on a step of theirs, the scales' and shifts') complete, `apply` is the optimizers.

// apply's own checks (with_config: not behind grads' checks, which have looked at the structs already)
int check_apply(const plnerf_depth_step_config* c, const plnerf_depth_step_io* io, const plnerf_depth_step_args* a,
                const float grad_scale, const bool with_config) {
    int rc;
    if (with_config && (!c || !io || !a)) return PLNERF_EINVAL;
    if (!(grad_scale > 0.0f) || !isfinite(grad_scale)) return PLNERF_EINVAL;
    if (a->adam_step < 1) return PLNERF_EINVAL;
    if (with_config) {
        if ((rc = check_net(&io->coarse)) || (rc = check_net(&io->fine))) return rc;
        if (a->ss_step && (c->n_views < 1 || a->ss_adam_step < 1 || !io->scale || !io->shift || !io->ss_grad || !io->ss_exp_avg ||
                           !io->ss_exp_avg_sq))
            return PLNERF_EINVAL;
        if (a->ss_step && c->n_views > (1 << 24)) return PLNERF_ERANGE;      // (plnerf_depth_ss_adam's limit: before the first launch)
    }
    return PLNERF_OK;
}

int enqueue_apply(const plnerf_depth_step_config* c, const plnerf_depth_step_io* io, const plnerf_depth_step_args* a,
                  const float grad_scale, plnerf_stream_t stream) {
    int rc;
    // ---- the one optimizer over both networks: its gradient lies in two runs, the coarse network's first
    //      (optim.FlatAdam.step), clipped inside the kernel (run_nerf_sample_based_depth.py:1155-1157) ----
    const plnerf_step_net* nets[2] = {&io->coarse, &io->fine};
    for (int j = 0; j < 2; ++j)
        STEP_OK(plnerf_adam_step(nets[j]->param_flat, nets[j]->grad_flat, nets[j]->exp_avg, nets[j]->exp_avg_sq, nets[j]->n_params,
                                 a->lr, c->beta1, c->beta2, c->adam_eps, a->adam_step, grad_scale, c->clip_value,
                                 nets[j]->skip_if_set, nets[j]->skip_if_set2, nets[j]->withheld, stream));
    // ---- the depth scales and shifts, unclipped (:1159-1161) ----
    if (a->ss_step)
        STEP_OK(plnerf_depth_ss_adam(io->scale, io->shift, io->ss_grad, io->ss_exp_avg, io->ss_exp_avg_sq, c->n_views, a->ss_lr,
                                     c->ss_beta1, c->ss_beta2, c->ss_adam_eps, a->ss_adam_step, grad_scale, stream));
    return PLNERF_OK;
}

// mode: the entry's.  The Plan is the same in either (depth_last_stage says what lies where).  whole_step: the one-call
// entry, whose optimizer launches follow -- their checks stand where they always stood.
int depth_train_step_grads(const plnerf_depth_step_config* c, const plnerf_depth_step_io* io, const plnerf_depth_step_args* a,
                           void* workspace, size_t workspace_bytes, plnerf_stream_t stream, const int mode,
                           const bool whole_step) {
    // ---- every check first: a refused call enqueues nothing ----
    int rc = check_config(c, mode);
    if (rc) return rc;
    if (!io || !a || !workspace || ((uintptr_t)workspace % ALIGN) != 0) return PLNERF_EINVAL;
    if (a->rays < 1 || a->rays > c->max_rays || a->ray_id0 < 0 || a->view < 0 || a->view >= c->n_views) return PLNERF_EINVAL;
    if (whole_step && (rc = check_apply(c, io, a, 1.0f, false))) return rc;
    if ((rc = check_net(&io->coarse)) || (rc = check_net(&io->fine))) return rc;
    if (!io->t_vals || !io->loss5 || (!c->perturb && !io->u_vals)) return PLNERF_EINVAL;
    if (!io->images || !io->hyp || !io->poses || !io->intrinsics) return PLNERF_EINVAL;
    const bool carve_on = a->carve != 0, ss = a->ss_step != 0;
    if (ss && (!carve_on || (whole_step && a->ss_adam_step < 1) || !io->scale || !io->shift || !io->ss_grad ||
               (whole_step && (!io->ss_exp_avg || !io->ss_exp_avg_sq))))
        return PLNERF_EINVAL;
    if ((uint64_t)a->ray_id0 + (uint64_t)a->rays > (uint64_t)c->H * (uint64_t)c->W) return PLNERF_ERANGE;
    const Plan p = carve(c, workspace);
    if (workspace_bytes < p.bytes) return PLNERF_EINVAL;
    const int layout = plnerf_mlp_saved_layout(c->precision, 0, c->fwd_kernel);
    if (layout < 0) return layout;
    if ((rc = check_params_aligned(io->coarse.params)) || (rc = check_params_aligned(io->fine.params))) return rc;

    const int R = a->rays, N = c->n_importance, F = c->n_samples + N;
    const int joint = c->is_joint ? 1 : 0;
    const Pass ps = pass_of(c, mode, R, a->ray_id0, a->step, io->t_vals, io->u_vals);
    const Rays& r = p.rays;

    // ---- this step's rays of view a->view, their target colours, scaled hypotheses, mask, raw hypotheses and pixels ----
    STEP_OK(plnerf_select_depth_rays(c->n_views, a->view, c->H, c->W, c->n_hyp, io->images, io->hyp, io->valid, io->poses,
                                     c->pose_rows, io->intrinsics, io->scale, io->shift, c->near, c->far, c->seed, a->step,
                                     a->ray_id0, R, r.o, r.d, r.viewdirs, r.near, r.far, p.target, p.target_h, p.mask,
                                     p.hyp_raw, p.pixels, stream));

    // ---- both passes up to the fine network's raw output; the last stage also draws the depth hypotheses from the final
    //      weights ----
    STEP_OK(plnerf_mlp_pack_weights(io->coarse.params, ps.precision, ps.input_ch, ps.input_ch_views, io->coarse.packed, stream));
    STEP_OK(plnerf_mlp_pack_weights(io->fine.params, ps.precision, ps.input_ch, ps.input_ch_views, io->fine.packed, stream));
    // the hypotheses' draws: the table (perturb == 0), one row from the counters of global ray 0 (is_joint), or drawn in
    // the kernel; u_seen / u_seen_stride: what the sampler's backward reads
    const float* u_in = nullptr;
    const float* u_seen = p.hyp.u_used;
    int u_seen_stride = N;
    if (!c->perturb) {
        u_in = u_seen = io->u_vals;
        u_seen_stride = 0;
    } else if (joint) {
        STEP_OK(plnerf_uniform(c->seed, HYP_STREAM, a->step, 0, 1, N, p.u_row, stream));
        u_in = p.u_row;
    }
    STEP_OK(forward(ps, r, io->coarse.packed, io->fine.packed, p.coarse, p.fine, p.maps0, stream));
    STEP_OK(depth_last_stage(ps, r, p.fine, u_in, p.maps, p.hyp, stream));

    // ---- loss and its gradients; the scales' and shifts' gradient from the hypotheses the loss chose ----
    STEP_OK(plnerf_depth_loss(p.maps.rgb, p.maps0.rgb0, p.target, carve_on ? p.hyp.hyp : nullptr, carve_on ? p.target_h : nullptr,
                              carve_on ? p.mask : nullptr, R, carve_on ? N : 1, carve_on ? c->n_hyp : 1, 1, joint, nullptr,
                              c->space_carving_weight, c->space_carving_threshold, io->loss5, p.g_rgb, p.g_rgb0,
                              carve_on ? p.g_hyp : nullptr, p.loss_ws, stream));
    if (ss)
        STEP_OK(plnerf_depth_scale_shift_grad(p.hyp.hyp, p.target_h, p.hyp_raw, p.mask, R, N, c->n_hyp, 1, joint, nullptr,
                                              c->space_carving_weight, c->space_carving_threshold, c->n_views, a->view,
                                              io->ss_grad, io->ss_grad + c->n_views, p.ss_ws, stream));

    // ---- backward: the hypotheses' gradient through the sampler and d loss / d raw of the fine pass (first, as autograd
    //      orders them), then the coarse pass's and both networks at once ----
    if (mode == PLNERF_MODE_CONSTANT) {      // (the sampler's backward, the padded sum and the quadrature's in one launch; without g_hyp the last alone)
        STEP_OK(plnerf_fine_epilogue_const_bwd(p.fine.raw, p.fine.z, r.near, r.far, r.d, p.fine.noise, p.hyp.tau, p.hyp.T, u_seen,
                                               u_seen_stride, p.hyp.inds, R, F, N, ps.white_bkgd, p.g_rgb, nullptr, nullptr, nullptr,
                                               carve_on ? p.g_hyp : nullptr, p.bwd.g_raw_f, p.bwd.absmax_f, stream));
    } else {
        if (carve_on)
            STEP_OK(plnerf_sample_pl_bwd(p.fine.z, p.hyp.tau, p.hyp.T, r.near, r.far, u_seen, u_seen_stride, p.hyp.inds, p.g_hyp, R,
                                         F, N, c->zero_tol, c->epsilon, p.g_tau, p.g_T, stream));
        STEP_OK(plnerf_quad_bwd(p.fine.raw, p.fine.z, r.near, r.far, r.d, p.fine.noise, R, F, PLNERF_MODE_LINEAR, ps.color_mode,
                                ps.white_bkgd, 0, p.g_rgb, nullptr, nullptr, nullptr, carve_on ? p.g_tau : nullptr,
                                carve_on ? p.g_T : nullptr, p.bwd.g_raw_f, p.bwd.absmax_f, stream));
    }
    return backward_nets(ps, r, p.coarse, p.fine, p.g_rgb0, p.bwd, layout, &io->coarse, &io->fine, stream);
}

int depth_train_step(const plnerf_depth_step_config* c, const plnerf_depth_step_io* io, const plnerf_depth_step_args* a,
                     void* workspace, size_t workspace_bytes, plnerf_stream_t stream, const int mode) {
    const int rc = depth_train_step_grads(c, io, a, workspace, workspace_bytes, stream, mode, true);
    return rc ? rc : enqueue_apply(c, io, a, 1.0f, stream);
}

}  // namespace

// ---- the two halves on their own (include/experimental/plnerf_hip_dpstep.h) ----
extern "C" int plnerf_depth_train_step_grads(const plnerf_depth_step_config* c, const plnerf_depth_step_io* io,
                                             const plnerf_depth_step_args* a, void* workspace, size_t workspace_bytes,
                                             plnerf_stream_t stream) {
    return depth_train_step_grads(c, io, a, workspace, workspace_bytes, stream, PLNERF_MODE_LINEAR, false);
}

extern "C" int plnerf_depth_train_step_const_grads(const plnerf_depth_step_config* c, const plnerf_depth_step_io* io,
                                                   const plnerf_depth_step_args* a, void* workspace, size_t workspace_bytes,
                                                   plnerf_stream_t stream) {
    return depth_train_step_grads(c, io, a, workspace, workspace_bytes, stream, PLNERF_MODE_CONSTANT, false);
}

extern "C" int plnerf_depth_train_step_apply(const plnerf_depth_step_config* c, const plnerf_depth_step_io* io,
                                             const plnerf_depth_step_args* a, float grad_scale, plnerf_stream_t stream) {
    const int rc = check_apply(c, io, a, grad_scale, true);
    return rc ? rc : enqueue_apply(c, io, a, grad_scale, stream);
}

extern "C" size_t plnerf_depth_train_step_workspace_bytes(const plnerf_depth_step_config* config) {
    return workspace_bytes_of(config, PLNERF_MODE_LINEAR);
}

extern "C" int plnerf_depth_train_step_layout(const plnerf_depth_step_config* config, plnerf_depth_step_views* out) {
    return layout_of(config, out, PLNERF_MODE_LINEAR);
}

extern "C" int plnerf_depth_train_step(const plnerf_depth_step_config* c, const plnerf_depth_step_io* io,
                                       const plnerf_depth_step_args* a, void* workspace, size_t workspace_bytes,
                                       plnerf_stream_t stream) {
    return depth_train_step(c, io, a, workspace, workspace_bytes, stream, PLNERF_MODE_LINEAR);
}

// ---- piecewise-constant mode (include/plnerf_hip_conststep.h): the same carve, so the same bytes and offsets ----
extern "C" size_t plnerf_depth_train_step_const_workspace_bytes(const plnerf_depth_step_config* config) {
    return workspace_bytes_of(config, PLNERF_MODE_CONSTANT);
}

extern "C" int plnerf_depth_train_step_const_layout(const plnerf_depth_step_config* config, plnerf_depth_step_views* out) {
    return layout_of(config, out, PLNERF_MODE_CONSTANT);
}

extern "C" int plnerf_depth_train_step_const(const plnerf_depth_step_config* c, const plnerf_depth_step_io* io,
                                             const plnerf_depth_step_args* a, void* workspace, size_t workspace_bytes,
                                             plnerf_stream_t stream) {
    return depth_train_step(c, io, a, workspace, workspace_bytes, stream, PLNERF_MODE_CONSTANT);
}
