// plnerf_depth_train_step (include/plnerf_hip_depthstep.h): one iteration of the depth-supervised loop as ONE library call.
// Like plnerf_train_step (train_step.hip) it is the sequence of this library's own entry points that the Python route
// -- depth.DepthTrainStep.step_view on render_rays' fused branch with train.backward_merged -- reaches through Python,
// ctypes and torch.autograd: the same launches with the same arguments, in the same order, on the one stream, so the two
// routes agree bit for bit.  The one kernel of its own is the depth scales' and shifts' Adam (plnerf_depth_ss_adam), which
// stands for the torch.optim.Adam over two [V, 1] tensors of that route.
#include <math.h>

#include "step_common.h"
#include "ray_bwd_dev.h"
#include "../../include/plnerf_hip_depthstep.h"
#include "../../include/plnerf_hip_conststep.h"

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
    float *rays_o, *rays_d, *viewdirs, *near, *far, *target, *target_h, *mask, *hyp_raw;
    int* pixels;
    float *z_c, *pts_c, *raw_c, *noise_c, *rgb0, *disp0, *acc0, *depth0, *z_std0;
    float *z_f, *pts_f, *raw_f, *noise_f, *u_row, *rgb, *disp, *acc, *depth, *w, *tau, *T, *hyp, *u_used, *z_std;
    int64_t* inds;
    float *g_rgb, *g_rgb0, *g_hyp, *g_tau, *g_T, *g_raw_c, *g_raw_f;
    uint32_t *absmax_c, *absmax_f;
    void *saved_c, *saved_f, *bwd_c, *bwd_f;
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
    p.rays_o = w.floats(3 * R); p.rays_d = w.floats(3 * R); p.viewdirs = w.floats(3 * R);
    p.near = w.floats(R); p.far = w.floats(R); p.target = w.floats(3 * R);
    p.target_h = w.floats(Hn * R); p.mask = w.floats(R); p.hyp_raw = w.floats(Hn * R);
    p.pixels = w.take<int>(2 * R * sizeof(int));
    p.z_c = w.floats(R * S); p.pts_c = w.floats(3 * R * S); p.raw_c = w.floats(4 * R * S);
    p.noise_c = w.floats(noise ? R * S : 0);
    p.rgb0 = w.floats(3 * R); p.disp0 = w.floats(R); p.acc0 = w.floats(R); p.depth0 = w.floats(R); p.z_std0 = w.floats(R);
    p.z_f = w.floats(R * F); p.pts_f = w.floats(3 * R * F); p.raw_f = w.floats(4 * R * F);
    p.noise_f = w.floats(noise ? R * F : 0);
    p.u_row = w.floats(c->is_joint && c->perturb ? N : 0);
    p.rgb = w.floats(3 * R); p.disp = w.floats(R); p.acc = w.floats(R); p.depth = w.floats(R);
    p.w = w.floats(R * (F + 1)); p.tau = w.floats(R * (F + 2)); p.T = w.floats(R * (F + 2));
    p.hyp = w.floats(R * N); p.u_used = w.floats(c->perturb ? R * N : 0); p.z_std = w.floats(R);
    p.inds = w.take<int64_t>(R * N * sizeof(int64_t));
    p.g_rgb = w.floats(3 * R); p.g_rgb0 = w.floats(3 * R); p.g_hyp = w.floats(R * N);
    p.g_tau = w.floats(R * (F + 2)); p.g_T = w.floats(R * (F + 2));
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

// constant: plnerf_depth_train_step_const's limits on top (its sampler needs one interior weight; the last stage's backward
// keeps a longer LDS row than any kernel of the linear step)
int check_config(const plnerf_depth_step_config* c, const bool constant) {
    if (!c) return PLNERF_EINVAL;
    if (c->max_rays < 1 || c->n_samples < (constant ? 3 : 2) || c->n_importance < 1) return PLNERF_EINVAL;
    if (c->color_mode != PLNERF_COLOR_MIDPOINT && c->color_mode != PLNERF_COLOR_LEFT) return PLNERF_EINVAL;
    if (c->n_views < 1 || c->H < 1 || c->W < 1 || c->n_hyp < 1 || (c->pose_rows != 3 && c->pose_rows != 4)) return PLNERF_EINVAL;
    if (c->fwd_kernel != PLNERF_FWD_KERNEL_AUTO && c->fwd_kernel != PLNERF_FWD_KERNEL_RR && c->fwd_kernel != PLNERF_FWD_KERNEL_PP)
        return PLNERF_EINVAL;
    if (!(c->raw_noise_std >= 0.0f) || !(c->density_beta >= 0.0f) || !(c->input_scale > 0.0f)) return PLNERF_EINVAL;
    // the in-kernel encoding's widths (plnerf_mlp_fwd without `embedded`)
    if (c->input_ch < 3 || c->input_ch > 63 || (c->input_ch - 3) % 6 != 0 || c->input_ch_views < 3 || c->input_ch_views > 27 ||
        (c->input_ch_views - 3) % 6 != 0)
        return PLNERF_EINVAL;
    if (plnerf_mlp_packed_bytes(c->precision) == 0) return PLNERF_ENOSYS;
    // (the last stage runs the quadrature over all n_samples + n_importance depths: plnerf_fine_epilogue's limit)
    if (c->n_samples > PLNERF_MAX_SAMPLES || c->n_samples + c->n_importance > PLNERF_MAX_SAMPLES) return PLNERF_ERANGE;
    if ((uint64_t)c->H * (uint64_t)c->W > (1ull << 30)) return PLNERF_ERANGE;
    // (row counts are ints throughout the ABI)
    if ((uint64_t)c->max_rays * (uint64_t)(c->n_samples + c->n_importance + 2) > (uint64_t)INT32_MAX / 4) return PLNERF_ERANGE;
    if ((uint64_t)c->max_rays * (uint64_t)c->n_hyp > (uint64_t)INT32_MAX / 4) return PLNERF_ERANGE;
    if (constant && (size_t)plnerf::RAY_WAVES * plnerf::fine_const_bwd_row_floats(c->n_samples + c->n_importance, c->n_importance) *
                            sizeof(float) > 160 * 1024)
        return PLNERF_ERANGE;
    return PLNERF_OK;
}

size_t workspace_bytes_of(const plnerf_depth_step_config* config, const bool constant) {
    if (check_config(config, constant) != PLNERF_OK) return 0;
    return carve(config, nullptr).bytes;
}

int layout_of(const plnerf_depth_step_config* config, plnerf_depth_step_views* out, const bool constant) {
    const int rc = check_config(config, constant);
    if (rc) return rc;
    if (!out) return PLNERF_EINVAL;
    const Plan p = carve(config, nullptr);      // (from a null base the addresses ARE the offsets)
    const auto off = [](const void* q) { return (size_t)(uintptr_t)q; };
    out->rgb = off(p.rgb); out->rgb0 = off(p.rgb0); out->depth = off(p.depth); out->depth0 = off(p.depth0);
    out->acc = off(p.acc); out->acc0 = off(p.acc0); out->disp = off(p.disp); out->disp0 = off(p.disp0);
    out->z_std = off(p.z_std); out->pred_hyp = off(p.hyp); out->z_vals = off(p.z_f); out->z_vals0 = off(p.z_c);
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

// constant: plnerf_depth_train_step_const.  The Plan is the linear step's: the last stage's weights [R,F] lie in the tau plane,
// its bins [R,F-1] in the T plane.
int depth_train_step(const plnerf_depth_step_config* c, const plnerf_depth_step_io* io, const plnerf_depth_step_args* a,
                     void* workspace, size_t workspace_bytes, plnerf_stream_t stream, const bool constant) {
    // ---- every check first: a refused call enqueues nothing ----
    int rc = check_config(c, constant);
    if (rc) return rc;
    if (!io || !a || !workspace || ((uintptr_t)workspace % ALIGN) != 0) return PLNERF_EINVAL;
    if (a->rays < 1 || a->rays > c->max_rays || a->ray_id0 < 0 || a->view < 0 || a->view >= c->n_views) return PLNERF_EINVAL;
    if (a->adam_step < 1) return PLNERF_EINVAL;
    if ((rc = check_net(&io->coarse)) || (rc = check_net(&io->fine))) return rc;
    if (!io->t_vals || !io->loss5 || (!c->perturb && !io->u_vals)) return PLNERF_EINVAL;
    if (!io->images || !io->hyp || !io->poses || !io->intrinsics) return PLNERF_EINVAL;
    const bool carve_on = a->carve != 0, ss = a->ss_step != 0;
    if (ss && (!carve_on || a->ss_adam_step < 1 || !io->scale || !io->shift || !io->ss_grad || !io->ss_exp_avg ||
               !io->ss_exp_avg_sq))
        return PLNERF_EINVAL;
    if ((uint64_t)a->ray_id0 + (uint64_t)a->rays > (uint64_t)c->H * (uint64_t)c->W) return PLNERF_ERANGE;
    const Plan p = carve(c, workspace);
    if (workspace_bytes < p.bytes) return PLNERF_EINVAL;
    const int layout = plnerf_mlp_saved_layout(c->precision, 0, c->fwd_kernel);
    if (layout < 0) return layout;
    if ((rc = check_params_aligned(io->coarse.params)) || (rc = check_params_aligned(io->fine.params))) return rc;

    hipStream_t st = (hipStream_t)stream;
    const int R = a->rays, S = c->n_samples, N = c->n_importance, F = S + N;
    const int prec = c->precision, xyz = c->input_ch, dir = c->input_ch_views;
    const int white = c->white_bkgd ? 1 : 0, joint = c->is_joint ? 1 : 0;
    const bool noise = c->raw_noise_std > 0.0f;
    const float beta = c->density_beta;
#define STEP_OK(call) do { rc = (call); if (rc) return rc; } while (0)

    // ---- this step's rays of view a->view, their target colours, scaled hypotheses, mask, raw hypotheses and pixels ----
    STEP_OK(plnerf_select_depth_rays(c->n_views, a->view, c->H, c->W, c->n_hyp, io->images, io->hyp, io->valid, io->poses,
                                     c->pose_rows, io->intrinsics, io->scale, io->shift, c->near, c->far, c->seed, a->step,
                                     a->ray_id0, R, p.rays_o, p.rays_d, p.viewdirs, p.near, p.far, p.target, p.target_h, p.mask,
                                     p.hyp_raw, p.pixels, stream));
    const float *o = p.rays_o, *d = p.rays_d;

    // ---- coarse pass ----
    STEP_OK(plnerf_coarse_samples(o, d, p.near, p.far, io->t_vals, nullptr, c->seed, a->step, a->ray_id0, R, S, c->lindisp ? 1 : 0,
                                  c->perturb ? 1 : 0, p.z_c, p.pts_c, stream));
    STEP_OK(plnerf_mlp_pack_weights(io->coarse.params, prec, xyz, dir, io->coarse.packed, stream));
    STEP_OK(plnerf_mlp_fwd(io->coarse.packed, prec, p.pts_c, p.viewdirs, nullptr, xyz, dir, R * S, S, c->input_scale, beta, p.raw_c,
                           p.saved_c, c->fwd_kernel, stream));
    if (noise) {
        STEP_OK(plnerf_normal(c->seed, NOISE_STREAM, a->step, a->ray_id0, R, S, p.noise_c, stream));
        if (c->raw_noise_std != 1.0f) STEP_OK(scale2(p.noise_c, (size_t)R * S, nullptr, 0, c->raw_noise_std, st));
    }
    // (the depth script's raw2outputs ignores farcolorfix: 0 throughout)
    if (!constant)
        STEP_OK(plnerf_coarse_epilogue(p.raw_c, p.z_c, p.near, p.far, o, d, noise ? p.noise_c : nullptr,
                                       c->perturb ? nullptr : io->u_vals, 0, c->seed, a->step, a->ray_id0, R, S, N, c->color_mode,
                                       white, 0, c->zero_tol, c->epsilon, p.rgb0, p.disp0, p.acc0, p.depth0, nullptr, nullptr,
                                       nullptr, p.z_f, p.pts_f, p.z_std0, stream));
    else
        STEP_OK(plnerf_coarse_epilogue_const(p.raw_c, p.z_c, p.near, p.far, o, d, noise ? p.noise_c : nullptr,
                                             c->perturb ? nullptr : io->u_vals, 0, c->seed, a->step, a->ray_id0, R, S, N, white,
                                             p.rgb0, p.disp0, p.acc0, p.depth0, nullptr, p.z_f, p.pts_f, p.z_std0, stream));

    // ---- fine pass; its last stage also draws the depth hypotheses from the final weights ----
    STEP_OK(plnerf_mlp_pack_weights(io->fine.params, prec, xyz, dir, io->fine.packed, stream));
    STEP_OK(plnerf_mlp_fwd(io->fine.packed, prec, p.pts_f, p.viewdirs, nullptr, xyz, dir, R * F, F, c->input_scale, beta, p.raw_f,
                           p.saved_f, c->fwd_kernel, stream));
    // the hypotheses' draws: the table (perturb == 0), one row from the counters of global ray 0 (is_joint), or drawn in
    // the kernel; u_seen / u_seen_stride: what the sampler's backward reads
    const float* u_in = nullptr;
    const float* u_seen = p.u_used;
    int u_seen_stride = N;
    if (!c->perturb) {
        u_in = u_seen = io->u_vals;
        u_seen_stride = 0;
    } else if (joint) {      // (the Python route draws the row before the fine pass's noise)
        STEP_OK(plnerf_uniform(c->seed, HYP_STREAM, a->step, 0, 1, N, p.u_row, stream));
        u_in = p.u_row;
    }
    if (noise) {
        STEP_OK(plnerf_normal(c->seed, NOISE_STREAM + 1, a->step, a->ray_id0, R, F, p.noise_f, stream));
        if (c->raw_noise_std != 1.0f) STEP_OK(scale2(p.noise_f, (size_t)R * F, nullptr, 0, c->raw_noise_std, st));
    }
    float *const w_const = p.tau, *const bins_const = p.T;
    if (!constant)
        STEP_OK(plnerf_fine_epilogue(p.raw_f, p.z_f, p.near, p.far, d, noise ? p.noise_f : nullptr, u_in, 0, c->seed, a->step,
                                     a->ray_id0, R, F, N, c->color_mode, white, 0, c->zero_tol, c->epsilon, p.rgb, p.disp, p.acc,
                                     p.depth, p.w, p.tau, p.T, p.hyp, p.inds, c->perturb ? p.u_used : nullptr, p.z_std, stream));
    else
        STEP_OK(plnerf_fine_epilogue_const(p.raw_f, p.z_f, p.near, p.far, d, noise ? p.noise_f : nullptr, u_in, 0, c->seed, a->step,
                                           a->ray_id0, R, F, N, white, p.rgb, p.disp, p.acc, p.depth, w_const, bins_const, p.hyp,
                                           p.inds, c->perturb ? p.u_used : nullptr, p.z_std, stream));

    // ---- loss and its gradients; the scales' and shifts' gradient from the hypotheses the loss chose ----
    STEP_OK(plnerf_depth_loss(p.rgb, p.rgb0, p.target, carve_on ? p.hyp : nullptr, carve_on ? p.target_h : nullptr,
                              carve_on ? p.mask : nullptr, R, carve_on ? N : 1, carve_on ? c->n_hyp : 1, 1, joint, nullptr,
                              c->space_carving_weight, c->space_carving_threshold, io->loss5, p.g_rgb, p.g_rgb0,
                              carve_on ? p.g_hyp : nullptr, p.loss_ws, stream));
    if (ss)
        STEP_OK(plnerf_depth_scale_shift_grad(p.hyp, p.target_h, p.hyp_raw, p.mask, R, N, c->n_hyp, 1, joint, nullptr,
                                              c->space_carving_weight, c->space_carving_threshold, c->n_views, a->view,
                                              io->ss_grad, io->ss_grad + c->n_views, p.ss_ws, stream));

    // ---- backward: the hypotheses' gradient through the sampler, d loss / d raw of either pass (the fine one first, as
    //      autograd orders them), then both networks at once ----
    if (constant) {      // (the sampler's backward, the padded sum and the quadrature's in one launch; without g_hyp the last alone)
        STEP_OK(plnerf_fine_epilogue_const_bwd(p.raw_f, p.z_f, p.near, p.far, d, noise ? p.noise_f : nullptr, w_const, bins_const,
                                               u_seen, u_seen_stride, p.inds, R, F, N, white, p.g_rgb, nullptr, nullptr, nullptr,
                                               carve_on ? p.g_hyp : nullptr, p.g_raw_f, p.absmax_f, stream));
    } else {
        if (carve_on)
            STEP_OK(plnerf_sample_pl_bwd(p.z_f, p.tau, p.T, p.near, p.far, u_seen, u_seen_stride, p.inds, p.g_hyp, R, F, N,
                                         c->zero_tol, c->epsilon, p.g_tau, p.g_T, stream));
        STEP_OK(plnerf_quad_bwd(p.raw_f, p.z_f, p.near, p.far, d, noise ? p.noise_f : nullptr, R, F, PLNERF_MODE_LINEAR,
                                c->color_mode, white, 0, p.g_rgb, nullptr, nullptr, nullptr, carve_on ? p.g_tau : nullptr,
                                carve_on ? p.g_T : nullptr, p.g_raw_f, p.absmax_f, stream));
    }
    STEP_OK(plnerf_quad_bwd(p.raw_c, p.z_c, p.near, p.far, d, noise ? p.noise_c : nullptr, R, S,
                            constant ? PLNERF_MODE_CONSTANT : PLNERF_MODE_LINEAR, c->color_mode, white, 0, p.g_rgb0, nullptr, nullptr,
                            nullptr, nullptr, nullptr, p.g_raw_c, p.absmax_c, stream));
    const plnerf_step_net* nets[2] = {&io->coarse, &io->fine};
    float* grads[2 * PLNERF_N_PARAM_TENSORS];
    for (int j = 0; j < 2; ++j)
        for (int i = 0; i < PLNERF_N_PARAM_TENSORS; ++i)
            grads[j * PLNERF_N_PARAM_TENSORS + i] = nets[j]->grad_flat + (nets[j]->params[i] - nets[j]->param_flat);
    const int groups = (R + PLNERF_QUAD_RAYS_PER_GROUP - 1) / PLNERF_QUAD_RAYS_PER_GROUP;
    // (max |g_raw| as the quadrature's by-product serves networks WITHOUT a density activation only: with one, the
    // backward scales by the maximum behind the activation's derivative and takes its own pass)
    const bool by_product = !(beta > 0.0f);
    const void* packed[2] = {io->coarse.packed, io->fine.packed};
    const float* g_raw[2] = {p.g_raw_c, p.g_raw_f};
    const uint32_t* absmax[2] = {by_product ? p.absmax_c : nullptr, by_product ? p.absmax_f : nullptr};
    const int n_absmax[2] = {by_product ? groups : 0, by_product ? groups : 0};
    const int n_rows[2] = {R * S, R * F};
    const void* saved[2] = {p.saved_c, p.saved_f};
    const int layouts[2] = {layout, layout};
    const float* raw_out[2] = {by_product ? nullptr : p.raw_c, by_product ? nullptr : p.raw_f};
    void* bwd_ws[2] = {p.bwd_c, p.bwd_f};
    float* status_out[2] = {io->coarse.grad_flat + io->coarse.n_params, io->fine.grad_flat + io->fine.n_params};
    STEP_OK(plnerf_mlp_bwd_multi(2, packed, prec, g_raw, absmax, n_absmax, xyz, dir, n_rows, saved, layouts, raw_out, beta, bwd_ws,
                                 grads, status_out, stream));

    // ---- the one optimizer over both networks: its gradient lies in two runs, the coarse network's first
    //      (optim.FlatAdam.step), clipped inside the kernel (run_nerf_sample_based_depth.py:1155-1157) ----
    for (int j = 0; j < 2; ++j)
        STEP_OK(plnerf_adam_step(nets[j]->param_flat, nets[j]->grad_flat, nets[j]->exp_avg, nets[j]->exp_avg_sq, nets[j]->n_params,
                                 a->lr, c->beta1, c->beta2, c->adam_eps, a->adam_step, 1.0f, c->clip_value, nets[j]->skip_if_set,
                                 nets[j]->skip_if_set2, nets[j]->withheld, stream));
    // ---- the depth scales and shifts, unclipped (:1159-1161) ----
    if (ss)
        STEP_OK(plnerf_depth_ss_adam(io->scale, io->shift, io->ss_grad, io->ss_exp_avg, io->ss_exp_avg_sq, c->n_views, a->ss_lr,
                                     c->ss_beta1, c->ss_beta2, c->ss_adam_eps, a->ss_adam_step, 1.0f, stream));
#undef STEP_OK
    return PLNERF_OK;
}

}  // namespace

extern "C" size_t plnerf_depth_train_step_workspace_bytes(const plnerf_depth_step_config* config) {
    return workspace_bytes_of(config, false);
}

extern "C" int plnerf_depth_train_step_layout(const plnerf_depth_step_config* config, plnerf_depth_step_views* out) {
    return layout_of(config, out, false);
}

extern "C" int plnerf_depth_train_step(const plnerf_depth_step_config* c, const plnerf_depth_step_io* io,
                                       const plnerf_depth_step_args* a, void* workspace, size_t workspace_bytes,
                                       plnerf_stream_t stream) {
    return depth_train_step(c, io, a, workspace, workspace_bytes, stream, false);
}

// ---- piecewise-constant mode (include/plnerf_hip_conststep.h): the same carve, so the same bytes and offsets ----
extern "C" size_t plnerf_depth_train_step_const_workspace_bytes(const plnerf_depth_step_config* config) {
    return workspace_bytes_of(config, true);
}

extern "C" int plnerf_depth_train_step_const_layout(const plnerf_depth_step_config* config, plnerf_depth_step_views* out) {
    return layout_of(config, out, true);
}

extern "C" int plnerf_depth_train_step_const(const plnerf_depth_step_config* c, const plnerf_depth_step_io* io,
                                             const plnerf_depth_step_args* a, void* workspace, size_t workspace_bytes,
                                             plnerf_stream_t stream) {
    return depth_train_step(c, io, a, workspace, workspace_bytes, stream, true);
}
