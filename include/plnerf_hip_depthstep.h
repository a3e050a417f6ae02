/*
 * plnerf_hip_depthstep.h -- one library call = one optimisation step of the depth-supervised loop (PLNERF_VERSION >= 601).
 *
 * The depth-supervised counterpart of plnerf_hip_step.h under the same conventions: the structs live in host memory and
 * are read during the call, device memory is owned by the caller, work is only enqueued on `stream`, the call allocates
 * nothing, waits for nothing, reads no device memory and no environment, and every argument is checked before the first
 * launch: a refused call has enqueued nothing.  A header of its own, so that the existing headers and their tests stay
 * what they are; tests/test_depth_step_abi.py holds this one to the same checks (plain C99, linked against the library,
 * ctypes mirror parsed from here).
 *
 * plnerf_depth_train_step enqueues one iteration of depth_supervised_exps/run_nerf_sample_based_depth.py:1104-1161 for
 * two native view-dependent 8 x 256 networks in piecewise-linear mode with importance sampling, as the sequence of this
 * library's own entry points:
 *
 *   plnerf_select_depth_rays -> plnerf_coarse_samples -> plnerf_mlp_pack_weights + plnerf_mlp_fwd (coarse) ->
 *   (plnerf_normal) -> plnerf_coarse_epilogue -> plnerf_mlp_pack_weights + plnerf_mlp_fwd (fine) ->
 *   (is_joint: plnerf_uniform, one row) -> (plnerf_normal) -> plnerf_fine_epilogue -> plnerf_depth_loss ->
 *   (ss_step: plnerf_depth_scale_shift_grad) -> (carve: plnerf_sample_pl_bwd) -> plnerf_quad_bwd (fine, coarse) ->
 *   plnerf_mlp_bwd_multi -> plnerf_adam_step (coarse, fine: the two runs of the ONE optimizer's gradient) ->
 *   (ss_step: plnerf_depth_ss_adam)
 *
 * on the one stream, in this order, with counter-based draws (stream ids 0 = jitter, 1 = importance samples, 2 / 3 = the
 * density noise of the coarse / fine pass, 4 = the depth hypotheses' draws).
 */
#ifndef PLNERF_HIP_DEPTHSTEP_H
#define PLNERF_HIP_DEPTHSTEP_H

#include "plnerf_hip.h"
#include "plnerf_hip_depthfeed.h"
#include "plnerf_hip_step.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Everything that is fixed for a run. */
typedef struct plnerf_depth_step_config {
    int max_rays;         /* the largest plnerf_depth_step_args.rays of the run: the workspace is laid out for it      */
    int n_samples;        /* coarse samples per ray, 2 .. PLNERF_MAX_SAMPLES                                          */
    int n_importance;     /* importance samples (and depth hypotheses) per ray, >= 1; n_samples + n_importance <= 1022 */
    int color_mode;       /* PLNERF_COLOR_MIDPOINT | PLNERF_COLOR_LEFT                                                */
    int lindisp;          /* coarse depths linear in disparity                                                        */
    int perturb;          /* != 0: stratified jitter and random draws; 0: io.t_vals / io.u_vals as they are           */
    int white_bkgd;
    float raw_noise_std;  /* > 0: density noise N(0, 1) * raw_noise_std on both passes                                */
    float zero_tol;       /* the samplers' zero_threshold (1e-4)                                                      */
    float epsilon;        /* ... and epsilon_ (1e-3)                                                                  */
    int n_views;          /* the device-resident training views (plnerf_select_depth_rays) ...                        */
    int H;                /* ... all H x W ...                                                                        */
    int W;
    int n_hyp;            /* ... with n_hyp depth hypotheses per pixel ...                                            */
    int pose_rows;        /* ... and poses of 3 or 4 rows                                                             */
    float near;           /* the near / far columns of the selected rays                                              */
    float far;
    int precision;        /* PLNERF_PREC_*, both networks                                                             */
    int fwd_kernel;       /* PLNERF_FWD_KERNEL_*                                                                      */
    int input_ch;         /* 3 + 6 L, L <= 10 (the in-kernel encoding)                                                */
    int input_ch_views;   /* 3 + 6 M, M <= 4                                                                          */
    float input_scale;    /* the encoder's input scale (pi for the depth script's networks)                           */
    float density_beta;   /* softplus beta of the density channel (10 there), 0 = none                                */
    int is_joint;         /* one row of hypothesis draws for the whole batch; the hypothesis is chosen per point column */
    float space_carving_weight;
    float space_carving_threshold;
    float clip_value;     /* clip_grad_value_ on the networks' gradients inside plnerf_adam_step (0.1), <= 0: none     */
    float beta1;          /* Adam of the two networks                                                                 */
    float beta2;
    float adam_eps;
    float ss_beta1;       /* Adam of the depth scales and shifts                                                      */
    float ss_beta2;
    float ss_adam_eps;
    uint64_t seed;        /* key of the draws and of the pixel choice                                                 */
} plnerf_depth_step_config;

/* Device memory the caller owns.  coarse / fine: plnerf_step_net (plnerf_hip_step.h); their param_flat, exp_avg and
 * exp_avg_sq are the two networks' slices of the ONE optimizer's flat buffers, and both carry the same guard words and
 * the same withheld counter. */
typedef struct plnerf_depth_step_io {
    plnerf_step_net coarse;
    plnerf_step_net fine;
    const float* t_vals;      /* [n_samples] = torch.linspace(0, 1, n_samples), written once by the caller             */
    const float* u_vals;      /* [n_importance] = torch.linspace(0, 1, n_importance); read only when perturb == 0      */
    const float* images;      /* [n_views, H, W, 3]              (the arrays of plnerf_select_depth_rays)              */
    const float* hyp;         /* [n_views, n_hyp, H, W]                                                                */
    const uint8_t* valid;     /* [n_views, H, W], nullable: every pixel valid                                          */
    const float* poses;       /* [n_views, pose_rows, 4]                                                               */
    const float* intrinsics;  /* [n_views, 4] = (fx, fy, cx, cy)                                                       */
    float* scale;             /* [n_views] DEPTH_SCALES, read on the device by every step (nullable: 1) ...            */
    float* shift;             /* [n_views] DEPTH_SHIFTS (nullable: 0); both required and stepped when args.ss_step     */
    float* ss_grad;           /* [2, n_views]: the dense gradient of (scales, shifts), written when args.ss_step       */
    float* ss_exp_avg;        /* [2, n_views]: their Adam moments                                                      */
    float* ss_exp_avg_sq;
    float* loss5;             /* out: {total, image, image (coarse), space carving, psnr} as plnerf_depth_loss leaves them */
} plnerf_depth_step_io;

/* What changes from step to step. */
typedef struct plnerf_depth_step_args {
    int view;             /* the training view of this step, 0 .. n_views - 1                                         */
    int rays;             /* 1 .. config.max_rays                                                                     */
    uint32_t step;        /* the global step: key of this step's draws and of its pixel choice                        */
    int ray_id0;          /* global id of the first ray; ray_id0 + rays <= H * W                                      */
    float lr;             /* learning rate of the networks' optimizer for THIS step                                   */
    int adam_step;        /* its step count AFTER this update (>= 1)                                                  */
    int carve;            /* != 0: the space-carving term is on (space_carving_weight > 0 && i > warm_start_nerf)     */
    int ss_step;          /* != 0: this step also steps the depth scales and shifts (needs carve)                     */
    float ss_lr;          /* their learning rate ...                                                                  */
    int ss_adam_step;     /* ... and step count AFTER this update (>= 1 when ss_step)                                 */
} plnerf_depth_step_args;

/* Byte offsets, inside the workspace, of what a step renders (fp32 unless noted; R = args.rays of that step, S =
 * n_samples, N = n_importance): valid from the end of a step's work on the stream until the next step is enqueued. */
typedef struct plnerf_depth_step_views {
    size_t rgb;           /* [R, 3] */
    size_t rgb0;          /* [R, 3] the coarse pass's */
    size_t depth;         /* [R] */
    size_t depth0;
    size_t acc;
    size_t acc0;
    size_t disp;
    size_t disp0;
    size_t z_std;         /* [R] std of pred_hyp */
    size_t pred_hyp;      /* [R, N] */
    size_t z_vals;        /* [R, S + N] */
    size_t z_vals0;       /* [R, S] */
    size_t pixels;        /* [R, 2] int32 (row, col) */
    size_t target_h;      /* [n_hyp, R] scaled and shifted */
    size_t mask;          /* [R] 1.0 where valid */
} plnerf_depth_step_views;

/* Bytes of the workspace for this configuration (0: the configuration is refused).  256-byte alignment; the caller
 * ZEROES it once before the first step (the loss kernel's partials are left zeroed by every step) and hands the same
 * memory to every step of the run. */
size_t plnerf_depth_train_step_workspace_bytes(const plnerf_depth_step_config* config);

/* Where the rendered outputs of a step lie inside that workspace.  PLNERF_EINVAL / _ERANGE / _ENOSYS as the size query
 * refuses; PLNERF_EINVAL for a null `out`. */
int plnerf_depth_train_step_layout(const plnerf_depth_step_config* config, plnerf_depth_step_views* out);

/* One optimisation step.  PLNERF_EINVAL: a null struct or required pointer, rays outside 1 .. max_rays, view outside
 * [0, n_views), a parameter outside its flat buffer, ss_step without carve, a workspace that is too small or misaligned;
 * PLNERF_ERANGE: sizes outside the compiled limits, ray_id0 + rays > H * W; PLNERF_ENOSYS: a precision that is not built. */
int plnerf_depth_train_step(const plnerf_depth_step_config* config, const plnerf_depth_step_io* io,
                            const plnerf_depth_step_args* args, void* workspace, size_t workspace_bytes,
                            plnerf_stream_t stream);

/* One Adam step (torch.optim.Adam semantics, no clipping: run_nerf_sample_based_depth.py:1159-1161) of the per-view depth
 * scales and shifts, scale / shift [n_views], from their dense gradient grad [2, n_views] (row 0 the scales') with the
 * moments exp_avg / exp_avg_sq [2, n_views], in one launch.  grad_scale multiplies the gradient first (1 / world after an
 * all-reduce sum); entries whose gradient is zero still move by their moments, as in torch.  step >= 1 is the step count
 * AFTER this update. */
int plnerf_depth_ss_adam(float* scale, float* shift, const float* grad, float* exp_avg, float* exp_avg_sq, int n_views,
                         float lr, float beta1, float beta2, float eps, int step, float grad_scale,
                         plnerf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PLNERF_HIP_DEPTHSTEP_H */
