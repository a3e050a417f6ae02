/*
 * plnerf_hip_step.h -- one library call = one optimisation step (PLNERF_VERSION >= 601).
 *
 * A companion of plnerf_hip.h under the same conventions (device pointers, caller-owned memory, work only enqueued on
 * `stream`, 0 or a negative PLNERF_E* code).  It is a header of its own so that plnerf_hip.h's list of entry points,
 * which tests/abi_check.c restates one by one, stays what it was; tests/test_step_abi.py holds this one to the same
 * checks (plain C99, linked against the library, ctypes mirror parsed from here).
 *
 * plnerf_train_step enqueues the loop body of run_plnerf.py:1235-1316 for the reference's two view-dependent 8 x 256
 * networks in piecewise-linear mode with importance sampling, as the sequence of this library's own entry points:
 *
 *   plnerf_select_rays | plnerf_select_bank_rays -> (plnerf_ndc_rays) -> plnerf_coarse_samples ->
 *   plnerf_mlp_pack_weights + plnerf_mlp_fwd (coarse) -> (plnerf_normal) -> plnerf_coarse_epilogue ->
 *   plnerf_mlp_pack_weights + plnerf_mlp_fwd (fine) -> (plnerf_normal) -> plnerf_quad_fwd -> plnerf_image_loss ->
 *   plnerf_quad_bwd (fine, coarse; each leaves max |g_raw|) -> plnerf_mlp_bwd_multi -> plnerf_adam_step (fine, coarse)
 *
 * on the one stream, in this order, with counter-based draws (stream ids 0 = jitter, 1 = importance samples, 2 / 3 =
 * the density noise of the coarse / fine pass).  The call allocates nothing, waits for nothing, reads no device memory
 * and no environment; the three structs live in host memory and are read during the call.  Every argument is checked
 * before the first launch: a refused call has enqueued nothing.
 */
#ifndef PLNERF_HIP_STEP_H
#define PLNERF_HIP_STEP_H

#include "plnerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PLNERF_STEP_RAYS_VIEW 0 /* rays of one view per step: plnerf_select_rays (the no_batching branch)            */
#define PLNERF_STEP_RAYS_BANK 1 /* rays of the shuffled bank of all views: plnerf_select_bank_rays (use_batching)    */

/* Everything that is fixed for a run. */
typedef struct plnerf_step_config {
    int max_rays;         /* the largest plnerf_step_args.rays of the run: the workspace is laid out for it           */
    int n_samples;        /* coarse samples per ray, 2 .. PLNERF_MAX_SAMPLES                                          */
    int n_importance;     /* importance samples per ray, >= 1; n_samples + n_importance <= 1024                       */
    int mode;             /* PLNERF_MODE_LINEAR (the only mode this entry serves)                                     */
    int color_mode;       /* PLNERF_COLOR_MIDPOINT | PLNERF_COLOR_LEFT                                                */
    int lindisp;          /* coarse depths linear in disparity                                                        */
    int perturb;          /* != 0: stratified jitter and random importance draws; 0: io.t_vals / io.u_vals as they are */
    int white_bkgd;
    int farcolorfix;
    float raw_noise_std;  /* > 0: density noise N(0, 1) * raw_noise_std on both passes                                */
    float zero_tol;       /* sample_pdf_reformulation's zero_threshold (1e-4)                                         */
    float epsilon;        /* ... and epsilon_ (1e-3)                                                                  */
    int ndc;              /* != 0: plnerf_ndc_rays(H, W, ndc_focal, 1) on the selected rays                           */
    double ndc_focal;
    int H;                /* the views' size and intrinsics                                                           */
    int W;
    float fx;
    float fy;
    float cx;
    float cy;
    float near;           /* the near / far columns of the selected rays                                              */
    float far;
    int precision;        /* PLNERF_PREC_*, both networks                                                             */
    int fwd_kernel;       /* PLNERF_FWD_KERNEL_*                                                                      */
    int input_ch;         /* 3 + 6 L, L <= 10 (the in-kernel encoding)                                                */
    int input_ch_views;   /* 3 + 6 M, M <= 4                                                                          */
    int ray_source;       /* PLNERF_STEP_RAYS_*                                                                       */
    int n_views;          /* bank source: entries of io.views                                                         */
    float beta1;          /* Adam, both optimizers                                                                    */
    float beta2;
    float adam_eps;
    uint64_t seed;        /* key of the draws and of the view source's pixel choice                                   */
    uint64_t bank_seed;   /* key of the bank's epoch orders                                                           */
} plnerf_step_config;

/* One network with its optimizer state.  The 24 parameter tensors are slices of param_flat [n_params], in any order
 * (optim.FlatAdam's layout) that leaves feature_linear.weight and .bias (params[18], [19]) 16-byte aligned, as
 * plnerf_mlp_pack_weights demands (else PLNERF_EINVAL, before the first launch); gradient k is written at the same offset
 * of grad_flat.  grad_flat holds n_params + 4 floats: [n_params] receives the network's range status as plnerf_mlp_bwd's
 * status_out leaves it; the three floats behind it are not touched. */
typedef struct plnerf_step_net {
    const float* params[PLNERF_N_PARAM_TENSORS];
    float* param_flat;
    float* grad_flat;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t n_params;
    void* packed;                 /* plnerf_mlp_packed_bytes(precision); status word zeroed by the caller once        */
    const uint32_t* skip_if_set;  /* plnerf_adam_step's guard words (nullable) ...                                    */
    const uint32_t* skip_if_set2;
    uint32_t* withheld;           /* ... and its counter of withheld launches (nullable)                              */
} plnerf_step_net;

/* Device memory the caller owns. */
typedef struct plnerf_step_io {
    plnerf_step_net coarse;
    plnerf_step_net fine;
    const float* t_vals;  /* [n_samples] = torch.linspace(0, 1, n_samples), written once by the caller               */
    const float* u_vals;  /* [n_importance] = torch.linspace(0, 1, n_importance); read only when perturb == 0         */
    const int* views;     /* bank source: [n_views] int32 view indices ...                                            */
    const float* poses;   /* ... [N_all, 12] camera-to-world rows ...                                                 */
    const float* images;  /* ... [N_all, H, W, 3]                                                                     */
    float* loss4;         /* out: {total, fine, coarse, psnr} as plnerf_image_loss leaves them                        */
} plnerf_step_io;

/* What changes from step to step. */
typedef struct plnerf_step_args {
    int rays;             /* 1 .. config.max_rays (an epoch's last batch is short)                                    */
    uint32_t step;        /* the global step: key of this step's draws and of the view source's pixel choice          */
    int ray_id0;          /* global id of the first ray                                                               */
    float c2w[12];        /* view source: rows of the 3 x 4 camera-to-world matrix ...                                */
    const float* image;   /* ... the view's image [H, W, 3] (device) ...                                              */
    int crop_r0;          /* ... and the window the pixels are drawn from (the whole view, or the precrop window)     */
    int crop_c0;
    int crop_rows;
    int crop_cols;
    uint32_t epoch;       /* bank source: the epoch ...                                                               */
    int pos0;             /* ... and the first position of its order                                                  */
    float lr_fine;        /* learning rate of either optimizer for THIS step                                          */
    float lr_coarse;
    int adam_step_fine;   /* step count of either optimizer AFTER this update (>= 1)                                  */
    int adam_step_coarse;
    float loss_scale;     /* factor on both image-loss gradients (1 = none)                                           */
} plnerf_step_args;

/* Bytes of the workspace for this configuration (0: the configuration is refused).  The library lays it out itself:
 * the loss kernel's partial sums, the rays' planes, both passes' samples, raw outputs, saved activations
 * (plnerf_mlp_saved_bytes) and the backward's scratch (plnerf_mlp_bwd_workspace_bytes).  256-byte alignment; the
 * caller ZEROES it once before the first step (the loss partials are left zeroed by every step) and hands the same
 * memory to every step of the run.  Nothing in it is carried from one step to the next beyond those zeros. */
size_t plnerf_train_step_workspace_bytes(const plnerf_step_config* config);

/* One optimisation step.  PLNERF_EINVAL: a null struct or pointer, rays outside 1 .. max_rays, a mode other than
 * PLNERF_MODE_LINEAR, a parameter outside its flat buffer, a workspace that is too small or misaligned;
 * PLNERF_ERANGE: sizes outside the compiled limits, rays past the pixel window or the epoch; PLNERF_ENOSYS: a precision
 * that is not built. */
int plnerf_train_step(const plnerf_step_config* config, const plnerf_step_io* io, const plnerf_step_args* args,
                      void* workspace, size_t workspace_bytes, plnerf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PLNERF_HIP_STEP_H */
