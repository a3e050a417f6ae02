/*
 * experimental/plnerf_hip_camcode.h -- test-time optimisation of one view's camera code on a cached colour head: the
 * objective's value and gradient in one streaming launch, and the optimiser's whole loop state on the device.
 *
 * EXPERIMENTAL: this header is not part of the registered ABI.  Like experimental/plnerf_hip_depthview.h it lives outside
 * the glob include/plnerf_hip*.h of the registry (plnerf_amd._lib.HEADERS); its entries are bound from a table of their own,
 * _lib.CAMCODE_HEADERS, and held to the registry's checks by tests/test_camcode_abi.py and tests/test_gpu_camcode.py.
 * Signatures and the struct layout may still change without a PLNERF_VERSION step.  A C host includes it as
 * "experimental/plnerf_hip_camcode.h" under -I include.
 *
 * The conventions are experimental/plnerf_hip_depthview.h's: device pointers, caller-owned memory, work only enqueued on
 * `stream`, 0 or a negative PLNERF_E* code; the calls allocate nothing, wait for nothing, read no device memory on the host
 * and no environment; every argument is checked before the first launch, so a refused call has enqueued nothing.
 *
 * What is optimised (depth_supervised_exps/run_nerf_sample_based_depth.py:311-347, optimize_camera_embedding: 100 Adam
 * iterations over every pixel of a view, the networks frozen).  With perturb = 0 and raw_noise_std = 0 the sample depths
 * and the quadrature weights depend on densities only, and the camera code enters behind the density head, as the last
 * n_cam input columns of views_linears[0] (model/run_nerf_helpers.py:190-200).  So with
 *   A_s   = the view layer's pre-activation of sample s without the code columns  (row s of A, `width` = netwidth / 2),
 *   c_s   = the coefficient with which sample s enters its ray's colour           (coef),
 * the objective is, over rays i of rows_per_ray consecutive rows each,
 *   z_s   = A_s + W_cam . cam
 *   rgb_s = sigmoid(W_rgb . relu(z_s) + b_rgb)
 *   rgb_i = sum_{s in ray i} c_s rgb_s + bkgd_i
 *   L     = sum_i ray_weight_i |rgb_i - target_i|^2
 * ray_weight_i = 1 / (3 n_b) for a ray of a batch of n_b rays makes L the sum of the batches' img2mse; bkgd_i = 1 - acc_i
 * is the white background's term (0 without it).
 */
#ifndef PLNERF_HIP_CAMCODE_H
#define PLNERF_HIP_CAMCODE_H

#include "../plnerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PLNERF_CAMCODE_MAX_WIDTH 128   /* columns of A                                                               */
#define PLNERF_CAMCODE_MAX_CAM 32      /* entries of the camera code                                                 */
#define PLNERF_CAMCODE_MAX_ROWS 1024   /* rows (samples) per ray                                                     */
#define PLNERF_CAMCODE_MAX_GROUPS 2048 /* workgroups of a sweep: ray i is summed by group i % min(n_rays, this)      */

/* Bytes of plnerf_camcode_sweep's workspace for n_rays rays (0 for n_rays < 1): one partial row per workgroup.  256-byte
 * alignment; nothing is carried between calls and nothing need be zeroed. */
size_t plnerf_camcode_sweep_workspace_bytes(int n_rays);

/* L and dL / dcam at `cam`, one pass over A.
 *   A [n_rows, width] fp32, 4-byte aligned (16-byte alignment with width % 4 == 0 takes the 16-byte loads);
 *   coef [n_rows]; rows_per_ray divides n_rows (n_rays = n_rows / rows_per_ray); cam [n_cam];
 *   w_cam: W_cam[j, c] = w_cam[j * w_cam_stride + c], j < width, c < n_cam (the code's columns inside
 *          views_linears.0.weight: w_cam_stride = that matrix's row length, in floats);
 *   w_rgb [3, width], b_rgb [3]; target [n_rays, 3]; bkgd [n_rays] or NULL (= 0); ray_weight [n_rays];
 *   loss_sum: one fp64 value, 8-byte aligned; g_cam [n_cam] fp32.
 * Everything is read as fp32 and computed in fp64 (vector ALU); g_cam is the fp64 gradient rounded to fp32 once.
 * A row whose coef is exactly 0 is not read; a ray whose ray_weight is exactly 0 contributes nothing and none of its rows
 * is read.  Workgroup partials are summed in a fixed order by a second launch: no floating-point atomics, the outputs' bits
 * do not depend on timing.  Exactly 8 bytes of loss_sum and 4 n_cam bytes of g_cam are written.
 * PLNERF_EINVAL: a null pointer other than bkgd (with n_rows > 0; loss_sum and g_cam always), width outside 1..128, n_cam
 * outside 1..32, rows_per_ray outside 1..1024, n_rows < 0 or not a multiple of rows_per_ray, w_cam_stride < n_cam, loss_sum
 * not 8-byte aligned, a workspace that is too small or not 256-byte aligned; PLNERF_ERANGE: n_rows over 2^30.
 * n_rows == 0: PLNERF_OK, nothing launched, nothing written. */
int plnerf_camcode_sweep(const float* A, const float* coef, int n_rows, int rows_per_ray, int width, const float* cam,
                         int n_cam, const float* w_cam, int w_cam_stride, const float* w_rgb, const float* b_rgb,
                         const float* target, const float* bkgd, const float* ray_weight, void* workspace,
                         size_t workspace_bytes, double* loss_sum, float* g_cam, plnerf_stream_t stream);

/* The loop's state, in DEVICE memory (the host fills a copy and uploads it once; plnerf_camcode_update alone changes it
 * afterwards, so that every iteration is enqueued without a host round trip).  Start: all zero but lr = 0.5,
 * best = -INFINITY, best_iter = -1. */
typedef struct plnerf_camcode_state {
    float cam[32];        /* the code (plnerf_camcode_sweep's `cam` may point here: the first field)                 */
    float exp_avg[32];    /* Adam's moments                                                                          */
    float exp_avg_sq[32];
    float best_cam[32];   /* the code AFTER the Adam step of the iteration with the best PSNR so far                 */
    float lr;             /* Adam's learning rate, halved by the scheduler                                           */
    float best;           /* ReduceLROnPlateau's best metric                                                         */
    float max_psnr;       /* the reference's own tracking (starts at 0)                                              */
    int step;             /* iterations done                                                                         */
    int num_bad_epochs;   /* ReduceLROnPlateau's counter                                                             */
    int best_iter;        /* the iteration that set max_psnr, -1: none                                               */
} plnerf_camcode_state;

/* One iteration's bookkeeping, in the order of run_nerf_sample_based_depth.py:340-345, one launch of one thread group:
 *   1. torch.optim.Adam's step on state->cam with g_cam at state->lr (betas and eps as given: 0.9, 0.999, 1e-8);
 *   2. psnr = -10 log(loss_sum / n_batches) / log(10), in fp32 as mse2psnr;
 *   3. torch.optim.lr_scheduler.ReduceLROnPlateau('max', factor, patience) with torch's other defaults (relative
 *      threshold 1e-4, cooldown 0, min_lr 0, eps 1e-8), best starting at -inf;
 *   4. if psnr > max_psnr: max_psnr = psnr, best_cam = cam AS IT IS AFTER STEP 1, best_iter = this iteration.
 * psnr_history / lr_history [n_history], nullable: entry state->step (before it advances) receives this iteration's psnr
 * and the learning rate its Adam step used; an iteration at or past n_history records nothing.
 * PLNERF_EINVAL: state, loss_sum or g_cam NULL, n_cam outside 1..32, n_batches < 1, n_history < 0, betas outside [0, 1),
 * eps < 0, factor outside (0, 1), patience < 0, state not 4-byte or loss_sum not 8-byte aligned. */
int plnerf_camcode_update(plnerf_camcode_state* state, int n_cam, const double* loss_sum, const float* g_cam,
                          int n_batches, float beta1, float beta2, float eps, float factor, int patience,
                          float* psnr_history, float* lr_history, int n_history, plnerf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PLNERF_HIP_CAMCODE_H */
