/*
 * plnerf_hip_depthfeed.h -- the data feed of the depth-supervised training loop of libplnerf_hip.so
 * (PLNERF_VERSION >= 601).
 *
 * A companion of plnerf_hip.h under the same conventions (device pointers, caller-owned memory, work only enqueued on
 * `stream`, 0 or a negative PLNERF_E* code).  Like plnerf_hip_batching.h and plnerf_hip_eval.h it is a header of its
 * own, so that plnerf_hip.h's list of entry points, which tests/abi_check.c restates one by one, stays what it was;
 * tests/test_depthfeed_abi.py holds this one to the same checks (plain C99, linked against the library, ctypes
 * signatures parsed from here).
 */
#ifndef PLNERF_HIP_DEPTHFEED_H
#define PLNERF_HIP_DEPTHFEED_H

#include "plnerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Caller-owned workspace of plnerf_depth_scale_shift_grad (8-byte aligned, no initialisation needed). */
#define PLNERF_DEPTH_SS_WORKSPACE_BYTES 4096

/* The training rays of one step of the depth-supervised loop (depth_supervised_exps/run_nerf_sample_based_depth.py:
 * 960-1001, 1111-1120) for view `view` of n_views device-resident training views, all H x W:
 *   images [n_views, H, W, 3] fp32; hyp [n_views, n_hyp, H, W] fp32 (the depth hypotheses); valid [n_views, H, W]
 *   (0 / nonzero, nullable: every pixel valid); poses [n_views, pose_rows, 4] fp32, pose_rows 3 or 4 (camera to world);
 *   intrinsics [n_views, 4] fp32 = (fx, fy, cx, cy); scale, shift [n_views] fp32 (nullable: 1 and 0).
 * Only the view index and the scalars come from the host.  Ray i is pixel perm(ray_id0 + i) = (row, col) of the view,
 * perm the keyed bijection of [0, H*W) of plnerf_select_rays for (seed, step): distinct within a call, disjoint for
 * disjoint id ranges; ray_id0 + R > H*W is PLNERF_ERANGE, as is H*W > 2^30.  Its direction is the depth script's
 * get_rays (model/run_nerf_helpers.py:243-263): dirs = (((col + 0.5) - cx) / fx, ((H - (row + 0.5)) - cy) / fy, -1)
 * rotated by the pose, each operation rounded separately and the three terms of each sum (and of |rays_d|^2) added as
 * torch adds them on the GPU, (t0 + t2) + t1 -- bit-equal to that script's get_rays on the device.  Outputs: rays_o, rays_d [R, 3]; viewdirs [R, 3] = rays_d /
 * |rays_d| (nullable); near_out, far_out [R]; target [R, 3] = images[view, row, col]; target_h [n_hyp, R] =
 * fl(fl(hyp[view, h, row, col] * scale[view]) + shift[view]); mask [R] = 1.0 where valid, else 0.0; hyp_raw [n_hyp, R]
 * (nullable) the unscaled hypotheses; pixels [R, 2] int32 (row, col) (nullable). */
int plnerf_select_depth_rays(int n_views, int view, int H, int W, int n_hyp, const float* images, const float* hyp,
                             const uint8_t* valid, const float* poses, int pose_rows, const float* intrinsics,
                             const float* scale, const float* shift, float near, float far, uint64_t seed, uint32_t step,
                             int ray_id0, int R, float* rays_o, float* rays_d, float* viewdirs, float* near_out,
                             float* far_out, float* target, float* target_h, float* mask, float* hyp_raw, int* pixels,
                             plnerf_stream_t stream);

/* The gradient of plnerf_depth_loss's total loss with respect to the per-view depth scale and shift of the view the
 * rays came from (run_nerf_sample_based_depth.py:1113-1120: target_h = hyp * scale[view] + shift[view]).  Inputs as
 * plnerf_depth_loss took them: pred_hyp [R, n_points], target_h [n_hyp, R, target_points] (scaled), hyp_raw of the same
 * shape (unscaled), mask [R] (nullable), is_joint, joint_choice [n_points] (nullable; is_joint only: the hypothesis of
 * each point column chosen over the global batch, else chosen here from these rays), space_carving_weight, threshold.
 * With g_t = d total / d target_h -- the negated gradient plnerf_depth_loss wrote for the chosen hypothesis of each
 * (ray, point), with its normaliser (the mean over R * n_points), tie rule, mask and threshold; 0 elsewhere -- it
 * writes g_scale[view] = sum g_t * hyp_raw, g_shift[view] = sum g_t and 0 into the other n_views - 1 entries of the
 * dense [n_views] fp32 arrays.  fp64 sums in a fixed order, no atomics: bit-reproducible.  `workspace`:
 * PLNERF_DEPTH_SS_WORKSPACE_BYTES.  PLNERF_EINVAL: a NULL required pointer, a size < 1, view outside [0, n_views),
 * target_points neither 1 nor n_points.  PLNERF_ERANGE: R * n_points > 2^30. */
int plnerf_depth_scale_shift_grad(const float* pred_hyp, const float* target_h, const float* hyp_raw, const float* mask,
                                  int R, int n_points, int n_hyp, int target_points, int is_joint, const int* joint_choice,
                                  float space_carving_weight, float threshold, int n_views, int view, float* g_scale,
                                  float* g_shift, void* workspace, plnerf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PLNERF_HIP_DEPTHFEED_H */
