/*
 * plnerf_hip_conststep.h -- piecewise-constant mode in one library call per optimisation step (PLNERF_VERSION >= 601).
 *
 * A companion of plnerf_hip_step.h and plnerf_hip_depthstep.h under their conventions: the structs are theirs, live in host
 * memory and are read during the call; the call allocates nothing, waits for nothing, reads no device memory and no
 * environment; every argument is checked before the first launch, so a refused call has enqueued nothing.  It is a header of
 * its own so that the existing entries, which refuse PLNERF_MODE_CONSTANT, stay what they were; tests/test_conststep_abi.py
 * holds this one to the same checks (plain C99, linked against the library, ctypes signatures parsed from here).
 *
 * Piecewise-constant mode is the vanilla-NeRF baseline, the `constant_init` warm-up of every PL-NeRF run and the depth
 * script's constant configuration.
 *
 * Workspaces.  Each const step carves its workspace exactly as its linear sibling does -- the loss kernel's partial sums
 * first, at the same offset, and every other plane where the sibling keeps it -- so a run that switches entries between
 * steps (K warm-up steps through plnerf_train_step_const, then plnerf_train_step) hands ONE workspace of
 * max(const bytes, linear bytes) to both, zeroed once before the first step.  Nothing is carried from step to step beyond
 * the zeros every step leaves in the loss partials.
 */
#ifndef PLNERF_HIP_CONSTSTEP_H
#define PLNERF_HIP_CONSTSTEP_H

#include "plnerf_hip.h"
#include "plnerf_hip_constepi.h"
#include "plnerf_hip_step.h"
#include "plnerf_hip_depthstep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The backward of plnerf_fine_epilogue_const (plnerf_hip_constepi.h) with respect to `raw` as one launch, one wavefront per
 * ray.  Bit-identical to the sequence
 *     g_in = plnerf_sample_const_bwd(bins, contiguous(weights[:, 1:-1]), u, inds, g_hyp, B = S - 1)      [R,S-2]
 *     g_w  = g_weights + pad(g_in, 1, 1)   (one fp32 add per element; pad(g_in) alone when g_weights is NULL)
 *     plnerf_quad_bwd(raw, ..., PLNERF_MODE_CONSTANT, ..., g_rgb, g_depth, g_acc, g_w, NULL, NULL, g_raw, absmax_out)
 * on the same inputs; g_in stays on chip.
 *   the forward's inputs: raw [R,S,4], z [R,S], near, far [R], rays_d [R,3], noise [R,S] or NULL;
 *   its saved outputs: weights [R,S] (the interior weights[:, 1:-1] is read in place, row stride S), bins [R,S-1], the
 *     draws u ([R,N] with u_row_stride == N, or one shared row with 0), inds int64 [R,N];
 *   upstream: g_rgb [R,3]; g_depth [R], g_acc [R], g_weights [R,S], g_hyp [R,N] each NULL = zero.  With g_hyp NULL the call
 *     is plnerf_quad_bwd in constant mode and weights, bins, u, inds are not read;
 *   outputs: g_raw [R,S,4] (16-byte aligned, like raw: else PLNERF_EINVAL);
 *     absmax_out NULL or ceil(R / PLNERF_QUAD_RAYS_PER_GROUP) words, every entry written with plain
 *     stores: plnerf_quad_bwd's contract.
 * Refused before anything touches a device: PLNERF_EINVAL for R < 0, S < 3, N < 1, a stride other than 0 or N, g_hyp given
 * without weights, bins, u or inds, a required pointer NULL (with R > 0); PLNERF_ERANGE for S > PLNERF_MAX_SAMPLES, N > 1024
 * or a wave's LDS row (S + max(6 (S - 1) + 4 N, 9 S + 12) floats) over the limit.  R == 0: PLNERF_OK, nothing launched. */
int plnerf_fine_epilogue_const_bwd(const float* raw, const float* z, const float* near, const float* far,
                                   const float* rays_d, const float* noise, const float* weights, const float* bins,
                                   const float* u, int u_row_stride, const int64_t* inds, int R, int S, int N, int white_bkgd,
                                   const float* g_rgb, const float* g_depth, const float* g_acc, const float* g_weights,
                                   const float* g_hyp, float* g_raw, uint32_t* absmax_out, plnerf_stream_t stream);

/* plnerf_train_step's piecewise-constant sibling: the same sequence with plnerf_coarse_epilogue_const in place of
 * plnerf_coarse_epilogue and PLNERF_MODE_CONSTANT in plnerf_quad_fwd and both plnerf_quad_bwd launches.  config.mode must
 * be PLNERF_MODE_CONSTANT (PLNERF_MODE_LINEAR: PLNERF_EINVAL, size 0) and n_samples >= 3; color_mode must be valid and is,
 * like farcolorfix, zero_tol and epsilon, ignored by the constant-mode kernels.  Everything else -- structs, checks, return
 * codes, draws -- as plnerf_train_step.  Bytes: 0 when the configuration is refused. */
size_t plnerf_train_step_const_workspace_bytes(const plnerf_step_config* config);
int plnerf_train_step_const(const plnerf_step_config* config, const plnerf_step_io* io, const plnerf_step_args* args,
                            void* workspace, size_t workspace_bytes, plnerf_stream_t stream);

/* plnerf_depth_train_step's piecewise-constant sibling (plnerf_depth_step_config has no mode: the entry's name is the mode):
 * plnerf_coarse_epilogue_const for the coarse epilogue; plnerf_fine_epilogue_const for the last stage, which leaves its
 * weights [R,F] and bins [R,F-1] (F = n_samples + n_importance) where the linear step keeps tau and T; with args.carve
 * plnerf_fine_epilogue_const_bwd in place of plnerf_sample_pl_bwd + the fine plnerf_quad_bwd, else that plnerf_quad_bwd in
 * PLNERF_MODE_CONSTANT; the coarse plnerf_quad_bwd in PLNERF_MODE_CONSTANT.  Ray selection, the is_joint row, the noise,
 * plnerf_depth_loss, plnerf_depth_scale_shift_grad, plnerf_mlp_bwd_multi, the clipped Adam launches and plnerf_depth_ss_adam
 * are the linear step's.  n_samples >= 3; a shape whose const kernels would refuse (the backward's LDS row over the limit) is
 * PLNERF_ERANGE and size 0.  The layout's offsets equal plnerf_depth_train_step_layout's. */
size_t plnerf_depth_train_step_const_workspace_bytes(const plnerf_depth_step_config* config);
int plnerf_depth_train_step_const_layout(const plnerf_depth_step_config* config, plnerf_depth_step_views* out);
int plnerf_depth_train_step_const(const plnerf_depth_step_config* config, const plnerf_depth_step_io* io,
                                  const plnerf_depth_step_args* args, void* workspace, size_t workspace_bytes,
                                  plnerf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PLNERF_HIP_CONSTSTEP_H */
