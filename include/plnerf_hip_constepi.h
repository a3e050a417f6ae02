/*
 * plnerf_hip_constepi.h -- the piecewise-constant mode's one-launch stages of libplnerf_hip.so (PLNERF_VERSION >= 601).
 *
 * A companion of plnerf_hip.h under the same conventions (device pointers, caller-owned memory, work only enqueued on
 * `stream`, 0 or a negative PLNERF_E* code).  Like plnerf_hip_sampleerr.h it is a header of its own, so that
 * plnerf_hip.h's list of entry points, which tests/abi_check.c restates one by one, stays what it was;
 * tests/test_constepi_abi.py holds this one to the same checks (plain C99, linked against the library, ctypes signatures
 * parsed from here).
 *
 * The two entries are the constant-mode siblings of plnerf_coarse_epilogue / plnerf_fine_epilogue (plnerf_hip.h): the same
 * kernel, one wavefront per ray, with compute_weights as the quadrature and sample_pdf as the sampler.  Piecewise-constant
 * mode is the vanilla-NeRF baseline, the `constant_init` warm-up of every PL-NeRF run and the depth script's constant
 * configuration.  There is no color_mode, farcolorfix, zero_tol or epsilon: constant mode ignores them.
 *
 * Both refuse, before anything touches a device:
 *   PLNERF_EINVAL  R < 0, S < 3 (the sampler needs one interior weight), N < 1; u given with a row stride other than 0 or
 *                  N; a required pointer NULL (with R > 0)
 *   PLNERF_ERANGE  S > PLNERF_MAX_SAMPLES; S + N > 1024 (coarse) or N > 1024 (final); the wave's LDS row over the limit
 * and return PLNERF_OK with nothing launched for R == 0.
 */
#ifndef PLNERF_HIP_CONSTEPI_H
#define PLNERF_HIP_CONSTEPI_H

#include "plnerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The coarse pass's epilogue in piecewise-constant mode as one launch (run_plnerf.py:714-735 with mode == "constant", or
 * under constant_init, :710-711): raw2outputs with compute_weights (:504-513, :553-624) -> z_vals_mid and
 * sample_pdf(z_vals_mid, weights[..., 1:-1]) (:722-725, run_nerf_helpers.py:241-284) -> clamp(near, far) (:731) ->
 * sort(cat) (:733-734) -> sample positions (:735), plus z_std = std(clamped samples, unbiased=False) (:752).
 * Bit-identical to the sequence plnerf_quad_fwd (PLNERF_MODE_CONSTANT), z_mid = .5 * (z[1:] + z[:-1]) in torch,
 * plnerf_sample_const on (z_mid, weights[:, 1:-1]), plnerf_merge_sort, plnerf_ray_points on the same inputs -- except
 * z_std, which is the fp64 two-pass value where torch.std works in fp32.  The weights, the bins and the cdf stay on chip.
 *   raw [R,S,4] (16-byte aligned, as plnerf_hip.h demands of it: else PLNERF_EINVAL), z [R,S], near, far [R],
 *   rays_o, rays_d [R,3], noise [R,S] or NULL.
 *   u: [R,N] draws (u_row_stride == N), one shared row (0), or NULL = drawn in the kernel from the counter-based
 *      generator of plnerf_hip.h (stream id 1) for global ray ids ray_id0 .. ray_id0 + R - 1.
 *   outputs: rgb_map [R,3], disp_map, acc_map, depth_map [R] (the coarse maps rgb0, ...), weights [R,S] or NULL,
 *            z_fine [R,S+N] sorted, pts [R,S+N,3], z_std [R].   S >= 3, S + N <= 1024.
 * Backward (with respect to raw, through the maps and the weights): plnerf_quad_bwd in PLNERF_MODE_CONSTANT. */
int plnerf_coarse_epilogue_const(const float* raw, const float* z, const float* near, const float* far,
                                 const float* rays_o, const float* rays_d, const float* noise, const float* u,
                                 int u_row_stride, uint64_t seed, uint32_t step, int ray_id0, int R, int S, int N,
                                 int white_bkgd, float* rgb_map, float* disp_map, float* acc_map, float* depth_map,
                                 float* weights, float* z_fine, float* pts, float* z_std, plnerf_stream_t stream);

/* The depth-supervised variant's LAST stage in piecewise-constant mode as one launch
 * (depth_supervised_exps/run_nerf_sample_based_depth.py:909-934, the constant branch :923-934): raw2outputs of the final
 * pass, then sample_pdf_return_u (model/run_nerf_helpers.py:343-394) on ITS z_vals_mid and weights[..., 1:-1] -> the depth
 * hypotheses pred_hyp (not clamped), and z_std = std(pred_hyp, unbiased=False).
 * Bit-identical to plnerf_quad_fwd (PLNERF_MODE_CONSTANT) followed by plnerf_sample_const on
 * (.5 * (z[1:] + z[:-1]), weights[:, 1:-1]) on the same inputs.  Outputs: the maps as above, weights [R,S] (required: the
 * caller returns them and the backward reads them), bins_out [R,S-1] or NULL (the sampler's bins z_vals_mid, the
 * contiguous operand of plnerf_sample_const_bwd), samples [R,N], inds int64 [R,N] and -- if u_out is given -- the draws
 * used [R,N].  u as above (NULL: drawn in the kernel, counter stream 4).   S >= 3, N <= 1024.
 * Backward: plnerf_sample_const_bwd on (bins_out, weights[:, 1:-1], the draws, inds) gives the gradient of the interior
 * weights, which joins the weights' upstream gradient; then plnerf_quad_bwd in PLNERF_MODE_CONSTANT. */
int plnerf_fine_epilogue_const(const float* raw, const float* z, const float* near, const float* far,
                               const float* rays_d, const float* noise, const float* u, int u_row_stride, uint64_t seed,
                               uint32_t step, int ray_id0, int R, int S, int N, int white_bkgd, float* rgb_map,
                               float* disp_map, float* acc_map, float* depth_map, float* weights, float* bins_out,
                               float* samples, int64_t* inds, float* u_out, float* z_std, plnerf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PLNERF_HIP_CONSTEPI_H */
