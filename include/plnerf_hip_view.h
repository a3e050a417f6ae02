/*
 * plnerf_hip_view.h -- one library call = one rendered view, with 8 / 16-bit export (PLNERF_VERSION >= 601).
 *
 * A companion of plnerf_hip_step.h under its conventions: device pointers, caller-owned memory, work only enqueued on
 * `stream`, 0 or a negative PLNERF_E* code; the structs live in host memory and are read during the call; the call
 * allocates nothing, waits for nothing, reads no device memory and no environment; every argument is checked before the
 * first launch, so a refused call has enqueued nothing.  tests/test_abi_headers.py and tests/test_view_abi.py hold this
 * header to the checks of the others (plain C99, linked against the library, ctypes mirror parsed from here).
 *
 * plnerf_render_view enqueues what render() -> batchify_rays() -> render_rays() (run_plnerf.py:95-175, 627-758) do for a
 * full view whose pose is a device tensor (its rays are then built on the device: see plnerf_view_rays) under
 * torch.no_grad(), for the two view-dependent 8 x 256 networks with importance sampling, as the sequence of this library's
 * own entry points, per block of at most config.max_rays pixels:
 *
 *   plnerf_view_rays -> (plnerf_ndc_rays) -> plnerf_coarse_samples -> plnerf_mlp_fwd (coarse) -> (plnerf_normal) ->
 *   plnerf_coarse_epilogue | plnerf_coarse_epilogue_const -> plnerf_mlp_fwd (fine) -> (plnerf_normal) -> plnerf_quad_fwd
 *
 * and, after the last block, one plnerf_frame_export over the call's pixels.  Draws are counter-based on the stream ids
 * of plnerf_hip_step.h, keyed by (config.seed, args.step) and the ray's global id = its pixel index: a frame depends neither
 * on max_rays nor on how a caller splits the pixel range over calls.
 */
#ifndef PLNERF_HIP_VIEW_H
#define PLNERF_HIP_VIEW_H

#include "plnerf_hip.h"
#include "plnerf_hip_constepi.h"
#include "plnerf_hip_step.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The rays of R consecutive pixels of a view: ray i looks through pixel p = pix0 + i in row-major order (row = p / W,
 * col = p % W).  The H x W grid is never built.
 *   c2w_host: 12 floats in HOST memory, rows of the 3 x 4 camera-to-world matrix (as plnerf_select_rays);
 *   rays_o, rays_d [R,3]; viewdirs [R,3] or NULL; near_out, far_out [R] (constant columns).
 * The convention is plnerf_select_rays' (run_nerf_helpers.py:162-171: camera direction ((col - cx) / fx, -(row - cy) / fy,
 * -1) rotated by c2w, origin = camera centre, no half-pixel offset); the fp32 ARITHMETIC is that of the torch expressions
 * of rays.get_rays and raybatch.unit_directions evaluated on the device, which is where render() evaluates them for a
 * device-resident pose: the division by a focal length is a multiply by its fp32 reciprocal, and the three terms of the
 * rotation and of the norm are summed (t0 + t2) + t1.  The outputs equal those expressions bit for bit on those pixels.
 * PLNERF_EINVAL: H or W < 1, R < 0, pix0 < 0, a focal length of 0, c2w_host or a required output NULL (with R > 0);
 * PLNERF_ERANGE: H W > 2^30 or pix0 + R > H W.  R == 0: PLNERF_OK, nothing launched. */
int plnerf_view_rays(int H, int W, float fx, float fy, float cx, float cy, const float* c2w_host, int pix0, int R,
                     float near, float far, float* rays_o, float* rays_d, float* viewdirs, float* near_out,
                     float* far_out, plnerf_stream_t stream);

/* Quantise a frame's planes for export, both in ONE launch (run_nerf_helpers.py:19-20, to8b / to16b):
 *   rgb [n,3] fp32 (nullable with rgb8)   -> rgb8 [n,3] uint8:  (uint8)(255.f * clip(x, 0, 1))
 *   gray [n] fp32 (nullable with gray16)  -> gray16 [n] uint16: (uint16)(65535.f * clip(gray * gray_scale, 0, 1))
 * Each product is a separately rounded fp32 multiply; the conversion truncates (numpy's astype).  NaN -> 0,
 * +inf -> 255 / 65535, -inf -> 0.  gray_scale is a MULTIPLIER: a caller that wants depth / far passes fp32(1) / fp32(far).
 * Exactly 3 n bytes of rgb8 and 2 n bytes of gray16 are written, for any n and any alignment of the four pointers.
 * PLNERF_EINVAL: n < 0, a plane given without its output or an output without its plane; PLNERF_ERANGE: n > 2^30.
 * n == 0 or both planes NULL: PLNERF_OK, nothing launched. */
int plnerf_frame_export(const float* rgb, uint8_t* rgb8, const float* gray, float gray_scale, uint16_t* gray16, int n,
                        plnerf_stream_t stream);

/* One network as the view call reads it: its 24 parameter tensors (plnerf_mlp_pack_weights' order and alignment:
 * feature_linear.weight and .bias 16 bytes, else PLNERF_EINVAL) and its packed buffer (plnerf_mlp_packed_bytes(precision),
 * 256-byte aligned; status word zeroed by the caller once). */
typedef struct plnerf_view_net {
    const float* params[PLNERF_N_PARAM_TENSORS];
    void* packed;
} plnerf_view_net;

/* Device memory the caller owns.  A frame plane holds one value (rgb, rgb0: three) per pixel of the H x W view, row-major;
 * a call writes the pixels of its range and no others.  A nullable plane that is left out is computed in the workspace
 * and dropped. */
typedef struct plnerf_view_io {
    plnerf_view_net coarse;
    plnerf_view_net fine;
    const float* t_vals;  /* [n_samples] = torch.linspace(0, 1, n_samples)                                            */
    const float* u_vals;  /* [n_importance] = torch.linspace(0, 1, n_importance); read only when perturb == 0         */
    float* rgb;           /* [H W, 3] the fine pass's colour (required)                                               */
    float* disp;          /* [H W] each, nullable: the fine pass's disparity, opacity and depth ...                   */
    float* acc;
    float* depth;
    float* rgb0;          /* ... the coarse pass's maps [H W, 3], [H W] x 3 ...                                       */
    float* disp0;
    float* acc0;
    float* depth0;
    float* z_std;         /* ... and the spread of the importance samples [H W]                                       */
    uint8_t* rgb8;        /* [H W, 3] nullable: to8b(rgb)                                                             */
    uint16_t* depth16;    /* [H W] nullable: to16b(depth * args.depth16_scale)                                        */
} plnerf_view_io;

/* What changes from call to call. */
typedef struct plnerf_view_args {
    float c2w[12];        /* rows of the view's 3 x 4 camera-to-world matrix                                          */
    uint32_t step;        /* key of this frame's draws (with config.seed)                                             */
    int pix0;             /* the call renders pixels [pix0, pix0 + n_pix) of the view, row-major                      */
    int n_pix;
    int pack_weights;     /* != 0: plnerf_mlp_pack_weights of both networks first (once per call)                     */
    float depth16_scale;  /* io.depth16 = to16b(depth * depth16_scale): fp32(1) / fp32(far) for the reference's files   */
} plnerf_view_args;

/* Bytes of the workspace for this configuration (0: the configuration is refused): one block's rays, samples and raw
 * outputs and the planes a caller may leave out -- no saved activations and no backward scratch, so less than
 * plnerf_train_step_workspace_bytes of the same configuration.  256-byte alignment; nothing is carried between calls and
 * nothing need be zeroed.  The configuration is plnerf_step_config: max_rays is the block; mode is PLNERF_MODE_LINEAR or
 * PLNERF_MODE_CONSTANT (n_samples >= 3), both served by this one entry; near / far, the intrinsics, ndc, seed and the
 * sampling fields mean what they mean there; ray_source, n_views, bank_seed and the Adam fields are ignored. */
size_t plnerf_render_view_workspace_bytes(const plnerf_step_config* config);

/* Render pixels [args.pix0, args.pix0 + args.n_pix) of one view into the frame planes.  PLNERF_EINVAL: a null struct or
 * required pointer, n_pix < 1 or pix0 < 0, n_importance < 1, a field of the configuration outside its values, depth16
 * given without a depth plane, a workspace that is too small or not 256-byte aligned; PLNERF_ERANGE: a pixel range outside
 * H W, sizes outside the compiled limits (max_rays (n_samples + n_importance) rows over INT32_MAX / 4); PLNERF_ENOSYS: a
 * precision that is not built. */
int plnerf_render_view(const plnerf_step_config* config, const plnerf_view_io* io, const plnerf_view_args* args,
                       void* workspace, size_t workspace_bytes, plnerf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PLNERF_HIP_VIEW_H */
