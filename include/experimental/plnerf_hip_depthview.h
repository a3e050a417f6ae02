/*
 * experimental/plnerf_hip_depthview.h -- one library call = one rendered view of the DEPTH-SUPERVISED variant, with its
 * sampling-error row and 8 / 16-bit export.
 *
 * EXPERIMENTAL: this header is not part of the registered ABI.  It lives outside the glob include/plnerf_hip*.h that the
 * registry of plnerf_amd._lib.HEADERS (and tests/test_abi_headers.py, tests/test_containment_table.py) covers; its entries
 * are bound from the second table _lib.EXPERIMENTAL_HEADERS and held to the same checks by tests/test_depthview_abi.py and
 * tests/test_gpu_depth_view.py.  Signatures and struct layouts may still change without a PLNERF_VERSION step.  Promoting
 * it is a later change: move the file to include/plnerf_hip_depthview.h, move its row into _lib.HEADERS and give its
 * entries rows in tests/containment.py.  A C host includes it as "experimental/plnerf_hip_depthview.h" under -I include.
 *
 * The conventions are plnerf_hip_view.h's: device pointers, caller-owned memory, work only enqueued on `stream`, 0 or a
 * negative PLNERF_E* code; the structs live in host memory and are read during the call; the call allocates nothing, waits
 * for nothing, reads no device memory and no environment; every argument is checked before the first launch, so a refused
 * call has enqueued nothing.
 *
 * plnerf_depth_render_view enqueues what render() -> batchify_rays() -> render_rays() of
 * depth_supervised_exps/run_nerf_sample_based_depth.py (:85-160, :71-83, :792-958) do for a full view whose pose and
 * intrinsics are device tensors, under torch.no_grad(), for the two view-dependent 8 x 256 networks with importance
 * sampling -- the forward half of plnerf_depth_train_step / plnerf_depth_train_step_const -- as the sequence of this
 * library's own entry points, per block of at most config.max_rays pixels:
 *
 *   plnerf_depth_view_rays -> plnerf_coarse_samples -> plnerf_mlp_fwd (coarse) -> (plnerf_normal) ->
 *   plnerf_coarse_epilogue | plnerf_coarse_epilogue_const -> plnerf_mlp_fwd (fine) -> (plnerf_normal) ->
 *   plnerf_fine_epilogue | plnerf_fine_epilogue_const -> (plnerf_sample_error, accumulating)
 *
 * and, after the last block, plnerf_frame_export and / or plnerf_frame_export_u16 over the call's pixels.  Draws are
 * counter-based on the stream ids of plnerf_hip_depthstep.h (0 jitter, 1 importance draws, 2 / 3 density noise, 4 the
 * hypotheses' draws), keyed by (config.seed, args.step) and the ray's global id = its pixel index: a frame depends neither
 * on max_rays nor on how a caller splits the pixel range over calls.
 */
#ifndef PLNERF_HIP_DEPTHVIEW_H
#define PLNERF_HIP_DEPTHVIEW_H

#include "../plnerf_hip.h"
#include "../plnerf_hip_constepi.h"
#include "../plnerf_hip_sampleerr.h"
#include "../plnerf_hip_view.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The rays of R consecutive pixels of a view in the depth script's convention: ray i looks through pixel p = pix0 + i in
 * row-major order (row = p / W, col = p % W).  The H x W grid is never built.
 *   c2w_host: 12 floats in HOST memory, rows of the 3 x 4 camera-to-world matrix;
 *   rays_o, rays_d [R,3]; viewdirs [R,3] or NULL; near_out, far_out [R] (constant columns).
 * Convention (depth_supervised_exps/model/run_nerf_helpers.py:243-263): pixel CENTRES and a flipped image row, camera
 * direction (((col + 0.5) - cx) / fx, ((H - (row + 0.5)) - cy) / fy, -1) rotated by c2w, origin = camera centre.  The fp32
 * ARITHMETIC is that of the torch expressions of depth.get_rays and raybatch.unit_directions evaluated on the device with
 * the intrinsics and the pose as device tensors (what depth.render evaluates there, and what plnerf_select_depth_rays
 * computes for its pixels): a true division by the focal length, and the three terms of the rotation and of the norm
 * summed (t0 + t2) + t1.  The outputs equal those expressions bit for bit on those pixels.
 * PLNERF_EINVAL: H or W < 1, R < 0, pix0 < 0, a focal length of 0, c2w_host or a required output NULL (with R > 0);
 * PLNERF_ERANGE: H W > 2^30 or pix0 + R > H W.  R == 0: PLNERF_OK, nothing launched. */
int plnerf_depth_view_rays(int H, int W, float fx, float fy, float cx, float cy, const float* c2w_host, int pix0, int R,
                           float near, float far, float* rays_o, float* rays_d, float* viewdirs, float* near_out,
                           float* far_out, plnerf_stream_t stream);

/* A grey plane as 16-bit integers of a caller's unit: out16[i] = (uint16) trunc(min(max(gray[i] * mult, 0), 65535)), the
 * product one rounded fp32 multiply, NaN -> 0, +inf -> 65535, -inf -> 0.  With mult = 1000 this is render_video's
 * (depth * 1000).astype(np.uint16) (run_nerf_sample_based_depth.py:277-295) for every value numpy defines, i.e. products
 * in [0, 65536); the clamp defines the rest.  Exactly 2 n bytes are written, for any n and any 2-byte aligned out16.
 * PLNERF_EINVAL: n < 0, gray or out16 NULL (with n > 0), out16 not 2-byte aligned; PLNERF_ERANGE: n > 2^30.
 * n == 0: PLNERF_OK, nothing launched. */
int plnerf_frame_export_u16(const float* gray, float mult, uint16_t* out16, int n, plnerf_stream_t stream);

/* Everything that is fixed for a renderer.  No NDC, no farcolorfix (that script ignores it), no is_joint, no camera code
 * and no bounding box: the restrictions of plnerf_depth_train_step. */
typedef struct plnerf_depth_view_config {
    int max_rays;         /* pixels per block: the workspace is laid out for it                                        */
    int n_samples;        /* coarse samples per ray, 2 (constant mode: 3) .. PLNERF_MAX_SAMPLES                        */
    int n_importance;     /* importance samples (and depth hypotheses) per ray, >= 1; n_samples + n_importance <= 1022 */
    int mode;             /* PLNERF_MODE_LINEAR | PLNERF_MODE_CONSTANT                                                 */
    int color_mode;       /* PLNERF_COLOR_MIDPOINT | PLNERF_COLOR_LEFT                                                 */
    int lindisp;          /* coarse depths linear in disparity                                                         */
    int perturb;          /* != 0: stratified jitter and random draws; 0: io.t_vals / io.u_vals as they are            */
    int white_bkgd;
    float raw_noise_std;  /* > 0: density noise N(0, 1) * raw_noise_std on both passes                                 */
    float zero_tol;       /* the samplers' zero_threshold (1e-4)                                                       */
    float epsilon;        /* ... and epsilon_ (1e-3)                                                                   */
    int H;                /* the view                                                                                  */
    int W;
    float near;           /* the near / far columns of the rays                                                        */
    float far;
    int precision;        /* PLNERF_PREC_*, both networks                                                              */
    int fwd_kernel;       /* PLNERF_FWD_KERNEL_*                                                                       */
    int input_ch;         /* 3 + 6 L, L <= 10 (the in-kernel encoding)                                                 */
    int input_ch_views;   /* 3 + 6 M, M <= 4                                                                           */
    float input_scale;    /* the encoder's input scale (pi for the depth script's networks)                            */
    float density_beta;   /* softplus beta of the density channel (10 there), 0 = none                                 */
    uint64_t seed;        /* key of the draws                                                                          */
} plnerf_depth_view_config;

/* Device memory the caller owns.  A frame plane holds one value (rgb, rgb0: three; pred_hyp: n_importance) per pixel of
 * the H x W view, row-major; a call writes the pixels of its range and no others.  A nullable plane that is left out is
 * computed in the workspace and dropped. */
typedef struct plnerf_depth_view_io {
    plnerf_view_net coarse;   /* plnerf_hip_view.h: 24 parameter tensors and the packed buffer                         */
    plnerf_view_net fine;
    const float* t_vals;      /* [n_samples] = torch.linspace(0, 1, n_samples)                                         */
    const float* u_vals;      /* [n_importance] = torch.linspace(0, 1, n_importance); read only when perturb == 0      */
    float* rgb;               /* [H W, 3] the fine pass's colour (required)                                            */
    float* disp;              /* [H W] each, nullable: the fine pass's disparity, opacity and depth ...                */
    float* acc;
    float* depth;
    float* rgb0;              /* ... the coarse pass's maps [H W, 3], [H W] x 3 ...                                    */
    float* disp0;
    float* acc0;
    float* depth0;
    float* z_std;             /* ... and the spread of the depth hypotheses [H W]                                      */
    float* pred_hyp;          /* [H W, n_importance] nullable: the hypotheses drawn from the final weights             */
    const uint8_t* valid;     /* [H W] nullable, with error_row: the pixels the sampling error counts (0 / nonzero)    */
    double* error_row;        /* [PLNERF_SAMPLEERR_ROW] nullable, with valid: every block adds plnerf_sample_error's two
                                 values; the caller zeroes it before a frame's first call                              */
    uint8_t* rgb8;            /* [H W, 3] nullable: to8b(rgb)                                                          */
    uint16_t* depth16;        /* [H W] nullable: to16b(depth * args.depth16_scale); needs the depth plane              */
    uint16_t* depth_mm16;     /* [H W] nullable: plnerf_frame_export_u16(depth, args.depth_mm_mult); needs the depth plane */
} plnerf_depth_view_io;

/* What changes from call to call. */
typedef struct plnerf_depth_view_args {
    float c2w[12];        /* rows of the view's 3 x 4 camera-to-world matrix                                           */
    float fx;             /* the view's intrinsics (per view in this script)                                           */
    float fy;
    float cx;
    float cy;
    uint32_t step;        /* key of this frame's draws (with config.seed)                                              */
    int pix0;             /* the call renders pixels [pix0, pix0 + n_pix) of the view, row-major                       */
    int n_pix;
    int pack_weights;     /* != 0: plnerf_mlp_pack_weights of both networks first (once per call)                      */
    float depth16_scale;  /* io.depth16 = to16b(depth * depth16_scale): fp32(1) / fp32(far)                            */
    float depth_mm_mult;  /* io.depth_mm16 = trunc(clamp(depth * depth_mm_mult, 0, 65535)): 1000 for millimetres       */
} plnerf_depth_view_args;

/* Bytes of the workspace for this configuration (0: the configuration is refused): one block's rays, samples, raw
 * outputs, noise, the last stage's weights and knots, its hypotheses and their search indices, the sampling error's
 * partial rows and a block of every plane a caller may leave out -- no saved activations and no backward scratch, so less
 * than plnerf_depth_train_step_workspace_bytes of the matching configuration.  256-byte alignment; nothing is carried
 * between calls and nothing need be zeroed. */
size_t plnerf_depth_render_view_workspace_bytes(const plnerf_depth_view_config* config);

/* Render pixels [args.pix0, args.pix0 + args.n_pix) of one view into the frame planes.  PLNERF_EINVAL: a null struct or
 * required pointer (u_vals is required when perturb == 0), n_pix < 1 or pix0 < 0, n_importance < 1, a field of the
 * configuration outside its values, valid without error_row or the reverse, depth16 or depth_mm16 without a depth plane,
 * depth16 or depth_mm16 not 2-byte aligned, error_row not 8-byte aligned, a focal length of 0, feature_linear tensors that
 * are not 16-byte aligned, a workspace that is too small or not 256-byte aligned; PLNERF_ERANGE: a pixel range outside
 * H W, sizes outside the compiled limits (n_samples or n_importance alone, or their sum, over PLNERF_MAX_SAMPLES; max_rays
 * (n_samples + n_importance + 2) rows over INT32_MAX / 4; H W over 2^30); PLNERF_ENOSYS: a precision that is not built. */
int plnerf_depth_render_view(const plnerf_depth_view_config* config, const plnerf_depth_view_io* io,
                             const plnerf_depth_view_args* args, void* workspace, size_t workspace_bytes,
                             plnerf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PLNERF_HIP_DEPTHVIEW_H */
