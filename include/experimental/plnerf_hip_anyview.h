/*
 * plnerf_hip_anyview.h -- EXPERIMENTAL: one library call = one rendered view for ANY pair of networks the reference's NeRF
 * class builds -- each of the two on the compiled 8 x 256 trunk or outside it (netwidth > 256, netdepth > 8, several live
 * skips, more than 10 | 4 frequency bands: the layer-by-layer route) -- and the fp32 layer loop of that route as one call.
 *
 * Experimental like the other headers of this directory: the library exports these entries and the binding binds them, but
 * they are outside the registered ABI -- no PLNERF_VERSION step, and they may still change.
 *
 * Conventions: those of plnerf_hip_view.h (device pointers unless said otherwise, caller-owned memory, the structs live in
 * host memory and are read during the call, the call enqueues on `stream` and returns, every argument is checked before the
 * first launch, nothing is allocated inside).
 */
#ifndef PLNERF_HIP_ANYVIEW_H
#define PLNERF_HIP_ANYVIEW_H

#include "../plnerf_hip_view.h"
#include "plnerf_hip_generic.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace plnerf_generic_fwd_f32 needs for `n` rows: two fp32 activation buffers [n, W], up to two fp32 buffers
 * for the rows a layer reads as a concatenation, and the partial products of a layer whose k range is dealt out.  0 when
 * the shape or n is one plnerf_generic_fwd_f32 refuses (and for n == 0, which needs none). */
size_t plnerf_generic_fwd_f32_workspace_bytes(const plnerf_generic_shape* shape, int n);

/* plnerf_generic_fwd (plnerf_hip_generic.h: the same shape, params, rows, out and refusals) in exact fp32: every layer is ONE
 * plnerf_gemm_f32 product C = relu?(A . W^T + bias) -- B is the weight with its strides swapped, bias and ReLU in the
 * epilogue, accumulate 0 -- as the layer-by-layer route issues it, so out equals that route's fp32 result for the same n
 * rows BIT FOR BIT.  k_splits of a layer [M = n, N, K]: tiles = ceil(M / 64) ceil(N / 64); 1 when tiles >= 256, else
 * max(1, min(1024 / tiles, K / 512)) (integer divisions); the partial products lie in the workspace.  (k_splits is 1 for
 * every K below 1,024.  Where it is not, the summation order -- not the exact result -- follows n: a layer with K >= 1,024
 * and fewer than 256 output tiles rounds differently for different n, here as in the route this restates.)
 * A layer whose input is a concatenation ([encoding | activation] behind a skip, [feature | view columns]) reads fp32 rows
 * of a workspace buffer that the producing layer (through its row stride) and a strided copy of the input columns filled:
 * one product over the whole row, one summation order.  The head layers write straight into `out`'s columns.
 * workspace: PLNERF_GENERIC_WORKSPACE_ALIGN-byte aligned, at least plnerf_generic_fwd_f32_workspace_bytes(shape, n) bytes;
 * needs no initialisation and holds nothing the caller may rely on afterwards.
 * n == 0: PLNERF_OK, no launch.
 * PLNERF_EINVAL: as plnerf_generic_fwd (there is no precision to refuse).  PLNERF_ERANGE: a size of the shape above 65,536;
 * n above 4,194,240 (plnerf_gemm_f32's limit).  The size query answers 0 for all of these.  plnerf_generic_fwd itself keeps
 * refusing PLNERF_PREC_FP32. */
int plnerf_generic_fwd_f32(const plnerf_generic_shape* shape, const float* const* params, const float* rows, int64_t ld_rows,
                           int n, void* workspace, size_t workspace_bytes, float* out, int64_t ld_out, plnerf_stream_t stream);

/* How a network slot of plnerf_render_view_any runs. */
#define PLNERF_ANYVIEW_FUSED 0    /* the compiled trunk: plnerf_mlp_fwd in config.precision with the in-kernel encoding      */
#define PLNERF_ANYVIEW_CHAIN16 1  /* plnerf_embed_rows, then plnerf_generic_fwd in the slot's own 16-bit precision            */
#define PLNERF_ANYVIEW_LAYERS32 2 /* plnerf_embed_rows, then plnerf_generic_fwd_f32                                           */

/* One network slot.  Only the fields of its route are read. */
typedef struct plnerf_anyview_net {
    int route;                   /* PLNERF_ANYVIEW_*                                                                          */
    plnerf_view_net fused;       /* FUSED: the 24 parameter tensors and the packed buffer, as plnerf_render_view takes them   */
    plnerf_generic_shape shape;  /* CHAIN16, LAYERS32: use_viewdirs != 0, input_ch = 3 + 6 L, view_ch = 3 + 6 M, L, M <= 16   */
    const float* const* params;  /* CHAIN16, LAYERS32: HOST table of device pointers in state_dict order (plnerf_generic_fwd) */
    int precision;               /* CHAIN16: one of the four 16-bit modes                                                     */
    int* status;                 /* CHAIN16: the range status word plnerf_generic_fwd ORs into, nullable                      */
} plnerf_anyview_net;

/* plnerf_view_io with a route per network and the bound on the rows one network call takes.  The planes mean what they
 * mean there. */
typedef struct plnerf_anyview_io {
    plnerf_anyview_net coarse;
    plnerf_anyview_net fine;
    int max_net_rows;     /* >= 1: a generic slot's pass runs in sub-blocks of at most this many rows (a ray may be cut)      */
    const float* t_vals;
    const float* u_vals;
    float* rgb;
    float* disp;
    float* acc;
    float* depth;
    float* rgb0;
    float* disp0;
    float* acc0;
    float* depth0;
    float* z_std;
    uint8_t* rgb8;
    uint16_t* depth16;
} plnerf_anyview_io;

/* Bytes of the workspace (0: refused): plnerf_render_view's for `config`, and -- with a generic slot -- the embedded rows and
 * the network workspace of one sub-block of min(config.max_rays (n_samples + n_importance), io.max_net_rows) rows.  Reads the
 * slots' routes, shapes and precisions and max_net_rows; no pointer of `io` is followed.  256-byte alignment. */
size_t plnerf_render_view_any_workspace_bytes(const plnerf_step_config* config, const plnerf_anyview_io* io);

/* plnerf_render_view (plnerf_hip_view.h: the same config, args, planes, draws, modes, NDC, density noise and export) with ONE
 * change: the network stage of a pass dispatches on its slot.  A FUSED slot is plnerf_mlp_fwd as there.  A generic slot is,
 * per sub-block of at most io.max_net_rows rows of the pass's [rays, K] samples,
 *   plnerf_embed_rows(pts, viewdirs, NULL, rows, K, L, M, 0, 1.0, NULL, 1.0, embedded) -> plnerf_generic_fwd (CHAIN16) or
 *   plnerf_generic_fwd_f32 (LAYERS32) into the pass's raw outputs,
 * (a sub-block that begins inside a ray embeds that ray's remaining rows in a call of their own), then the pass's density
 * noise as plnerf_render_view draws it.  Rows are independent in both routes, so the frame depends neither on max_net_rows
 * nor on max_rays nor on how the pixel range is split over calls (but for the k_splits remark above: K >= 1,024).
 * Both slots must describe the same (input_ch, view_ch): a FUSED slot's are config.input_ch / input_ch_views (which, like
 * config.precision and fwd_kernel, are ignored when no slot is FUSED), a generic slot's its shape's.
 * args.pack_weights: plnerf_mlp_pack_weights of the FUSED slots once ahead of the first block; a CHAIN16 slot's weights are
 * split by plnerf_generic_fwd in every call of that entry, whatever pack_weights says.
 * PLNERF_EINVAL / PLNERF_ERANGE / PLNERF_ENOSYS: what plnerf_render_view refuses; a route outside the three; max_net_rows < 1;
 * slots of different widths; a generic slot whose shape, params or precision plnerf_generic_fwd / _f32 refuses (the same
 * code), that lacks use_viewdirs, or whose widths are not 3 + 6 L | 3 + 6 M with L, M <= 16. */
int plnerf_render_view_any(const plnerf_step_config* config, const plnerf_anyview_io* io, const plnerf_view_args* args,
                           void* workspace, size_t workspace_bytes, plnerf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PLNERF_HIP_ANYVIEW_H */
