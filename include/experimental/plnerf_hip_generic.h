/*
 * plnerf_hip_generic.h -- EXPERIMENTAL: the whole forward of a network OUTSIDE the compiled trunk (netwidth > 256,
 * netdepth > 8, several live skips, multires > 10: the layer-by-layer route) in ONE library call, without autograd, in the
 * arithmetic of the 16-bit precision modes, with the activations between the layers kept as 16-bit planes in a workspace.
 *
 * Experimental like the other headers of this directory: the library exports these entries and the binding binds them, but
 * they are outside the registered ABI -- no PLNERF_VERSION step, and they may still change.
 *
 * The arithmetic is plnerf_gemm_h16's (plnerf_hip_gemm16.h), layer by layer, BIT FOR BIT: that entry splits both operands in
 * its loader (IEEE-half modes: clamp to +-65,504 and note the range bit; hi = the value rounded to nearest even; split
 * modes: lo = the exact fp32 residual x - hi rounded to nearest even).  Here the weights are split once per call
 * (plnerf_pack_h16) and a layer's epilogue applies the same functions to relu?(acc + bias) and stores the halves, so the
 * next layer's MFMA operands are the same bits, k ascends in the same 16-deep steps from 0, and the same range bit is
 * raised -- by the producer instead of the consumer.
 *
 * PACKED ROWS.  A packed matrix [rows, K] is a `hi` plane of 16-bit elements (IEEE half in PLNERF_PREC_F16X3 / _F16, bf16
 * in PLNERF_PREC_BF16X3 / _BF16), row i at byte offset 2 i ldp with ldp = PLNERF_PACK_LD(K) = K rounded up to a multiple of 8
 * (every row starts 16-byte aligned when the plane does); in the split modes (PLNERF_PREC_F16X3, _BF16X3) a `lo` plane of the
 * same shape follows it at byte offset 2 rows ldp.  Columns K .. ldp - 1 are never read and never written.  The planes
 * must be 16-byte aligned.  PLNERF_PACK_BYTES(rows, K, planes) is the size of a packed matrix.
 *
 * Conventions: those of plnerf_hip.h (device pointers unless said otherwise, the call enqueues on `stream` and returns,
 * every argument is checked before the first launch, nothing is allocated inside).
 */
#ifndef PLNERF_HIP_GENERIC_H
#define PLNERF_HIP_GENERIC_H

#include "../plnerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PLNERF_PACK_LD(K) (((K) + 7) / 8 * 8)
#define PLNERF_PACK_BYTES(rows, K, planes) ((size_t)(planes) * (size_t)(rows) * (size_t)PLNERF_PACK_LD(K) * 2u)
#define PLNERF_GENERIC_MAX_SKIPS 16
#define PLNERF_GENERIC_WORKSPACE_ALIGN 16

/* What the reference's NeRF class builds (run_nerf_helpers.py:76-128; view_ch = the direction encoding plus the
 * depth-supervised variant's camera code).  Host memory.
 * Trunk: D layers of width W; layer 0 takes input_ch columns, layer i + 1 takes [encoding | activation] (input_ch + W) when
 * i is in `skips`, W otherwise.  n_view_layers: the modules of views_linears (the class always builds one; they are in the
 * state_dict with or without use_viewdirs).  use_viewdirs != 0: alpha_linear [1, W], feature_linear [W, W], n_view_layers >= 1
 * view layers of width W / 2 (the first takes [feature | view columns], W + view_ch), rgb_linear [3, W / 2]; the output is
 * [rgb | alpha], 4 columns; output_ch is ignored.  use_viewdirs == 0: output_linear [output_ch, W]; the view layers do not
 * run (n_view_layers only counts their slots in `params`).
 * skips: n_skips <= PLNERF_GENERIC_MAX_SKIPS entries, each in [0, D - 2] (an entry of D - 1 would concatenate behind the LAST
 * trunk layer, which no head layer of the class can consume; entries beyond it the class ignores -- leave them out);
 * repeats are allowed. */
typedef struct plnerf_generic_shape {
    int D;
    int W;
    int input_ch;
    int view_ch;
    int use_viewdirs;
    int output_ch;
    int n_view_layers;
    int n_skips;
    int skips[PLNERF_GENERIC_MAX_SKIPS];
} plnerf_generic_shape;

/* src [rows, K] fp32 (row i at src + i ld, ld >= K) -> the packed matrix at dst (see PACKED ROWS; PLNERF_PACK_BYTES(rows, K,
 * 2 in the split modes, 1 in the plain ones) bytes, 16-byte aligned).  One streaming kernel.
 * IEEE-half modes: an element beyond +-65,504 or not finite is packed clamped to +-65,504 and ORs `range_bit`
 * (PLNERF_RANGE_ACTIVATION or PLNERF_RANGE_WEIGHT) into *status -- at most one atomic per workgroup; status NULL: silent.
 * bf16-element modes set nothing.  rows == 0 or K == 0: PLNERF_OK, no launch.
 * PLNERF_EINVAL: a negative size, ld < K, src or dst NULL, dst not 16-byte aligned, a precision that is none of the four 16-bit
 * modes, a range_bit that is neither of the two.  PLNERF_ERANGE: more than 2^31 - 1 workgroups (of 256 eight-column chunks), or
 * K above 2^31 - 16. */
int plnerf_pack_h16(const float* src, int64_t ld, int rows, int K, int precision, void* dst, int* status, int range_bit,
                    plnerf_stream_t stream);

/* Bytes of workspace plnerf_generic_fwd needs for `n` rows: the packed weights of every layer, two packed activation
 * buffers [n, W], and up to two fp32 buffers for the rows a layer reads as a concatenation.  0 when the shape, n or the
 * precision is one plnerf_generic_fwd refuses. */
size_t plnerf_generic_fwd_workspace_bytes(const plnerf_generic_shape* shape, int n, int precision);

/* out[n, 4 or output_ch] = the network applied to rows[n, input_ch + view_ch] (fp32, row i at rows + i ld_rows; the view
 * columns are read only with use_viewdirs).  The density column is RAW: an activation on it (the depth-supervised variant's
 * softplus) is the caller's.
 * params: HOST array of device pointers, fp32, contiguous, in the class's state_dict order: pts_linears.{0 .. D-1}.weight,
 * .bias; views_linears.{0 .. n_view_layers-1}.weight, .bias (not read without use_viewdirs: may be NULL); then
 * feature_linear, alpha_linear, rgb_linear (weight, bias each) with use_viewdirs, output_linear (weight, bias) without.
 * Enqueues: the weight packs (plnerf_pack_h16, PLNERF_RANGE_WEIGHT), then every layer.  A layer reads packed planes and
 * writes packed planes; the first layer reads `rows` in place; a layer whose input is a concatenation reads fp32 rows of a
 * workspace buffer that the producing layer (fp32, through its row stride) and a strided copy of the encoding columns
 * filled; the head layers write straight into `out`'s columns.  A row's result does not depend on n, on the rows beside
 * it or on how rows are split over calls.
 * workspace: PLNERF_GENERIC_WORKSPACE_ALIGN-byte aligned, at least plnerf_generic_fwd_workspace_bytes(shape, n, precision)
 * bytes; needs no initialisation and holds nothing the caller may rely on afterwards.
 * status: the range status word to OR into (PLNERF_RANGE_ACTIVATION: an input row element or a hidden activation beyond the
 * IEEE-half range was clamped; PLNERF_RANGE_WEIGHT: a weight), or NULL.
 * n == 0: PLNERF_OK, no launch.
 * PLNERF_EINVAL: shape NULL or not one described above (D < 1, W < 1 -- < 2 with use_viewdirs --, input_ch < 1, view_ch < 0,
 * output_ch < 1 without use_viewdirs, n_view_layers < 1 with it, n_skips outside [0, PLNERF_GENERIC_MAX_SKIPS], a skip outside
 * [0, D - 2]); a precision that is none of the four 16-bit modes; n < 0; params or one of the pointers it must hold NULL;
 * rows, workspace or out NULL with n > 0; ld_rows < input_ch + view_ch; ld_out < the output's columns; a workspace that is
 * misaligned or shorter than the size query's answer.  PLNERF_ERANGE: D, W, input_ch, view_ch, n_view_layers or output_ch above
 * 65,536 (the size query answers 0); a layer with more than 2^31 - 1 output tiles (128 rows x 128 columns) or a copy of the
 * encoding columns with more than 2^31 - 1 workgroups (256 elements each). */
int plnerf_generic_fwd(const plnerf_generic_shape* shape, const float* const* params, const float* rows, int64_t ld_rows, int n,
                       int precision, void* workspace, size_t workspace_bytes, float* out, int64_t ld_out, int* status,
                       plnerf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PLNERF_HIP_GENERIC_H */
