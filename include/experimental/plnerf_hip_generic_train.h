/*
 * plnerf_hip_generic_train.h -- EXPERIMENTAL: one TRAINING forward and one backward of a network OUTSIDE the compiled trunk
 * (the layer-by-layer route, plnerf_hip_generic.h) as one library call each, in the arithmetic of the 16-bit precision modes.
 *
 * Experimental like the other headers of this directory: the library exports these entries and the binding binds them, but
 * they are outside the registered ABI -- no PLNERF_VERSION step, and they may still change.
 *
 * The forward is plnerf_generic_fwd's, BIT FOR BIT, but keeps what the backward needs in a caller-owned `saved` state: the
 * weights as packed at the start of the call, every hidden layer's output as the packed planes it produces anyway (a layer in
 * front of a concatenation: the fp32 rows of that concatenation), and per ReLU layer a GATE PLANE: one bit per output
 * element, acc + bias > 0 evaluated in fp32 before the split (a NaN: 0) -- the packed halves do not keep the sign of a
 * positive value below the element's range.  Row i of a gate plane of N columns is (N + 31) / 32 words; bit j & 31 of word
 * j >> 5 belongs to column j.
 *
 * The backward is, layer by layer and BIT FOR BIT, plnerf_gemm_h16_dgrad / plnerf_gemm_h16_wgrad (plnerf_hip_gemm16_bwd.h) as
 * the layered route calls them: the contraction ascends in 16-deep steps, each step hi.hi, lo.hi, hi.lo (the plain modes:
 * hi.hi); the gated, scaled gradient is the first operand, split in the loader; the IEEE-half modes scale a layer's
 * gradient by the 2^s of its max |g|; a weight gradient over many rows is dealt over k_splits workgroups per tile whose
 * partial sums are added in split order; no floating-point atomics.  What differs is where the operands come from: the
 * gate from the gate plane, W and a packed layer's output from their planes (a copy instead of a split), and max |g| from
 * an integer atomic maximum over the bit patterns of |g| in the epilogue of the product that writes g (order-independent,
 * so deterministic; a NaN compares above infinity and gives s = 0).  Only the columns of a gradient that a layer consumes
 * are computed: none for the first layer's input, the activation columns behind a concatenation, the feature columns
 * behind the view concatenation.  No gradient with respect to `rows`.
 *
 * Conventions: those of plnerf_hip.h (device pointers unless said otherwise, the call enqueues on `stream` and returns,
 * every argument is checked before the first launch, nothing is allocated inside, a refused call enqueues nothing).
 */
#ifndef PLNERF_HIP_GENERIC_TRAIN_H
#define PLNERF_HIP_GENERIC_TRAIN_H

#include "plnerf_hip_generic.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the saved state of one forward over `n` rows: the packed weights of every layer that runs, then per such layer
 * its gate plane (ReLU layers) and its output -- packed [n, N], or the fp32 concatenation rows [n, input_ch + W] behind a
 * skip and [n, W + view_ch] behind feature_linear (row strides rounded up to 4 floats) --, every piece rounded up to 256
 * bytes.  Per hidden element: 4 bytes in the split modes, 2 in the plain ones, plus one bit.  0 when the shape, n or the
 * precision is one plnerf_generic_train_fwd refuses. */
size_t plnerf_generic_train_saved_bytes(const plnerf_generic_shape* shape, int n, int precision);

/* Bytes of the backward's scratch for `n` rows: one fp32 max-|g| word per layer, two fp32 gradient buffers [n, W] that
 * alternate between the layers, and the largest `partials` of a weight gradient (k_splits [N, K + 1] blocks).  0 as above. */
size_t plnerf_generic_train_workspace_bytes(const plnerf_generic_shape* shape, int n, int precision);

/* The k_splits the backward uses for the weight gradient [N, K1 = K + 1] of a layer over M rows.  No device work.
 * The rule: tiles = ceil(N / 64) ceil(K1 / 64); 1 when tiles >= 256, otherwise max(1, min(1024 / tiles, M / 512)), the
 * divisions rounding down.  Split z takes the 32-row stages [z P, min(S, (z + 1) P)), S = ceil(M / 32),
 * P = ceil(S / k_splits); the split order is part of the result's bits. */
int plnerf_generic_train_wgrad_splits(int N, int K1, int M);

/* plnerf_generic_fwd with the same arguments, the same bits in `out` and the same bits raised in *status, except that
 * `saved` (PLNERF_GENERIC_WORKSPACE_ALIGN-byte aligned, at least plnerf_generic_train_saved_bytes(shape, n, precision) bytes,
 * no initialisation needed) holds afterwards what plnerf_generic_train_bwd reads: nothing in it is reused within the call.
 * n == 0: PLNERF_OK, no launch.  Refusals: those of plnerf_generic_fwd, `saved` in the workspace's place. */
int plnerf_generic_train_fwd(const plnerf_generic_shape* shape, const float* const* params, const float* rows, int64_t ld_rows,
                             int n, int precision, void* saved, size_t saved_bytes, float* out, int64_t ld_out, int* status,
                             plnerf_stream_t stream);

/* The gradients of every layer's weight and bias, given g_out[n, 4 or output_ch] (fp32, row i at g_out + i ld_g): the
 * gradient of the forward's `out`.
 * shape, rows, ld_rows, n, precision, saved: what the forward was given and what it left (layer 0's weight gradient reads
 * `rows`; `saved` is only read).
 * grads: HOST array of device pointers, one per layer in the layer order of the forward's `params` (pts_linears, views_linears,
 * then feature_linear, alpha_linear, rgb_linear or output_linear): layer l's [N, K + 1] fp32 block [dW | db], row stride
 * K + 1, the layout plnerf_gemm_h16_wgrad writes.  The slot of a layer that does not run (the view layers without
 * use_viewdirs) may be NULL and is not touched.
 * workspace: PLNERF_GENERIC_WORKSPACE_ALIGN-byte aligned, at least plnerf_generic_train_workspace_bytes(shape, n, precision)
 * bytes; needs no initialisation and holds nothing the caller may rely on afterwards.
 * status: the range status word to OR into (PLNERF_RANGE_ACTIVATION: a scaled gradient, or an element of `rows` or of a
 * concatenation, beyond the IEEE-half range was clamped), or NULL.
 * n == 0: every [dW | db] of a layer that runs is written with zeros (plnerf_gemm_h16_wgrad's M == 0 rule); rows, saved,
 * g_out and workspace are not read and may be NULL.
 * PLNERF_EINVAL: a shape or precision plnerf_generic_train_fwd refuses; n < 0; grads NULL, or the slot of a layer that runs;
 * ld_rows < input_ch + view_ch; ld_g < the output's columns; rows, g_out, saved or workspace NULL with n > 0; saved or
 * workspace misaligned or shorter than its size query's answer.  PLNERF_ERANGE: as plnerf_generic_train_fwd. */
int plnerf_generic_train_bwd(const plnerf_generic_shape* shape, const float* rows, int64_t ld_rows, int n, int precision,
                             const void* saved, size_t saved_bytes, const float* g_out, int64_t ld_g, float* const* grads,
                             void* workspace, size_t workspace_bytes, int* status, plnerf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PLNERF_HIP_GENERIC_TRAIN_H */
