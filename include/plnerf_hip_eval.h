/*
 * plnerf_hip_eval.h -- held-out view metrics of libplnerf_hip.so (PLNERF_VERSION >= 601).
 *
 * A companion of plnerf_hip.h under the same conventions (device pointers, caller-owned memory, work only enqueued on
 * `stream`, 0 or a negative PLNERF_E* code).  Like plnerf_hip_batching.h it is a header of its own, so that
 * plnerf_hip.h's list of entry points, which tests/abi_check.c restates one by one, stays what it was;
 * tests/test_eval_abi.py holds this one to the same checks (plain C99, linked against the library, ctypes signatures
 * parsed from here).
 */
#ifndef PLNERF_HIP_EVAL_H
#define PLNERF_HIP_EVAL_H

#include "plnerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One row of PLNERF_EVAL_ROW fp64 values per frame. */
#define PLNERF_EVAL_ROW 5
#define PLNERF_EVAL_SSE_RGB 0     /* sum over H*W*3 of (pred - target)^2, pred NOT clamped                           */
#define PLNERF_EVAL_SSE_RGB0 1    /* the same for pred0; NaN when pred0 is NULL                                       */
#define PLNERF_EVAL_SSIM 2        /* mean SSIM (7x7 box windows, sample covariance, data range 1) of clamp(pred, 0, 1) */
#define PLNERF_EVAL_DEPTH_SSE 3   /* sum over the pixels with valid != 0 of (depth - target_depth)^2; 0 without depth  */
#define PLNERF_EVAL_DEPTH_COUNT 4 /* the number of those pixels                                                       */

/* Output tile of one workgroup, and the caller-owned workspace of a call: one partial row per tile per frame. */
#define PLNERF_EVAL_TILE_H 32
#define PLNERF_EVAL_TILE_W 64
#define PLNERF_EVAL_WORKSPACE_BYTES(n, H, W)                                                                       \
    ((size_t)(n) * (size_t)(((H) + PLNERF_EVAL_TILE_H - 1) / PLNERF_EVAL_TILE_H) *                                 \
     (size_t)(((W) + PLNERF_EVAL_TILE_W - 1) / PLNERF_EVAL_TILE_W) * PLNERF_EVAL_ROW * sizeof(double))

/* Scores n frames of H x W (run_plnerf.py:318-340, run_nerf_helpers.py:537): frame i reads pred, target and pred0
 * (nullable) at offset i*H*W*3 of [n,H,W,3] fp32 arrays, and depth, target_depth ([n,H,W] fp32) and valid ([n,H,W],
 * 0 / nonzero) at offset i*H*W -- the three depth arrays are all given or all NULL.  It writes rows[i*PLNERF_EVAL_ROW
 * .. +PLNERF_EVAL_ROW) (fp64, columns PLNERF_EVAL_*).  SSIM is skimage's structural_similarity(clamp(pred, 0, 1),
 * target, data_range=1, channel_axis=-1) with its defaults: per channel the mean over [3, H-3) x [3, W-3) of
 * (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), moments of 7x7 windows, covariances scaled by
 * 49/48, C1 = 1e-4, C2 = 9e-4; then the mean over the channels.  Moments and sums are fp64.
 * Deterministic: no atomics; each workgroup writes its tile's partial row to `workspace`
 * (PLNERF_EVAL_WORKSPACE_BYTES(n, H, W), 8-byte aligned, no initialisation needed)
 * and a second launch adds the tiles of a frame in a
 * fixed order, so a row does not depend on n or on the other frames of the call.
 * PLNERF_EINVAL: n < 1, H < 7 or W < 7 (smaller than one window), a NULL required pointer, a partial depth triple.
 * PLNERF_ERANGE: n > 65535 or H*W > 2^28. */
int plnerf_eval_metrics(int n, int H, int W, const float* pred, const float* target, const float* pred0,
                        const float* depth, const float* target_depth, const uint8_t* valid, void* workspace,
                        double* rows, plnerf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PLNERF_HIP_EVAL_H */
