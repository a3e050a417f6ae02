/*
 * plnerf_hip_sampleerr.h -- the importance-sampling error of libplnerf_hip.so (PLNERF_VERSION >= 601).
 *
 * A companion of plnerf_hip.h under the same conventions (device pointers, caller-owned memory, work only enqueued on
 * `stream`, 0 or a negative PLNERF_E* code).  Like plnerf_hip_eval.h it is a header of its own, so that plnerf_hip.h's
 * list of entry points, which tests/abi_check.c restates one by one, stays what it was; tests/test_sampleerr_abi.py
 * holds this one to the same checks (plain C99, linked against the library, ctypes signatures parsed from here).
 */
#ifndef PLNERF_HIP_SAMPLEERR_H
#define PLNERF_HIP_SAMPLEERR_H

#include "plnerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One row of PLNERF_SAMPLEERR_ROW fp64 values per call (or per frame, accumulated over its chunks). */
#define PLNERF_SAMPLEERR_ROW 2
#define PLNERF_SAMPLEERR_SUM 0      /* sum over the counted rays of mean_k |pred_hyp[r,k] - depth[r]| */
#define PLNERF_SAMPLEERR_COUNT 1    /* the number of counted rays                                      */

/* Rays per workgroup of the first launch, and the hypotheses per ray the kernel takes. */
#define PLNERF_SAMPLEERR_RAYS_PER_GROUP 64
#define PLNERF_SAMPLEERR_MAX_N 1024

/* Bytes of the caller-owned workspace of a call over R rays: one partial row per workgroup; 0 for R <= 0. */
size_t plnerf_sample_error_workspace_bytes(int R);

/* The per-view term of test_images_samples (depth_supervised_exps/run_nerf_sample_based_depth.py:396-411) over R rays:
 * ray r reads pred_hyp[r*N .. r*N+N) ([R,N] fp32, ray-major), depth[r] ([R] fp32, the rendered depth_map) and
 * valid[r] ([R] uint8, 0 / nonzero; NULL = every ray counts).  Over the rays with valid[r] != 0 it forms, in fp64 from
 * the fp32 inputs, row[PLNERF_SAMPLEERR_SUM] = sum_r (1/N) sum_k |pred_hyp[r,k] - depth[r]| and
 * row[PLNERF_SAMPLEERR_COUNT] = their number; sum / count is the reference's per-view mean (NaN without a counted ray).
 * N being the same for every ray, the kernel adds |h - d| over all counted (r, k) and divides by N once, at the end.
 * A NaN in a counted ray makes the sum NaN; an uncounted ray is not read into it.
 * accumulate = 0 writes the row; accumulate != 0 adds the call's two values to it on the device, so that a frame can be
 * scored chunk by chunk in stream order with no host read in between.  R = 0 writes zeros (accumulate = 0) or leaves
 * the row untouched (accumulate != 0).
 * Deterministic: no atomics; each workgroup of PLNERF_SAMPLEERR_RAYS_PER_GROUP rays writes its partial row to
 * `workspace` (plnerf_sample_error_workspace_bytes(R), 8-byte aligned, no initialisation needed)
 * and a second launch adds the partials
 * in a fixed order, so the row is bit-identical from run to run.
 * PLNERF_EINVAL: row NULL, or pred_hyp, depth or workspace NULL with R > 0.
 * PLNERF_ERANGE: R < 0, N < 1 or N > PLNERF_SAMPLEERR_MAX_N. */
int plnerf_sample_error(int R, int N, const float* pred_hyp, const float* depth, const uint8_t* valid, int accumulate,
                        void* workspace, double* row, plnerf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PLNERF_HIP_SAMPLEERR_H */
