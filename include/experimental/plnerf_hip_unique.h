/*
 * plnerf_hip_unique.h -- EXPERIMENTAL: the fine pass's MLP forward over the rows it needs.  After importance sampling and the
 * merge sort a ray's fine pass holds RUNS of bit-identical positions (the sampler returns the left knot wherever the density
 * is flat; every draw of a ray through empty space lands in the last interval); on one ray equal position is equal
 * direction, so such rows are identical network inputs.  plnerf_mlp_fwd_unique evaluates each run's first and last row only.
 *
 * Experimental like the other headers of this directory: the library exports these entries and the binding binds them, but
 * they are outside the registered ABI -- no PLNERF_VERSION step, and they may still change.
 *
 * The rule: row i is INTERIOR when rows i - 1 and i + 1 belong to its ray (the same i / samples_per_ray) and pts[i - 1],
 * pts[i], pts[i + 1] are equal bitwise in all three components (+0.0 and -0.0 differ).  Interior rows are not evaluated; their
 * raw_out is a copy of the run's first row's.  A run's first and last row, and every ray's first and last row, are evaluated.
 * An interior row borders zero-length intervals only: the quadrature hands it an upstream gradient of exactly zero, so the
 * rows that carry gradient, and their order, are the plain forward's -- a training step stays bit-identical.
 *
 * One training use is three calls:
 *   plnerf_mlp_fwd_unique    list + gather + forward over the n_eval evaluated rows + expand: raw_out for ALL n_rows rows;
 *                            `saved` holds the planes of the evaluated rows in COMPACT order (same size and layout as
 *                            plnerf_mlp_fwd's: plnerf_mlp_saved_bytes(n_rows), plnerf_mlp_saved_layout)
 *   plnerf_mlp_unique_fold   g_raw [n_rows][4] -> the compact gradient (workspace + layout.g_raw_u): compact row c gets the
 *                            sum of its run's rows in row order (a term that is exactly zero is skipped, so the sign of a
 *                            zero survives), rows from n_eval on are zero; and its per-workgroup maxima (layout.absmax,
 *                            layout.n_absmax words)
 *   plnerf_mlp_bwd_multi     unchanged, on n_rows, with g_raw = workspace + layout.g_raw_u, g_absmax = workspace +
 *                            layout.absmax / n_absmax = layout.n_absmax (or NULL / 0), and the compact `saved`.  Its live-row
 *                            list drops the zero tail.  The dense backward (PLNERF_BWD_COMPACT=0) would read planes nobody
 *                            wrote: plnerf_mlp_fwd_unique_served says no then.  With a density activation (density_beta > 0)
 *                            its raw_out argument is the COMPACT output, workspace + layout.raw_u; the library's own callers
 *                            take the route without an activation only.
 * The host reads nothing back: n_eval stays on the device, grids are sized by n_rows.
 *
 * Conventions: those of plnerf_hip.h (device pointers, the call enqueues on `stream` and returns, every argument is checked
 * before the first launch).
 */
#ifndef PLNERF_HIP_UNIQUE_H
#define PLNERF_HIP_UNIQUE_H

#include "../plnerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Byte offsets of the workspace's sections (all multiples of 256), P = n_rows rounded up to a multiple of 256:
 *   words    uint32: [0] = n_eval, the number of evaluated rows; the rest is the scan's
 *   rows_u   uint32 [P]: the original row of compact row c, c < n_eval
 *   src      uint32 [P]: the compact row whose output `row` takes = (evaluated rows in [0, row]) - 1, row < n_rows
 *   pts_u, dirs_u   float [P][3]: position and direction of the compact rows, filled with copies of the last evaluated row
 *            up to the next multiple of 256
 *   raw_u    float [P][4]: the forward's output in compact order
 *   g_raw_u  float [P][4]: plnerf_mlp_unique_fold's result
 *   absmax   uint32 [n_absmax]: max |g_raw_u| per workgroup of the fold, as fp32 bits */
typedef struct plnerf_unique_layout {
    size_t words;
    size_t rows_u;
    size_t src;
    size_t pts_u;
    size_t dirs_u;
    size_t raw_u;
    size_t g_raw_u;
    size_t absmax;
    size_t n_absmax;
    size_t total;
} plnerf_unique_layout;

/* layout->total; 0 for n_rows < 1 */
size_t plnerf_mlp_unique_workspace_bytes(int n_rows);
/* PLNERF_EINVAL: layout NULL or n_rows < 1 */
int plnerf_mlp_unique_layout(int n_rows, plnerf_unique_layout* layout);

/* 1: plnerf_mlp_fwd_unique serves this call; 0: take plnerf_mlp_fwd.  Decided on the host, before anything is launched.
 * Served: the register-resident kernel of the split modes (PLNERF_PREC_F16X3 / _BF16X3 with fwd_kernel AUTO or RR), the
 * in-kernel encoding (has_embedded == 0), samples_per_ray >= 3, n_rows a multiple of it, and -- for a training forward
 * (training != 0: `saved` will be given) -- the backward over live rows (PLNERF_BWD_COMPACT is not 0 and n_rows fits its
 * list).  PLNERF_FWD_UNIQUE=0 in the environment (read at every call: A/B measurements) switches the route off. */
int plnerf_mlp_fwd_unique_served(int precision, int has_embedded, int fwd_kernel, int samples_per_ray, int n_rows, int training);

/* plnerf_mlp_fwd's arguments without `embedded`, plus the workspace (plnerf_mlp_unique_workspace_bytes(n_rows) bytes,
 * 256-byte aligned; its contents need not be initialised).  raw_out [n_rows][4] is bitwise what plnerf_mlp_fwd writes.
 * PLNERF_EINVAL: what plnerf_mlp_fwd refuses, a call plnerf_mlp_fwd_unique_served does not serve, workspace NULL or
 * misaligned.  n_rows == 0: PLNERF_OK, no launch. */
int plnerf_mlp_fwd_unique(const void* packed, int precision, const float* pts, const float* viewdirs, int input_ch,
                          int input_ch_views, int n_rows, int samples_per_ray, float input_scale, float density_beta,
                          float* raw_out, void* saved, int fwd_kernel, void* workspace, plnerf_stream_t stream);

/* The fold, on the workspace a plnerf_mlp_fwd_unique of the same n_rows left.  g_raw: [n_rows][4], 16-byte aligned. */
int plnerf_mlp_unique_fold(const float* g_raw, int n_rows, void* workspace, plnerf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PLNERF_HIP_UNIQUE_H */
