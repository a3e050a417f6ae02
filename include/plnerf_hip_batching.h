/*
 * plnerf_hip_batching.h -- the use_batching ray source of libplnerf_hip.so (PLNERF_VERSION >= 601).
 *
 * A companion of plnerf_hip.h under the same conventions (device pointers, caller-owned memory, work only enqueued on
 * `stream`, 0 or a negative PLNERF_E* code).  It is a header of its own so that plnerf_hip.h's list of entry points,
 * which tests/abi_check.c restates one by one, stays what it was; tests/test_batching_abi.py holds this one to the
 * same checks (plain C99, linked against the library, ctypes signatures parsed from here).
 */
#ifndef PLNERF_HIP_BATCHING_H
#define PLNERF_HIP_BATCHING_H

#include "plnerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Training rays of a shuffled bank of every pixel of every training view (run_plnerf.py:1199-1249, the reference's
 * default use_batching branch), without materialising the bank.  The bank is the views views[0 .. n_views-1] (device
 * int32, entries in [0, N_all) -- not checked here), all H x W with one intrinsic matrix; bank index
 * b = t*H*W + row*W + col names pixel (row, col) of view views[t] (the row order of the reference's rays_rgb before its
 * shuffle), M = n_views*H*W <= 2^30.  Epoch `epoch` visits the bank in the order perm_e(0), ..., perm_e(M-1), perm_e a
 * bijection of [0, M) keyed by (seed, epoch); ray i is bank entry perm_e(pos0 + i), pos0 + R <= M (else PLNERF_ERANGE).
 * c2w [N_all,12] and images [N_all,H,W,3] (nullable) are DEVICE arrays.  Outputs as plnerf_select_rays, bit-identical
 * to it for the same pixel and pose: rays_o, rays_d [R,3]; viewdirs [R,3] (nullable); near_out, far_out [R];
 * target [R,3] = images[views[t], row, col, :] (nullable); bank_index [R] int32 (nullable). */
int plnerf_select_bank_rays(int n_views, const int* views, int H, int W, float fx, float fy, float cx, float cy,
                            const float* c2w, const float* images, uint64_t seed, uint32_t epoch, int pos0, int R,
                            float near, float far, float* rays_o, float* rays_d, float* viewdirs, float* near_out,
                            float* far_out, float* target, int* bank_index, plnerf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PLNERF_HIP_BATCHING_H */
