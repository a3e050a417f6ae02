/*
 * plnerf_hip_dpstep.h -- EXPERIMENTAL: the one-call training steps cut in two at the gradient exchange, for data-parallel
 * runs (one process per GPU, each with a shard of the step's rays).
 *
 * Experimental like the other headers of this directory: the library exports these entries and the binding binds them, but
 * they are outside the registered ABI -- no PLNERF_VERSION step, and they may still change.
 *
 * A one-call step (plnerf_train_step, plnerf_train_step_const, plnerf_depth_train_step, plnerf_depth_train_step_const) ends
 * in its own Adam launches on this process's gradients.  A data-parallel step has to SUM the gradients over the ranks
 * between the backward and the optimizer, so each of the four steps is offered here as two calls:
 *
 *     *_grads(config, io, args, workspace, workspace_bytes, stream)    everything up to and including the backward of both
 *                                                                      networks: io.{coarse,fine}.grad_flat[0 .. n_params)
 *                                                                      hold this rank's gradients, [n_params] the range
 *                                                                      status of this rank's forward; no optimizer launch
 *     (the caller's exchange, on the same stream or ordered behind it: a SUM all-reduce over the ranks)
 *     *_apply(config, io, args, grad_scale, stream)                    the step's optimizer launches, every gradient entry
 *                                                                      multiplied by grad_scale (1 / world for a SUM)
 *
 * The existing entry IS `grads` followed by `apply(1.0f)`: the same launches, the same arguments, the same order.
 *
 * Conventions: those of plnerf_hip_step.h.  The structs are that header's and plnerf_hip_depthstep.h's, unchanged, live in
 * host memory and are read during the call; the workspace is the one-call step's (the *_workspace_bytes and *_layout queries
 * of the existing entries answer for these too: the carve does not change); a call allocates nothing, waits for nothing,
 * reads no device memory and no environment; every argument is checked before the first launch, so a refused call has
 * enqueued nothing.
 *
 * The exchange.  When both networks' gradient blocks lie back to back -- coarse.grad_flat[0 .. n_c + 4) directly followed by
 * fine.grad_flat[0 .. n_f + 4) -- ONE in-place SUM all-reduce over n_c + n_f + 8 floats carries both gradients and both range
 * status words.  A status word is non-zero AS A 32-BIT WORD after the SUM exactly when some rank's forward of that network
 * left the IEEE-half range, on every rank alike: hand `apply` the ADDRESSES OF THE REDUCED WORDS as guard words
 * (io.fine.skip_if_set = &fine.grad_flat[n_f], io.fine.skip_if_set2 = &coarse.grad_flat[n_c], io.coarse.skip_if_set =
 * &coarse.grad_flat[n_c]; the depth step guards both halves of its one optimizer by both words) and every rank withholds
 * the same steps.  `apply` takes the guard words and `withheld` from io as given.
 */
#ifndef PLNERF_HIP_DPSTEP_H
#define PLNERF_HIP_DPSTEP_H

#include "../plnerf_hip.h"
#include "../plnerf_hip_step.h"
#include "../plnerf_hip_depthstep.h"
#include "../plnerf_hip_conststep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* plnerf_train_step / plnerf_train_step_const up to and including the backward of both networks: ray selection, both
 * weight packs, the forward, the loss (io.loss4 is written; args.loss_scale applies), both plnerf_quad_bwd launches and
 * plnerf_mlp_bwd_multi.  Checks and return codes are the whole step's, but for the Adam step counts and the guard words,
 * which these calls do not read.  config.mode must be the entry's. */
int plnerf_train_step_grads(const plnerf_step_config* config, const plnerf_step_io* io, const plnerf_step_args* args,
                            void* workspace, size_t workspace_bytes, plnerf_stream_t stream);
int plnerf_train_step_const_grads(const plnerf_step_config* config, const plnerf_step_io* io, const plnerf_step_args* args,
                                  void* workspace, size_t workspace_bytes, plnerf_stream_t stream);

/* The two plnerf_adam_step launches of plnerf_train_step / plnerf_train_step_const, the fine network's first, with
 * grad_scale in place of 1.0f: reads config.beta1 / beta2 / adam_eps, args.lr_* and args.adam_step_*, and of io the two
 * networks (param_flat, grad_flat, exp_avg, exp_avg_sq, n_params, skip_if_set, skip_if_set2, withheld).  Serves both modes
 * (config.mode may be either).  PLNERF_EINVAL: a NULL struct, a grad_scale that is not finite and > 0, a step count < 1, a
 * network the whole step would refuse. */
int plnerf_train_step_apply(const plnerf_step_config* config, const plnerf_step_io* io, const plnerf_step_args* args,
                            float grad_scale, plnerf_stream_t stream);

/* plnerf_depth_train_step / plnerf_depth_train_step_const up to and including the backward of both networks; with
 * args.ss_step that includes the plnerf_depth_scale_shift_grad launch that fills io.ss_grad [2, n_views] (this rank's: it is
 * SUMmed over the ranks like the networks' gradients).  io.loss5 is written.  Checks and return codes are the whole
 * step's, but for the Adam step counts (args.adam_step, args.ss_adam_step), which these calls do not read. */
int plnerf_depth_train_step_grads(const plnerf_depth_step_config* config, const plnerf_depth_step_io* io,
                                  const plnerf_depth_step_args* args, void* workspace, size_t workspace_bytes,
                                  plnerf_stream_t stream);
int plnerf_depth_train_step_const_grads(const plnerf_depth_step_config* config, const plnerf_depth_step_io* io,
                                        const plnerf_depth_step_args* args, void* workspace, size_t workspace_bytes,
                                        plnerf_stream_t stream);

/* The two clipped plnerf_adam_step launches of the depth step (coarse half first, config.clip_value) and, with
 * args.ss_step, plnerf_depth_ss_adam over io.scale / io.shift: all three with grad_scale in place of 1.0f.  Serves both
 * modes.  PLNERF_EINVAL: a NULL struct, a grad_scale that is not finite and > 0, args.adam_step < 1, with ss_step
 * args.ss_adam_step < 1 or one of io.scale, shift, ss_grad, ss_exp_avg, ss_exp_avg_sq NULL, config.n_views < 1, a network the
 * whole step would refuse. */
int plnerf_depth_train_step_apply(const plnerf_depth_step_config* config, const plnerf_depth_step_io* io,
                                  const plnerf_depth_step_args* args, float grad_scale, plnerf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PLNERF_HIP_DPSTEP_H */
