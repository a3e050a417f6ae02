"""ctypes binding of libplnerf_hip.so (C ABI declared in include/plnerf_hip.h).

There is NO CPU fallback: if the shared library is missing or a tensor is not on a HIP
device, the call raises.  Build the library with `python __graft_entry__.py` (or
`make -C pl-nerf_amd/csrc`); hipcc cross-compiles gfx950 without a GPU present.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# PLNERF_HIP_LIB overrides the library path (kernel experiments: ablation builds under /tmp)
LIB_PATH = os.environ.get("PLNERF_HIP_LIB") or os.path.join(_HERE, "libplnerf_hip.so")

MODE = {"constant": 0, "linear": 1}
COLOR = {"midpoint": 0, "left": 1}
PRECISION = {"fp32": 0, "bf16x3": 1, "bf16": 2, "f16x3": 3, "f16": 4}
GUARDED_PRECISIONS = ("f16x3", "f16", "bf16x3", "bf16")      # modes whose kernels can set a bit of the range status word
N_PARAM_TENSORS = 24
ABI_VERSION = 601                      # PLNERF_VERSION of include/plnerf_hip.h this binding was written against
QUAD_RAYS_PER_GROUP = 4                # PLNERF_QUAD_RAYS_PER_GROUP: rays per workgroup of plnerf_quad_bwd (its absmax_out)
DEPTH_LOSS_WORKSPACE_BYTES = 4096      # PLNERF_DEPTH_LOSS_WORKSPACE_BYTES
IMAGE_LOSS_WORKSPACE_BYTES = 4096      # PLNERF_IMAGE_LOSS_WORKSPACE_BYTES
# plnerf_mlp_fwd's `fwd_kernel` argument (PLNERF_FWD_KERNEL_*).  The library has no setting of its own; this BINDING
# takes its default from the environment (PLNERF_FWD_KERNEL=rr | pp: the test suite's and tools/' passes over both
# forward kernels) and hands it to every call.
FWD_KERNELS = {"auto": 0, "rr": 1, "pp": 2}
FWD_KERNEL = FWD_KERNELS.get(os.environ.get("PLNERF_FWD_KERNEL") or "auto", 0)
RANGE_ACTIVATION, RANGE_WEIGHT, RANGE_SAVED = 1, 2, 4      # bits of the packed buffer's status word (plnerf_hip.h)

c_f = ctypes.c_void_p      # device pointer
c_i = ctypes.c_int
c_s = ctypes.c_void_p      # hipStream_t

# name -> (restype, argtypes); mirrors include/plnerf_hip.h one to one
SIGNATURES = {
    "plnerf_version": (c_i, []),
    "plnerf_build_flags": (c_i, []),
    "plnerf_error_string": (ctypes.c_char_p, [c_i]),
    "plnerf_quad_fwd": (c_i, [c_f] * 6 + [c_i] * 6 + [c_f] * 7 + [c_s]),
    "plnerf_quad_bwd": (c_i, [c_f] * 6 + [c_i] * 6 + [c_f] * 7 + [c_f, c_s]),
    "plnerf_quad_bwd_rays": (c_i, [c_f] * 6 + [c_i] * 6 + [c_f] * 7 + [c_f] * 4 + [c_s]),
    "plnerf_sample_const": (c_i, [c_f] * 3 + [c_i] * 4 + [c_f] * 2 + [c_s]),
    "plnerf_sample_const_bwd": (c_i, [c_f] * 3 + [c_i] + [c_f] * 2 + [c_i] * 3 + [c_f] + [c_s]),
    "plnerf_sample_pl": (c_i, [c_f] * 7 + [c_i] * 4 + [ctypes.c_float] * 2 + [c_f] * 5 + [c_s]),
    "plnerf_sample_pl_bwd": (c_i, [c_f] * 6 + [c_i] + [c_f] * 2 + [c_i] * 3 + [ctypes.c_float] * 2 + [c_f] * 2 + [c_s]),
    "plnerf_sample_pl_bwd_rays": (c_i, [c_f] * 6 + [c_i] + [c_f] * 2 + [c_i] * 3 + [ctypes.c_float] * 2 + [c_f] * 3 + [c_s]),
    "plnerf_stratified_z": (c_i, [c_f] * 4 + [c_i] * 3 + [c_f] + [c_s]),
    "plnerf_ray_points": (c_i, [c_f] * 3 + [c_i] * 2 + [c_f] + [c_s]),
    "plnerf_merge_sort": (c_i, [c_f] * 4 + [c_i] * 3 + [c_f] + [c_s]),
    "plnerf_coarse_epilogue": (c_i, [c_f] * 8 + [c_i, ctypes.c_uint64, ctypes.c_uint32] + [c_i] * 7 +
                               [ctypes.c_float] * 2 + [c_f] * 10 + [c_s]),
    "plnerf_fine_epilogue": (c_i, [c_f] * 7 + [c_i, ctypes.c_uint64, ctypes.c_uint32] + [c_i] * 7 + [ctypes.c_float] * 2 +
                             [c_f] * 11 + [c_s]),
    "plnerf_uniform": (c_i, [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, c_i, c_i, c_i, c_f, c_s]),
    "plnerf_normal": (c_i, [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, c_i, c_i, c_i, c_f, c_s]),
    "plnerf_select_rays": (c_i, [c_i, c_i] + [ctypes.c_float] * 4 + [ctypes.POINTER(ctypes.c_float), c_f] + [c_i] * 4 +
                           [ctypes.c_uint64, ctypes.c_uint32, c_i, c_i, ctypes.c_float, ctypes.c_float] + [c_f] * 7 +
                           [c_s]),
    "plnerf_ndc_rays": (c_i, [c_i, c_i, ctypes.c_double, ctypes.c_double, c_f, c_f, c_i, c_f, c_f, c_s]),
    "plnerf_coarse_samples": (c_i, [c_f] * 6 + [ctypes.c_uint64, ctypes.c_uint32] + [c_i] * 5 + [c_f] * 2 + [c_s]),
    "plnerf_image_loss": (c_i, [c_f] * 3 + [c_i] + [c_f] * 5 + [c_s]),
    "plnerf_depth_loss": (c_i, [c_f] * 6 + [c_i] * 5 + [c_f] + [ctypes.c_float] * 2 + [c_f] * 5 + [c_s]),
    "plnerf_depth_joint_sums": (c_i, [c_f] * 3 + [c_i] * 4 + [ctypes.c_float, c_f, c_s]),
    "plnerf_embed_rows": (c_i, [c_f] * 3 + [c_i] * 5 + [ctypes.c_float, ctypes.POINTER(ctypes.c_float), ctypes.c_float,
                                c_f, c_s]),
    "plnerf_gemm_f32": (c_i, [c_f, ctypes.c_int64, ctypes.c_int64, c_f, ctypes.c_int64, ctypes.c_int64, c_f, c_f] + [c_i] * 6 +
                        [c_f, ctypes.c_int64, c_i, c_f, c_s]),
    "plnerf_mlp_packed_bytes": (ctypes.c_size_t, [c_i]),
    "plnerf_mlp_pack_weights": (c_i, [ctypes.POINTER(ctypes.c_void_p), c_i, c_i, c_i, c_f, c_s]),
    "plnerf_mlp_input_grad": (c_i, [ctypes.POINTER(ctypes.c_void_p), c_i, c_i, c_i, c_i, c_f, c_f, c_s]),
    "plnerf_mlp_saved_bytes": (ctypes.c_size_t, [c_i, c_i]),
    "plnerf_mlp_bwd_workspace_bytes": (ctypes.c_size_t, [c_i, c_i]),
    "plnerf_mlp_fwd": (c_i, [c_f, c_i, c_f, c_f, c_f, c_i, c_i, c_i, c_i, ctypes.c_float, ctypes.c_float, c_f, c_f, c_i, c_s]),
    "plnerf_mlp_bwd": (c_i, [c_f, c_i, c_f, c_f, c_i, c_i, c_i, c_i, c_f, c_i, c_f, ctypes.c_float, c_f,
                             ctypes.POINTER(ctypes.c_void_p), c_f, c_s]),
    "plnerf_mlp_bwd_multi": (c_i, [c_i, ctypes.POINTER(ctypes.c_void_p), c_i, ctypes.POINTER(ctypes.c_void_p),
                                   ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int), c_i, c_i,
                                   ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int),
                                   ctypes.POINTER(ctypes.c_void_p), ctypes.c_float, ctypes.POINTER(ctypes.c_void_p),
                                   ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), c_s]),
    "plnerf_mlp_saved_layout": (c_i, [c_i, c_i, c_i]),
    "plnerf_adam_step": (c_i, [c_f, c_f, c_f, c_f, ctypes.c_int64] + [ctypes.c_float] * 4 + [c_i, ctypes.c_float, ctypes.c_float,
                                c_f, c_f, c_f, c_s]),
    "plnerf_mlp_status_offset": (ctypes.c_size_t, [c_i]),
}

# ... and include/plnerf_hip_batching.h (ABI 601): the use_batching ray source
BATCHING_SIGNATURES = {
    "plnerf_select_bank_rays": (c_i, [c_i, c_f, c_i, c_i] + [ctypes.c_float] * 4 + [c_f, c_f, ctypes.c_uint64, ctypes.c_uint32,
                                c_i, c_i, ctypes.c_float, ctypes.c_float] + [c_f] * 7 + [c_s]),
}

# ... and include/plnerf_hip_eval.h (ABI 601): held-out view metrics
EVAL_SIGNATURES = {
    "plnerf_eval_metrics": (c_i, [c_i] * 3 + [c_f] * 8 + [c_s]),
}
EVAL_ROW = 5                               # PLNERF_EVAL_ROW: fp64 values per frame, columns PLNERF_EVAL_*
EVAL_SSE_RGB, EVAL_SSE_RGB0, EVAL_SSIM, EVAL_DEPTH_SSE, EVAL_DEPTH_COUNT = range(EVAL_ROW)
EVAL_TILE_H, EVAL_TILE_W = 32, 64          # PLNERF_EVAL_TILE_H / _W


def eval_workspace_bytes(n, H, W):
    """PLNERF_EVAL_WORKSPACE_BYTES(n, H, W)."""
    return n * -(-H // EVAL_TILE_H) * -(-W // EVAL_TILE_W) * EVAL_ROW * 8

# ... and include/plnerf_hip_depthfeed.h (ABI 601): the depth-supervised loop's data feed and depth scale / shift gradient
DEPTHFEED_SIGNATURES = {
    "plnerf_select_depth_rays": (c_i, [c_i] * 5 + [c_f] * 4 + [c_i] + [c_f] * 3 + [ctypes.c_float] * 2 +
                                 [ctypes.c_uint64, ctypes.c_uint32, c_i, c_i] + [c_f] * 10 + [c_s]),
    "plnerf_depth_scale_shift_grad": (c_i, [c_f] * 4 + [c_i] * 5 + [c_f] + [ctypes.c_float] * 2 + [c_i] * 2 + [c_f] * 3 +
                                      [c_s]),
}
DEPTH_SS_WORKSPACE_BYTES = 4096        # PLNERF_DEPTH_SS_WORKSPACE_BYTES

# ... and include/plnerf_hip_sampleerr.h (ABI 601): the importance-sampling error of the depth script's evaluation
SAMPLEERR_SIGNATURES = {
    "plnerf_sample_error_workspace_bytes": (ctypes.c_size_t, [c_i]),
    "plnerf_sample_error": (c_i, [c_i, c_i] + [c_f] * 3 + [c_i, c_f, c_f, c_s]),
}
SAMPLEERR_ROW = 2                          # PLNERF_SAMPLEERR_ROW: fp64 values per row, columns PLNERF_SAMPLEERR_*
SAMPLEERR_SUM, SAMPLEERR_COUNT = range(SAMPLEERR_ROW)
SAMPLEERR_RAYS_PER_GROUP = 64              # PLNERF_SAMPLEERR_RAYS_PER_GROUP
SAMPLEERR_MAX_N = 1024                     # PLNERF_SAMPLEERR_MAX_N


def sample_error_workspace_bytes(R):
    """plnerf_sample_error_workspace_bytes(R), restated: one partial row per group of rays."""
    return -(-R // SAMPLEERR_RAYS_PER_GROUP) * SAMPLEERR_ROW * 8 if R > 0 else 0


# ... and include/plnerf_hip_constepi.h (ABI 601): piecewise-constant mode's coarse epilogue and final stage, one launch each
CONSTEPI_SIGNATURES = {
    "plnerf_coarse_epilogue_const": (c_i, [c_f] * 8 + [c_i, ctypes.c_uint64, ctypes.c_uint32] + [c_i] * 5 + [c_f] * 8 + [c_s]),
    "plnerf_fine_epilogue_const": (c_i, [c_f] * 7 + [c_i, ctypes.c_uint64, ctypes.c_uint32] + [c_i] * 5 + [c_f] * 10 + [c_s]),
}

# ... and include/plnerf_hip_step.h (ABI 601): one call = one optimisation step.  The three structs live in host memory;
# every pointer field is a device pointer (c_void_p: assign `tensor.data_ptr()`).
STEP_RAYS_VIEW, STEP_RAYS_BANK = 0, 1      # PLNERF_STEP_RAYS_*


class StepConfig(ctypes.Structure):
    """plnerf_step_config."""
    _fields_ = [("max_rays", c_i), ("n_samples", c_i), ("n_importance", c_i), ("mode", c_i), ("color_mode", c_i),
                ("lindisp", c_i), ("perturb", c_i), ("white_bkgd", c_i), ("farcolorfix", c_i),
                ("raw_noise_std", ctypes.c_float), ("zero_tol", ctypes.c_float), ("epsilon", ctypes.c_float), ("ndc", c_i),
                ("ndc_focal", ctypes.c_double), ("H", c_i), ("W", c_i), ("fx", ctypes.c_float), ("fy", ctypes.c_float),
                ("cx", ctypes.c_float), ("cy", ctypes.c_float), ("near", ctypes.c_float), ("far", ctypes.c_float),
                ("precision", c_i), ("fwd_kernel", c_i), ("input_ch", c_i), ("input_ch_views", c_i), ("ray_source", c_i),
                ("n_views", c_i), ("beta1", ctypes.c_float), ("beta2", ctypes.c_float), ("adam_eps", ctypes.c_float),
                ("seed", ctypes.c_uint64), ("bank_seed", ctypes.c_uint64)]


class StepNet(ctypes.Structure):
    """plnerf_step_net."""
    _fields_ = [("params", ctypes.c_void_p * N_PARAM_TENSORS), ("param_flat", c_f), ("grad_flat", c_f), ("exp_avg", c_f),
                ("exp_avg_sq", c_f), ("n_params", ctypes.c_int64), ("packed", c_f), ("skip_if_set", c_f),
                ("skip_if_set2", c_f), ("withheld", c_f)]


class StepIo(ctypes.Structure):
    """plnerf_step_io."""
    _fields_ = [("coarse", StepNet), ("fine", StepNet), ("t_vals", c_f), ("u_vals", c_f), ("views", c_f), ("poses", c_f),
                ("images", c_f), ("loss4", c_f)]


class StepArgs(ctypes.Structure):
    """plnerf_step_args."""
    _fields_ = [("rays", c_i), ("step", ctypes.c_uint32), ("ray_id0", c_i), ("c2w", ctypes.c_float * 12), ("image", c_f),
                ("crop_r0", c_i), ("crop_c0", c_i), ("crop_rows", c_i), ("crop_cols", c_i), ("epoch", ctypes.c_uint32),
                ("pos0", c_i), ("lr_fine", ctypes.c_float), ("lr_coarse", ctypes.c_float), ("adam_step_fine", c_i),
                ("adam_step_coarse", c_i), ("loss_scale", ctypes.c_float)]


STEP_STRUCTS = {"plnerf_step_config": StepConfig, "plnerf_step_net": StepNet, "plnerf_step_io": StepIo,
                "plnerf_step_args": StepArgs}
STEP_SIGNATURES = {
    "plnerf_train_step_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(StepConfig)]),
    "plnerf_train_step": (c_i, [ctypes.POINTER(StepConfig), ctypes.POINTER(StepIo), ctypes.POINTER(StepArgs), c_f,
                                ctypes.c_size_t, c_s]),
}
STEP_WORKSPACE_ALIGN = 256                 # the workspace's alignment (include/plnerf_hip_step.h)

# ... and include/plnerf_hip_depthstep.h (ABI 601): one call = one step of the depth-supervised loop, under the same
# conventions (host structs, device pointers as c_void_p)
c_fl = ctypes.c_float


class DepthStepConfig(ctypes.Structure):
    """plnerf_depth_step_config."""
    _fields_ = [("max_rays", c_i), ("n_samples", c_i), ("n_importance", c_i), ("color_mode", c_i), ("lindisp", c_i),
                ("perturb", c_i), ("white_bkgd", c_i), ("raw_noise_std", c_fl), ("zero_tol", c_fl), ("epsilon", c_fl),
                ("n_views", c_i), ("H", c_i), ("W", c_i), ("n_hyp", c_i), ("pose_rows", c_i), ("near", c_fl), ("far", c_fl),
                ("precision", c_i), ("fwd_kernel", c_i), ("input_ch", c_i), ("input_ch_views", c_i), ("input_scale", c_fl),
                ("density_beta", c_fl), ("is_joint", c_i), ("space_carving_weight", c_fl), ("space_carving_threshold", c_fl),
                ("clip_value", c_fl), ("beta1", c_fl), ("beta2", c_fl), ("adam_eps", c_fl), ("ss_beta1", c_fl),
                ("ss_beta2", c_fl), ("ss_adam_eps", c_fl), ("seed", ctypes.c_uint64)]


class DepthStepIo(ctypes.Structure):
    """plnerf_depth_step_io."""
    _fields_ = [("coarse", StepNet), ("fine", StepNet), ("t_vals", c_f), ("u_vals", c_f), ("images", c_f), ("hyp", c_f),
                ("valid", c_f), ("poses", c_f), ("intrinsics", c_f), ("scale", c_f), ("shift", c_f), ("ss_grad", c_f),
                ("ss_exp_avg", c_f), ("ss_exp_avg_sq", c_f), ("loss5", c_f)]


class DepthStepArgs(ctypes.Structure):
    """plnerf_depth_step_args."""
    _fields_ = [("view", c_i), ("rays", c_i), ("step", ctypes.c_uint32), ("ray_id0", c_i), ("lr", c_fl), ("adam_step", c_i),
                ("carve", c_i), ("ss_step", c_i), ("ss_lr", c_fl), ("ss_adam_step", c_i)]


DEPTH_STEP_MAX_SAMPLES = 1022              # n_samples + n_importance of plnerf_depth_train_step (PLNERF_MAX_SAMPLES)
DEPTH_STEP_VIEWS = ("rgb", "rgb0", "depth", "depth0", "acc", "acc0", "disp", "disp0", "z_std", "pred_hyp", "z_vals", "z_vals0",
                    "pixels", "target_h", "mask")


class DepthStepViews(ctypes.Structure):
    """plnerf_depth_step_views: byte offsets inside the workspace."""
    _fields_ = [(name, ctypes.c_size_t) for name in DEPTH_STEP_VIEWS]


DEPTHSTEP_STRUCTS = {"plnerf_depth_step_config": DepthStepConfig, "plnerf_depth_step_io": DepthStepIo,
                     "plnerf_depth_step_args": DepthStepArgs, "plnerf_depth_step_views": DepthStepViews}
DEPTHSTEP_SIGNATURES = {
    "plnerf_depth_train_step_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(DepthStepConfig)]),
    "plnerf_depth_train_step_layout": (c_i, [ctypes.POINTER(DepthStepConfig), ctypes.POINTER(DepthStepViews)]),
    "plnerf_depth_train_step": (c_i, [ctypes.POINTER(DepthStepConfig), ctypes.POINTER(DepthStepIo),
                                      ctypes.POINTER(DepthStepArgs), c_f, ctypes.c_size_t, c_s]),
    "plnerf_depth_ss_adam": (c_i, [c_f] * 5 + [c_i] + [c_fl] * 4 + [c_i, c_fl, c_s]),
}

# ... and include/plnerf_hip_conststep.h (ABI 601): piecewise-constant mode's one-call steps, on the structs above, and the
# one-launch backward of plnerf_fine_epilogue_const they need
CONSTSTEP_SIGNATURES = {
    "plnerf_fine_epilogue_const_bwd": (c_i, [c_f] * 9 + [c_i, c_f] + [c_i] * 4 + [c_f] * 7 + [c_s]),
    "plnerf_train_step_const_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(StepConfig)]),
    "plnerf_train_step_const": (c_i, [ctypes.POINTER(StepConfig), ctypes.POINTER(StepIo), ctypes.POINTER(StepArgs), c_f,
                                      ctypes.c_size_t, c_s]),
    "plnerf_depth_train_step_const_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(DepthStepConfig)]),
    "plnerf_depth_train_step_const_layout": (c_i, [ctypes.POINTER(DepthStepConfig), ctypes.POINTER(DepthStepViews)]),
    "plnerf_depth_train_step_const": (c_i, [ctypes.POINTER(DepthStepConfig), ctypes.POINTER(DepthStepIo),
                                            ctypes.POINTER(DepthStepArgs), c_f, ctypes.c_size_t, c_s]),
}

# ... and include/plnerf_hip_view.h (ABI 601): one call = one rendered view (on plnerf_step_config), the rays of a view's
# consecutive pixels and the 8 / 16-bit export of a frame's planes


class ViewNet(ctypes.Structure):
    """plnerf_view_net."""
    _fields_ = [("params", ctypes.c_void_p * N_PARAM_TENSORS), ("packed", c_f)]


VIEW_PLANES = ("rgb", "disp", "acc", "depth", "rgb0", "disp0", "acc0", "depth0", "z_std")      # fp32 frame planes of plnerf_view_io


class ViewIo(ctypes.Structure):
    """plnerf_view_io."""
    _fields_ = [("coarse", ViewNet), ("fine", ViewNet), ("t_vals", c_f), ("u_vals", c_f)] + \
               [(name, c_f) for name in VIEW_PLANES] + [("rgb8", c_f), ("depth16", c_f)]


class ViewArgs(ctypes.Structure):
    """plnerf_view_args."""
    _fields_ = [("c2w", ctypes.c_float * 12), ("step", ctypes.c_uint32), ("pix0", c_i), ("n_pix", c_i), ("pack_weights", c_i),
                ("depth16_scale", c_fl)]


VIEW_STRUCTS = {"plnerf_view_net": ViewNet, "plnerf_view_io": ViewIo, "plnerf_view_args": ViewArgs}
VIEW_SIGNATURES = {
    "plnerf_view_rays": (c_i, [c_i, c_i] + [c_fl] * 4 + [ctypes.POINTER(ctypes.c_float), c_i, c_i, c_fl, c_fl] + [c_f] * 5 + [c_s]),
    "plnerf_frame_export": (c_i, [c_f, c_f, c_f, c_fl, c_f, c_i, c_s]),
    "plnerf_render_view_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(StepConfig)]),
    "plnerf_render_view": (c_i, [ctypes.POINTER(StepConfig), ctypes.POINTER(ViewIo), ctypes.POINTER(ViewArgs), c_f,
                                 ctypes.c_size_t, c_s]),
}

# Every header of the C ABI, in binding order: (file under include/, its signatures, its struct mirrors).  A new header is
# one row here; tests/test_abi_headers.py compares each row with its header and with the library.
HEADERS = (
    ("plnerf_hip.h", SIGNATURES, {}),
    ("plnerf_hip_batching.h", BATCHING_SIGNATURES, {}),
    ("plnerf_hip_eval.h", EVAL_SIGNATURES, {}),
    ("plnerf_hip_depthfeed.h", DEPTHFEED_SIGNATURES, {}),
    ("plnerf_hip_sampleerr.h", SAMPLEERR_SIGNATURES, {}),
    ("plnerf_hip_constepi.h", CONSTEPI_SIGNATURES, {}),
    ("plnerf_hip_step.h", STEP_SIGNATURES, STEP_STRUCTS),
    ("plnerf_hip_depthstep.h", DEPTHSTEP_SIGNATURES, DEPTHSTEP_STRUCTS),
    ("plnerf_hip_conststep.h", CONSTSTEP_SIGNATURES, {}),
    ("plnerf_hip_view.h", VIEW_SIGNATURES, VIEW_STRUCTS),
)


def _merge(headers):
    """name -> (restype, argtypes) over every header; a name declared twice would be bound twice, the later list winning."""
    merged, owner = {}, {}
    for header, signatures, _ in headers:
        for name, signature in signatures.items():
            if name in merged:
                raise ValueError(f"{name} is declared by both {owner[name]} and {header}: one entry point, one header")
            merged[name], owner[name] = signature, header
    return merged


ALL_SIGNATURES = _merge(HEADERS)      # every entry point of the registered ABI

# ---- experimental headers (include/experimental/): entry points the library exports and lib() binds, OUTSIDE the registered
# ABI above -- their signatures and structs may still change without a PLNERF_VERSION step.  Same row shape as HEADERS; the
# header's own tests hold a row to the checks the registry gives the others.  Promoting a header moves its file up to
# include/ and its row into HEADERS.

# include/experimental/plnerf_hip_depthview.h: one call = one rendered view of the depth-supervised variant


class DepthViewConfig(ctypes.Structure):
    """plnerf_depth_view_config."""
    _fields_ = [("max_rays", c_i), ("n_samples", c_i), ("n_importance", c_i), ("mode", c_i), ("color_mode", c_i),
                ("lindisp", c_i), ("perturb", c_i), ("white_bkgd", c_i), ("raw_noise_std", c_fl), ("zero_tol", c_fl),
                ("epsilon", c_fl), ("H", c_i), ("W", c_i), ("near", c_fl), ("far", c_fl), ("precision", c_i), ("fwd_kernel", c_i),
                ("input_ch", c_i), ("input_ch_views", c_i), ("input_scale", c_fl), ("density_beta", c_fl),
                ("seed", ctypes.c_uint64)]


class DepthViewIo(ctypes.Structure):
    """plnerf_depth_view_io."""
    _fields_ = [("coarse", ViewNet), ("fine", ViewNet), ("t_vals", c_f), ("u_vals", c_f)] + \
               [(name, c_f) for name in VIEW_PLANES] + \
               [("pred_hyp", c_f), ("valid", c_f), ("error_row", c_f), ("rgb8", c_f), ("depth16", c_f), ("depth_mm16", c_f)]


class DepthViewArgs(ctypes.Structure):
    """plnerf_depth_view_args."""
    _fields_ = [("c2w", ctypes.c_float * 12), ("fx", c_fl), ("fy", c_fl), ("cx", c_fl), ("cy", c_fl), ("step", ctypes.c_uint32),
                ("pix0", c_i), ("n_pix", c_i), ("pack_weights", c_i), ("depth16_scale", c_fl), ("depth_mm_mult", c_fl)]


DEPTHVIEW_STRUCTS = {"plnerf_depth_view_config": DepthViewConfig, "plnerf_depth_view_io": DepthViewIo,
                     "plnerf_depth_view_args": DepthViewArgs}
DEPTHVIEW_SIGNATURES = {
    "plnerf_depth_view_rays": (c_i, [c_i, c_i] + [c_fl] * 4 + [ctypes.POINTER(ctypes.c_float), c_i, c_i, c_fl, c_fl] + [c_f] * 5 +
                               [c_s]),
    "plnerf_frame_export_u16": (c_i, [c_f, c_fl, c_f, c_i, c_s]),
    "plnerf_depth_render_view_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(DepthViewConfig)]),
    "plnerf_depth_render_view": (c_i, [ctypes.POINTER(DepthViewConfig), ctypes.POINTER(DepthViewIo),
                                       ctypes.POINTER(DepthViewArgs), c_f, ctypes.c_size_t, c_s]),
}

EXPERIMENTAL_HEADERS = (
    ("experimental/plnerf_hip_depthview.h", DEPTHVIEW_SIGNATURES, DEPTHVIEW_STRUCTS),
)
EXPERIMENTAL_SIGNATURES = _merge(EXPERIMENTAL_HEADERS)


def _disjoint(experimental, registered):
    """An experimental entry that the registered ABI also declares would be bound twice, the later list winning."""
    for name in experimental:
        if name in registered:
            raise ValueError(f"{name} is declared by an experimental header and by the registered ABI: one entry point, "
                             "one header")


_disjoint(EXPERIMENTAL_SIGNATURES, ALL_SIGNATURES)

# ---- a third table, same row shape, for include/experimental/plnerf_hip_camcode.h: the test-time optimisation of a view's
# camera code (plnerf_amd.camcode).  Experimental like the table above (no PLNERF_VERSION step) and kept apart from it: each
# of the two existing tables is pinned row by row by its own tests, so a header that neither of them lists gets its own.
CAMCODE_MAX_WIDTH, CAMCODE_MAX_CAM, CAMCODE_MAX_ROWS, CAMCODE_MAX_GROUPS = 128, 32, 1024, 2048      # PLNERF_CAMCODE_MAX_*


class CamcodeState(ctypes.Structure):
    """plnerf_camcode_state (device memory: filled on the host, uploaded once)."""
    _fields_ = [("cam", c_fl * 32), ("exp_avg", c_fl * 32), ("exp_avg_sq", c_fl * 32), ("best_cam", c_fl * 32), ("lr", c_fl),
                ("best", c_fl), ("max_psnr", c_fl), ("step", c_i), ("num_bad_epochs", c_i), ("best_iter", c_i)]


CAMCODE_STRUCTS = {"plnerf_camcode_state": CamcodeState}
CAMCODE_SIGNATURES = {
    "plnerf_camcode_sweep_workspace_bytes": (ctypes.c_size_t, [c_i]),
    "plnerf_camcode_sweep": (c_i, [c_f, c_f, c_i, c_i, c_i, c_f, c_i, c_f, c_i] + [c_f] * 6 + [ctypes.c_size_t, c_f, c_f, c_s]),
    # (the state lives in DEVICE memory: a device pointer like every other, not a ctypes pointer the host could follow)
    "plnerf_camcode_update": (c_i, [c_f, c_i, c_f, c_f, c_i] + [c_fl] * 4 + [c_i, c_f, c_f, c_i, c_s]),
}
CAMCODE_HEADERS = (
    ("experimental/plnerf_hip_camcode.h", CAMCODE_SIGNATURES, CAMCODE_STRUCTS),
)
CAMCODE_TABLE_SIGNATURES = _merge(CAMCODE_HEADERS)
_disjoint(CAMCODE_TABLE_SIGNATURES, ALL_SIGNATURES)
_disjoint(CAMCODE_TABLE_SIGNATURES, EXPERIMENTAL_SIGNATURES)

# ---- a fourth table, for include/experimental/plnerf_hip_dpstep.h: the one-call training steps cut in two at the gradient
# exchange of a data-parallel run (stepplan's run_grads / apply).  Experimental, and apart from the three tables above for the
# reason the third is apart from the first two.  The structs are the registered steps' (no mirrors of its own); the workspace
# is theirs too, so there is no size query.
_STEP_GRADS = (c_i, [ctypes.POINTER(StepConfig), ctypes.POINTER(StepIo), ctypes.POINTER(StepArgs), c_f, ctypes.c_size_t, c_s])
_DEPTH_STEP_GRADS = (c_i, [ctypes.POINTER(DepthStepConfig), ctypes.POINTER(DepthStepIo), ctypes.POINTER(DepthStepArgs), c_f,
                           ctypes.c_size_t, c_s])
DPSTEP_SIGNATURES = {
    "plnerf_train_step_grads": _STEP_GRADS,
    "plnerf_train_step_const_grads": _STEP_GRADS,
    "plnerf_train_step_apply": (c_i, [ctypes.POINTER(StepConfig), ctypes.POINTER(StepIo), ctypes.POINTER(StepArgs), c_fl, c_s]),
    "plnerf_depth_train_step_grads": _DEPTH_STEP_GRADS,
    "plnerf_depth_train_step_const_grads": _DEPTH_STEP_GRADS,
    "plnerf_depth_train_step_apply": (c_i, [ctypes.POINTER(DepthStepConfig), ctypes.POINTER(DepthStepIo),
                                            ctypes.POINTER(DepthStepArgs), c_fl, c_s]),
}
DPSTEP_HEADERS = (
    ("experimental/plnerf_hip_dpstep.h", DPSTEP_SIGNATURES, {}),
)
DPSTEP_TABLE_SIGNATURES = _merge(DPSTEP_HEADERS)
_disjoint(DPSTEP_TABLE_SIGNATURES, ALL_SIGNATURES)
_disjoint(DPSTEP_TABLE_SIGNATURES, EXPERIMENTAL_SIGNATURES)
_disjoint(DPSTEP_TABLE_SIGNATURES, CAMCODE_TABLE_SIGNATURES)

# ---- a fifth table, for include/experimental/plnerf_hip_gemm16.h: one layer of the layer-by-layer route (generic.py) in the
# 16-bit modes' arithmetic.  Experimental, and apart from the four tables above for the reason the third is apart from the
# first two.
GEMM16_SIGNATURES = {
    "plnerf_gemm_h16": (c_i, [c_f, ctypes.c_int64, c_f, ctypes.c_int64, c_f] + [c_i] * 5 + [c_f, ctypes.c_int64, c_f, c_s]),
}
GEMM16_HEADERS = (
    ("experimental/plnerf_hip_gemm16.h", GEMM16_SIGNATURES, {}),
)
GEMM16_TABLE_SIGNATURES = _merge(GEMM16_HEADERS)
_disjoint(GEMM16_TABLE_SIGNATURES, ALL_SIGNATURES)
_disjoint(GEMM16_TABLE_SIGNATURES, EXPERIMENTAL_SIGNATURES)
_disjoint(GEMM16_TABLE_SIGNATURES, CAMCODE_TABLE_SIGNATURES)
_disjoint(GEMM16_TABLE_SIGNATURES, DPSTEP_TABLE_SIGNATURES)

# ---- a sixth table, for include/experimental/plnerf_hip_gemm16_bwd.h: the two backward products of such a layer (dgrad,
# wgrad) in the same arithmetic.  Experimental, and a table of its own because the fifth is pinned to its one entry.
_c_i64 = ctypes.c_int64
GEMM16_BWD_SIGNATURES = {
    "plnerf_gemm_h16_dgrad": (c_i, [c_f, _c_i64, c_f, _c_i64, c_f, _c_i64] + [c_i] * 4 + [c_f, c_f, _c_i64, c_f, c_s]),
    "plnerf_gemm_h16_wgrad": (c_i, [c_f, _c_i64, c_f, _c_i64, c_f, _c_i64] + [c_i] * 4 + [c_f, c_f, _c_i64, c_i, c_f, c_f, c_s]),
}
GEMM16_BWD_HEADERS = (
    ("experimental/plnerf_hip_gemm16_bwd.h", GEMM16_BWD_SIGNATURES, {}),
)
GEMM16_BWD_TABLE_SIGNATURES = _merge(GEMM16_BWD_HEADERS)
for _table in (ALL_SIGNATURES, EXPERIMENTAL_SIGNATURES, CAMCODE_TABLE_SIGNATURES, DPSTEP_TABLE_SIGNATURES, GEMM16_TABLE_SIGNATURES):
    _disjoint(GEMM16_BWD_TABLE_SIGNATURES, _table)

# ---- a seventh table, for include/experimental/plnerf_hip_generic.h: the layer-by-layer route's whole no-grad forward in one
# call, on 16-bit activation planes (generic.CHAIN_INFERENCE), and the pack of fp32 rows into such planes.  Experimental, and a
# table of its own because the fifth and sixth are pinned to their entries.
GENERIC_MAX_SKIPS = 16                     # PLNERF_GENERIC_MAX_SKIPS
GENERIC_WORKSPACE_ALIGN = 16               # PLNERF_GENERIC_WORKSPACE_ALIGN


class GenericShape(ctypes.Structure):
    """plnerf_generic_shape."""
    _fields_ = [("D", c_i), ("W", c_i), ("input_ch", c_i), ("view_ch", c_i), ("use_viewdirs", c_i), ("output_ch", c_i),
                ("n_view_layers", c_i), ("n_skips", c_i), ("skips", c_i * GENERIC_MAX_SKIPS)]


def pack_ld(K):
    """PLNERF_PACK_LD(K): elements per row of a packed plane."""
    return -(-K // 8) * 8


GENERIC_FWD_STRUCTS = {"plnerf_generic_shape": GenericShape}
GENERIC_FWD_SIGNATURES = {
    "plnerf_pack_h16": (c_i, [c_f, _c_i64, c_i, c_i, c_i, c_f, c_f, c_i, c_s]),
    "plnerf_generic_fwd_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(GenericShape), c_i, c_i]),
    "plnerf_generic_fwd": (c_i, [ctypes.POINTER(GenericShape), ctypes.POINTER(ctypes.c_void_p), c_f, _c_i64, c_i, c_i, c_f,
                                 ctypes.c_size_t, c_f, _c_i64, c_f, c_s]),
}
GENERIC_FWD_HEADERS = (
    ("experimental/plnerf_hip_generic.h", GENERIC_FWD_SIGNATURES, GENERIC_FWD_STRUCTS),
)
GENERIC_FWD_TABLE_SIGNATURES = _merge(GENERIC_FWD_HEADERS)
for _table in (ALL_SIGNATURES, EXPERIMENTAL_SIGNATURES, CAMCODE_TABLE_SIGNATURES, DPSTEP_TABLE_SIGNATURES, GEMM16_TABLE_SIGNATURES,
               GEMM16_BWD_TABLE_SIGNATURES):
    _disjoint(GENERIC_FWD_TABLE_SIGNATURES, _table)

# ---- an eighth table, for include/experimental/plnerf_hip_generic_train.h: the layer-by-layer route's TRAINING forward and
# backward as one call each (generic.CHAIN_TRAINING).  Experimental, and a table of its own because the seventh is pinned to
# its entries; the struct is the seventh's (no mirror of its own).
GENERIC_TRAIN_SIGNATURES = {
    "plnerf_generic_train_saved_bytes": (ctypes.c_size_t, [ctypes.POINTER(GenericShape), c_i, c_i]),
    "plnerf_generic_train_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(GenericShape), c_i, c_i]),
    "plnerf_generic_train_wgrad_splits": (c_i, [c_i, c_i, c_i]),
    "plnerf_generic_train_fwd": (c_i, [ctypes.POINTER(GenericShape), ctypes.POINTER(ctypes.c_void_p), c_f, _c_i64, c_i, c_i, c_f,
                                       ctypes.c_size_t, c_f, _c_i64, c_f, c_s]),
    "plnerf_generic_train_bwd": (c_i, [ctypes.POINTER(GenericShape), c_f, _c_i64, c_i, c_i, c_f, ctypes.c_size_t, c_f, _c_i64,
                                       ctypes.POINTER(ctypes.c_void_p), c_f, ctypes.c_size_t, c_f, c_s]),
}
GENERIC_TRAIN_HEADERS = (
    ("experimental/plnerf_hip_generic_train.h", GENERIC_TRAIN_SIGNATURES, {}),
)
GENERIC_TRAIN_TABLE_SIGNATURES = _merge(GENERIC_TRAIN_HEADERS)
for _table in (ALL_SIGNATURES, EXPERIMENTAL_SIGNATURES, CAMCODE_TABLE_SIGNATURES, DPSTEP_TABLE_SIGNATURES, GEMM16_TABLE_SIGNATURES,
               GEMM16_BWD_TABLE_SIGNATURES, GENERIC_FWD_TABLE_SIGNATURES):
    _disjoint(GENERIC_TRAIN_TABLE_SIGNATURES, _table)

# ---- a ninth table, for include/experimental/plnerf_hip_anyview.h: one call = one rendered view for any pair of networks
# create_nerf builds, each slot on the compiled trunk or outside it (plnerf_amd.anyview), and the layer-by-layer route's fp32
# forward as one call.  Experimental, and a table of its own because the other eight are pinned to their entries.
ANYVIEW_FUSED, ANYVIEW_CHAIN16, ANYVIEW_LAYERS32 = 0, 1, 2      # PLNERF_ANYVIEW_*: a network slot's route


class AnyViewNet(ctypes.Structure):
    """plnerf_anyview_net."""
    _fields_ = [("route", c_i), ("fused", ViewNet), ("shape", GenericShape), ("params", c_f), ("precision", c_i), ("status", c_f)]


class AnyViewIo(ctypes.Structure):
    """plnerf_anyview_io."""
    _fields_ = [("coarse", AnyViewNet), ("fine", AnyViewNet), ("max_net_rows", c_i), ("t_vals", c_f), ("u_vals", c_f)] + \
               [(name, c_f) for name in VIEW_PLANES] + [("rgb8", c_f), ("depth16", c_f)]


ANYVIEW_STRUCTS = {"plnerf_anyview_net": AnyViewNet, "plnerf_anyview_io": AnyViewIo}
ANYVIEW_SIGNATURES = {
    "plnerf_generic_fwd_f32_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(GenericShape), c_i]),
    "plnerf_generic_fwd_f32": (c_i, [ctypes.POINTER(GenericShape), ctypes.POINTER(ctypes.c_void_p), c_f, _c_i64, c_i, c_f,
                                     ctypes.c_size_t, c_f, _c_i64, c_s]),
    "plnerf_render_view_any_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(StepConfig), ctypes.POINTER(AnyViewIo)]),
    "plnerf_render_view_any": (c_i, [ctypes.POINTER(StepConfig), ctypes.POINTER(AnyViewIo), ctypes.POINTER(ViewArgs), c_f,
                                     ctypes.c_size_t, c_s]),
}
ANYVIEW_HEADERS = (
    ("experimental/plnerf_hip_anyview.h", ANYVIEW_SIGNATURES, ANYVIEW_STRUCTS),
)
ANYVIEW_TABLE_SIGNATURES = _merge(ANYVIEW_HEADERS)
for _table in (ALL_SIGNATURES, EXPERIMENTAL_SIGNATURES, CAMCODE_TABLE_SIGNATURES, DPSTEP_TABLE_SIGNATURES, GEMM16_TABLE_SIGNATURES,
               GEMM16_BWD_TABLE_SIGNATURES, GENERIC_FWD_TABLE_SIGNATURES, GENERIC_TRAIN_TABLE_SIGNATURES):
    _disjoint(ANYVIEW_TABLE_SIGNATURES, _table)

# ---- a tenth table, for include/experimental/plnerf_hip_unique.h: the fine pass's MLP forward over the rows it needs (runs of
# bit-identical rows are evaluated at their two ends), the fold of the upstream gradient onto those rows, the workspace's layout
# and the host-side predicate.  Experimental, and a table of its own because the other nine are pinned to their entries.


class UniqueLayout(ctypes.Structure):
    """plnerf_unique_layout: byte offsets inside the workspace (n_absmax: a count)."""
    _fields_ = [(name, ctypes.c_size_t) for name in ("words", "rows_u", "src", "pts_u", "dirs_u", "raw_u", "g_raw_u", "absmax",
                                                     "n_absmax", "total")]


UNIQUE_STRUCTS = {"plnerf_unique_layout": UniqueLayout}
UNIQUE_SIGNATURES = {
    "plnerf_mlp_unique_workspace_bytes": (ctypes.c_size_t, [c_i]),
    "plnerf_mlp_unique_layout": (c_i, [c_i, ctypes.POINTER(UniqueLayout)]),
    "plnerf_mlp_fwd_unique_served": (c_i, [c_i] * 6),
    "plnerf_mlp_fwd_unique": (c_i, [c_f, c_i, c_f, c_f, c_i, c_i, c_i, c_i, c_fl, c_fl, c_f, c_f, c_i, c_f, c_s]),
    "plnerf_mlp_unique_fold": (c_i, [c_f, c_i, c_f, c_s]),
}
UNIQUE_HEADERS = (
    ("experimental/plnerf_hip_unique.h", UNIQUE_SIGNATURES, UNIQUE_STRUCTS),
)
UNIQUE_TABLE_SIGNATURES = _merge(UNIQUE_HEADERS)
for _table in (ALL_SIGNATURES, EXPERIMENTAL_SIGNATURES, CAMCODE_TABLE_SIGNATURES, DPSTEP_TABLE_SIGNATURES, GEMM16_TABLE_SIGNATURES,
               GEMM16_BWD_TABLE_SIGNATURES, GENERIC_FWD_TABLE_SIGNATURES, GENERIC_TRAIN_TABLE_SIGNATURES, ANYVIEW_TABLE_SIGNATURES):
    _disjoint(UNIQUE_TABLE_SIGNATURES, _table)

# ---- an eleventh table, for include/experimental/plnerf_hip_mesh.h: mesh extraction (plnerf_amd.mesh) -- one network's density on
# a lattice in one call (on the ninth table's slot struct) and indexed marching cubes of a device field.  Experimental, and a
# table of its own because the other ten are pinned to their entries.
GRID_STATS = 4                             # PLNERF_GRID_STATS: fp64 values of a stats row, columns PLNERF_GRID_*
GRID_MIN, GRID_MAX, GRID_SUM, GRID_SUMSQ = range(GRID_STATS)
MC_MAX_POINTS = 1 << 30                    # lattice points of either entry
MC_COUNT_SATURATED = 0xFFFFFFFF            # a count of plnerf_mc_count that does not fit its word
MESH_SIGNATURES = {
    "plnerf_density_grid_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(AnyViewNet)] + [c_i] * 5),
    "plnerf_density_grid": (c_i, [ctypes.POINTER(AnyViewNet)] + [c_i] * 4 + [c_f] * 3 + [c_i, c_i, c_f, c_f, c_f, ctypes.c_size_t, c_s]),
    "plnerf_mc_workspace_bytes": (ctypes.c_size_t, [c_i] * 3),
    "plnerf_mc_count": (c_i, [c_f, c_i, c_i, c_i, ctypes.c_double, c_f, ctypes.c_size_t, c_f, c_s]),
    "plnerf_mc_emit": (c_i, [c_f, c_i, c_i, c_i, ctypes.c_double, c_f, ctypes.c_size_t, c_f, _c_i64, c_f, _c_i64, c_s]),
}
MESH_HEADERS = (
    ("experimental/plnerf_hip_mesh.h", MESH_SIGNATURES, {}),
)
MESH_TABLE_SIGNATURES = _merge(MESH_HEADERS)
for _table in (ALL_SIGNATURES, EXPERIMENTAL_SIGNATURES, CAMCODE_TABLE_SIGNATURES, DPSTEP_TABLE_SIGNATURES, GEMM16_TABLE_SIGNATURES,
               GEMM16_BWD_TABLE_SIGNATURES, GENERIC_FWD_TABLE_SIGNATURES, GENERIC_TRAIN_TABLE_SIGNATURES, ANYVIEW_TABLE_SIGNATURES,
               UNIQUE_TABLE_SIGNATURES):
    _disjoint(MESH_TABLE_SIGNATURES, _table)

_lib = None


def lib():
    """The loaded library; raises ImportError (with the build recipe) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` or "
                "`make -C pl-nerf_amd/csrc` (hipcc --offload-arch=gfx950). "
                "plnerf_amd has no CPU fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        tools_build = os.environ.get("PLNERF_ALLOW_TOOLS_BUILD") == "1"
        for name, (res, args) in {**ALL_SIGNATURES, **EXPERIMENTAL_SIGNATURES, **CAMCODE_TABLE_SIGNATURES,
                                  **DPSTEP_TABLE_SIGNATURES, **GEMM16_TABLE_SIGNATURES, **GEMM16_BWD_TABLE_SIGNATURES,
                                  **GENERIC_FWD_TABLE_SIGNATURES, **GENERIC_TRAIN_TABLE_SIGNATURES,
                                  **ANYVIEW_TABLE_SIGNATURES, **UNIQUE_TABLE_SIGNATURES, **MESH_TABLE_SIGNATURES}.items():
            fn = getattr(handle, name, None)
            if fn is None:
                if tools_build:      # (tools/ab.sh against a library of an earlier commit: entry points it lacks stay unbound)
                    continue
                raise AttributeError(f"{LIB_PATH} does not export {name}: header / library mismatch")
            fn.restype = res
            fn.argtypes = args
        # The argument lists above are positional: a library of another ABI (a stale build, a variant linked from old
        # objects) would be called with shifted pointers -- compare before the first call.  tools/ A/B legs
        # against an older library whose signatures are known to match set PLNERF_ALLOW_TOOLS_BUILD=1.
        version = handle.plnerf_version()
        if version != ABI_VERSION and not tools_build:
            raise ImportError(
                f"{LIB_PATH} reports plnerf_version() = {version}, this binding is written against {ABI_VERSION} "
                "(include/plnerf_hip.h): rebuild with `make -C pl-nerf_amd/csrc clean all`.")
        flags = handle.plnerf_build_flags()
        if flags and os.environ.get("PLNERF_ALLOW_TOOLS_BUILD") != "1":
            raise ImportError(
                f"{LIB_PATH} was built with tools-only switches (plnerf_build_flags() = {flags}: bit 2 = trace hooks; "
                "bits 0 / 1 = the timing ablations of builds before round 5).  It is not the "
                "product library: rebuild with `make -C pl-nerf_amd/csrc` (no -D switches), or set "
                "PLNERF_ALLOW_TOOLS_BUILD=1 for a measurement script under tools/.")
        _lib = handle
    return _lib


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {lib().plnerf_error_string(rc).decode()} (code {rc})")


def dptr(t, name="tensor", dtype=torch.float32):
    """Device pointer of a contiguous tensor on a HIP device (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(
            f"plnerf_amd: `{name}` is on {t.device}; the HIP path needs a GPU tensor "
            "(there is no CPU fallback)")
    if t.dtype != dtype:
        raise RuntimeError(f"plnerf_amd: `{name}` must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"plnerf_amd: `{name}` must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream():
    """The current HIP stream of the current device as the ABI's `plnerf_stream_t` (every entry point enqueues on the
    stream it is handed).  torch.cuda.current_stream() builds a Stream object through three Python layers (11 us; a
    training step makes ~11 calls); the raw getter is the same value without them."""
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr_table(tensors, name="params"):
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = dptr(t, f"{name}[{i}]").value
    return arr
