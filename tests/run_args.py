"""The argument Namespaces of the two training scripts, as the tests hand them to create_nerf, TrainStep and DepthTrainStep:
one builder per script.  Neither pytest nor torch is imported here, so the data-parallel worker programs (one process per
rank) and the host-only tests load it cheaply.  A test that needs another value, or one more field (N_rand, ckpt_dir, chunk,
dataset, ...), passes it by keyword."""
from argparse import Namespace


def nvs_args(ckpt_dir, precision=None, **over):
    """run_plnerf.py's arguments: 64 + 128 samples, linear mode, blender settings, no checkpoint reloaded.  `precision` None
    leaves the field out (the package's default arithmetic)."""
    a = dict(multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=128, N_samples=64, netdepth=8,
             netwidth=256, netdepth_fine=8, netwidth_fine=256, netchunk=65536, lrate=5e-4, coarse_lrate=5e-4,
             ft_path=None, ckpt_dir=ckpt_dir, expname="exp", no_reload=True, perturb=1.0, white_bkgd=True,
             raw_noise_std=0.0, mode="linear", color_mode="midpoint", dataset="blender", no_ndc=False, lindisp=False,
             lrate_decay=250, constant_init=0, chunk=32768)
    if precision is not None:
        a["precision"] = precision
    a.update(over)
    return Namespace(**a)


def depth_args(train=True, **over):
    """run_nerf_sample_based_depth.py's arguments: 64 + 32 samples, no camera code, f16x3.  train=False leaves out the five
    fields only the training loss reads (what the tests of the evaluation loops pass)."""
    a = dict(multires=9, i_embed=0, use_viewdirs=True, multires_views=0, input_ch_cam=0, N_importance=32, N_samples=64,
             netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, netchunk=65536, lrate=5e-4, perturb=1.0,
             white_bkgd=True, raw_noise_std=0.0, mode="linear", color_mode="midpoint", lindisp=False, no_reload=True,
             precision="f16x3", bb_center=0.0, bb_scale=1.0)
    if train:
        a.update(space_carving_weight=0.007, warm_start_nerf=0, is_joint=False, norm_p=2, space_carving_threshold=0.0)
    a.update(over)
    return Namespace(**a)


def depth_args_of(gd, precision="fp32", **over):
    """depth_args at a golden file's sampling and space-carving weight (g8_depth_variant.npz and its kin)."""
    at = dict(N_importance=int(gd["N_importance"]), N_samples=int(gd["N_samples"]),
              space_carving_weight=float(gd["space_carving_weight"]), precision=precision)
    return depth_args(**dict(at, **over))
