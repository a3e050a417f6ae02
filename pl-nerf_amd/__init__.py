"""plnerf_amd -- MI355X-native implementation of PL-NeRF's volume-rendering hot path.

Drop-in for the render operator surface of the reference's run_plnerf.py /
run_nerf_helpers.py (create_nerf, render, render_rays, raw2outputs, sample_pdf,
sample_pdf_reformulation, NeRF, get_embedder, run_network, ...).  All numerical work runs
in the hand-written gfx950 kernels of libplnerf_hip.so; there is no CPU fallback.
"""
from . import _lib
from .nerf import NeRF, Embedder, get_embedder
from .rays import get_rays, get_rays_np, ndc_rays
from .optim import FlatAdam
from .train import (RayBank, TrainStep, batch_schedule, checkpoint_path, img2mse, save_checkpoint, select_rays,
                    select_view_rays)
from .raybatch import RayColumns
from .functional import DrawSource, set_draw_source
from .evaluate import (MeanTracker, compute_rmse, image_metrics, metric_rows, render_images_with_metrics,
                       sample_error_rows, write_images_with_metrics, write_images_with_metrics_testdist)
from . import depth   # depth-supervised variant of the path (depth_supervised_exps/)
from .depth import DepthTrainStep, DepthViews
from .render import (batchify, batchify_rays, compute_weights, compute_weights_piecewise_linear, create_nerf,
                     raw2outputs, render, render_path, render_rays, run_network, sample_pdf,
                     sample_pdf_reformulation)
from .png import read_png, write_png
from .view import ViewRenderer, render_path_frames
from . import anyview     # plnerf_render_view_any: frames of any pair of networks create_nerf builds, one library call each
from .anyview import AnyViewRenderer
from . import depthview   # plnerf_depth_render_view: the depth-supervised variant's frames, one library call each
from .depthview import DepthViewRenderer, render_video_frames
from . import camcode     # test-time optimisation of a held-out view's camera code (plnerf_camcode_sweep / _update)
from .camcode import CameraCodeOptimizer, optimize_camera_embedding
from . import mesh        # mesh extraction: plnerf_density_grid (one call = extract_fields) and marching cubes on the device
from .mesh import (extract_fields, extract_geometry, extract_iso_level, keep_components, marching_cubes, read_ply, write_ply)


def library_path():
    return _lib.LIB_PATH


def library_version():
    return _lib.lib().plnerf_version()


__all__ = [
    "NeRF", "Embedder", "get_embedder", "get_rays", "get_rays_np", "ndc_rays", "batchify", "batchify_rays",
    "compute_weights", "compute_weights_piecewise_linear", "create_nerf", "raw2outputs", "render", "render_path",
    "render_rays", "run_network", "sample_pdf", "sample_pdf_reformulation", "img2mse", "library_path",
    "library_version", "depth", "FlatAdam", "TrainStep", "save_checkpoint", "checkpoint_path", "select_rays", "select_view_rays", "RayBank", "batch_schedule", "RayColumns", "DrawSource",
    "set_draw_source", "MeanTracker", "compute_rmse", "image_metrics", "metric_rows", "render_images_with_metrics",
    "sample_error_rows", "DepthViews", "DepthTrainStep", "ViewRenderer", "render_path_frames", "write_png", "read_png",
    "write_images_with_metrics", "write_images_with_metrics_testdist", "depthview", "DepthViewRenderer", "render_video_frames",
    "camcode", "CameraCodeOptimizer", "optimize_camera_embedding", "anyview", "AnyViewRenderer",
    "mesh", "extract_fields", "extract_geometry", "extract_iso_level", "marching_cubes", "keep_components", "write_ply", "read_ply",
]
