"""Held-out view evaluation: run_plnerf.py:284-363 (render_images_with_metrics) with the evaluation utilities of
run_nerf_helpers.py:537-570 (compute_rmse, MeanTracker).

A frame's metrics -- img2mse and PSNR of rgb and rgb0, SSIM of the clamped frame, depth RMSE over the valid pixels --
come from one launch of plnerf_eval_metrics (csrc/metrics.hip) on the frame where it already is, in HBM.  The reference
copies the frame to the host and runs skimage's SSIM on the CPU; here each frame's fp64 row stays on the device until
the loop ends and is read back once.  LPIPS is a network the caller supplies (`lpips_alex`), as in the reference; this
package ships no LPIPS weights.

The frames an evaluation keeps (`res`) are written by write_images_with_metrics / write_images_with_metrics_testdist
(run_plnerf.py:365-415) as 8-bit RGB and 16-bit depth PNGs through png.py.
"""
import math
import os

import numpy as np
import torch

from . import _lib as L
from . import raybatch as RB
from .png import write_png
from .nerf import NeRF
from .render import render


def compute_rmse(prediction, target):
    """run_nerf_helpers.py:537: root mean square difference; NaN for empty inputs (the mean of nothing)."""
    return torch.sqrt(torch.mean((prediction - target) ** 2))


class MeanTracker:
    """run_nerf_helpers.py:540-570: running means of named values.  One total weight serves every key, so a key that
    skips an add is averaged as the reference averages it; the update is the reference's, (m * w + l) / (w + weight)."""

    def __init__(self):
        self.reset()

    def add(self, input, weight=1.):
        for key, value in input.items():
            previous = self.mean_dict.get(key, 0)
            self.mean_dict[key] = (previous * self.total_weight + value) / (self.total_weight + weight)
        self.total_weight += weight

    def has(self, key):
        return key in self.mean_dict

    def get(self, key):
        return self.mean_dict[key]

    def as_dict(self):
        return self.mean_dict

    def reset(self):
        self.mean_dict = dict()
        self.total_weight = 0

    def print(self, f=None):
        for key, value in self.mean_dict.items():
            print("{}: {}".format(key, value), file=f)


def _psnr(mse):
    """mse2psnr on a Python float: -10 log10(mse); inf for 0, as torch gives."""
    if mse == 0:
        return math.inf
    return -10. * math.log(mse) / math.log(10.) if mse > 0 else math.nan


def metric_rows(rgb, target, rgb0=None, depth=None, target_depth=None, valid=None, out=None, workspace=None):
    """The [n, EVAL_ROW] fp64 device rows of plnerf_eval_metrics (columns _lib.EVAL_*) for frames rgb, target (and rgb0)
    [n,H,W,3] or [H,W,3] fp32, depth / target_depth [n,H,W] or [H,W] fp32 and valid of that shape (bool or uint8) --
    the depth three together or not at all.  One launch; nothing is synchronised.  `out` and `workspace`
    (_lib.eval_workspace_bytes uint8) may be given to reuse buffers."""
    lead = rgb.shape[:-3]
    if rgb.dim() not in (3, 4) or rgb.shape[-1] != 3:
        raise ValueError(f"rgb must be [H,W,3] or [n,H,W,3], got {tuple(rgb.shape)}")
    for name, t in (("target", target), ("rgb0", rgb0)):
        if t is not None and t.shape != rgb.shape:
            raise ValueError(f"{name} {tuple(t.shape)} does not match rgb {tuple(rgb.shape)}")
    given = [t is not None for t in (depth, target_depth, valid)]
    if any(given) and not all(given):
        raise ValueError("depth, target_depth and valid go together")
    if all(given):
        for name, t in (("depth", depth), ("target_depth", target_depth), ("valid", valid)):
            if t.shape != rgb.shape[:-1]:
                raise ValueError(f"{name} {tuple(t.shape)} does not match rgb's pixels {tuple(rgb.shape[:-1])}")
        valid = valid.contiguous()
        valid = valid.view(torch.uint8) if valid.dtype == torch.bool else valid
    n = int(np.prod(lead)) if len(lead) else 1
    H, W = rgb.shape[-3], rgb.shape[-2]
    if out is None:
        out = torch.empty(n, L.EVAL_ROW, dtype=torch.float64, device=rgb.device)
    if workspace is None:
        workspace = torch.empty(L.eval_workspace_bytes(n, H, W), dtype=torch.uint8, device=rgb.device)
    if out.shape != (n, L.EVAL_ROW) or workspace.numel() < L.eval_workspace_bytes(n, H, W):
        raise ValueError("out must be [n, EVAL_ROW] and workspace at least eval_workspace_bytes(n, H, W)")
    L.check(L.lib().plnerf_eval_metrics(
        n, H, W, L.dptr(rgb, "rgb"), L.dptr(target, "target"), L.dptr(rgb0, "rgb0"), L.dptr(depth, "depth"),
        L.dptr(target_depth, "target_depth"), L.dptr(valid, "valid", torch.uint8), L.dptr(workspace, "workspace", torch.uint8),
        L.dptr(out, "out", torch.float64), L.stream()), "plnerf_eval_metrics")
    return out


def sample_error_rows(pred_hyp, depth, valid=None, out=None, workspace=None, accumulate=False):
    """The [SAMPLEERR_ROW] fp64 device row of plnerf_sample_error (columns _lib.SAMPLEERR_SUM / _COUNT) for hypotheses
    pred_hyp [..., N] fp32 against depth [...] fp32 (the rendered depth_map), over the rays where valid [...] (bool or
    uint8; None = every ray) is set: the sum over those rays of mean_k |pred_hyp - depth|, and their number.
    accumulate=True adds both to `out` on the device instead of overwriting it (a frame scored chunk by chunk in stream
    order).  One call, two launches; nothing is synchronised.  `out` and `workspace`
    (_lib.sample_error_workspace_bytes(R) uint8, R = depth.numel()) may be given to reuse buffers."""
    if pred_hyp.dim() < 1:
        raise ValueError("pred_hyp must be [..., N]")
    if depth.shape != pred_hyp.shape[:-1]:
        raise ValueError(f"depth {tuple(depth.shape)} does not match pred_hyp's rays {tuple(pred_hyp.shape[:-1])}")
    if valid is not None:
        if valid.shape != depth.shape:
            raise ValueError(f"valid {tuple(valid.shape)} does not match depth {tuple(depth.shape)}")
        valid = valid.contiguous()
        valid = valid.view(torch.uint8) if valid.dtype == torch.bool else valid
    R, N = depth.numel(), pred_hyp.shape[-1]
    if out is None:
        if accumulate:
            raise ValueError("accumulate=True adds to `out`: pass the row to add to")
        out = torch.empty(L.SAMPLEERR_ROW, dtype=torch.float64, device=pred_hyp.device)
    if workspace is None:
        workspace = torch.empty(L.sample_error_workspace_bytes(R), dtype=torch.uint8, device=pred_hyp.device)
    if out.shape != (L.SAMPLEERR_ROW,) or workspace.numel() < L.sample_error_workspace_bytes(R):
        raise ValueError("out must be [SAMPLEERR_ROW] and workspace at least sample_error_workspace_bytes(R)")
    L.check(L.lib().plnerf_sample_error(
        R, N, L.dptr(pred_hyp, "pred_hyp"), L.dptr(depth, "depth"), L.dptr(valid, "valid", torch.uint8),
        1 if accumulate else 0, L.dptr(workspace, "workspace", torch.uint8), L.dptr(out, "out", torch.float64),
        L.stream()), "plnerf_sample_error")
    return out


def row_metrics(row, H, W, with_rgb0):
    """One host row -> {img_loss, psnr, ssim[, img_loss0, psnr0][, depth_rmse]}; depth_rmse is left out when it is NaN
    (no valid pixel), as the reference drops it."""
    mse = float(row[L.EVAL_SSE_RGB]) / (3 * H * W)
    m = {"img_loss": mse, "psnr": _psnr(mse), "ssim": float(row[L.EVAL_SSIM])}
    if with_rgb0:
        mse0 = float(row[L.EVAL_SSE_RGB0]) / (3 * H * W)
        m.update({"img_loss0": mse0, "psnr0": _psnr(mse0)})
    count = float(row[L.EVAL_DEPTH_COUNT])
    rmse = math.sqrt(float(row[L.EVAL_DEPTH_SSE]) / count) if count > 0 else math.nan
    if not math.isnan(rmse):
        m["depth_rmse"] = rmse
    return m


def image_metrics(rgb, target, rgb0=None, depth=None, target_depth=None, valid=None):
    """Metrics of one frame ([H,W,3] device tensors: a dict) or of a batch ([n,H,W,3]: a list of dicts), one kernel
    launch: img_loss (mean square error of the UNCLAMPED rgb, as img2mse before the clamp), psnr, ssim (skimage's
    structural_similarity of clamp(rgb, 0, 1) and target, data_range 1, 7x7 box windows), img_loss0 / psnr0 with rgb0,
    depth_rmse over the valid pixels when there is one."""
    rows = metric_rows(rgb, target, rgb0, depth, target_depth, valid).cpu().numpy()
    H, W = rgb.shape[-3], rgb.shape[-2]
    out = [row_metrics(r, H, W, rgb0 is not None) for r in rows]
    return out[0] if rgb.dim() == 3 else out


def _on_device(x, device, dtype=torch.float32):
    return torch.as_tensor(x).to(device=device, dtype=dtype).contiguous()


def _check_range(render_kwargs):
    for net in (render_kwargs.get('network_fn'), render_kwargs.get('network_fine')):
        if isinstance(net, NeRF) and net.precision in L.GUARDED_PRECISIONS and net.is_supported():
            net.check_range()       # a clamped frame must not be scored silently


def _choose_views(count, indices):
    """The views an evaluation loop renders (run_plnerf.py:285-294): every index in order for count None, else
    np.random.choice(indices, min(count, len), replace=False) under the caller's seed.  Returns (count, views)."""
    if count is None:
        return len(indices), indices
    count = min(count, len(indices))
    return count, np.random.choice(indices, size=count, replace=False)


def _score_views(count, indices, images, depths, valid_depths, poses, H, W, lpips_alex, chunk, render_kwargs_test,
                 render_fn, intrinsic_of, with_depth, before_frame, keep_images):
    """The loop of render_images_with_metrics (run_plnerf.py:284-363; run_nerf_sample_based_depth.py:424-510)."""
    far = render_kwargs_test['far']
    count, img_i = _choose_views(count, indices)
    dev = RB.default_device()

    rows = torch.empty(count, L.EVAL_ROW, dtype=torch.float64, device=dev)
    workspace = torch.empty(L.eval_workspace_bytes(1, H, W), dtype=torch.uint8, device=dev)
    lpips_vals = torch.empty(count, dtype=torch.float64, device=dev) if lpips_alex is not None else None
    if keep_images:
        rgbs_res = torch.empty(count, 3, H, W)
        rgbs0_res = torch.empty(count, 3, H, W)
        target_rgbs_res = torch.empty(count, 3, H, W)
        depths_res = torch.empty(count, 1, H, W)
        depths0_res = torch.empty(count, 1, H, W)
        target_depths_res = torch.empty(count, 1, H, W)
        target_valid_depths_res = torch.empty(count, 1, H, W, dtype=bool)
    extras = {}
    with torch.no_grad():
        for n, img_idx in enumerate(img_i):
            before_frame(img_idx)
            target = _on_device(images[img_idx], dev)
            rgb, _, _, extras = render_fn(H, W, intrinsic_of(img_idx), chunk=chunk, c2w=poses[img_idx, :3, :4],
                                          **render_kwargs_test)
            rgb0 = extras.get('rgb0')
            depth_args = ()
            if with_depth:
                target_depth = _on_device(depths[img_idx], dev)[:, :, 0].contiguous()
                target_valid = torch.as_tensor(valid_depths[img_idx]).to(device=dev, dtype=torch.bool).contiguous()
                depth_args = (extras['depth_map'].contiguous(), target_depth, target_valid)
            metric_rows(rgb.contiguous(), target, None if rgb0 is None else rgb0.contiguous(), *depth_args,
                        out=rows[n:n + 1], workspace=workspace)
            if lpips_alex is not None:
                lpips = lpips_alex(rgb.clamp(0, 1).permute(2, 0, 1).unsqueeze(0), target.permute(2, 0, 1).unsqueeze(0),
                                   normalize=True)[0]
                lpips_vals[n] = torch.as_tensor(lpips[0, 0, 0])
            if keep_images:
                rgbs_res[n] = rgb.clamp(0., 1.).permute(2, 0, 1).cpu()
                target_rgbs_res[n] = target.permute(2, 0, 1).cpu()
                depths_res[n] = (extras['depth_map'] / far).unsqueeze(0).cpu()
                if with_depth:
                    target_depths_res[n] = (target_depth / far).unsqueeze(0).cpu()
                    target_valid_depths_res[n] = target_valid.unsqueeze(0).cpu()
                else:
                    target_depths_res[n] = 0.
                    target_valid_depths_res[n] = False
                if rgb0 is not None:
                    depths0_res[n] = (extras['depth0'] / far).unsqueeze(0).cpu()
                    rgbs0_res[n] = rgb0.clamp(0, 1).permute(2, 0, 1).cpu()
    _check_range(render_kwargs_test)

    host_rows = rows.cpu().numpy()
    host_lpips = lpips_vals.cpu().tolist() if lpips_vals is not None else None
    mean_metrics, mean_depth_metrics = MeanTracker(), MeanTracker()
    with_rgb0 = 'rgb0' in extras
    for n in range(count):
        frame = row_metrics(host_rows[n], H, W, with_rgb0)
        metrics = {"img_loss": frame["img_loss"], "psnr": frame["psnr"], "ssim": frame["ssim"]}
        if host_lpips is not None:
            metrics["lpips"] = host_lpips[n]
        if with_rgb0:
            metrics.update({"img_loss0": frame["img_loss0"], "psnr0": frame["psnr0"]})
        if "depth_rmse" in frame:
            mean_depth_metrics.add({"depth_rmse": frame["depth_rmse"]})
        mean_metrics.add(metrics)

    res = None
    if keep_images:
        res = {"rgbs": rgbs_res, "target_rgbs": target_rgbs_res, "depths": depths_res, "target_depths": target_depths_res,
               "target_valid_depths": target_valid_depths_res}
        if with_rgb0:
            res.update({"rgbs0": rgbs0_res, "depths0": depths0_res})
    all_mean_metrics = MeanTracker()
    all_mean_metrics.add({**mean_metrics.as_dict(), **mean_depth_metrics.as_dict()})
    return all_mean_metrics, res


def render_images_with_metrics(count, indices, images, depths, valid_depths, poses, H, W, K, lpips_alex, args,
                               render_kwargs_test, embedcam_fn=None, with_test_time_optimization=False, *,
                               keep_images=True, one_call=False):
    """run_plnerf.py:284-363: renders `count` views of `indices` (all of them in order for None, else
    np.random.choice(indices, count, replace=False)) and returns (MeanTracker of img_loss, psnr, ssim[, lpips]
    [, img_loss0, psnr0][, depth_rmse], res).  res holds CPU [count,3,H,W] / [count,1,H,W] tensors as the reference
    builds them (frames clamped, depths divided by far; rgbs0 / depths0 when the renders carry rgb0).  Depths are scored
    for args.dataset == "scannet" only, from depths[i] [H,W,1] and valid_depths[i] [H,W], as there.

    lpips_alex: a callable called as the reference calls it (clamped frame and target, [1,3,H,W], normalize=True), its
    [0][0,0,0] recorded as "lpips"; None leaves "lpips" out.  embedcam_fn and with_test_time_optimization are accepted
    and unused, as in the reference.  keep_images=False (extension) skips res (None is returned for it), and with it
    every per-frame copy to the host: the metric rows are read back once, after the last frame.
    one_call (extension, off by default): each view comes from the one-call renderer that serves the configuration
    (anyview.frame_renderer: view.ViewRenderer, else anyview.AnyViewRenderer; blocks of args.chunk), built once per call, its
    planes scored in place -- where one serves it, the kwargs ask for no draws (perturb 0, no density noise: the test-time
    settings) AND the entries' fp32 focal reciprocals are the ones torch's device kernels use for K (entry_rays_are_renders):
    then its frames are render()'s bit for bit for device poses, and so are the rows; any other configuration keeps
    render(), silently.  The renderer's range status words are read once, after the last view."""
    with_depth = args.dataset == "scannet"
    renderer = _frame_renderer(render_kwargs_test, H, W, K, args) if one_call else None
    if renderer is None:
        return _score_views(count, indices, images, depths, valid_depths, poses, H, W, lpips_alex, args.chunk,
                            render_kwargs_test, render, lambda img_idx: K, with_depth, lambda img_idx: None, keep_images)
    host_poses = torch.as_tensor(poses).detach().to(device="cpu", dtype=torch.float32)      # (the call reads host floats)

    def render_fn(H, W, K, chunk=None, c2w=None, **kwargs):
        renderer.enqueue(c2w)
        return renderer._result(False)
    out = _score_views(count, indices, images, depths, valid_depths, host_poses, H, W, lpips_alex, args.chunk,
                       render_kwargs_test, render_fn, lambda img_idx: K, with_depth, lambda img_idx: None, keep_images)
    renderer.check_range()      # (sticky words: read once)
    return out


def entry_rays_are_renders(K):
    """Are the one-call entries' rays those render() builds on the device for these intrinsics, bit for bit?  rays.get_rays
    divides by the focal lengths as Python floats, which torch's device kernel turns into a multiply by the fp32 rounding of
    the DOUBLE reciprocal, float(1.0 / f); the entries hold fx / fy as fp32 and multiply by 1.0f / float(f)
    (csrc/pixel_select.h).  The two reciprocals are the same fp32 number for many focal lengths (11.3, 9.7, 1111.111) and an
    ulp apart for others (10.77): there the frames agree to rounding only, and a loop that promises render()'s rows keeps
    render()."""
    return all(np.float32(1.0 / float(f)) == np.float32(1.0) / np.float32(float(f)) for f in (K[0][0], K[1][1]))


def _frame_renderer(render_kwargs_test, H, W, K, args):
    """The one-call renderer of an evaluation loop (blocks of args.chunk), or None when the loop stays with render(): a
    configuration neither entry serves, kwargs that ask for draws -- the renderers' are counter-based and keyed by their
    own (seed, step), not what render() would draw -- or focal lengths at which the entries' rays are an ulp from render()'s."""
    from .anyview import frame_renderer
    kw = {k: v for k, v in render_kwargs_test.items() if k not in ("near", "far", "ndc")}
    if kw.get("perturb", 0.) > 0. or kw.get("raw_noise_std", 0.) > 0.:
        return None
    if not entry_rays_are_renders(K):
        return None
    return frame_renderer(kw, H, W, K, min(int(args.chunk), H * W), render_kwargs_test.get("near", 0.),
                          render_kwargs_test.get("far", 1.), ndc=render_kwargs_test.get("ndc", True))


def to8b(x):
    """run_nerf_helpers.py:19: [0, 1] floats -> 8-bit codes, truncating."""
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


def to16b(x):
    """run_nerf_helpers.py:20: [0, 1] floats -> 16-bit codes, truncating."""
    return (65535 * np.clip(x, 0, 1)).astype(np.uint16)


def _write_result_dir(result_dir, images, mean_metrics):
    """run_plnerf.py:372-386: {n}_rgb.png, {n}_gt.png (8-bit RGB), {n}_d.png (16-bit grey) per frame and metrics.txt.
    (The reference hands OpenCV a BGR copy of each colour frame, which stores it as RGB: the files hold RGB.)"""
    os.makedirs(result_dir, exist_ok=True)
    planes = [images[k].permute(0, 2, 3, 1).cpu().numpy() for k in ("rgbs", "depths", "target_rgbs")]
    for n, (rgb, depth, gt_rgb) in enumerate(zip(*planes)):
        write_png(os.path.join(result_dir, f"{n}_rgb.png"), to8b(rgb))
        write_png(os.path.join(result_dir, f"{n}_gt.png"), to8b(gt_rgb))
        write_png(os.path.join(result_dir, f"{n}_d.png"), to16b(depth))
    with open(os.path.join(result_dir, "metrics.txt"), "w") as f:
        mean_metrics.print(f)
    mean_metrics.print()
    return result_dir


def _optimization_tag(with_test_time_optimization):
    return "with_optimization_" if with_test_time_optimization else ""


def write_images_with_metrics(images, mean_metrics, far, args, with_test_time_optimization=False, test_samples=False):
    """run_plnerf.py:365-386: write `images` (render_images_with_metrics' res: CPU fp32 frames already clamped, depths
    already divided by far) under args.ckpt_dir / args.expname.  The directory name is the reference's, as it builds it:
    the sample counts appear twice with test_samples, and nothing separates "samples" from the mode there.  `far` is
    accepted and unused, as in the reference.  Returns the directory (extension)."""
    counts = f"{args.N_samples}_{args.N_importance}"
    tag = _optimization_tag(with_test_time_optimization)
    if not test_samples:
        name = f"test_images_{args.mode}_{counts}{tag}{args.scene_id}"
    else:
        name = f"test_images_samples{args.mode}_{counts}{tag}{counts}{args.scene_id}"
    return _write_result_dir(os.path.join(args.ckpt_dir, args.expname, name), images, mean_metrics)


def write_images_with_metrics_testdist(images, mean_metrics, far, args, test_dist, with_test_time_optimization=False,
                                       test_samples=False):
    """run_plnerf.py:388-415: the same files under a directory named after the test distance."""
    tag = _optimization_tag(with_test_time_optimization)
    if not test_samples:
        name = f"test_images_dist{test_dist}_{tag}{args.scene_id}"
    else:
        name = f"test_images_samples_dist{test_dist}_{tag}{args.N_samples}_{args.N_importance}{args.scene_id}"
    return _write_result_dir(os.path.join(args.ckpt_dir, args.expname, name), images, mean_metrics)
