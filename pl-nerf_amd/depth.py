"""Depth-supervised variant of the path (BASELINE config 5): the caller-side
mirror of depth_supervised_exps/run_nerf_sample_based_depth.py and
depth_supervised_exps/model/run_nerf_helpers.py, on the same HIP kernels.

What differs from the NVS path (render.py):
  * the encoder multiplies by pi (model/run_nerf_helpers.py:123) and the default widths are
    multires 9 / multires_views 0 -> input_ch 57, input_ch_views 3 (run_nerf_sample_based_depth.py:
    1306-1309): the encoding is evaluated here and handed to the fused MLP as `embedded`;
  * positions pass through (x - bb_center) * bb_scale first (:56);
  * the density channel goes through softplus(beta=10) (model/run_nerf_helpers.py:200);
  * render_rays draws a third set of samples, `pred_hyp`, from the final weights WITHOUT detaching them
    (:923-934): the space-carving loss back-propagates through the sampler (plnerf_sample_pl_bwd) and
    the transmittance / density knots (g_tau, g_T of plnerf_quad_bwd);
  * one Adam over both networks, gradient values clipped to 0.1 (:1155-1157).
"""
import math
import os
import sys

import numpy as np
import torch

from . import _lib as L
from . import functional as Fn
from . import raybatch as RB
from .evaluate import MeanTracker, _check_range, _choose_views, _score_views, sample_error_rows
from .nerf import Embedder, NeRF
from .optim import FlatAdam
from .render import (MAX_ROWS_PER_LAUNCH, _draw_noise, _refuse_unsupported, _rgb_sigma, batchify, raw2outputs as _raw2outputs, sample_pdf,
                     sample_pdf_reformulation)

_RENDER = sys.modules[__name__.rsplit(".", 1)[0] + ".render"]      # (the package attribute `render` is the function)


def _nvs_draw_u(*args):
    """The importance draw of the NVS sampler (render._draw_u), looked up at call time like sample_pdf_reformulation
    itself does (a test that injects its draws there reaches both routes)."""
    return _RENDER._draw_u(*args)


def get_embedder(multires, i=0):
    """model/run_nerf_helpers.py:132-148: gamma(x) with sin/cos(x * pi * 2^k)."""
    if i == -1:
        return torch.nn.Identity(), 3
    emb = Embedder(include_input=True, input_dims=3, max_freq_log2=multires - 1, num_freqs=multires,
                   log_sampling=True, periodic_fns=[torch.sin, torch.cos], input_scale=np.pi)
    return emb, emb.out_dim


def _kernel_encoding(embed_fn, embeddirs_fn, viewdirs):
    """(fx, fd, input scale) when plnerf_embed_rows evaluates these two encoders, else None: gamma(x) = [x, sin / cos of
    x s 2^k, k < L] with s = 1 (run_nerf_helpers.py:24-54) or pi (depth_supervised_exps/model/run_nerf_helpers.py:123)."""
    def freqs(e):
        if not isinstance(e, Embedder):
            return None
        sc = 1.0 if e.input_scale is None else float(e.input_scale)
        ok = (e.input_dims == 3 and e.include_input and e.log_sampling and list(e.periodic_fns) == [torch.sin, torch.cos]
              and e.max_freq_log2 == e.num_freqs - 1 and 0 <= e.num_freqs <= 16)
        return (e.num_freqs, sc) if ok else None
    fx = freqs(embed_fn)
    if fx is None:
        return None
    if viewdirs is None:
        return fx[0], 0, fx[1]
    fd = freqs(embeddirs_fn)
    if fd is None:
        return None
    scales = {sc for n, sc in (fx, fd) if n > 0}      # (an encoder without frequency bands has no use for its scale)
    if len(scales) > 1:
        return None
    return fx[0], fd[0], (scales.pop() if scales else 1.0)


FUSE_STAGES = True      # (tests switch it off to compare the one-launch stages with the separate launches, bit for bit)
# Tests only (tests/test_gpu_fullsize.py), as render.STAGE_TAP: a dict that render_rays fills with its intermediate tensors
# (coarse weights / tau / T and importance samples, final weights / tau / T and the hypotheses' search indices); while it
# is set the stages run as their separate launches, which is where those tensors exist in HBM.
STAGE_TAP = None
_BOX_CACHE = {}


def _host_box(bb_center, bb_scale):
    """The bounding-box affine as host floats ((cx, cy, cz), scale, is-identity).  The reference script keeps the box as
    device tensors (run_nerf_sample_based_depth.py:52-56); reading them costs a host synchronisation, which must not
    happen on every network evaluation of a training step: resolved once per (tensor, version)."""
    def key(x):
        return (id(x), x._version) if isinstance(x, torch.Tensor) else ("v", repr(x))
    k = (key(bb_center), key(bb_scale))
    hit = _BOX_CACHE.get(k)
    hit = hit[0] if hit is not None else None
    if hit is None:
        c = torch.as_tensor(bb_center, dtype=torch.float32).reshape(-1).cpu()
        center = tuple(float(c[i if c.numel() == 3 else 0]) for i in range(3))
        scale = float(torch.as_tensor(bb_scale))
        hit = (center, scale, scale == 1.0 and not any(center))
        if len(_BOX_CACHE) > 64:
            _BOX_CACHE.clear()
        # (the entry keeps the two objects alive: an id() can otherwise be handed to a new tensor after the old one died)
        _BOX_CACHE[k] = (hit, bb_center, bb_scale)
    return hit


def run_network(inputs, viewdirs, embedded_cam, fn, embed_fn, embeddirs_fn, bb_center, bb_scale, netchunk=1024 * 64):
    """run_nerf_sample_based_depth.py:52-68: bounding-box affine, encodings (positions | per-ray direction | per-image
    camera code, each repeated over the ray's samples), then the MLP in row chunks.  inputs [R, S, 3].

    On the GPU the whole input assembly is ONE launch (plnerf_embed_rows) instead of ~100 element-wise / cat launches
    per network evaluation (1.2 ms of a 10.8 ms depth-supervised step, profiles/r03_depth_kernel_stats_before.csv).  A
    camera code that requires grad (trained through the network input, :1091-1093, 1122-1123; optimised alone,
    :311-345) is handed to the MLP as `cam` and gets its gradient there (functional.MlpFn)."""
    R, S = inputs.shape[0], inputs.shape[1]
    on_hip = isinstance(fn, NeRF) and fn.is_supported() and inputs.is_cuda
    # `netchunk` "does not affect final results" (rows are independent): on the HIP MLP the rows go in launches as large
    # as the saved-activation buffer allows instead of the reference's 65,536-row chunks (a training step would
    # otherwise pay one forward, one backward and one weight-gradient reduction PER CHUNK)
    if on_hip:
        netchunk = max(int(netchunk), MAX_ROWS_PER_LAUNCH)
    enc = _kernel_encoding(embed_fn, embeddirs_fn, viewdirs) if on_hip else None
    cam = None if (viewdirs is None or embedded_cam is None or embedded_cam.numel() == 0) else embedded_cam
    if enc is not None and not (torch.is_grad_enabled() and (inputs.requires_grad or
                                                             (viewdirs is not None and viewdirs.requires_grad))):
        fx, fd, scale = enc
        bb_center, bb_scale, identity_box = _host_box(bb_center, bb_scale)      # (host floats: no sync per evaluation)
        if (cam is None and identity_box and fn.has_fused_encoding() and fn.input_ch == 3 + 6 * fx and
                (not fn.use_viewdirs or fn.input_ch_views == 3 + 6 * fd)):
            # the encoding in the MLP kernel's own prologue, as on the NVS path: no `embedded` matrix at all
            rays_per_launch = max(1, MAX_ROWS_PER_LAUNCH // max(S, 1))
            if not torch.is_grad_enabled():      # (inference saves nothing: one launch whatever the size)
                rays_per_launch = max(R, 1)
            else:                                # equal shares (a remainder launch of a few rows costs a whole tile walk)
                rays_per_launch = -(-R // max(-(-R // rays_per_launch), 1)) if R > 0 else 1
            vd = viewdirs if fn.use_viewdirs else None
            outs = [fn.query(inputs[i:i + rays_per_launch], None if vd is None else vd[i:i + rays_per_launch],
                             input_scale=scale) for i in range(0, R, rays_per_launch)]
            return outs[0] if len(outs) == 1 else torch.cat(outs, 0)
        embedded = Fn.embed_rows(inputs, viewdirs, cam, fx, fd, input_scale=scale, bb_center=bb_center,
                                 bb_scale=bb_scale)
        cam_grad = cam if (cam is not None and torch.is_grad_enabled() and cam.requires_grad) else None
        blocks = [fn(block, cam=cam_grad) if cam_grad is not None else fn(block)
                  for block in torch.split(embedded, netchunk, dim=0)]
        raw = blocks[0] if len(blocks) == 1 else torch.cat(blocks, 0)
        return raw.reshape(*inputs.shape[:-1], raw.shape[-1])
    columns = [embed_fn(((inputs.reshape(-1, inputs.shape[-1]) - bb_center) * bb_scale))]
    if viewdirs is not None:
        per_ray = embeddirs_fn(viewdirs)                              # row-wise encoder: encode once per ray ...
        columns.append(per_ray[:, None, :].expand(R, S, per_ray.shape[-1]).reshape(R * S, -1))   # ... then repeat
        columns.append(embedded_cam.reshape(1, -1).expand(R * S, embedded_cam.shape[0]))
    raw = batchify(fn, netchunk)(torch.cat(columns, -1))
    return raw.reshape(*inputs.shape[:-1], raw.shape[-1])


def raw2outputs(raw, z_vals, near, far, rays_d, mode, color_mode, raw_noise_std=0, pytest=False, white_bkgd=False,
                farcolorfix=False):
    """run_nerf_sample_based_depth.py:709-773.  `farcolorfix` is accepted and ignored there."""
    return _raw2outputs(raw, z_vals, near, far, rays_d, mode, color_mode, raw_noise_std, pytest=pytest,
                        white_bkgd=white_bkgd, farcolorfix=False)


def _draw_u(n_rays, N_samples, det, pytest, load_u, joint, device):
    """The draw of the *_return_u samplers (model/run_nerf_helpers.py:619-638; joint: 792-812)."""
    if load_u is not None:
        return load_u
    draws = None if pytest else Fn.DRAWS
    if det:
        u = Fn.cpu_linspace(N_samples, device).expand(n_rays, N_samples)
    elif joint:      # one row for the whole image
        row = (_joint_row(draws, N_samples, device) if draws is not None else torch.rand(N_samples, device=device))
        u = row.unsqueeze(0).repeat(n_rays, 1)
    elif draws is not None:
        u = draws.uniform(n_rays, N_samples, Fn.FineEpilogueFn.HYP_STREAM, device)
    else:
        u = torch.rand(n_rays, N_samples, device=device)
    if pytest:
        np.random.seed(0)
        if det:
            u = torch.Tensor(np.broadcast_to(np.linspace(0., 1., N_samples), [n_rays, N_samples]).copy()).to(device)
        else:
            u = torch.Tensor(np.random.rand(n_rays, N_samples)).to(device)
    return u


def _joint_row(draws, n, device):
    """The is_joint draw -- ONE row of u for the whole image -- from the counters of global ray 0, so that every rank of
    a sharded batch sees the same row."""
    keep = draws.ray_id0, draws.chunk_offset
    draws.ray_id0, draws.chunk_offset = 0, 0
    try:
        return draws.uniform(1, n, Fn.FineEpilogueFn.HYP_STREAM, device).reshape(-1)
    finally:
        draws.ray_id0, draws.chunk_offset = keep


def sample_pdf_reformulation_return_u(bins, weights, tau, T, near, far, N_samples, det=False, pytest=False,
                                      load_u=None, quad_solution_v2=True, zero_threshold=1e-4, epsilon_=1e-3,
                                      joint=False):
    """model/run_nerf_helpers.py:607-692 (and :780- for joint=True).  Returns (samples, T_below, tau_below,
    bin_below, u); `samples` is differentiable with respect to tau and T."""
    u = _draw_u(bins.shape[0], N_samples, det, pytest, load_u, joint, bins.device).contiguous()
    s, Tb, taub, binb = Fn.sample_pl(bins, weights, tau, T, near, far, u, zero_threshold, epsilon_, want_extras=True)
    return s, Tb, taub, binb, u


def sample_pdf_return_u(bins, weights, N_samples, det=False, pytest=False, load_u=None, joint=False):
    """model/run_nerf_helpers.py:343-394 (piecewise-constant mode; :446- for joint=True).  Returns (samples, u);
    `samples` is differentiable with respect to `weights` (plnerf_sample_const_bwd)."""
    u = _draw_u(bins.shape[0], N_samples, det, pytest, load_u, joint, bins.device).contiguous()
    return Fn.sample_const(bins, weights, u), u


def _draw_t_rand(n_rays, n_samples, pytest, device):
    """The stratified jitter of run_nerf_sample_based_depth.py:781-788: np.random.seed(0) draws under pytest; else from
    an installed functional.DrawSource (counter-based on the global ray id: the step does not depend on how the batch
    is sharded), else torch.rand as the reference."""
    if pytest:
        return Fn.numpy_uniform([n_rays, n_samples], device)
    if Fn.DRAWS is not None:
        return Fn.DRAWS.uniform(n_rays, n_samples, Fn.DrawSource.T_RAND, device)
    return torch.rand(n_rays, n_samples, device=device)


def perturb_z_vals(z_vals, pytest):
    """run_nerf_sample_based_depth.py:775-790."""
    mids = .5 * (z_vals[..., 1:] + z_vals[..., :-1])
    upper = torch.cat([mids, z_vals[..., -1:]], -1)
    lower = torch.cat([z_vals[..., :1], mids], -1)
    t_rand = _draw_t_rand(z_vals.shape[0], z_vals.shape[1], pytest, z_vals.device)
    return lower + (upper - lower) * t_rand


def render_rays(ray_batch, use_viewdirs, network_fn, network_query_fn, N_samples, mode, color_mode,
                precomputed_z_samples=None, embedded_cam=None, retraw=False, lindisp=False, perturb=0.,
                N_importance=0, network_fine=None, raw_noise_std=0., verbose=False, pytest=False, white_bkgd=False,
                is_joint=False, cached_u=None, scale_sample_gradient=False, quad_solution_v2=False, zero_tol=1e-4,
                epsilon=1e-3, farcolorfix=False):
    """run_nerf_sample_based_depth.py:792-958.  Returns the reference's dict: rgb_map, disp_map, acc_map,
    depth_map, z_vals, weights, pred_hyp, u (+ raw; + rgb0, disp0, acc0, depth0, z_vals0, weights0, z_std)."""
    dev = ray_batch.device
    N_rays = ray_batch.shape[0]
    if isinstance(ray_batch, RB.RayColumns):      # (what plnerf_select_rays writes: no packing, no slice copies)
        rays_o, rays_d, near, far = ray_batch.rays_o, ray_batch.rays_d, ray_batch.near.reshape(-1, 1), \
            ray_batch.far.reshape(-1, 1)
        viewdirs = ray_batch.viewdirs if use_viewdirs else None
    else:
        rays_o, rays_d = ray_batch[:, 0:3].contiguous(), ray_batch[:, 3:6].contiguous()
        viewdirs = ray_batch[:, 8:11].contiguous() if use_viewdirs else None
        near, far = ray_batch[:, 6:7].contiguous(), ray_batch[:, 7:8].contiguous()
    # A ray batch that requires a gradient (no training path of the reference has one): as in render.py, the glue then runs
    # as the reference's own torch expressions, the quadrature and the samplers return the geometry's gradient
    # (plnerf_quad_bwd_rays; plnerf_sample_pl_bwd_rays / SampleConstFn's bins -- here the depth hypotheses STAY attached to the
    # sampler's bins, :923-934), the networks their inputs' (plnerf_mlp_input_grad).
    rays_grad = torch.is_grad_enabled() and any(
        t is not None and t.requires_grad for t in (rays_o, rays_d, near, far, viewdirs))
    t_vals = Fn.cpu_linspace(N_samples, dev)
    fused_glue = ray_batch.is_cuda and N_rays > 0 and not rays_grad
    draws = None if pytest else Fn.DRAWS      # counter-based draws inside the consuming kernels (functional.DrawSource)
    if draws is not None:
        draws.noise_calls = 0
    # The stages between and behind the two network evaluations as ONE launch each, like the NVS path's (piecewise-linear
    # mode): plnerf_coarse_epilogue (raw2outputs + importance sampling + clamp + sort + positions) and
    # plnerf_fine_epilogue (raw2outputs + the hypotheses' sampler + z_std); bit-identical to the separate calls below.
    tap = STAGE_TAP
    # Piecewise-constant mode likewise (plnerf_coarse_epilogue_const / plnerf_fine_epilogue_const; the sampler needs three depths).
    fused = FUSE_STAGES and fused_glue and tap is None and (
        (mode == "linear" and color_mode in ("midpoint", "left")) or (mode == "constant" and N_samples >= 3))
    if fused_glue:
        # depths, jitter and positions in one launch (plnerf_coarse_samples: bit-identical to the expressions below,
        # which are :775-790 and run_plnerf.py:683-708 alike); the jitter from the reference's draw, or in the kernel
        t_rand = _draw_t_rand(N_rays, N_samples, pytest, dev) if (perturb > 0. and draws is None) else None
        z_vals, pts = Fn.coarse_samples(rays_o, rays_d, near, far, t_vals, t_rand, lindisp, perturb > 0., draws)
    else:
        if not lindisp:
            z_vals = near * (1. - t_vals) + far * t_vals
        else:
            z_vals = 1. / (1. / near * (1. - t_vals) + 1. / far * t_vals)
        if perturb > 0.:
            z_vals = perturb_z_vals(z_vals, pytest)
        pts = rays_o[..., None, :] + rays_d[..., None, :] * z_vals[..., :, None]
    raw = network_query_fn(pts, viewdirs, embedded_cam, network_fn)
    if tap is not None:
        tap.update(z_vals0=z_vals, raw0=raw)

    def last_stage(raw, z_vals, n, load_u):
        """raw2outputs of the final pass + the depth hypotheses on its weights (:909-934), one launch."""
        det = perturb == 0.
        if load_u is not None or det or pytest or draws is None:
            u = _draw_u(N_rays, n, det, pytest, load_u, is_joint, dev).contiguous()
        else:      # drawn inside the kernel; is_joint: one row from the counters of ray 0
            u = _joint_row(draws, n, dev) if is_joint else None
        rgb, disp, acc, depth, w, tau, T, hyp, u_used, _, z_std = Fn.FineEpilogueFn.apply(
            _rgb_sigma(raw), z_vals, near, far, rays_d, _draw_noise(raw, raw_noise_std, pytest), u, n, color_mode,
            white_bkgd, False, zero_tol, epsilon, draws, mode)
        return rgb, disp, acc, w, depth, hyp, u_used, z_std

    if fused and N_importance == 0:
        rgb_map, disp_map, acc_map, weights, depth_map, pred_depth_hyp, u, _ = last_stage(raw, z_vals, N_samples, None)
    elif fused:
        z_vals_0 = z_vals
        det = perturb == 0.
        u0 = _nvs_draw_u([N_rays], N_importance, det, pytest, dev) if (pytest or det or draws is None) else None
        rgb_map_0, disp_map_0, acc_map_0, depth_map_0, z_vals, pts, _, weights_0 = Fn.CoarseEpilogueFn.apply(
            _rgb_sigma(raw), z_vals, near, far, rays_o, rays_d, _draw_noise(raw, raw_noise_std, pytest), u0,
            N_importance, color_mode, white_bkgd, False, zero_tol, epsilon, draws, True, mode)
        run_fn = network_fn if network_fine is None else network_fine
        raw = network_query_fn(pts, viewdirs, embedded_cam, run_fn)
        rgb_map, disp_map, acc_map, weights, depth_map, pred_depth_hyp, u, z_std = last_stage(raw, z_vals, N_importance,
                                                                                             cached_u)
    else:
        rgb_map, disp_map, acc_map, weights, depth_map, tau, T = raw2outputs(
            raw, z_vals, near, far, rays_d, mode, color_mode, raw_noise_std, pytest=pytest, white_bkgd=white_bkgd,
            farcolorfix=farcolorfix)

    def hypotheses(z_vals, weights, tau, T, n, load_u):
        if mode == "linear" and tap is not None:
            u = _draw_u(N_rays, n, perturb == 0., pytest, load_u, is_joint, dev).contiguous()
            s, inds = Fn.sample_pl(z_vals, weights, tau, T, near, far, u, zero_tol, epsilon, want_inds=True)
            tap.update(weights_full=weights, tau=tau, T=T, hyp_inds=inds)
        elif mode == "linear":
            s, _, _, _, u = sample_pdf_reformulation_return_u(
                z_vals, weights, tau, T, near, far, n, det=(perturb == 0.), pytest=pytest, load_u=load_u,
                quad_solution_v2=quad_solution_v2, zero_threshold=zero_tol, epsilon_=epsilon, joint=is_joint)
        elif mode == "constant":
            z_mid = .5 * (z_vals[..., 1:] + z_vals[..., :-1])
            s, u = sample_pdf_return_u(z_mid, weights[..., 1:-1], n, det=(perturb == 0.), pytest=pytest,
                                       load_u=load_u, joint=is_joint)
        else:
            raise ValueError("mode must be 'linear' or 'constant'")
        return s, u

    if fused:
        pass
    elif N_importance == 0:
        pred_depth_hyp, u = hypotheses(z_vals, weights, tau, T, N_samples, None)
    else:
        rgb_map_0, disp_map_0, acc_map_0, depth_map_0, z_vals_0, weights_0 = \
            rgb_map, disp_map, acc_map, depth_map, z_vals, weights
        if mode == "linear" and tap is not None:
            u0 = _nvs_draw_u(z_vals.shape[:-1], N_importance, perturb == 0., pytest, dev)
            z_samples, inds0 = Fn.sample_pl(z_vals, weights, tau, T, near, far, u0, zero_tol, epsilon, want_inds=True)
            tap.update(weights0_full=weights, tau0=tau, T0=T, u0=u0, inds0=inds0, z_samples=z_samples)
        elif mode == "linear":
            with torch.set_grad_enabled(torch.is_grad_enabled() and not rays_grad):      # (detached below either way)
                z_samples = sample_pdf_reformulation(z_vals, weights, tau, T, near, far, N_importance, det=(perturb == 0.),
                                                     pytest=pytest, quad_solution_v2=quad_solution_v2,
                                                     zero_threshold=zero_tol, epsilon_=epsilon)[0]
        else:
            z_mid = .5 * (z_vals[..., 1:] + z_vals[..., :-1])
            z_samples = sample_pdf(z_mid, weights[..., 1:-1], N_importance, det=(perturb == 0.), pytest=pytest)
        z_samples = z_samples.detach()
        if rays_grad:      # :902-906 as written: the clamp's bounds and the coarse depths carry the batch's gradient
            z_vals, order = torch.sort(torch.cat([z_vals, torch.clamp(z_samples, near, far)], -1), -1)
            if tap is not None:
                tap.update(sort_order=order)      # (ties: render.py)
        else:
            z_vals = Fn.merge_sort(z_vals, z_samples, near, far)          # clamp + cat + sort (:902-906)
        if fused_glue:
            pts = Fn.ray_points(rays_o, rays_d, z_vals)
        else:
            pts = rays_o[..., None, :] + rays_d[..., None, :] * z_vals[..., :, None]
        run_fn = network_fn if network_fine is None else network_fine
        raw = network_query_fn(pts, viewdirs, embedded_cam, run_fn)
        rgb_map, disp_map, acc_map, weights, depth_map, tau, T = raw2outputs(
            raw, z_vals, near, far, rays_d, mode, color_mode, raw_noise_std, pytest=pytest, white_bkgd=white_bkgd)
        pred_depth_hyp, u = hypotheses(z_vals, weights, tau, T, N_importance, cached_u)
        z_std = torch.std(pred_depth_hyp, dim=-1, unbiased=False)

    if mode == "linear":
        weights = weights[..., 1:]
    ret = {'rgb_map': rgb_map, 'disp_map': disp_map, 'acc_map': acc_map, 'depth_map': depth_map,
           'z_vals': z_vals, 'weights': weights, 'pred_hyp': pred_depth_hyp, 'u': u}
    if retraw:
        ret['raw'] = raw
    if N_importance > 0:
        ret['rgb0'] = rgb_map_0
        ret['disp0'] = disp_map_0
        ret['acc0'] = acc_map_0
        ret['depth0'] = depth_map_0
        ret['z_vals0'] = z_vals_0
        ret['weights0'] = weights_0
        ret['z_std'] = z_std
    return ret


def get_ray_dirs(H, W, intrinsic, c2w, coords=None):
    """model/run_nerf_helpers.py:243-257: intrinsic = (fx, fy, cx, cy); pixel CENTRES (+0.5) and a flipped image
    row, unlike the NVS script's get_rays.  coords [n, 2] = (row, col) selects pixels."""
    fx, fy, cx, cy = intrinsic[0], intrinsic[1], intrinsic[2], intrinsic[3]
    if coords is None:
        dev = c2w.device
        cols, rows = torch.meshgrid(torch.linspace(0, W - 1, W, device=dev), torch.linspace(0, H - 1, H, device=dev),
                                    indexing='ij')
        cols, rows = cols.t(), rows.t()
    else:
        cols, rows = coords[:, 1], coords[:, 0]
    dirs = torch.stack([((cols + 0.5) - cx) / fx, (H - (rows + 0.5) - cy) / fy, -torch.ones_like(cols)], -1)
    return torch.sum(dirs[..., None, :] * c2w[:3, :3], -1)


def get_rays(H, W, intrinsic, c2w, coords=None):
    """model/run_nerf_helpers.py:259-263."""
    rays_d = get_ray_dirs(H, W, intrinsic, c2w, coords)
    return c2w[:3, -1].expand(rays_d.shape), rays_d


def batchify_rays(rays_flat, chunk=1024 * 32, use_viewdirs=False, **kwargs):
    """run_nerf_sample_based_depth.py:71-83."""
    return RB.map_row_chunks(lambda rows, first_row: render_rays(rows, use_viewdirs, **kwargs), rays_flat, chunk)


def render(H, W, intrinsic, chunk=1024 * 32, rays=None, c2w=None, ndc=True, near=0., far=1., with_5_9=False,
           use_viewdirs=False, c2w_staticcam=None, rays_depth=None, **kwargs):
    """run_nerf_sample_based_depth.py:85-160 (render_hyp, :162-248, is the same function).  Returns
    [rgb_map, disp_map, acc_map, extras]; `ndc` is accepted and unused, as there.  `rays` = (origins, directions) or
    (origins, directions, depth columns); a full view comes from `c2w`, optionally centre-cropped to 5.33:9."""
    if c2w is not None:
        rays_o, rays_d = get_rays(H, W, intrinsic, c2w)
        if with_5_9:
            crop = int(H / 9. * 16. / 3.)
            crop -= crop % 2
            first = (W - crop) // 2
            rays_o, rays_d, W = rays_o[:, first:first + crop, :], rays_d[:, first:first + crop, :], crop
    elif rays.shape[0] == 2:
        rays_o, rays_d = rays
    else:
        rays_o, rays_d, rays_depth = rays
    extra = []
    if use_viewdirs:
        extra.append(RB.unit_directions(rays_d))
        if c2w_staticcam is not None:
            rays_o, rays_d = get_rays(H, W, intrinsic, c2w_staticcam)
    if rays_depth is not None:
        extra.append(rays_depth.reshape(-1, 3).float())
    rows, lead = RB.pack_rays(rays_o, rays_d, near, far, extra)
    return RB.unflatten_outputs(batchify_rays(rows, chunk, use_viewdirs, **kwargs), lead)


render_hyp = render


def render_images_with_metrics(count, indices, images, depths, valid_depths, poses, H, W, intrinsics, lpips_alex, args,
                               render_kwargs_test, embedcam_fn=None, with_test_time_optimization=False, *,
                               keep_images=True, one_call=False):
    """run_nerf_sample_based_depth.py:424-510: evaluate.render_images_with_metrics on this variant's render, with the
    per-view intrinsics[i] = (fx, fy, cx, cy) and the sensor depths[i] [H,W,1] / valid_depths[i] [H,W] of every view.
    With args.input_ch_cam > 0 the camera code is embedcam_fn(i), or zeros when embedcam_fn is None (set in
    render_kwargs_test["embedded_cam"], as there).  with_test_time_optimization: with embedcam_fn None, the code of every view is
    optimised first where the reference does (:458-463; camcode.optimize_camera_embedding, one CameraCodeOptimizer kept across
    the views where the cached route serves the configuration); with args.input_ch_cam == 0 there is no code to optimise and
    the flag raises (the reference ignores it there).
    one_call: frames come from a depthview.DepthViewRenderer (one library call per frame, blocks of args.chunk) when it
    serves the configuration AND the kwargs ask for no draws (perturb 0, no density noise: the test-time settings, at which
    its frames are render()'s bit for bit); any other configuration takes render() as before.
    The poses and intrinsics are copied to the host once for all views (the call reads host floats), and the renderer's range
    status words are read once, after the last view."""
    optimise = _test_time_optimizer(with_test_time_optimization, args, render_kwargs_test, embedcam_fn, images, poses,
                                    intrinsics, H, W)
    set_camera_code = _camera_code_setter(args, render_kwargs_test, embedcam_fn, RB.default_device(), optimise)
    renderer = _view_renderer(render_kwargs_test, H, W, args) if one_call else None
    if renderer is None:
        return _score_views(count, indices, images, depths, valid_depths, poses, H, W, lpips_alex, args.chunk,
                            render_kwargs_test, render, lambda img_idx: intrinsics[img_idx, :], True, set_camera_code,
                            keep_images)
    host_poses, host_intrinsics = _on_host(poses), _on_host(intrinsics)

    def render_fn(H, W, intrinsic, chunk=None, c2w=None, **kwargs):
        return renderer.render(c2w, intrinsic, check=False)
    out = _score_views(count, indices, images, depths, valid_depths, host_poses, H, W, lpips_alex, args.chunk,
                       render_kwargs_test, render_fn, lambda img_idx: host_intrinsics[img_idx, :], True, set_camera_code,
                       keep_images)
    renderer.check_range()      # (its own packed buffers carry the status words of its frames: sticky, read once)
    return out


def _on_host(x):
    """A float32 host copy (one transfer for all views: DepthViewRenderer.enqueue reads host floats)."""
    return torch.as_tensor(x).detach().to(device="cpu", dtype=torch.float32)


def _view_renderer(render_kwargs_test, H, W, args):
    """The DepthViewRenderer of an evaluation loop (blocks of args.chunk), or None when the loop stays with render(): a
    configuration plnerf_depth_render_view does not serve (a camera code, say, with args.input_ch_cam > 0), or kwargs that
    ask for draws (perturb > 0 or density noise) -- the renderer's are counter-based and keyed by its own (seed, step), not
    what render() would draw, so only the draw-free test-time settings, where the two routes agree bit for bit, go there."""
    from .depthview import DepthViewRenderer
    kw = {k: v for k, v in render_kwargs_test.items() if k not in ("near", "far", "ndc")}
    if kw.get("perturb", 0.) > 0. or kw.get("raw_noise_std", 0.) > 0.:
        return None
    if getattr(args, "input_ch_cam", 0) > 0 or not DepthViewRenderer.supported(kw):
        return None
    return DepthViewRenderer(kw, H, W, min(int(args.chunk), H * W), render_kwargs_test.get("near", 0.),
                             render_kwargs_test.get("far", 1.))


def _camera_code_setter(args, render_kwargs_test, embedcam_fn, dev, optimise=None):
    """The evaluation loops' camera code of view img_idx (run_nerf_sample_based_depth.py:384-395, 458-469): with
    args.input_ch_cam > 0, embedcam_fn(i), or zeros when embedcam_fn is None, set in render_kwargs_test["embedded_cam"];
    optimise(img_idx) (_test_time_optimizer) then replaces the zeros by the view's optimised code."""
    def set_camera_code(img_idx):
        if getattr(args, "input_ch_cam", 0) > 0:
            render_kwargs_test["embedded_cam"] = (torch.zeros((args.input_ch_cam,), device=dev) if embedcam_fn is None
                                                  else embedcam_fn(torch.tensor(img_idx, device=dev)))
            if optimise is not None and embedcam_fn is None:
                optimise(img_idx)
    return set_camera_code


def _test_time_optimizer(with_test_time_optimization, args, render_kwargs_test, embedcam_fn, images, poses, intrinsics, H, W):
    """with_test_time_optimization of the two evaluation loops (:384-389, :458-463): None without the flag, else
    optimise(img_idx), which leaves the view's optimised code in render_kwargs_test["embedded_cam"].  One
    camcode.CameraCodeOptimizer serves all views where the cached route takes the configuration; elsewhere each view runs
    the plain route.  (The reference also writes the code to test_latent_codes_<scene>/<i>.txt; that stays with the caller.)"""
    if not with_test_time_optimization:
        return None
    if getattr(args, "input_ch_cam", 0) < 1:
        raise NotImplementedError("with_test_time_optimization: args.input_ch_cam is 0, there is no code to optimise")
    from . import camcode
    fast = []

    def optimise(img_idx):
        if not fast:
            ok = camcode.CameraCodeOptimizer.unsupported_reason(render_kwargs_test, args, H, W, 32 << 30) is None
            fast.append(camcode.CameraCodeOptimizer(render_kwargs_test, H, W, args) if ok else None)
        camcode.optimize_camera_embedding(images[img_idx], poses[img_idx, :3, :4], H, W, intrinsics[img_idx, :], args,
                                          render_kwargs_test, optimizer=fast[0], route="auto" if fast[0] else "plain")
    return optimise


def test_images_samples(count, indices, images, depths, valid_depths, poses, H, W, intrinsics, lpips_alex, args,
                        render_kwargs_test, embedcam_fn=None, with_test_time_optimization=False, *, one_call=False):
    """run_nerf_sample_based_depth.py:349-421 (`--task test_samples_error`): how close the importance samples land to
    the rendered surface.  For each of `count` views of `indices` (all of them in order for None, else
    np.random.choice(indices, count, replace=False)), rendered under no_grad with the per-view intrinsics[i] =
    (fx, fy, cx, cy) and camera code (as render_images_with_metrics sets it), the mean over the pixels where
    valid_depths[i] [H,W] is set of mean_k |pred_hyp - depth_map|.  Returns a MeanTracker of "importance_sampling_error",
    one add per view whose mean is not NaN (a view without a valid pixel adds nothing).

    The frame is rendered in args.chunk-ray chunks with get_rays and render; each chunk's hypotheses are scored on the
    device by plnerf_sample_error as soon as they exist (added to the view's fp64 row) and dropped, so no [H,W,N]
    hypothesis plane is ever held.  The rows are read back once, after the last view; the means are fp64 (the
    reference's are fp32).  images, depths and lpips_alex are accepted and unused, as there; the reference's
    metrics_depth_samples.txt is MeanTracker.print(f) on the caller's side.  with_test_time_optimization: as
    render_images_with_metrics (`images` is read then: the optimisation's targets).

    one_call: each view is ONE library call (depthview.DepthViewRenderer, blocks of args.chunk) that scores every block's
    hypotheses while they are in its workspace -- the same blocks added in the same order, so the same rows -- and no
    hypotheses reach Python.  Only where the call serves the configuration and the kwargs ask for no draws (perturb 0, no
    density noise: the test-time settings); any other configuration takes the route above.  The poses and intrinsics are
    copied to the host once for all views."""
    optimise = _test_time_optimizer(with_test_time_optimization, args, render_kwargs_test, embedcam_fn, images, poses,
                                    intrinsics, H, W)
    dev = RB.default_device()
    count, img_i = _choose_views(count, indices)
    set_camera_code = _camera_code_setter(args, render_kwargs_test, embedcam_fn, dev, optimise)
    chunk, n_rays = args.chunk, H * W
    rows = torch.zeros(count, L.SAMPLEERR_ROW, dtype=torch.float64, device=dev)
    renderer = _view_renderer(render_kwargs_test, H, W, args) if one_call else None
    if renderer is None:
        workspace = torch.empty(L.sample_error_workspace_bytes(min(chunk, n_rays)), dtype=torch.uint8, device=dev)
    else:
        host_poses, host_intrinsics = _on_host(poses), _on_host(intrinsics)
    with torch.no_grad():
        for n, img_idx in enumerate(img_i):
            if renderer is not None:
                renderer.error_row.zero_()
                renderer.enqueue(host_poses[img_idx, :3, :4], host_intrinsics[img_idx, :], valid=valid_depths[img_idx])
                rows[n].copy_(renderer.error_row)
                continue
            set_camera_code(img_idx)
            intrinsic = intrinsics[img_idx, :]
            rays_o, rays_d = get_rays(H, W, intrinsic, poses[img_idx, :3, :4])
            rays_o, rays_d = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)
            valid = torch.as_tensor(valid_depths[img_idx]).to(device=dev, dtype=torch.bool).reshape(-1)
            for first in range(0, n_rays, chunk):
                last = min(first + chunk, n_rays)
                rays = torch.stack([rays_o[first:last], rays_d[first:last]])
                _, _, _, extras = render(H, W, intrinsic, chunk=chunk, rays=rays, **render_kwargs_test)
                sample_error_rows(extras['pred_hyp'].contiguous(), extras['depth_map'].contiguous(), valid[first:last],
                                  out=rows[n], workspace=workspace, accumulate=True)
                del extras
    _check_range(render_kwargs_test)
    if renderer is not None:
        renderer.check_range()      # (its own packed buffers carry the status words of its frames)

    mean_depth_metrics = MeanTracker()
    for total, counted in rows.cpu().tolist():
        error = total / counted if counted > 0 else math.nan      # torch.mean of no pixel is NaN
        if not math.isnan(error):
            mean_depth_metrics.add({"importance_sampling_error": error})
    return mean_depth_metrics


class _SpaceCarvingFn(torch.autograd.Function):
    """compute_space_carving_loss on the GPU: plnerf_depth_loss's carving term and its gradient (the image terms of that
    launch run on a dummy pixel and are discarded)."""

    @staticmethod
    def forward(ctx, pred, target_h, mask, threshold, is_joint):
        # (a dummy image pair one apart: the discarded image term's psnr stays finite)
        dummy, other = pred.new_zeros(pred.shape[0], 3), pred.new_ones(pred.shape[0], 3)
        # weight 1: loss5[3] is the unweighted term, g_hyp its gradient
        loss5, _, _, g_hyp = Fn.depth_loss_and_grads(dummy, None, other, pred, target_h, 1.0, threshold=threshold, mask=mask,
                                                     is_joint=is_joint)
        ctx.g = g_hyp
        return loss5[3]

    @staticmethod
    def backward(ctx, g):
        return ctx.g * g, None, None, None, None


def compute_space_carving_loss(pred_depth, target_hypothesis, is_joint=False, mask=None, norm_p=2, threshold=0.0):
    """model/run_nerf_helpers.py:52-86.  pred_depth [n_rays, n_points]; target_hypothesis [n_hyp, n_rays, 1 or
    n_points]; returns the scalar loss, differentiable with respect to pred_depth.  The distance is a p-norm over a
    trailing axis of length ONE, i.e. |pred - target| for every p >= 1; the reductions (per ray: min over hypotheses,
    mean; is_joint: mean over rays, min over hypotheses per point, mean) run in plnerf_depth_loss."""
    if not norm_p >= 1:
        raise ValueError("norm_p must be >= 1 (the norm runs over an axis of length one: it is the absolute value)")
    if not pred_depth.is_cuda:
        raise RuntimeError(f"plnerf_amd: compute_space_carving_loss runs in plnerf_depth_loss and needs GPU tensors, got "
                           f"{pred_depth.device} (there is no CPU fallback)")
    return _SpaceCarvingFn.apply(pred_depth, target_hypothesis, mask, float(threshold), bool(is_joint))


def get_space_carving_idx(pred_depth, target_hypothesis, is_joint=False, mask=None, norm_p=2, threshold=0.0):
    """model/run_nerf_helpers.py:19-49: which hypothesis compute_space_carving_loss would pick, for the caller's
    hypothesis cache -- per ray and point [H, W, n_points], or (is_joint) the one index of the whole image repeated to
    [H, W, 1].  pred_depth [H, W, n_points]; target_hypothesis [n_hyp, H, W, 1].  (A data-pipeline helper, off the
    training step: a few torch reductions.)"""
    d = (pred_depth[None] - target_hypothesis).abs()                     # [n_hyp, H, W, n_points]
    if mask is not None:                                                  # one value per pixel, [H, W] or flat
        d = d * mask.reshape(1, pred_depth.shape[0], pred_depth.shape[1], 1)
    if threshold > 0:
        d = d.masked_fill(d < threshold, 0.0)
    if is_joint:
        best = d.flatten(1).mean(1).argmin()
        return best.expand(pred_depth.shape[0], pred_depth.shape[1], 1)
    return d.argmin(0)


def create_nerf(args, scene_render_params=None, device=None):
    """run_nerf_sample_based_depth.py:547-644: (render_kwargs_train, render_kwargs_test, start, grad_vars,
    optimizer).  One Adam over the parameters of both networks; no nn.DataParallel (ray shards go through
    dp.py instead, one process per GPU)."""
    device = RB.default_device(device)
    embed_fn, input_ch = get_embedder(args.multires, args.i_embed)
    embeddirs_fn, input_ch_views = (get_embedder(args.multires_views, args.i_embed) if args.use_viewdirs
                                    else (None, 0))

    def network(depth, width):
        return NeRF(D=depth, W=width, input_ch=input_ch, output_ch=5 if args.N_importance > 0 else 4, skips=[4],
                    input_ch_views=input_ch_views, input_ch_cam=getattr(args, "input_ch_cam", 0),
                    use_viewdirs=args.use_viewdirs, precision=getattr(args, "precision", "fp32"),
                    density_activation="softplus", dense_layer_init=True).to(device)
    model = network(args.netdepth, args.netwidth)
    model_fine = network(args.netdepth_fine, args.netwidth_fine) if args.N_importance > 0 else None
    _refuse_unsupported(model, model_fine)      # (at the boundary, not at the first query: render.create_nerf)
    grad_vars = list(model.parameters()) + (list(model_fine.parameters()) if model_fine is not None else [])
    box = (getattr(args, "bb_center", 0.0), getattr(args, "bb_scale", 1.0))

    def network_query_fn(inputs, viewdirs, embedded_cam, network_fn):
        return run_network(inputs, viewdirs, embedded_cam, network_fn, embed_fn=embed_fn, embeddirs_fn=embeddirs_fn,
                           bb_center=box[0], bb_scale=box[1], netchunk=getattr(args, "netchunk", 1024 * 64))
    # (what the query function encodes with and its bounding box: DepthTrainStep's one-call route asks, as train.TrainStep's)
    network_query_fn.embedders, network_query_fn.box = (embed_fn, embeddirs_fn), box
    # (optim.FlatAdam on the GPU: one launch per network's gradient buffer)
    half_range = device.type == "cuda" and getattr(args, "precision", "fp32") in L.GUARDED_PRECISIONS
    guarded = [n for n in (model, model_fine) if n is not None and n.is_supported()]      # (the layer-by-layer route is fp32: no word)
    extra = {"guards": guarded} if (half_range and guarded) else {}
    optimizer = (FlatAdam if device.type == "cuda" else torch.optim.Adam)(params=grad_vars, lr=args.lrate,
                                                                           betas=(0.9, 0.999), **extra)
    start = 0
    if not getattr(args, "no_reload", True) and os.path.isdir(os.path.join(getattr(args, "ckpt_dir", ""),
                                                                           getattr(args, "expname", ""))):
        found = [f for f in RB.checkpoint_candidates(args) if f.endswith('.tar')]
        if found:
            start = RB.restore_checkpoint(found[-1], device, model, model_fine, optimizer)
    render_kwargs_train = RB.base_render_kwargs(args, network_query_fn, model, model_fine,
                                                embedded_cam=torch.tensor((), device=device))
    render_kwargs_train.update(scene_render_params or {})
    render_kwargs_train['lindisp'] = getattr(args, "lindisp", False)
    return render_kwargs_train, RB.test_time_kwargs(render_kwargs_train, perturb=False), start, grad_vars, optimizer


class DepthViews:
    """The training views of the depth-supervised loop, resident on the device (run_nerf_sample_based_depth.py:1043-1068),
    and their per-step ray batch (plnerf_select_depth_rays): what get_ray_batch_from_one_image_hypothesis_idx (:960-1001)
    and :1111-1120 compute on the host from the full H x W ray grid, in one launch for the step's rays alone.

    images [V, H, W, 3]; poses [V, 3 or 4, 4] (camera to world); intrinsics [V, 4] = (fx, fy, cx, cy) per view;
    hypotheses [V, n_hyp, H, W] (a trailing axis of one allowed: the reference's [V, n_hyp, H, W, 1]; the gt-depth
    override of :1066-1068 is n_hyp = 1); valid: the space-carving mask, V * H * W values in any shape (gt_valid_depths
    [V, 1, H, W, 1] there), non-zero = valid, or None (every pixel); near, far: the ray bounds."""

    def __init__(self, images, poses, intrinsics, hypotheses, valid, near, far, device=None):
        dev = RB.default_device(device if device is not None else
                                (images.device if isinstance(images, torch.Tensor) and images.is_cuda else None))
        f32 = lambda t: torch.as_tensor(t).to(device=dev, dtype=torch.float32).contiguous()
        self.images = f32(images)
        if self.images.dim() != 4 or self.images.shape[-1] != 3:
            raise ValueError(f"images must be [V, H, W, 3], got {tuple(self.images.shape)}")
        V, H, W = self.images.shape[:3]
        self.poses = f32(poses)
        if self.poses.dim() != 3 or self.poses.shape[0] != V or self.poses.shape[1] not in (3, 4) or self.poses.shape[2] != 4:
            raise ValueError(f"poses must be [V, 3 or 4, 4], got {tuple(self.poses.shape)}")
        self.intrinsics = f32(intrinsics).reshape(V, -1)
        if self.intrinsics.shape[1] != 4:
            raise ValueError(f"intrinsics must be [V, 4] = (fx, fy, cx, cy), got {tuple(self.intrinsics.shape)}")
        hyp = f32(hypotheses)
        if hyp.dim() == 5 and hyp.shape[-1] == 1:
            hyp = hyp[..., 0]
        if hyp.dim() != 4 or hyp.shape[0] != V or tuple(hyp.shape[2:]) != (H, W):
            raise ValueError(f"hypotheses must be [V, n_hyp, H, W], got {tuple(torch.as_tensor(hypotheses).shape)}")
        self.hypotheses = hyp.contiguous()
        self.valid = None
        if valid is not None:
            v = torch.as_tensor(valid).to(dev)
            if v.numel() != V * H * W:
                raise ValueError(f"valid must hold V * H * W = {V * H * W} values, got {tuple(v.shape)}")
            self.valid = (v.reshape(V, H, W) != 0).to(torch.uint8).contiguous()
        self.n_views, self.H, self.W, self.n_hyp = V, H, W, hyp.shape[1]
        self.near, self.far, self.device = float(near), float(far), dev

    def select(self, view, step, R, ray_id0=0, scale=None, shift=None, seed=0, want_viewdirs=True, want_extras=False):
        """Rays ray_id0 .. ray_id0 + R - 1 of step `step`'s pixel sample of view `view` (a host integer: the reference's
        img_i), drawn without replacement by the keyed bijection of plnerf_select_rays (seed, step): distinct within the
        step, disjoint across ranks with disjoint id ranges.  scale, shift: the per-view DEPTH_SCALES / DEPTH_SHIFTS
        ([V] or [V, 1] fp32 on the device, read there), or None (1 and 0).
        Returns (RayColumns, target_s [R, 3], target_h [n_hyp, R, 1] = hyp * scale[view] + shift[view], mask [R] 0. / 1.);
        want_extras: also (hyp_raw [n_hyp, R, 1], pixels [R, 2] int32 (row, col))."""
        dev, R = self.device, int(R)
        o, d = torch.empty(R, 3, device=dev), torch.empty(R, 3, device=dev)
        vd = torch.empty(R, 3, device=dev) if want_viewdirs else None
        nr, fr = torch.empty(R, device=dev), torch.empty(R, device=dev)
        target = torch.empty(R, 3, device=dev)
        th, mask = torch.empty(self.n_hyp, R, 1, device=dev), torch.empty(R, device=dev)
        raw = torch.empty(self.n_hyp, R, 1, device=dev) if want_extras else None
        pix = torch.empty(R, 2, device=dev, dtype=torch.int32) if want_extras else None
        for name, t in (("scale", scale), ("shift", shift)):
            if t is not None and t.numel() != self.n_views:
                raise ValueError(f"{name} must hold one value per view ({self.n_views}), got {tuple(t.shape)}")
        L.check(L.lib().plnerf_select_depth_rays(
            self.n_views, int(view), self.H, self.W, self.n_hyp, L.dptr(self.images, "images"),
            L.dptr(self.hypotheses, "hypotheses"), L.dptr(self.valid, "valid", torch.uint8), L.dptr(self.poses, "poses"), self.poses.shape[1],
            L.dptr(self.intrinsics, "intrinsics"), L.dptr(None if scale is None else scale.detach(), "scale"),
            L.dptr(None if shift is None else shift.detach(), "shift"), self.near, self.far, int(seed), int(step),
            int(ray_id0), R, L.dptr(o), L.dptr(d), L.dptr(vd), L.dptr(nr), L.dptr(fr), L.dptr(target), L.dptr(th),
            L.dptr(mask), L.dptr(raw), L.dptr(pix, "pixels", torch.int32), L.stream()), "plnerf_select_depth_rays")
        cols = RB.RayColumns(o, d, nr, fr, vd)
        if want_extras:
            return cols, target, th, mask, raw, pix
        return cols, target, th, mask


def learning_rate(i, lrate, start_decay_lrate=400000, end_decay_lrate=500000):
    """The depth script's learning rate at iteration i (run_nerf_sample_based_depth.py:1105-1108):
    lrate * 0.1^((i - start) / (end - start)) for start < i <= end; None outside that window, where the loop leaves the
    optimizer's rate as it was (after the window: the last value written, lrate / 10)."""
    if i > start_decay_lrate and i <= end_decay_lrate:
        portion = (i - start_decay_lrate) / (end_decay_lrate - start_decay_lrate)
        return lrate * (0.1 ** portion)
    return None


def scaleshift_steps(i, warm_start_nerf, freeze_ss, space_carving_weight):
    """Whether iteration i steps the depth scale / shift Adam (:1142, 1159-1161): only the space-carving term reaches
    them, so before it first switches on (i > warm_start_nerf) their gradients are None and Adam skips them; from then on
    the term is on at every iteration and optimizer_ss steps while i < freeze_ss."""
    return space_carving_weight > 0. and i > warm_start_nerf and i < freeze_ss


def save_checkpoint(path, global_step, network_fn, network_fine, optimizer, depth_scales=None, depth_shifts=None):
    """The depth script's checkpoint dict (run_nerf_sample_based_depth.py:1168-1183): global_step, both networks, the one
    optimizer, and the per-view depth_scales / depth_shifts ([V, 1] fp32).  create_nerf's reload restores the step
    counter, the networks and the optimizer; like the reference it does NOT reload the scales and shifts (train_nerf
    re-initialises them from scale_init / shift_init): a resumed run that needs them reads the two keys itself."""
    d = {'global_step': global_step,
         'network_fn_state_dict': network_fn.state_dict(),
         'optimizer_state_dict': optimizer.state_dict()}
    if network_fine is not None:
        d['network_fine_state_dict'] = network_fine.state_dict()
    if depth_shifts is not None:
        d['depth_shifts'] = depth_shifts.detach().reshape(-1, 1).float().clone()
    if depth_scales is not None:
        d['depth_scales'] = depth_scales.detach().reshape(-1, 1).float().clone()
    torch.save(d, path)


class DepthTrainStep:
    """One iteration of the reference's depth-supervised loop (run_nerf_sample_based_depth.py:1126-1157):
    loss = mse(rgb) + space_carving_weight * space_carving(pred_hyp, target_h) + mse(rgb0); backward;
    clip_grad_value_(0.1); Adam.  `ray_batch` is the packed [R, 11] batch render_rays takes.

    step_view is the whole loop body from the view on (:1104-1161): learning-rate schedule, the step's rays of a
    DepthViews view, this call, and the per-view depth scale / shift Adam.  The iteration counter is the reference's
    i = start + 1, start + 2, ...: it keys the pixel sample and the draws, the schedule, warm_start_nerf and freeze_ss.

    one_call=True: step_view hands every step that qualifies (_one_call_ok) to the library as ONE call --
    plnerf_depth_train_step (include/plnerf_hip_depthstep.h) enqueues the launch sequence of the fused route of _step itself,
    bit for bit the same step, without the Python -> ctypes -> autograd round trips between the launches
    (stepplan.DepthStepPlan holds its buffers).  A step that does not qualify, and every __call__ on a caller-made batch,
    takes the existing route, silently; one_call_steps counts the ones that did.  Such a step returns (loss, img_loss,
    space_carving, out) with `out` holding rgb_map, rgb0, depth_map, depth0, acc_map, acc0, disp_map, disp0, pred_hyp, z_std,
    z_vals and z_vals0 as VIEWS of the plan's workspace -- valid until that plan's next step, like last_pixels; `raw`,
    `weights`, `weights0` and `u` are not provided on this route.  With one_call=True the depth scales' and shifts' Adam is
    plnerf_depth_ss_adam on EVERY step of this object, one-call or not (moments in a [2, V] pair the step owns: a mixed run
    has one arithmetic); with one_call=False it stays torch.optim.Adam.  Under data parallelism a qualifying step (not
    is_joint; train.ONE_CALL_DP) is two library calls around the gradient all-reduce (_run_plan) and counts the same."""

    def __init__(self, args, render_kwargs_train, optimizer, grad_vars, distributed=None, range_check_every=100, seed=0,
                 counter_rng=True, start=0, n_views=None, one_call=False, one_call_const=False):
        """counter_rng: the step's draws (stratified jitter, importance samples, the hypotheses' u) come from a
        functional.DrawSource keyed on (seed, step, GLOBAL ray id) and are generated inside the kernels that consume
        them -- a global batch gives the same step whether one rank renders it or N ranks a shard each, like
        train.TrainStep.  False: torch.rand, as the reference draws.
        start: create_nerf's restored step count (the next iteration is start + 1).  n_views: allocate the per-view
        depth scales / shifts now (else at the first step_view, from its DepthViews)."""
        from . import dp
        self.args, self.kw, self.optimizer, self.grad_vars = args, render_kwargs_train, optimizer, grad_vars
        self.global_step = int(start)
        self.seed = seed
        self.last_pixels = None      # step_view: this rank's pixels [R, 2] (row, col) of its last step
        # DEPTH_SCALES / DEPTH_SHIFTS [V, 1] and their own Adam (:1071-1082)
        self.depth_scales = self.depth_shifts = self.optimizer_ss = None
        self._ss_grad = None
        self.one_call = bool(one_call)
        self.one_call_steps = 0
        # one_call_const=True (on its own or beside one_call): a step that qualifies in every respect but renders in
        # piecewise-constant mode (kw["mode"] == "constant", N_samples >= 3) goes to plnerf_depth_train_step_const
        # (include/plnerf_hip_conststep.h) and counts in one_call_const_steps, never in one_call_steps.  Either switch moves
        # the scales' and shifts' Adam to plnerf_depth_ss_adam, as the class docstring says of one_call.
        self.one_call_const = bool(one_call_const)
        self.one_call_const_steps = 0
        self._plan = self._plan_key = None
        self._ss_m = self._ss_v = None      # one_call: the scale / shift Adam's moments [2, V] and its step count
        self._ss_steps = 0
        # the 16-bit modes guard their Adam steps with the networks' range status words; the host looks every
        # `range_check_every` steps, as train.TrainStep does (0: never -- the caller does)
        self.range_check_every = int(range_check_every)
        nets = self.nets = [n for n in (self.kw["network_fn"], self.kw.get("network_fine")) if n is not None]
        distributed = torch.distributed.is_initialized() if distributed is None else distributed
        self.bucket = None
        self.rank = torch.distributed.get_rank() if distributed else 0
        self.world = torch.distributed.get_world_size() if distributed else 1
        self.draws = Fn.DrawSource(seed=seed) if counter_rng else None
        # both networks' backward as one launch sequence, as train.TrainStep (train.backward_merged)
        self.merged_backward = os.environ.get("PLNERF_MERGED_BWD", "1") != "0"
        self.merged_steps = 0      # steps that took it (the rest went through torch.autograd.backward)
        if distributed and torch.distributed.get_world_size() > 1:
            dp.broadcast_parameters(nets)      # replicas start from rank 0's weights (see train.TrainStep)
            dp.broadcast_optimizer_state([optimizer])
            self.global_step = dp.broadcast_scalar(self.global_step, device=next(nets[0].parameters()).device)
            self.bucket = dp.GradientBucket(nets)
        if n_views is not None:
            self.init_depth_scale_shift(n_views, next(nets[0].parameters()).device)

    def init_depth_scale_shift(self, n_views, device):
        """DEPTH_SCALES = ones([V, 1]) * scale_init, DEPTH_SHIFTS = ones([V, 1]) * shift_init, leaf tensors, and their Adam
        at scaleshift_lr (:1071-1082; defaults 1.0, 0.0, 1e-6).  Identical on every rank: no broadcast."""
        a = self.args
        ones = torch.ones((int(n_views), 1), dtype=torch.float, device=device)
        self.depth_scales = (ones * getattr(a, "scale_init", 1.0)).requires_grad_(True)
        self.depth_shifts = (ones * getattr(a, "shift_init", 0.0)).requires_grad_(True)
        self._ss_grad = torch.zeros(2, int(n_views), device=device)
        if self.one_call or self.one_call_const:      # plnerf_depth_ss_adam: torch.optim.Adam's defaults, moments and step count kept here
            self.optimizer_ss = None
            self._ss_m, self._ss_v, self._ss_steps = torch.zeros_like(self._ss_grad), torch.zeros_like(self._ss_grad), 0
        else:
            self.optimizer_ss = torch.optim.Adam(params=(self.depth_scales, self.depth_shifts),
                                                 lr=getattr(a, "scaleshift_lr", 1e-6))

    def learning_rate(self, i=None):
        """The rate the schedule writes into every param group before iteration i (default: the next one,
        global_step + 1), or None where it leaves the rate alone (module function learning_rate)."""
        a = self.args
        i = self.global_step + 1 if i is None else i
        return learning_rate(i, a.lrate, getattr(a, "start_decay_lrate", 400000), getattr(a, "end_decay_lrate", 500000))

    def check_range(self):
        """As train.TrainStep.check_range: reconcile withheld steps, raise on a set range status word."""
        withheld = self.optimizer.withheld_steps() if hasattr(self.optimizer, "withheld_steps") else 0
        for net in self.nets:
            if getattr(net, "precision", None) in L.GUARDED_PRECISIONS and net.is_supported() and \
                    next(net.parameters()).is_cuda:
                net.check_range()
        if withheld and self.bucket is not None:
            raise FloatingPointError(
                f"plnerf_amd: {withheld} optimizer step(s) were withheld because another rank's forward left the "
                "IEEE-half range (that rank's check_range() says which network)")

    def step_view(self, views, img_i, n_rand=None):
        """The loop body from the drawn view on (run_nerf_sample_based_depth.py:1104-1161) for view `img_i` of `views` (a
        DepthViews; the caller draws img_i, as np.random.choice(i_train) there, the same on every rank): the learning-rate
        schedule written into every param group; this rank's n_rand rays (ray ids rank * n_rand ...) of the step's pixel
        sample with target_h = hyp * DEPTH_SCALES[img_i] + DEPTH_SHIFTS[img_i] (plnerf_select_depth_rays); the step of
        __call__; then, while scaleshift_steps(i, ...), the scale / shift gradient (plnerf_depth_scale_shift_grad, summed
        over the ranks and scaled by 1 / world like the networks') and their Adam step -- unclipped: clip_grad_value_
        applies to the networks only (:1156).  Returns what __call__ returns."""
        a = self.args
        n_rand = int(n_rand if n_rand is not None else a.N_rand)
        if self.depth_scales is None:
            self.init_depth_scale_shift(views.n_views, views.device)
        if self.depth_scales.shape[0] != views.n_views:
            raise ValueError(f"the depth scales hold {self.depth_scales.shape[0]} views, `views` {views.n_views}")
        i = self.global_step + 1
        lr = self.learning_rate(i)
        if lr is not None:      # train_utils/hyperparameter_update.py:3-5
            for group in self.optimizer.param_groups:
                group['lr'] = lr
        if self.one_call or self.one_call_const:
            done = self._step_view_one_call(views, img_i, n_rand, i)
            if done is not None:
                return done
        cols, target_s, target_h, mask, hyp_raw, pix = views.select(
            img_i, self.global_step, n_rand, ray_id0=self.rank * n_rand, scale=self.depth_scales, shift=self.depth_shifts,
            seed=self.seed, want_viewdirs=bool(self.kw.get("use_viewdirs", True)), want_extras=True)
        self.last_pixels = pix
        ss = None
        if scaleshift_steps(i, getattr(a, "warm_start_nerf", 0), getattr(a, "freeze_ss", 0),
                            getattr(a, "space_carving_weight", 0.)):
            ss = (int(img_i), hyp_raw)
        return self._step(cols, target_s, target_h, mask, None, False, ss)

    def _one_call_ok(self, views, n_rays):
        """Can this step go to the library as one call (plnerf_depth_train_step)?  What the entry enqueues is the fused route
        of _step with the merged backward: two native networks in one 16-bit guarded precision and with one density
        activation, piecewise-linear mode with importance sampling, counter-based draws, the kernels' own encoding on an
        identity bounding box, no camera code, a batch that fits one launch per network, nobody watching the stages
        (STAGE_TAP, functional.KERNEL_TIMER), not `pytest`, and one process -- or, with train.ONE_CALL_DP, a rank of a
        data-parallel run without is_joint (whose hypothesis choice needs a collective in the middle of the forward,
        functional.joint_choice): its step is then two library calls around the gradient exchange (_run_plan).  kw["mode"] == "constant" qualifies the same way for
        plnerf_depth_train_step_const when one_call_const is set (N_samples >= 3), piecewise-linear mode when one_call is.
        Returns the networks' input scale, or None."""
        kw = self.kw
        if not (self.merged_backward and self.draws is not None and len(self.nets) == 2):
            return None
        if self.bucket is not None:
            from . import train
            if not train.ONE_CALL_DP or getattr(self.args, "is_joint", False):
                return None
        if STAGE_TAP is not None or Fn.KERNEL_TIMER is not None or not FUSE_STAGES or not isinstance(views, DepthViews):
            return None
        S, N = int(kw.get("N_samples", 0)), int(kw.get("N_importance", 0))
        mode = kw.get("mode")
        if not ((mode == "linear" and self.one_call) or (mode == "constant" and self.one_call_const and S >= 3)):
            return None
        if kw.get("color_mode") not in ("midpoint", "left") or kw.get("pytest", False) or \
                not kw.get("use_viewdirs", False) or N < 1 or S < 2 or S + N > L.DEPTH_STEP_MAX_SAMPLES:
            return None
        if kw.get("precomputed_z_samples") is not None or kw.get("cached_u") is not None:
            return None
        cam = kw.get("embedded_cam")
        if cam is not None and cam.numel() > 0:
            return None
        if not 1 <= n_rays or n_rays * (S + N) > MAX_ROWS_PER_LAUNCH:
            return None
        qfn = kw.get("network_query_fn")
        emb, box = getattr(qfn, "embedders", None), getattr(qfn, "box", None)      # (create_nerf's query function says them)
        if emb is None or box is None:
            return None
        enc = _kernel_encoding(emb[0], emb[1], True)
        if enc is None or not _host_box(*box)[2]:
            return None
        fx, fd, scale = enc
        c, f = self.nets
        ok = c is not f and c.precision == f.precision and c.density_beta == f.density_beta and all(
            n.is_native() and n.precision in L.GUARDED_PRECISIONS and n.has_fused_encoding() and n.input_ch == 3 + 6 * fx
            and n.input_ch_views == 3 + 6 * fd and all(p.is_cuda and p.requires_grad and p.device == views.device
                                                       for p in n.param_list()) for n in (c, f))
        return scale if ok else None

    def _plan_for(self, views, max_rays, input_scale):
        """The DepthStepPlan of this configuration: the one in hand while it still describes the live buffers, else a new
        one (None: the optimizer is not a FlatAdam over exactly the two networks)."""
        from . import stepplan
        sharded = self.bucket is not None      # (a data-parallel plan is guarded by the reduced status tails)
        key = stepplan.depth_plan_key(self.args, self.kw, max_rays, views, self.seed) + (input_scale, sharded) + tuple(
            t.data_ptr() for t in (self.depth_scales, self.depth_shifts, self._ss_grad, self._ss_m, self._ss_v))
        plan = self._plan
        if plan is not None and key == self._plan_key and plan.current():
            return plan
        self._plan = self._plan_key = None
        if not stepplan.DepthStepPlan.supported(self.nets, self.optimizer):
            return None
        self._plan = stepplan.DepthStepPlan(self.args, self.kw, self.nets, self.optimizer, views, max_rays, self.seed,
                                            input_scale, self.depth_scales.detach(), self.depth_shifts.detach(), self._ss_grad,
                                            self._ss_m, self._ss_v, data_parallel=sharded)
        self._plan_key = key
        return self._plan

    def _run_plan(self, plan, *args, ss_step=False, **kw):
        """One step through `plan` (DepthStepPlan.run's arguments and return value).  One process: ONE library call.  A rank
        of a data-parallel run: the gradients' half; ONE in-place SUM all-reduce of the plan's gradient block (both
        networks' gradients and status tails; dp.GradientBucket.reduce_block) and, on a step of the scales and shifts, the
        small one of their gradient, as _scale_shift_grad issues it; then the optimizers' half with 1 / world inside the
        step kernels, guarded by the reduced tails -- what _step does on the Python-driven route."""
        if self.bucket is None:
            return plan.run(*args, ss_step=ss_step, **kw)
        loss5 = plan.run_grads(*args, ss_step=ss_step, **kw)
        ss_work = None
        if ss_step:
            ss_work = torch.distributed.all_reduce(self._ss_grad, op=torch.distributed.ReduceOp.SUM, group=self.bucket.group,
                                                   async_op=True)
        scale = self.bucket.reduce_block(plan.grad_block)
        if ss_work is not None:
            ss_work.wait()
        plan.apply(scale)
        return loss5

    def _step_view_one_call(self, views, img_i, n_rand, i):
        """step_view through plnerf_depth_train_step; None when the step does not qualify (nothing has happened then)."""
        input_scale = self._one_call_ok(views, n_rand)
        if input_scale is None or not 0 <= int(img_i) < views.n_views or self.rank * n_rand + n_rand > views.H * views.W:
            return None
        plan = self._plan_for(views, n_rand, input_scale)
        mode = self.kw["mode"]
        adam_step = plan.adam_step() if (plan is not None and mode in plan.modes) else None
        if adam_step is None:
            return None
        a = self.args
        weight, warm = getattr(a, "space_carving_weight", 0.), getattr(a, "warm_start_nerf", 0)
        ss_step = scaleshift_steps(i, warm, getattr(a, "freeze_ss", 0), weight)
        if ss_step:
            self._ss_steps += 1
        loss5 = self._run_plan(plan, int(img_i), n_rand, self.global_step, self.rank * n_rand,
                               self.optimizer.param_groups[0]['lr'], adam_step, weight > 0. and i > warm, ss_step=ss_step,
                               ss_lr=float(getattr(a, "scaleshift_lr", 1e-6)), ss_adam_step=self._ss_steps, mode=mode)
        self.last_pixels = plan.view_of("pixels", (n_rand, 2), torch.int32)
        self.global_step += 1
        if mode == "constant":
            self.one_call_const_steps += 1
        else:
            self.one_call_steps += 1
        if self.range_check_every and self.global_step % self.range_check_every == 0:
            self.check_range()
        return loss5[0], loss5[1], loss5[3], plan.outputs(n_rand)

    def __call__(self, ray_batch, target_s, target_h, space_carving_mask=None, cached_u=None, pytest=False):
        return self._step(ray_batch, target_s, target_h, space_carving_mask, cached_u, pytest)

    def _step(self, ray_batch, target_s, target_h, space_carving_mask, cached_u, pytest, ss=None):
        """__call__'s body; ss = (view, hyp_raw [n_hyp, R, 1]): also step the depth scales / shifts."""
        a = self.args
        ss_work = None
        kw = {k: v for k, v in self.kw.items() if k not in ("ndc", "near", "far")}
        prev = Fn.DRAWS
        if self.draws is not None and ray_batch.is_cuda:
            self.draws.step, self.draws.ray_id0 = self.global_step, self.rank * ray_batch.shape[0]
            Fn.set_draw_source(self.draws)
        tape = Fn.MlpTape() if self.merged_backward else None
        Fn.MLP_TAPE = tape
        try:
            out = render_rays(ray_batch, retraw=True, is_joint=getattr(a, "is_joint", False), cached_u=cached_u,
                              quad_solution_v2=getattr(a, "quad_solution_v2", False), pytest=pytest, **kw)
        finally:
            Fn.set_draw_source(prev)
            Fn.MLP_TAPE = None
        self.optimizer.zero_grad()
        carve = getattr(a, "space_carving_weight", 0.) > 0. and self.global_step + 1 > getattr(a, "warm_start_nerf", 0)
        rgb, rgb0 = out['rgb_map'], out.get('rgb0')
        fused = rgb.is_cuda and rgb.dim() == 2 and rgb.shape == target_s.shape
        if fused:
            # both image terms, the space-carving term and the three gradients in one launch (plnerf_depth_loss);
            # backward((rgb, rgb0, pred_hyp), (their gradients)) is loss.backward()
            hyp = out["pred_hyp"] if carve else None
            loss5, g_rgb, g_rgb0, g_hyp, choice = Fn.depth_loss_and_grads(
                rgb, rgb0, target_s, hyp, target_h if carve else None, getattr(a, "space_carving_weight", 0.),
                threshold=getattr(a, "space_carving_threshold", 0.0), mask=space_carving_mask if carve else None,
                is_joint=getattr(a, "is_joint", False), sharded=self.bucket is not None,
                group=self.bucket.group if self.bucket is not None else None, want_choice=True)
            if ss is not None and carve:
                # d loss / d (DEPTH_SCALES, DEPTH_SHIFTS), dense over the views, from the hypotheses the loss chose; a
                # sharded batch sums them over the ranks in one small all-reduce, waited together with the networks'
                ss_work = self._scale_shift_grad(ss, hyp, target_h, space_carving_mask, choice)
            loss, img_loss, sc = loss5[0], loss5[1], loss5[3]
            roots = [(rgb, g_rgb)] + ([(rgb0, g_rgb0)] if rgb0 is not None else []) + ([(hyp, g_hyp)] if carve else [])
            from .train import backward_merged, merged_backward_ok
            if tape is not None and rgb0 is not None and merged_backward_ok(tape, self.nets):
                backward_merged(tape, self.nets, [r for r, _ in roots], [gr for _, gr in roots], self.bucket)
                self.merged_steps += 1
            else:
                torch.autograd.backward(tuple(r for r, _ in roots), tuple(gr for _, gr in roots))
        else:
            if ss is not None and carve:
                raise NotImplementedError("plnerf_amd: the depth scale / shift gradient needs the fused loss (CUDA tensors, "
                                          "rgb [R, 3])")
            img_loss = torch.mean((rgb - target_s) ** 2)
            loss = img_loss
            sc = torch.zeros((), device=ray_batch.device)
            if carve:
                if getattr(a, "is_joint", False) and self.bucket is not None:
                    # (is_joint chooses the hypothesis from the mean over the WHOLE batch: a rank's shard alone would choose
                    # its own -- the fused path adds the shards' column sums first, functional.joint_choice)
                    raise NotImplementedError("plnerf_amd: is_joint=True under data parallelism needs the fused loss "
                                              "(CUDA tensors, rgb [R, 3]); this call took the torch expressions")
                sc = compute_space_carving_loss(out["pred_hyp"], target_h, is_joint=getattr(a, "is_joint", False),
                                                norm_p=getattr(a, "norm_p", 2),
                                                threshold=getattr(a, "space_carving_threshold", 0.0),
                                                mask=space_carving_mask)
                loss = loss + a.space_carving_weight * sc
            if rgb0 is not None:
                loss = loss + torch.mean((rgb0 - target_s) ** 2)
            loss.backward()
        flat_adam = isinstance(self.optimizer, FlatAdam) and all(fl is not None for fl in self.optimizer._flat)
        scale, tails = 1.0, None
        if self.bucket is not None:
            # one wait for the two collectives; the 1 / world factor and the guard (the ranks' summed range status, which
            # travelled behind the gradients) go into the step kernel (dp.GradientBucket)
            scale = self.bucket.finish(defer_scale=flat_adam)
            tails = self.bucket.tails()
            tails = tails if len(tails) == len(self.nets) else None
        ss_step = ss is not None and carve
        if ss_step and ss_work is not None:
            ss_work.wait()
            if not (self.one_call or self.one_call_const):      # (plnerf_depth_ss_adam takes the factor as its grad_scale)
                self._ss_grad.mul_(1.0 / self.world)
        if flat_adam:
            # clip_grad_value_(0.1) folded into the step kernel (:1156), applied to the averaged gradient
            self.optimizer.step(clip_value=0.1, grad_scale=scale, guards=tails)
        elif isinstance(self.optimizer, FlatAdam):
            self.optimizer.step(clip_value=0.1)
        else:
            torch.nn.utils.clip_grad_value_(self.grad_vars, 0.1)
            self.optimizer.step()
        if ss_step and (self.one_call or self.one_call_const):
            self._ss_steps += 1
            L.check(L.lib().plnerf_depth_ss_adam(
                L.dptr(self.depth_scales.detach(), "depth_scales"), L.dptr(self.depth_shifts.detach(), "depth_shifts"),
                L.dptr(self._ss_grad), L.dptr(self._ss_m), L.dptr(self._ss_v), self._ss_grad.shape[1],
                float(getattr(a, "scaleshift_lr", 1e-6)), 0.9, 0.999, 1e-8, self._ss_steps,
                1.0 / self.world if ss_work is not None else 1.0, L.stream()), "plnerf_depth_ss_adam")
        elif ss_step:      # (:1159-1161: after the networks' step, no clipping)
            self.depth_scales.grad = self._ss_grad[0].reshape(-1, 1)
            self.depth_shifts.grad = self._ss_grad[1].reshape(-1, 1)
            self.optimizer_ss.step()
        self.global_step += 1
        if self.range_check_every and self.global_step % self.range_check_every == 0:
            self.check_range()
        return loss.detach(), img_loss.detach(), sc.detach(), out

    def _scale_shift_grad(self, ss, pred_hyp, target_h, mask, choice):
        """Writes this rank's d loss / d (scales, shifts) into self._ss_grad [2, V]; returns the pending all-reduce (SUM)
        of a sharded batch, or None."""
        view, hyp_raw = ss
        a = self.args
        Fn.depth_scale_shift_grad(pred_hyp, target_h, hyp_raw, getattr(a, "space_carving_weight", 0.), view,
                                  self._ss_grad.shape[1], threshold=getattr(a, "space_carving_threshold", 0.0), mask=mask,
                                  is_joint=getattr(a, "is_joint", False), joint_choice=choice, out=self._ss_grad)
        if self.bucket is None:
            return None
        return torch.distributed.all_reduce(self._ss_grad, op=torch.distributed.ReduceOp.SUM, group=self.bucket.group,
                                            async_op=True)
