"""Test-time optimisation of a held-out view's camera code: optimize_camera_embedding of
depth_supervised_exps/run_nerf_sample_based_depth.py:311-347 (100 Adam iterations at lr 0.5 over every pixel of the view,
the networks frozen; ReduceLROnPlateau('max', 0.5, patience 3); the code of the best PSNR is kept).

Two routes:

  * plain -- the reference's loop on the package's autograd path: depth.render(rays=...) with a code that requires a
    gradient (functional.MlpFn returns d loss / d cam), torch.optim.Adam and torch's ReduceLROnPlateau.  100 forward and
    backward passes of both networks over every pixel.
  * fast (CameraCodeOptimizer) -- with perturb = 0 and no density noise the sample depths and the quadrature weights depend
    on densities only, and the code enters BEHIND the density head, as the last input columns of views_linears[0]
    (model/run_nerf_helpers.py:190-200).  So the depths, the weights, the trunk and the view layer's pre-activation without
    the code columns (A, netwidth / 2 floats per sample) are computed once per view, and an iteration is one streaming pass
    over A (plnerf_camcode_sweep) and one tiny launch for Adam, the scheduler and the best-code tracking
    (plnerf_camcode_update), all enqueued without a host round trip; one readback at the end.

The batches: the reference draws them with random_split from compute_samples_per_subset(H W, 2 N_rand)'s sizes.  Only the
SIZES enter the objective (ray i of a batch of n_b rays weighs 1 / (3 n_b): the sum of the batches' img2mse); both routes
here take consecutive pixels for a batch, not random_split's draw."""
import ctypes
import math

import torch

from . import _lib as L
from . import functional as Fn
from . import generic as G
from . import raybatch as RB
from .nerf import NeRF

N_ITERS, LR, FACTOR, PATIENCE = 100, 0.5, 0.5, 3      # :313-314, :327
BETAS, ADAM_EPS = (0.9, 0.999), 1e-8                  # torch.optim.Adam's defaults
TRUNK_ROWS = 1 << 18                                  # rows of one exact-fp32 trunk pass of the cache build


def compute_samples_per_subset(n, at_least):
    """What data/dataset_sampling.py:4-10 computes for n samples in subsets of at least `at_least`: (size of a normal
    subset, how many of them, how many subsets of one sample more)."""
    n_subsets = n // min(at_least, n)
    size = n // n_subsets
    larger = n % size
    return size, n_subsets - larger, larger


def batch_sizes(n_pix, n_rand):
    """The sizes create_random_subsets(range(n_pix), 2 n_rand) hands to random_split (data/dataset_sampling.py:12-16)."""
    per, normal, extra = compute_samples_per_subset(int(n_pix), 2 * int(n_rand))
    if normal < 0:
        raise ValueError(f"compute_samples_per_subset({n_pix}, {2 * n_rand}) asks for {normal} subsets of {per}: the "
                         "reference's random_split refuses these sizes too")
    return [per] * normal + [per + 1] * extra


def ray_weights(sizes, device=None):
    """lambda_i = 1 / (3 n_b) for the rays of consecutive batches of the given sizes: sum_i lambda_i |rgb_i - t_i|^2 is the sum
    of the batches' img2mse."""
    return torch.cat([torch.full((n,), 1.0 / (3.0 * n), dtype=torch.float32) for n in sizes]).to(device)


def coef_from_weights(weights, mode, color_mode):
    """The coefficient with which sample s enters its ray's colour, from raw2outputs' weights (:733-762): linear mode has
    S + 1 weights (the bins near, s_0, ..., s_{S-1}, far) for S samples,
      midpoint: rgb_mid = .5 (rgb_concat[1:] + rgb_concat[:-1]) with the first and last colour duplicated:
                c_s = .5 (w_s + w_{s+1}), the two ends taking the duplicate's half as well;
      left:     rgb_concat = [rgb_0, rgb_0, ..., rgb_{S-1}]: c_0 = w_0 + w_1, c_s = w_{s+1};
    constant mode: c_s = w_s."""
    if mode == "constant":
        return weights
    if mode != "linear" or color_mode not in ("midpoint", "left"):
        raise ValueError(f"no colour rule for mode {mode!r}, color_mode {color_mode!r}")
    if color_mode == "left":
        return torch.cat([weights[..., :1] + weights[..., 1:2], weights[..., 2:]], -1)
    c = 0.5 * (weights[..., :-1] + weights[..., 1:])
    c[..., 0] = c[..., 0] + 0.5 * weights[..., 0]
    c[..., -1] = c[..., -1] + 0.5 * weights[..., -1]
    return c


def _psnr(mse):
    """mse2psnr (model/run_nerf_helpers.py): -10 log(x) / log(10) in fp32."""
    mse = torch.as_tensor(mse, dtype=torch.float32)
    return -10.0 * torch.log(mse) / torch.log(torch.tensor([10.0]))[0]


def _final_net(kw):
    return kw.get("network_fine") if kw.get("network_fine") is not None else kw.get("network_fn")


_RENDER_ONLY = ("near", "far", "ndc", "use_viewdirs", "c2w_staticcam", "with_5_9", "rays_depth", "embedded_cam")


class CameraCodeOptimizer:
    """The fast route for one configuration (networks, sampling, view size); build(image, pose, intrinsic) caches a view,
    run() optimises its code.  The metric loops keep one object across their views."""

    @staticmethod
    def unsupported_reason(render_kwargs_test, args=None, H=None, W=None, cache_bytes_limit=None):
        """Why this configuration takes the plain route, or None."""
        kw = render_kwargs_test
        net = _final_net(kw)
        if not isinstance(net, NeRF) or not isinstance(kw.get("network_fn"), NeRF):
            return "the networks are not plnerf_amd.NeRF modules"
        if not net.use_viewdirs or net.input_ch_cam < 1:
            return "the final network takes no camera code"
        if not kw.get("use_viewdirs", False):
            return "the render does not pass view directions"
        if net.input_ch_cam > L.CAMCODE_MAX_CAM or net.W // 2 > L.CAMCODE_MAX_WIDTH:
            return (f"a code of {net.input_ch_cam} entries or a view layer of {net.W // 2} units is over the kernel's "
                    f"{L.CAMCODE_MAX_CAM} / {L.CAMCODE_MAX_WIDTH}")
        if not (net.is_supported() and kw["network_fn"].is_supported()):
            return "a network off the fused trunk"
        if len(net.views_linears) != 1:
            return "more than one view layer"
        if next(net.parameters()).device.type != "cuda":
            return "the networks are not on a GPU"
        if kw.get("pytest", False):
            return "pytest draws"
        if kw.get("c2w_staticcam") is not None:
            return "c2w_staticcam"
        if kw.get("perturb", 0.) > 0. or kw.get("raw_noise_std", 0.) > 0.:
            return "draws (perturb or raw_noise_std): the weights are not constants of the loop"
        if kw.get("mode") not in ("linear", "constant") or (kw.get("mode") == "linear" and
                                                            kw.get("color_mode") not in ("midpoint", "left")):
            return "no colour rule for this mode"
        query = kw.get("network_query_fn")
        if not hasattr(query, "embedders") or not hasattr(query, "box"):
            return "the query function does not say what it encodes with"
        from .depth import _kernel_encoding
        enc = _kernel_encoding(query.embedders[0], query.embedders[1], True)
        if enc is None or net.input_ch != 3 + 6 * enc[0] or net.input_ch_views != 3 + 6 * enc[1]:
            return "an encoding plnerf_embed_rows does not evaluate"
        rows = (kw.get("N_samples", 0) + kw.get("N_importance", 0))
        if not 1 <= rows <= L.CAMCODE_MAX_ROWS:
            return f"{rows} samples per ray are over the kernel's {L.CAMCODE_MAX_ROWS}"
        if H is not None and W is not None and cache_bytes_limit is not None:
            need = H * W * rows * (net.W // 2) * 4
            if need > cache_bytes_limit:
                return f"a cache of {need} bytes is over cache_bytes_limit = {cache_bytes_limit}"
        return None

    def __init__(self, render_kwargs_test, H, W, args, cache_bytes_limit=32 << 30):
        reason = self.unsupported_reason(render_kwargs_test, args, H, W, cache_bytes_limit)
        if reason is not None:
            raise NotImplementedError(f"plnerf_amd: the cached camera-code route does not serve this configuration: {reason}")
        self.kw, self.H, self.W, self.args = render_kwargs_test, int(H), int(W), args
        self.net = _final_net(render_kwargs_test)
        self.n_cam, self.width = self.net.input_ch_cam, self.net.W // 2
        self.rows_per_ray = render_kwargs_test["N_samples"] + render_kwargs_test.get("N_importance", 0)
        self.n_rays = self.H * self.W
        self.sizes = batch_sizes(self.n_rays, args.N_rand)
        self.dev = next(self.net.parameters()).device
        self.ray_weight = ray_weights(self.sizes, self.dev)
        nbytes = L.lib().plnerf_camcode_sweep_workspace_bytes(self.n_rays)
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        self.loss_sum = torch.zeros(1, dtype=torch.float64, device=self.dev)
        self.g_cam = torch.zeros(self.n_cam, dtype=torch.float32, device=self.dev)
        self.A = self.coef = self.z_vals = self.target = self.bkgd = None

    # ---- the cache
    def trunk(self, embedded):
        """One exact-fp32 pass of the final network over embedded rows [n, input_ch + input_ch_views] (no code columns),
        layer by layer through generic.linear (plnerf_gemm_f32): (density [n] after its activation, A [n, netwidth / 2] =
        views_linears[0] applied to [feature | direction encoding | 0 ... 0] without its ReLU)."""
        net = self.net
        xyz = embedded[:, :net.input_ch]
        act = xyz
        for depth, fc in enumerate(net.pts_linears):
            act = G.linear(act, fc, relu=True)
            if depth in net.skips:
                act = torch.cat((xyz, act), 1)
        sigma = G.linear(act, net.alpha_linear, relu=False)[:, 0]
        if net.density_activation == "softplus":
            sigma = torch.nn.functional.softplus(sigma, beta=10)
        side = embedded[:, net.input_ch:net.input_ch + net.input_ch_views]
        head = torch.cat((G.linear(act, net.feature_linear, relu=False), side, side.new_zeros(side.shape[0], self.n_cam)), 1)
        return sigma, G.linear(head, net.views_linears[0], relu=False)

    def cache_rays(self, rows):
        """(z_vals [R, S], coef [R, S], bkgd [R] or None, A [R S, width]) of packed ray rows [R, 11]: the coarse pass and the
        sampler exactly as depth.render runs them (their depths do not depend on the code), the trunk above on the final
        depths, the weights from the quadrature entry on its densities."""
        from . import depth as Dp
        kw = self.kw
        rr = {k: v for k, v in kw.items() if k not in _RENDER_ONLY}
        zero_cam = torch.zeros(self.n_cam, device=self.dev)
        z_vals = Dp.render_rays(rows, True, embedded_cam=zero_cam, **rr)["z_vals"].contiguous()
        R, S = z_vals.shape
        rays_o, rays_d, viewdirs = rows[:, 0:3].contiguous(), rows[:, 3:6].contiguous(), rows[:, 8:11].contiguous()
        near, far = rows[:, 6:7].contiguous(), rows[:, 7:8].contiguous()
        query = kw["network_query_fn"]
        fx, fd, scale = Dp._kernel_encoding(query.embedders[0], query.embedders[1], True)
        center, bscale, _ = Dp._host_box(*query.box)
        sigma = torch.empty(R, S, device=self.dev)
        A = torch.empty(R * S, self.width, device=self.dev)
        step = max(1, TRUNK_ROWS // S)
        for first in range(0, R, step):
            last = min(first + step, R)
            pts = Fn.ray_points(rays_o[first:last], rays_d[first:last], z_vals[first:last])
            emb = Fn.embed_rows(pts, viewdirs[first:last], None, fx, fd, input_scale=scale, bb_center=center, bb_scale=bscale)
            s, a = self.trunk(emb)
            sigma[first:last] = s.reshape(last - first, S)
            A[first * S:last * S] = a
        raw = torch.cat([sigma.new_zeros(R, S, 3), sigma[..., None]], -1)
        mode = kw["mode"]
        cm = kw["color_mode"] if mode == "linear" else "midpoint"
        white = bool(kw.get("white_bkgd", False))
        out = Fn.QuadratureFn.apply(raw, z_vals, near, far, rays_d, None, mode, cm, white, False)
        coef = coef_from_weights(out[3], mode, cm).contiguous()
        return z_vals, coef, (1.0 - out[2]) if white else None, A

    def build(self, image, pose, intrinsic):
        """Cache the view (under no_grad): A, coef, the target and the background term of every pixel, row-major."""
        from . import depth as Dp
        kw = self.kw
        with torch.no_grad():
            rays_o, rays_d = Dp.get_rays(self.H, self.W, intrinsic, pose)
            rows, _ = RB.pack_rays(rays_o, rays_d, kw.get("near", 0.), kw.get("far", 1.), [RB.unit_directions(rays_d)])
            chunk = max(1, int(getattr(self.args, "chunk", 1024 * 32)))
            parts = [self.cache_rays(rows[i:i + chunk]) for i in range(0, rows.shape[0], chunk)]
            cat = lambda k: parts[0][k] if len(parts) == 1 else torch.cat([p[k] for p in parts], 0)
            self.z_vals, self.coef, self.A = cat(0), cat(1).reshape(-1).contiguous(), cat(3)
            self.bkgd = None if parts[0][2] is None else cat(2).contiguous()
            self.target = torch.as_tensor(image).to(device=self.dev, dtype=torch.float32).reshape(-1, 3).contiguous()
        if self.target.shape[0] != self.n_rays:
            raise ValueError(f"the image holds {self.target.shape[0]} pixels, the view {self.n_rays}")
        return self

    # ---- the loop
    def _sweep(self, cam_ptr):
        net = self.net
        vw = net.views_linears[0].weight
        stride = vw.shape[1]
        w_cam = ctypes.c_void_p(L.dptr(vw, "views_linears.0.weight").value + 4 * (net.W + net.input_ch_views))
        L.check(L.lib().plnerf_camcode_sweep(
            L.dptr(self.A, "A"), L.dptr(self.coef, "coef"), self.n_rays * self.rows_per_ray, self.rows_per_ray, self.width,
            cam_ptr, self.n_cam, w_cam, stride, L.dptr(net.rgb_linear.weight, "rgb_linear.weight"),
            L.dptr(net.rgb_linear.bias, "rgb_linear.bias"), L.dptr(self.target, "target"), L.dptr(self.bkgd, "bkgd"),
            L.dptr(self.ray_weight, "ray_weight"), L.dptr(self.workspace, "workspace", torch.uint8), self.workspace.numel(),
            L.dptr(self.loss_sum, "loss_sum", torch.float64), L.dptr(self.g_cam, "g_cam"), L.stream()), "plnerf_camcode_sweep")

    def loss_and_grad(self, cam):
        """(L, dL / dcam) of the cached view at `cam` (synchronises: the A/B and test entry)."""
        cam = torch.as_tensor(cam, dtype=torch.float32).to(self.dev).contiguous()
        self._sweep(L.dptr(cam, "cam"))
        return float(self.loss_sum.cpu()[0]), self.g_cam.detach().clone()

    def run(self, n_iters=N_ITERS, lr=LR):
        """The iterations as sweep -> update pairs on the current stream, one readback at the end.  Returns the record:
        psnr (per iteration), lr (per iteration, as Adam used it), best_psnr, best_iter, best_cam, cam (the last code)."""
        if self.A is None:
            raise RuntimeError("build() caches a view first")
        host = L.CamcodeState(lr=float(lr), best=-math.inf, best_iter=-1)
        state = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(self.dev)
        psnr = torch.zeros(max(n_iters, 1), device=self.dev)
        lrs = torch.zeros(max(n_iters, 1), device=self.dev)
        sp = ctypes.c_void_p(state.data_ptr())
        for _ in range(n_iters):
            self._sweep(sp)      # (cam is the state's first field)
            L.check(L.lib().plnerf_camcode_update(sp, self.n_cam, L.dptr(self.loss_sum, "loss_sum", torch.float64),
                                                  L.dptr(self.g_cam, "g_cam"), len(self.sizes), BETAS[0], BETAS[1], ADAM_EPS,
                                                  FACTOR, PATIENCE, L.dptr(psnr), L.dptr(lrs), n_iters, L.stream()),
                    "plnerf_camcode_update")
        back = L.CamcodeState.from_buffer_copy(state.cpu().numpy().tobytes())
        n = self.n_cam
        return {"psnr": psnr[:n_iters].cpu().tolist(), "lr": lrs[:n_iters].cpu().tolist(), "best_psnr": float(back.max_psnr),
                "best_iter": int(back.best_iter), "best_cam": torch.tensor(list(back.best_cam)[:n], device=self.dev),
                "cam": torch.tensor(list(back.cam)[:n], device=self.dev), "route": "fast"}


def plain_loss_and_grad(cam, image, pose, H, W, intrinsic, args, render_kwargs_test):
    """(sum of the batches' img2mse, its gradient) at `cam` on the autograd path: the body of the reference's iteration
    (:328-339) over consecutive-pixel batches."""
    from . import depth as Dp
    from .train import img2mse
    dev = RB.default_device()
    kw = dict(render_kwargs_test)
    cam = torch.as_tensor(cam, dtype=torch.float32).to(dev).detach().clone().requires_grad_(True)
    kw["embedded_cam"] = cam
    with torch.no_grad():
        rays_o, rays_d = Dp.get_rays(H, W, intrinsic, pose)
        rays_o, rays_d = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)
        target = torch.as_tensor(image).to(device=dev, dtype=torch.float32).reshape(-1, 3)
    total, first = torch.zeros((), device=dev), 0
    with torch.enable_grad():
        for n in batch_sizes(H * W, args.N_rand):
            rays = torch.stack([rays_o[first:first + n], rays_d[first:first + n]], 0)
            rgb = Dp.render(H, W, None, chunk=args.chunk, rays=rays, **kw)[0]
            loss = img2mse(rgb, target[first:first + n])
            loss.backward()
            total += loss.detach()
            first += n
    return total, cam.grad.detach()


def _optimize_plain(image, pose, H, W, intrinsic, args, render_kwargs_test, n_iters, lr):
    dev = RB.default_device()
    n_batches = len(batch_sizes(H * W, args.N_rand))
    cam = torch.zeros(args.input_ch_cam, device=dev, requires_grad=True)
    optimizer = torch.optim.Adam(params=(cam,), lr=lr)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, 'max', factor=FACTOR, patience=PATIENCE)
    max_psnr, best, best_iter, history, lrs = 0.0, torch.zeros(args.input_ch_cam, device=dev), -1, [], []
    for i in range(n_iters):
        total, grad = plain_loss_and_grad(cam.detach(), image, pose, H, W, intrinsic, args, render_kwargs_test)
        cam.grad = grad
        lrs.append(optimizer.param_groups[0]["lr"])
        optimizer.step()
        psnr = float(_psnr(total.cpu() / n_batches))
        scheduler.step(psnr)
        history.append(psnr)
        # (the reference's quirk, :343-345: the code stored is the one after this iteration's step, one step ahead of the
        # code whose PSNR selected it)
        if psnr > max_psnr:
            max_psnr, best, best_iter = psnr, cam.detach().clone(), i
    return {"psnr": history, "lr": lrs, "best_psnr": max_psnr, "best_iter": best_iter, "best_cam": best,
            "cam": cam.detach().clone(), "route": "plain"}


def optimize_camera_embedding(image, pose, H, W, intrinsic, args, render_kwargs_test, *, n_iters=N_ITERS, lr=LR, route="auto",
                              cache_bytes_limit=32 << 30, optimizer=None):
    """run_nerf_sample_based_depth.py:311-347: on return render_kwargs_test["embedded_cam"] is the best code, detached.
    Returns the record {psnr, lr, best_psnr, best_iter, best_cam, cam, route}.  route: "auto" (fast where
    CameraCodeOptimizer.unsupported_reason is None), "fast" (raises where it is not), "plain".  optimizer: a
    CameraCodeOptimizer of this configuration to reuse (the metric loops keep one across their views)."""
    if route not in ("auto", "fast", "plain"):
        raise ValueError(f"route must be 'auto', 'fast' or 'plain', got {route!r}")
    if getattr(args, "input_ch_cam", 0) < 1:
        raise NotImplementedError("optimize_camera_embedding: args.input_ch_cam is 0, there is no code to optimise")
    if route != "plain":
        reason = None if optimizer is not None else CameraCodeOptimizer.unsupported_reason(render_kwargs_test, args, H, W,
                                                                                           cache_bytes_limit)
        if reason is None:
            fast = optimizer if optimizer is not None else CameraCodeOptimizer(render_kwargs_test, H, W, args, cache_bytes_limit)
            record = fast.build(image, pose, intrinsic).run(n_iters, lr)
            render_kwargs_test["embedded_cam"] = record["best_cam"]
            return record
        if route == "fast":
            raise NotImplementedError(f"plnerf_amd: the cached camera-code route does not serve this configuration: {reason}")
    record = _optimize_plain(image, pose, H, W, intrinsic, args, render_kwargs_test, n_iters, lr)
    render_kwargs_test["embedded_cam"] = record["best_cam"]
    return record
