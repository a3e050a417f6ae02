"""The camera-code objective and its update rule restated in torch on the CPU, in any dtype (fp64: the yardstick of
tests/test_camopt_host.py and tests/test_gpu_camcode.py), from the arrays of fixture g10_camera_code_opt.npz.

The scene is the one tests/golden/make_golden_camopt.py built for the reference: the closed-form depth weights of seeds 0
and 1 (sharpened) with the fixture's four extra view-layer columns, a 4 x 6 view, 8 + 8 samples, linear / midpoint, white
background.  Everything the code does not reach is evaluated once (cache): the coarse pass, the deterministic importance
samples, the final network's trunk, A = the view layer's pre-activation without the code columns, the weights and coef.
objective(cache, cam) is then the few lines of the issue's formula; torch.autograd gives its gradient."""
import math
import os

import numpy as np
import torch

from oracle import plnerf_oracle as orc

# The bounds of tests/test_camopt_host.py and tests/test_gpu_camcode.py against the fixture.  What fp32 against fp64 gives on
# this fixture's scene, measured with this restatement evaluated in both dtypes at the 100 recorded codes (errors over the
# largest recorded loss / gradient entry): loss 3.02e-4, gradient 2.53e-4.  (The fp32 and fp64 runs place the importance
# samples up to 1e-4 apart; the loss is a sum of squares of colour differences ~1e-2 of colours near 1.)  Factor 4: two
# summation orders meet.
LOSS_FP32_VS_FP64, GRAD_FP32_VS_FP64 = 3.02e-4, 2.53e-4
LOSS_BOUND, GRAD_BOUND = 4 * LOSS_FP32_VS_FP64, 4 * GRAD_FP32_VS_FP64
CODE_TOL = 2e-6      # tests/test_gpu_step.py's Adam tolerance

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g10_camera_code_opt.npz")


def fixture():
    return dict(np.load(GOLDEN))


def state_dicts(g, dtype=torch.float64):
    out = []
    for seed, key in ((0, "view_weight_extra_coarse"), (1, "view_weight_extra_fine")):
        sd = orc.closed_form_state_dict_depth(seed, sharpen=True)
        sd["views_linears.0.weight"] = torch.cat([sd["views_linears.0.weight"], torch.from_numpy(g[key])], 1)
        out.append({k: v.to(dtype) for k, v in sd.items()})
    return out


def ray_batch(g, dtype=torch.float64):
    """[H W, 11] rows of the view in the depth script's convention (model/run_nerf_helpers.py:243-263: pixel centres, a
    flipped image row), row-major."""
    H, W = int(g["H"]), int(g["W"])
    fx, fy, cx, cy = [float(v) for v in g["intrinsic"]]
    c2w = torch.from_numpy(g["pose"]).to(dtype)
    rows, cols = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    dirs = torch.stack([((cols + 0.5) - cx) / fx, (H - (rows + 0.5) - cy) / fy, -torch.ones_like(cols)], -1)
    rays_d = torch.sum(dirs[..., None, :] * c2w[:3, :3], -1).reshape(-1, 3)
    rays_o = c2w[:3, -1].expand(rays_d.shape)
    n = rays_d.shape[0]
    return torch.cat([rays_o, rays_d, torch.full((n, 1), float(g["near"]), dtype=dtype),
                      torch.full((n, 1), float(g["far"]), dtype=dtype), rays_d / rays_d.norm(dim=-1, keepdim=True)], -1)


def trunk(sd, embedded, n_cam):
    """oracle.nerf_mlp_depth split at the view layer: (density after softplus [n], A [n, W / 2] without the code columns)."""
    F = torch.nn.functional
    xyz_ch = sd["pts_linears.0.weight"].shape[1]
    enc_xyz, enc_dir = embedded[..., :xyz_ch], embedded[..., xyz_ch:]
    h = enc_xyz
    for i in range(orc.DEPTH):
        h = F.relu(F.linear(h, sd[f"pts_linears.{i}.weight"], sd[f"pts_linears.{i}.bias"]))
        if i == orc.SKIP_AFTER:
            h = torch.cat([enc_xyz, h], dim=-1)
    alpha = F.linear(h, sd["alpha_linear.weight"], sd["alpha_linear.bias"])
    feat = F.linear(h, sd["feature_linear.weight"], sd["feature_linear.bias"])
    vw = sd["views_linears.0.weight"]
    A = F.linear(torch.cat([feat, enc_dir], dim=-1), vw[:, :vw.shape[1] - n_cam], sd["views_linears.0.bias"])
    return F.softplus(alpha, beta=10)[..., 0], A


def coef_reference(weights, mode, color_mode):
    """c_s by raw2outputs' own expressions (run_nerf_sample_based_depth.py:733-762): the colour map is linear in the
    samples' colours, so c_s is what a one-hot colour at sample s renders to."""
    R, n = weights.shape
    S = n - 1 if mode == "linear" else n
    rgb = torch.eye(S, dtype=weights.dtype).expand(R, S, S)      # sample s has "colour" e_s
    if mode == "constant":
        return torch.sum(weights[..., None] * rgb, -2)
    if color_mode == "midpoint":      # both end colours doubled, then the mean of neighbours
        padded = torch.cat([rgb[:, :1], rgb, rgb[:, -1:]], 1)
        return torch.sum(weights[..., None] * (0.5 * (padded[:, 1:] + padded[:, :-1])), -2)
    return torch.sum(weights[..., None] * torch.cat([rgb[:, :1], rgb], 1), -2)      # left: the first colour doubled


def ray_weight(sizes, dtype=torch.float64):
    return torch.cat([torch.full((n,), 1.0 / (3.0 * n), dtype=dtype) for n in sizes])


def cache(g, dtype=torch.float64):
    """Everything the code does not reach, for the fixture's scene: dict(z, A [R, S, W/2], coef [R, S], bkgd [R], target,
    ray_weight, w_cam [W/2, n_cam], w_rgb, b_rgb, rows (the ray batch), weights)."""
    n_cam, NS, NI = int(g["n_cam"]), int(g["N_samples"]), int(g["N_importance"])
    sd_c, sd_f = state_dicts(g, dtype)
    rows = ray_batch(g, dtype)
    rays_o, rays_d, near, far, viewdirs = rows[:, 0:3], rows[:, 3:6], rows[:, 6:7], rows[:, 7:8], rows[:, 8:11]
    R = rows.shape[0]
    zero = torch.zeros(n_cam, dtype=dtype)
    t = torch.linspace(0.0, 1.0, NS).to(dtype)      # (the fp32 grid, as every route evaluates it)
    z = near * (1.0 - t) + far * t
    pts = rays_o[..., None, :] + rays_d[..., None, :] * z[..., :, None]
    raw = orc.query_network_depth(sd_c, pts, viewdirs, embedded_cam=zero)
    _, _, _, w, _, tau, T = orc.raw2outputs(raw, z, near, far, rays_d, "linear", "midpoint", 0.0, False, True)
    u = torch.linspace(0.0, 1.0, NI).to(dtype).expand(R, NI).contiguous()
    z_new = orc.sample_pdf_reformulation(z, w, tau, T, near, far, NI, u=u)[0]
    z, _ = torch.sort(torch.cat([z, torch.clamp(z_new, near, far)], -1), -1)
    S = z.shape[1]
    pts = rays_o[..., None, :] + rays_d[..., None, :] * z[..., :, None]
    emb = torch.cat([orc.positional_encoding_pi(pts.reshape(-1, 3), orc.DEPTH_XYZ_FREQS),
                     viewdirs[:, None, :].expand(R, S, 3).reshape(-1, 3)], -1)
    sigma, A = trunk(sd_f, emb, n_cam)
    raw = torch.cat([torch.zeros(R, S, 3, dtype=dtype), sigma.reshape(R, S, 1)], -1)
    _, _, acc, w, _, _, _ = orc.raw2outputs(raw, z, near, far, rays_d, "linear", "midpoint", 0.0, False, True)
    vw = sd_f["views_linears.0.weight"]
    H, W = int(g["H"]), int(g["W"])
    sizes = [H * W // int(g["n_batches"])] * int(g["n_batches"])
    return dict(z=z, A=A.reshape(R, S, -1), coef=coef_reference(w, "linear", "midpoint"), bkgd=1.0 - acc,
                target=torch.from_numpy(g["image"]).to(dtype).reshape(-1, 3), ray_weight=ray_weight(sizes, dtype),
                w_cam=vw[:, vw.shape[1] - n_cam:], w_rgb=sd_f["rgb_linear.weight"], b_rgb=sd_f["rgb_linear.bias"], rows=rows,
                weights=w)


def objective(A, coef, w_cam, w_rgb, b_rgb, target, bkgd, ray_weight, cam):
    """L(cam): A [R, S, width], coef [R, S], bkgd [R] or None."""
    z = A + w_cam @ cam
    rgb = torch.sigmoid(torch.relu(z) @ w_rgb.T + b_rgb)
    rgb_i = torch.sum(coef[..., None] * rgb, -2)
    if bkgd is not None:
        rgb_i = rgb_i + bkgd[:, None]
    return torch.sum(ray_weight[:, None] * (rgb_i - target) ** 2)


def loss_and_grad(c, cam):
    cam = torch.as_tensor(cam).to(c["A"].dtype).clone().requires_grad_(True)
    loss = objective(c["A"], c["coef"], c["w_cam"], c["w_rgb"], c["b_rgb"], c["target"], c["bkgd"], c["ray_weight"], cam)
    loss.backward()
    return loss.detach(), cam.grad.detach()


class Update:
    """One iteration's bookkeeping as run_nerf_sample_based_depth.py:340-345 orders it: torch.optim.Adam's step (fp32, the
    single-tensor formulas), mse2psnr in fp32, ReduceLROnPlateau('max', 0.5, patience 3; relative threshold 1e-4) in Python
    floats, and the reference's own tracking -- the stored code is the one AFTER the step."""

    def __init__(self, n_cam, n_batches, lr=0.5, betas=(0.9, 0.999), eps=1e-8, factor=0.5, patience=3):
        self.cam = torch.zeros(n_cam)
        self.m, self.v = torch.zeros(n_cam), torch.zeros(n_cam)
        self.lr, self.betas, self.eps, self.factor, self.patience = lr, betas, eps, factor, patience
        self.n_batches, self.t = n_batches, 0
        self.best, self.bad = -math.inf, 0
        self.max_psnr, self.best_cam, self.best_iter = 0.0, torch.zeros(n_cam), -1

    def step(self, grad, loss_sum):
        b1, b2 = self.betas
        g = torch.as_tensor(grad, dtype=torch.float32)
        self.t += 1
        self.m = self.m + (g - self.m) * (1 - b1)
        self.v = self.v * b2 + (1 - b2) * g * g
        bc1, bc2 = 1 - b1 ** self.t, 1 - b2 ** self.t
        self.cam = self.cam - (self.lr / bc1) * (self.m / (self.v.sqrt() / math.sqrt(bc2) + self.eps))
        mse = torch.as_tensor(loss_sum, dtype=torch.float32) / self.n_batches
        psnr = float(-10.0 * torch.log(mse) / torch.log(torch.tensor([10.0]))[0])
        if psnr > self.best * (1.0 + 1e-4):
            self.best, self.bad = psnr, 0
        else:
            self.bad += 1
        if self.bad > self.patience:
            new_lr = max(self.lr * self.factor, 0.0)
            if self.lr - new_lr > 1e-8:
                self.lr = new_lr
            self.bad = 0
        if psnr > self.max_psnr:
            self.max_psnr, self.best_cam, self.best_iter = psnr, self.cam.clone(), self.t - 1
        return psnr
