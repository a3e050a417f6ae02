"""Held-out view evaluation of one 800x800 Blender-style frame (64 + 128 samples, f16x3): the render, the metrics kernel
(plnerf_eval_metrics: SSE of rgb and rgb0, SSIM, depth SSE, timed with HIP events over repeated calls), and, for
comparison, the host route the reference takes -- the frame and its target copied to the host, then SSIM in fp32
numpy / scipy (skimage 0.19's structural_similarity restated on scipy.ndimage.uniform_filter), host threads <= 16.
Prints one JSON line."""
import os
os.environ.setdefault("OMP_NUM_THREADS", "16")           # (before numpy: the host route's thread pools)
os.environ.setdefault("OPENBLAS_NUM_THREADS", "16")
import argparse, json, sys, tempfile, time
from argparse import Namespace
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from scipy.ndimage import uniform_filter
import plnerf_amd as P
from plnerf_amd import _lib as L

HBM_TBPS = 6.29      # MI355X measured copy rate (float4 copy), the roofline's bandwidth


def ssim_host_fp32(x, y):
    """skimage 0.19.3 structural_similarity(x, y, data_range=1, channel_axis=-1) on float32 inputs, as it runs there:
    float32 uniform filters per channel, the mean over the interior in float64, then over the channels."""
    out = []
    for c in range(x.shape[-1]):
        a, b = x[..., c], y[..., c]
        ux, uy = uniform_filter(a, 7), uniform_filter(b, 7)
        uxx, uyy, uxy = uniform_filter(a * a, 7), uniform_filter(b * b, 7), uniform_filter(a * b, 7)
        cn = np.float32(49.0 / 48.0)
        vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
        C1, C2 = np.float32(1e-4), np.float32(9e-4)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        out.append(S[3:-3, 3:-3].mean(dtype=np.float64))
    return float(np.mean(out))


ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=3)
ap.add_argument("--reps", type=int, default=200, help="metrics-kernel calls per timing")
ap.add_argument("--host-reps", type=int, default=3)
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_eval.py measures on the GPU; none is visible")
dev = torch.device("cuda:0")
H = W = 800
focal = 0.5 * W / np.tan(0.5 * 0.6911112)
K = [[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]]
d = tempfile.mkdtemp(); os.makedirs(os.path.join(d, "exp"))
args = Namespace(multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=128, N_samples=64,
                 netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, netchunk=65536, lrate=5e-4,
                 coarse_lrate=5e-4, ft_path=None, ckpt_dir=d, expname="exp", no_reload=True, perturb=1.0,
                 white_bkgd=True, raw_noise_std=0.0, mode="linear", color_mode="midpoint", dataset="blender",
                 no_ndc=False, lindisp=False, precision="f16x3")
so = sys.stdout; sys.stdout = open(os.devnull, "w")
torch.manual_seed(0)
_, kw, _, _, _, _ = P.create_nerf(args, device=dev)
sys.stdout = so
kw.update(near=2.0, far=6.0)
poses = [P.rays.pose_spherical(th, -30.0, 4.0)[:3, :4].to(dev) for th in (0.0, 90.0, 180.0)]
chunk = 32768

with torch.no_grad():
    target = P.render(H, W, K, chunk=chunk, c2w=poses[2], **kw)[0].contiguous()      # (also the warm-up)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for f in range(a.frames):
        rgb, _, _, ex = P.render(H, W, K, chunk=chunk, c2w=poses[f % 2], **kw)
    e.record(); torch.cuda.synchronize()
    render_ms = s.elapsed_time(e) / a.frames
    rgb, rgb0, depth = rgb.contiguous(), ex["rgb0"].contiguous(), ex["depth_map"].contiguous()
    g = torch.Generator(device=dev).manual_seed(1)
    target_depth = (depth + 0.05 * torch.randn(depth.shape, device=dev, generator=g)).contiguous()
    valid = (torch.rand(depth.shape, device=dev, generator=g) < 0.7).contiguous()

    rows = torch.empty(1, L.EVAL_ROW, dtype=torch.float64, device=dev)
    ws = torch.empty(L.eval_workspace_bytes(1, H, W), dtype=torch.uint8, device=dev)
    legs = {"rgb+rgb0+depth": (rgb0, depth, target_depth, valid), "rgb": (None, None, None, None)}
    kernel_us = {}
    for name, (p0, dd, td, vv) in legs.items():
        for _ in range(10):
            P.metric_rows(rgb, target, p0, dd, td, vv, out=rows, workspace=ws)
        torch.cuda.synchronize()
        s.record()
        for _ in range(a.reps):
            P.metric_rows(rgb, target, p0, dd, td, vv, out=rows, workspace=ws)
        e.record(); torch.cuda.synchronize()
        kernel_us[name] = s.elapsed_time(e) * 1e3 / a.reps
    row = P.metric_rows(rgb, target, rgb0, depth, target_depth, valid).cpu().numpy()[0]

# the host route: the frame and its target to the host, SSIM there
host = []
for _ in range(a.host_reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x, y = rgb.clamp(0, 1).cpu().numpy(), target.cpu().numpy()
    t1 = time.perf_counter()
    ssim_h = ssim_host_fp32(x, y)
    t2 = time.perf_counter()
    host.append((t1 - t0, t2 - t1))
copy_ms = 1e3 * min(h[0] for h in host)
ssim_ms = 1e3 * min(h[1] for h in host)

bytes_full = H * W * (3 * 3 * 4 + 2 * 4 + 1)     # pred, target, pred0 fp32 x3; depth, target_depth fp32; valid u8
bytes_rgb = H * W * 2 * 3 * 4
out = {"what": "held-out view metrics of one 800x800 frame (64+128 samples, f16x3)", "render_ms": render_ms,
       "kernel_us": kernel_us,
       "roofline": {"bound": "hbm", "tbps": HBM_TBPS, "note": "input bytes / measured HBM rate vs HIP-event time per call",
                    "rgb+rgb0+depth": {"bytes": bytes_full, "us": bytes_full / (HBM_TBPS * 1e12) * 1e6,
                                       "frac": bytes_full / (HBM_TBPS * 1e12) * 1e6 / kernel_us["rgb+rgb0+depth"]},
                    "rgb": {"bytes": bytes_rgb, "us": bytes_rgb / (HBM_TBPS * 1e12) * 1e6,
                            "frac": bytes_rgb / (HBM_TBPS * 1e12) * 1e6 / kernel_us["rgb"]}},
       "host_route_ms": {"d2h_copy": copy_ms, "ssim_fp32_numpy_scipy": ssim_ms, "total": copy_ms + ssim_ms,
                         "threads": int(os.environ["OMP_NUM_THREADS"])},
       "ssim_kernel": float(row[L.EVAL_SSIM]), "ssim_host_fp32": ssim_h,
       "ssim_kernel_minus_host_fp32": float(row[L.EVAL_SSIM]) - ssim_h,
       "psnr": -10 * np.log10(row[L.EVAL_SSE_RGB] / (3 * H * W))}
line = json.dumps(out)
print(line, flush=True)
if a.out:
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
