"""The depth script's sampling-error evaluation (`--task test_samples_error`): plnerf_sample_error per call, and one
800x800 frame of the synthetic Blender camera ring through depth.test_images_samples against the reference-shaped route
(the whole frame rendered with depth.render, then run_nerf_sample_based_depth.py:396-405 in torch on [H,W,N] planes).

Kernel legs: HIP events over repeated calls on device-resident rays (depths in [2, 6), hypotheses around them, 70 % of
the rays valid), at 32,768 rays (a render chunk; its 8-17 MB stay in the Infinity Cache across calls) and at 640,000 rays
(a whole frame, 164-327 MB: past the Infinity Cache).  Frame legs: default-initialised networks (torch.manual_seed(0)),
time per frame (host clock around the call, which ends in a device read) and torch.cuda.max_memory_allocated over it.
Prints one JSON line.
    python tools/bench_sample_error.py [--precision f16x3] [--reps 200] [--frame-reps 2] [--out FILE]"""
import argparse, json, os, sys, time
from argparse import Namespace
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import plnerf_amd as P
from plnerf_amd import _lib as L
from plnerf_amd import depth as Dp

HBM_TBPS = 6.29      # MI355X measured copy rate (float4 copy), the roofline's bandwidth

ap = argparse.ArgumentParser()
ap.add_argument("--precision", default="f16x3", choices=["fp32", "bf16x3", "bf16", "f16x3", "f16"])
ap.add_argument("--reps", type=int, default=200, help="kernel calls per timing")
ap.add_argument("--frame-reps", type=int, default=2, help="timed frames per route (after one warm-up frame)")
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_sample_error.py measures on the GPU; none is visible")
dev = torch.device("cuda:0")
s_ev, e_ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

# ---- the kernel alone
kernel = {}
for R in (32768, 640000):
    for N in (64, 128):
        g = torch.Generator(device=dev).manual_seed(R + N)
        depth = torch.rand(R, device=dev, generator=g) * 4 + 2
        hyp = (depth[:, None] + torch.randn(R, N, device=dev, generator=g) * 0.5).contiguous()
        valid = torch.rand(R, device=dev, generator=g) < 0.7
        row = torch.empty(L.SAMPLEERR_ROW, dtype=torch.float64, device=dev)
        ws = torch.empty(L.sample_error_workspace_bytes(R), dtype=torch.uint8, device=dev)
        for _ in range(10):
            P.sample_error_rows(hyp, depth, valid, out=row, workspace=ws)
        torch.cuda.synchronize()
        s_ev.record()
        for _ in range(a.reps):
            P.sample_error_rows(hyp, depth, valid, out=row, workspace=ws)
        e_ev.record(); torch.cuda.synchronize()
        us = s_ev.elapsed_time(e_ev) * 1e3 / a.reps
        nbytes = R * (4 * N + 5)
        kernel[f"{R}x{N}"] = {"us": us, "bytes": nbytes, "tbps": nbytes / us * 1e-6,
                              "frac_of_hbm": nbytes / (HBM_TBPS * 1e12) * 1e6 / us}
        del hyp, depth, valid, ws

# ---- one 800x800 frame, both routes
H = W = 800
focal = 0.5 * W / np.tan(0.5 * 0.6911112)
intrinsics = torch.tensor([[focal, focal, 0.5 * W, 0.5 * H]] * 2, device=dev)
poses = torch.stack([P.rays.pose_spherical(th, -30.0, 4.0) for th in (0.0, 90.0)]).to(dev)
g = torch.Generator(device=dev).manual_seed(7)
valid = torch.rand(2, H, W, device=dev, generator=g) < 0.7
chunk = 32768


def reference_route(kw, i):
    """run_nerf_sample_based_depth.py:396-405 as written, on the whole frame's planes."""
    with torch.no_grad():
        _, _, _, extras = Dp.render(H, W, intrinsics[i], chunk=chunk, c2w=poses[i, :3, :4], **kw)
        repeated = extras['depth_map'].unsqueeze(-1).repeat(1, 1, extras["pred_hyp"].shape[-1])
        dists = torch.norm(extras["pred_hyp"].unsqueeze(-1) - repeated.unsqueeze(-1), p=2, dim=-1)
        depth_rmse = torch.mean(torch.mean(dists, axis=-1)[valid[i]])
        return depth_rmse.item()


frames = {}
for mode, n_samples, n_importance in (("linear", 128, 64), ("constant", 64, 128)):
    args = Namespace(multires=9, i_embed=0, use_viewdirs=True, multires_views=0, input_ch_cam=0,
                     N_importance=n_importance, N_samples=n_samples, netdepth=8, netwidth=256, netdepth_fine=8,
                     netwidth_fine=256, netchunk=65536, lrate=5e-4, perturb=1.0, white_bkgd=True, raw_noise_std=0.0,
                     mode=mode, color_mode="midpoint", lindisp=False, no_reload=True, precision=a.precision,
                     bb_center=0.0, bb_scale=1.0, chunk=chunk, dataset="scannet")
    torch.manual_seed(0)
    _, kw, _, _, _ = Dp.create_nerf(args, device=dev)
    kw.update(near=2.0, far=6.0)
    leg = {}
    for route in ("test_images_samples", "reference_shaped"):
        def run(i):
            if route == "test_images_samples":
                return Dp.test_images_samples(None, [i], None, None, valid, poses, H, W, intrinsics, None, args,
                                              kw).get("importance_sampling_error")
            return reference_route(kw, i)
        run(1)                                               # warm-up (and the other view's value)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        times, value = [], None
        for _ in range(a.frame_reps):
            t0 = time.perf_counter()
            value = run(0)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        leg[route] = {"ms": 1e3 * min(times), "ms_all": [1e3 * t for t in times], "value": value,
                      "peak_mb": (torch.cuda.max_memory_allocated() - base) / 2 ** 20}
    leg["value_rel_diff"] = abs(leg["test_images_samples"]["value"] - leg["reference_shaped"]["value"]) / \
        abs(leg["reference_shaped"]["value"])
    frames[f"{mode}_{n_samples}_{n_importance}"] = leg
    del kw

out = {"what": "importance-sampling error (test_samples_error): plnerf_sample_error per call, and one 800x800 frame "
               "through test_images_samples vs the reference-shaped whole-frame route",
       "precision": a.precision, "chunk": chunk, "kernel": kernel, "hbm_tbps": HBM_TBPS,
       "frame": frames, "note": "peak_mb = torch.cuda.max_memory_allocated over the timed frames, above what was "
                                "allocated before them (networks, poses, masks)"}
line = json.dumps(out)
print(line, flush=True)
if a.out:
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
