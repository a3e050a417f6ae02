"""Piecewise-constant mode's one-launch stages against the separate launches they replace.

(a) kernel level: plnerf_coarse_epilogue_const (draws made in the kernel) against the Python-level chain it replaces, timed on
    the stream with its torch operations -- plnerf_quad_fwd, plnerf_uniform, z_mid, the weights' slice, plnerf_sample_const,
    plnerf_merge_sort, clamp + torch.std, plnerf_ray_points -- at R in {1024, 4096, 32768} x (64, 128), (128, 64);
    algorithmic bytes / time next to the 6.29 TB/s copy rate.
(b) step level: TrainStep.step_view in constant mode (the vanilla-NeRF settings, f16x3) at 1024 and 4096 rays with
    render.FUSE_CONST_EPILOGUE on against off, and DepthTrainStep at 64 + 128 constant with depth.FUSE_STAGES on against off;
    a second off arm gives the A/A spread.
HIP events; 5 warm-up + `--reps` calls (or `--steps` steps) per timing, the arms interleaved, 3 repeats: median [min - max].
Prints one JSON line.
    python tools/bench_const_epilogue.py [--reps 200] [--steps 20] [--skip-steps] [--out FILE]"""
import argparse, json, os, statistics, sys, tempfile
from argparse import Namespace
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import plnerf_amd as P
from plnerf_amd import depth as Dp
from plnerf_amd import functional as Fn

HBM_TBPS = 6.29      # MI355X measured copy rate (float4 copy), the roofline's bandwidth
WARMUP, REPEATS = 5, 3

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200, help="calls per kernel-level timing")
ap.add_argument("--steps", type=int, default=20, help="steps per step-level timing")
ap.add_argument("--skip-steps", action="store_true", help="kernel level only")
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_const_epilogue.py measures on the GPU; none is visible")
dev = torch.device("cuda:0")
Rd = sys.modules["plnerf_amd.render"]      # (the package attribute `render` is the function)


def timed(fn, n):
    s_ev, e_ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s_ev.record()
    for _ in range(n):
        fn()
    e_ev.record()
    torch.cuda.synchronize()
    return s_ev.elapsed_time(e_ev) * 1e3 / n      # us per call


def interleaved(arms, n):
    """{name: callable} -> {name: {"median", "min", "max", "all"}} in us per call; every repeat visits every arm."""
    times = {k: [] for k in arms}
    for fn in arms.values():
        timed(fn, WARMUP)
    for _ in range(REPEATS):
        for k, fn in arms.items():
            times[k].append(timed(fn, n))
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v} for k, v in times.items()}


# ---- (a) the coarse entry against the chain it replaces
kernel = {}
for R in (1024, 4096, 32768):
    for S, N in ((64, 128), (128, 64)):
        g = torch.Generator(device=dev).manual_seed(R + S)
        raw = torch.randn(R, S, 4, device=dev, generator=g)
        raw[..., 3] = raw[..., 3] * 4.0 + 1.0
        z, _ = torch.sort(2.0 + 4.0 * torch.rand(R, S, device=dev, generator=g), -1)
        near, far = torch.full((R, 1), 2.0, device=dev), torch.full((R, 1), 6.0, device=dev)
        o, d = torch.randn(R, 3, device=dev, generator=g), torch.randn(R, 3, device=dev, generator=g)
        src = Fn.DrawSource(seed=1, ray_id0=0, step=3)

        def fused():
            return Fn.CoarseEpilogueFn.apply(raw, z, near, far, o, d, None, None, N, "midpoint", True, False, 1e-4, 1e-3, src,
                                             False, "constant")

        def separate():
            rgb, disp, acc, w, depth, _, _ = Fn.QuadratureFn.apply(raw, z, near, far, d, None, "constant", "midpoint", True, False)
            u = src.uniform(R, N, Fn.DrawSource.U, dev)
            zs = Fn.sample_const(.5 * (z[..., 1:] + z[..., :-1]), w[..., 1:-1], u)
            z_fine = Fn.merge_sort(z, zs, near, far)
            z_std = torch.std(torch.clamp(zs, near, far), dim=-1, unbiased=False)
            return rgb, disp, acc, depth, z_fine, Fn.ray_points(o, d, z_fine), z_std
        with torch.no_grad():
            same = all(torch.equal(x, y) for x, y in zip(fused()[:6], separate()[:6]))
            t = interleaved({"fused": fused, "separate": separate, "separate_again": separate}, a.reps)
        nbytes = R * (20 * S + 44 + 16 * (S + N) + 32)      # raw, z, near, far, o, d in; maps, z_fine, pts, z_std out
        kernel[f"{R}x{S}+{N}"] = {
            "fused_us": t["fused"], "separate_us": t["separate"], "separate_again_us": t["separate_again"],
            "speedup": t["separate"]["median"] / t["fused"]["median"], "outputs_bit_identical": same, "bytes": nbytes,
            "fused_tbps": nbytes / t["fused"]["median"] * 1e-6,
            "fused_frac_of_hbm": nbytes / (HBM_TBPS * 1e12) * 1e6 / t["fused"]["median"]}
        del raw, z, o, d

# ---- (b) the training steps
steps = {}
if not a.skip_steps:
    def nvs_step(R):
        d = tempfile.mkdtemp()
        os.makedirs(os.path.join(d, "exp"))
        args = Namespace(multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=128, N_samples=64, netdepth=8,
                         netwidth=256, netdepth_fine=8, netwidth_fine=256, netchunk=1 << 22, lrate=5e-4, coarse_lrate=5e-4,
                         ft_path=None, ckpt_dir=d, expname="exp", no_reload=True, perturb=1.0, white_bkgd=True,
                         raw_noise_std=0.0, mode="constant", color_mode="midpoint", dataset="blender", no_ndc=False,
                         lindisp=False, lrate_decay=250, constant_init=0, chunk=32768, precision="f16x3", N_rand=R)
        torch.manual_seed(0)
        kw, _, _, _, opt, opt_c = P.create_nerf(args, device=dev)
        return P.TrainStep(args, kw, opt, opt_c, distributed=False, seed=5, one_call=False, range_check_every=0)

    H = W = 100
    K = [[120.0, 0, W / 2], [0, 120.0, H / 2], [0, 0, 1]]
    pose = P.rays.pose_spherical(40.0, -30.0, 4.0)[:3, :4]
    image = torch.rand(H, W, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    for R in (1024, 4096):
        arms = {}
        for name, fuse in (("on", True), ("off", False), ("off_again", False)):
            ts = nvs_step(R)

            def one(ts=ts, fuse=fuse):
                Rd.FUSE_CONST_EPILOGUE = fuse
                try:
                    ts.step_view(H, W, K, pose, image, near=2.0, far=6.0, n_rand=R)
                finally:
                    Rd.FUSE_CONST_EPILOGUE = True
            arms[name] = one
        t = interleaved(arms, a.steps)
        steps[f"step_view_constant_64+128_{R}"] = dict(t, speedup=t["off"]["median"] / t["on"]["median"],
                                                       aa_spread=abs(t["off_again"]["median"] / t["off"]["median"] - 1.0))

    R = 4096
    batch, target, _ = P.rays.synthetic_blender_rays(R, seed=0, device="cpu")
    vd = batch[1] / batch[1].norm(dim=-1, keepdim=True)
    ray_batch = torch.cat([batch[0], batch[1], torch.full((R, 1), 2.0), torch.full((R, 1), 6.0), vd], -1).to(dev)
    target = target.to(dev)
    target_h = (2.0 + 4.0 * torch.rand(3, R, 1, generator=torch.Generator().manual_seed(0))).to(dev)
    arms = {}
    for name, fuse in (("on", True), ("off", False), ("off_again", False)):
        args = Namespace(multires=9, i_embed=0, use_viewdirs=True, multires_views=0, input_ch_cam=0, N_importance=128,
                         N_samples=64, netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, netchunk=1 << 22, lrate=5e-4,
                         perturb=1.0, white_bkgd=True, raw_noise_std=0.0, mode="constant", color_mode="midpoint", lindisp=False,
                         no_reload=True, space_carving_weight=0.007, warm_start_nerf=0, is_joint=False, norm_p=2,
                         space_carving_threshold=0.0, precision="f16x3")
        torch.manual_seed(0)
        kw, _, _, grad_vars, opt = Dp.create_nerf(args, device=dev)
        step = Dp.DepthTrainStep(args, kw, opt, grad_vars, distributed=False)

        def one(step=step, fuse=fuse):
            Dp.FUSE_STAGES = fuse
            try:
                step(ray_batch, target, target_h)
            finally:
                Dp.FUSE_STAGES = True
        arms[name] = one
    t = interleaved(arms, a.steps)
    steps[f"depth_step_constant_64+128_{R}"] = dict(t, speedup=t["off"]["median"] / t["on"]["median"],
                                                    aa_spread=abs(t["off_again"]["median"] / t["off"]["median"] - 1.0))

out = {"what": "piecewise-constant mode: plnerf_coarse_epilogue_const vs the separate launches (kernel level, us per call), and the "
               "constant-mode training steps with the one-launch stages on vs off (us per step)",
       "method": f"HIP events, {WARMUP} warm-up + {a.reps} calls / {a.steps} steps, arms interleaved, {REPEATS} repeats: "
                 "median / min / max; *_again = the same arm a second time (A/A)",
       "hbm_tbps": HBM_TBPS, "kernel": kernel, "steps": steps}
line = json.dumps(out)
print(line, flush=True)
if a.out:
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
