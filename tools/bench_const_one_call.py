"""A/B of the two routes of the piecewise-constant training step, and of the one kernel they needed.

  nvs     TrainStep(one_call_const=True) -- every step one plnerf_train_step_const call -- against the Python route
          (one_call_const=False: the same kernels reached through Python, ctypes and torch.autograd), mode = "constant", f16x3,
          bench.py's synthetic Blender scene at 4096 rays x (64 + 128) samples, step_view.
  depth   DepthTrainStep likewise (plnerf_depth_train_step_const), the benchmark's depth shape: 4096 rays x (128 + 64), three
          hypotheses, the space-carving term on, the scales and shifts stepping (tools/bench_depth_one_call.py's views).
  kernel  plnerf_fine_epilogue_const_bwd against the sequence it replaces (the contiguous copy of weights[:, 1:-1],
          plnerf_sample_const_bwd, the zero fill, the slice assignment, plnerf_quad_bwd in constant mode) at the depth step's
          shape (R = 4096, S = 192, N = 64), HIP events around --kernel-iters back-to-back repetitions.

Each arm has its own networks and optimizers (same initial weights); the arms alternate A / B / A / B within one process, and
every leg measures, after its warm-up, ms_per_step (HIP events around --steps steps) and host_ms_per_step (the wall time of an
enqueue loop of --host-steps steps with the stream left to run, started on an idle device and kept shorter than the launch
queue: tools/bench_one_call.py).  Min, median and max over the legs are reported per arm with `aa_spread` = (max - min) /
median over the Python route's (the separate sequence's) own legs: a difference between the arms inside it is no difference.
One JSON line per section, then one summary line; --out writes them all as one JSON document.  Run it as one GPU step under
its own time limit:

    timeout -k 10 600 python tools/bench_const_one_call.py --out profiles/const_one_call.json && ...
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import bench
import plnerf_amd as P
from plnerf_amd import _lib as L
from plnerf_amd import depth
from tools.bench_depth_one_call import make_views


def stats(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v), "all": [round(x, 5) for x in v]}


def spread(s):
    return (s["max"] - s["min"]) / s["median"]


def nvs_trainer(n_rand, ns, ni, dev, one_call_const):
    ck = tempfile.mkdtemp()
    os.makedirs(os.path.join(ck, "exp"))
    args = bench.make_args(argparse.Namespace(workload="blender_64_128", n_samples=ns, n_importance=ni, rays=n_rand), ck, "f16x3")
    args.mode = "constant"
    torch.manual_seed(0)
    _stdout = sys.stdout
    sys.stdout = open(os.devnull, "w")
    try:
        kw, _, _, _, opt, opt_c = P.create_nerf(args, device=dev)
    finally:
        sys.stdout = _stdout
    return P.TrainStep(args, kw, opt, opt_c, distributed=False, seed=0, one_call_const=one_call_const)


def depth_trainer(n_rand, ns, ni, dev, one_call_const):
    args = argparse.Namespace(
        multires=9, i_embed=0, use_viewdirs=True, multires_views=0, input_ch_cam=0, N_importance=ni, N_samples=ns, netdepth=8,
        netwidth=256, netdepth_fine=8, netwidth_fine=256, netchunk=65536, lrate=5e-4, perturb=1.0, white_bkgd=False,
        raw_noise_std=0.0, mode="constant", color_mode="midpoint", lindisp=False, no_reload=True, space_carving_weight=0.007,
        warm_start_nerf=0, is_joint=False, norm_p=2, space_carving_threshold=0.0, precision="f16x3", bb_center=0.0,
        bb_scale=1.0, N_rand=n_rand, freeze_ss=10 ** 9, scaleshift_lr=1e-6)
    torch.manual_seed(0)
    kw, _, _, grad_vars, opt = depth.create_nerf(args, device=dev)
    return depth.DepthTrainStep(args, kw, opt, grad_vars, distributed=False, seed=0, one_call_const=one_call_const)


def ab_steps(arms, step, a):
    """Alternate the arms' legs; returns (device ms per step, host ms per step) per arm."""
    dev_ms, host_ms = {k: [] for k in arms}, {k: [] for k in arms}
    for _ in range(a.repeats):
        for name, ts in arms.items():
            for i in range(a.warmup):
                step(ts, i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.host_steps):
                step(ts, i)
            host = time.perf_counter() - t0      # (the enqueue loop alone: the stream is still running)
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for i in range(a.steps):
                loss = step(ts, i)[0]
            e.record()
            torch.cuda.synchronize()
            assert torch.isfinite(loss), (name, float(loss))
            dev_ms[name].append(s.elapsed_time(e) / a.steps)
            host_ms[name].append(1e3 * host / a.host_steps)
    per_arm = a.repeats * (a.warmup + a.host_steps + a.steps)
    assert arms["one_call"].one_call_const_steps == per_arm and arms["python"].one_call_const_steps == 0
    return dev_ms, host_ms


def step_row(section, n_rand, ns, ni, dev_ms, host_ms, a):
    py, oc = stats(dev_ms["python"]), stats(dev_ms["one_call"])
    hpy, hoc = stats(host_ms["python"]), stats(host_ms["one_call"])
    return {"section": section, "mode": "constant", "n_rand": n_rand, "n_samples": ns, "n_importance": ni, "precision": "f16x3",
            "steps": a.steps, "host_steps": a.host_steps, "warmup": a.warmup, "repeats": a.repeats,
            "ms_per_step": {"python": py, "one_call": oc}, "host_ms_per_step": {"python": hpy, "one_call": hoc},
            "aa_spread": spread(py), "host_aa_spread": spread(hpy),
            "one_call_over_python": oc["median"] / py["median"], "host_one_call_over_python": hoc["median"] / hpy["median"],
            "one_call_slower_beyond_spread": oc["median"] / py["median"] - 1.0 > spread(py)}


def kernel_ab(a, dev):
    """The fused backward against the separate sequence, on the forward outputs of plnerf_fine_epilogue_const."""
    R, S, N = a.rays, a.depth_samples + a.depth_importance, a.depth_importance
    gen = torch.Generator().manual_seed(0)
    raw = torch.randn(R, S, 4, generator=gen)
    raw[..., 3] = raw[..., 3] * 4.0 + 1.0
    z, _ = torch.sort(2.0 + 4.0 * torch.rand(R, S, generator=gen), -1)
    t = lambda x: x.to(dev).contiguous()
    raw, z = t(raw), t(z)
    near, far, d = torch.full((R,), 2.0, device=dev), torch.full((R,), 6.0, device=dev), t(torch.randn(R, 3, generator=gen))
    u, g_rgb, g_hyp = t(torch.rand(R, N, generator=gen)), t(torch.randn(R, 3, generator=gen)), t(torch.randn(R, N, generator=gen))
    rgb = torch.empty(R, 3, device=dev)
    disp, acc, dep, z_std = (torch.empty(R, device=dev) for _ in range(4))
    w, bins = torch.empty(R, S, device=dev), torch.empty(R, S - 1, device=dev)
    hyp, inds = torch.empty(R, N, device=dev), torch.empty(R, N, device=dev, dtype=torch.int64)
    lib = L.lib()
    L.check(lib.plnerf_fine_epilogue_const(
        L.dptr(raw), L.dptr(z), L.dptr(near), L.dptr(far), L.dptr(d), None, L.dptr(u), N, 0, 0, 0, R, S, N, 0, L.dptr(rgb),
        L.dptr(disp), L.dptr(acc), L.dptr(dep), L.dptr(w), L.dptr(bins), L.dptr(hyp), L.dptr(inds, "inds", torch.int64), None,
        L.dptr(z_std), L.stream()), "plnerf_fine_epilogue_const")
    groups = (R + L.QUAD_RAYS_PER_GROUP - 1) // L.QUAD_RAYS_PER_GROUP
    g_raw, absmax = torch.empty(R, S, 4, device=dev), torch.empty(groups, device=dev, dtype=torch.int32)
    g_in = torch.empty(R, S - 2, device=dev)

    def separate():
        L.check(lib.plnerf_sample_const_bwd(L.dptr(bins), L.dptr(w[:, 1:-1].contiguous()), L.dptr(u), N,
                                            L.dptr(inds, "inds", torch.int64), L.dptr(g_hyp), R, S - 1, N, L.dptr(g_in),
                                            L.stream()), "plnerf_sample_const_bwd")
        g_s = torch.zeros(R, S, device=dev)
        g_s[:, 1:-1] = g_in
        L.check(lib.plnerf_quad_bwd(L.dptr(raw), L.dptr(z), L.dptr(near), L.dptr(far), L.dptr(d), None, R, S, L.MODE["constant"],
                                    L.COLOR["midpoint"], 0, 0, L.dptr(g_rgb), None, None, L.dptr(g_s), None, None, L.dptr(g_raw),
                                    L.dptr(absmax, "absmax", torch.int32), L.stream()), "plnerf_quad_bwd")

    def fused():
        L.check(lib.plnerf_fine_epilogue_const_bwd(
            L.dptr(raw), L.dptr(z), L.dptr(near), L.dptr(far), L.dptr(d), None, L.dptr(w), L.dptr(bins), L.dptr(u), N,
            L.dptr(inds, "inds", torch.int64), R, S, N, 0, L.dptr(g_rgb), None, None, None, L.dptr(g_hyp), L.dptr(g_raw),
            L.dptr(absmax, "absmax", torch.int32), L.stream()), "plnerf_fine_epilogue_const_bwd")
    arms = {"separate": separate, "fused": fused}
    us = {k: [] for k in arms}
    for _ in range(a.repeats):
        for name, fn in arms.items():
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.kernel_iters):
                fn()
            e.record()
            torch.cuda.synchronize()
            us[name].append(1e3 * s.elapsed_time(e) / a.kernel_iters)
    sep, fus = stats(us["separate"]), stats(us["fused"])
    return {"section": "kernel", "R": R, "S": S, "N": N, "iters": a.kernel_iters, "repeats": a.repeats,
            "us_per_call": {"separate": sep, "fused": fus}, "aa_spread": spread(sep),
            "fused_over_separate": fus["median"] / sep["median"],
            "fused_slower_beyond_spread": fus["median"] / sep["median"] - 1.0 > spread(sep)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="nvs,depth,kernel")
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--nvs-samples", type=int, default=64)
    ap.add_argument("--nvs-importance", type=int, default=128)
    ap.add_argument("--depth-samples", type=int, default=128)
    ap.add_argument("--depth-importance", type=int, default=64)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--host-steps", type=int, default=30)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3, help="legs per arm (A / B alternate)")
    ap.add_argument("--out", default=None, help="write every row and the summary as one JSON document")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    sections = a.sections.split(",")
    if "nvs" in sections:
        scene = bench.Scene(P, "blender_64_128", a.views, dev)
        arms = {"python": nvs_trainer(a.rays, a.nvs_samples, a.nvs_importance, dev, False),
                "one_call": nvs_trainer(a.rays, a.nvs_samples, a.nvs_importance, dev, True)}
        step = lambda ts, i: ts.step_view(scene.H, scene.W, scene.K, scene.poses[i % a.views], scene.images[i % a.views],
                                          near=scene.near, far=scene.far, n_rand=a.rays)
        rows.append(step_row("nvs", a.rays, a.nvs_samples, a.nvs_importance, *ab_steps(arms, step, a), a))
        print(json.dumps(rows[-1]), flush=True)
        del arms
        torch.cuda.empty_cache()
    if "depth" in sections:
        views = make_views(a.views, 80, 96, 3, dev)
        arms = {"python": depth_trainer(a.rays, a.depth_samples, a.depth_importance, dev, False),
                "one_call": depth_trainer(a.rays, a.depth_samples, a.depth_importance, dev, True)}
        step = lambda ts, i: ts.step_view(views, i % a.views, a.rays)
        rows.append(step_row("depth", a.rays, a.depth_samples, a.depth_importance, *ab_steps(arms, step, a), a))
        print(json.dumps(rows[-1]), flush=True)
        del arms
        torch.cuda.empty_cache()
    if "kernel" in sections:
        rows.append(kernel_ab(a, dev))
        print(json.dumps(rows[-1]), flush=True)
    summary = {"tool": "bench_const_one_call", "device": torch.cuda.get_device_name(0),
               "ratios": {r["section"]: round(r.get("one_call_over_python", r.get("fused_over_separate")), 4) for r in rows},
               "slower_beyond_spread": {r["section"]: bool(r.get("one_call_slower_beyond_spread", r.get("fused_slower_beyond_spread")))
                                        for r in rows}}
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"summary": summary, "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
