"""A/B of the two routes of the depth-supervised step: DepthTrainStep(one_call=True) -- every step_view one
plnerf_depth_train_step call -- against the existing route (one_call=False: its launches reached through Python, ctypes and
torch.autograd, the depth scales' torch.optim.Adam included), f16x3, at 256 / 1024 / 4096 rays with 64 + 128 and 128 + 64
samples, on synthetic device-resident views (random colours and hypotheses: the step's cost does not depend on them) with
the space-carving term on and the scales and shifts stepping (i < freeze_ss).  Each arm has its own networks and optimizer
(same initial weights); the arms alternate A / B / A / B within one process, and every leg measures, after its warm-up,

  ms_per_step       HIP events around --steps steps (the step as the GPU sees it), and
  host_ms_per_step  the wall time of an enqueue loop of --host-steps steps with the stream left to run, started on an idle
                    device and kept shorter than the launch queue (tools/bench_one_call.py).

Min, median and max over the legs are reported per arm and per cell with `aa_spread` = (max - min) / median over the
existing route's own legs, for the step and for the host time alike: a difference between the arms inside it is no
difference.  One JSON line per cell, then one summary line; --out writes them all as one JSON document
(profiles/r08_depth_one_call.json).  Run it as one GPU step under its own time limit:

    timeout -k 10 900 python tools/bench_depth_one_call.py --out profiles/r08_depth_one_call.json && ...
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import plnerf_amd as P
from plnerf_amd import depth


def make_views(n_views, H, W, n_hyp, dev):
    gen = torch.Generator().manual_seed(0)
    poses = torch.stack([P.rays.pose_spherical(-180.0 + 360.0 * i / n_views, -30.0, 4.0) for i in range(n_views)])
    intr = torch.tensor([[1.1 * W, 1.1 * W, 0.5 * W, 0.5 * H]] * n_views)
    images = torch.rand(n_views, H, W, 3, generator=gen)
    hyp = 2.0 + 4.0 * torch.rand(n_views, n_hyp, H, W, generator=gen)
    valid = torch.rand(n_views, H, W, generator=gen) > 0.3
    return depth.DepthViews(images.to(dev), poses.to(dev), intr.to(dev), hyp.to(dev), valid.to(dev), 2.0, 6.0)


def make_trainer(n_samples, n_importance, n_rand, dev, one_call):
    args = argparse.Namespace(
        multires=9, i_embed=0, use_viewdirs=True, multires_views=0, input_ch_cam=0, N_importance=n_importance,
        N_samples=n_samples, netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, netchunk=65536, lrate=5e-4,
        perturb=1.0, white_bkgd=False, raw_noise_std=0.0, mode="linear", color_mode="midpoint", lindisp=False, no_reload=True,
        space_carving_weight=0.007, warm_start_nerf=0, is_joint=False, norm_p=2, space_carving_threshold=0.0,
        precision="f16x3", bb_center=0.0, bb_scale=1.0, N_rand=n_rand, freeze_ss=10 ** 9, scaleshift_lr=1e-6)
    torch.manual_seed(0)
    kw, _, _, grad_vars, opt = depth.create_nerf(args, device=dev)
    return depth.DepthTrainStep(args, kw, opt, grad_vars, distributed=False, seed=0, one_call=one_call)


def stats(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v), "all": [round(x, 5) for x in v]}


def spread(s):
    return (s["max"] - s["min"]) / s["median"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="256:64:128,256:128:64,1024:64:128,1024:128:64,4096:64:128,4096:128:64",
                    help="rays:N_samples:N_importance, comma separated")
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--height", type=int, default=80)
    ap.add_argument("--width", type=int, default=96)
    ap.add_argument("--n-hyp", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--host-steps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3, help="legs per arm (A / B alternate)")
    ap.add_argument("--out", default=None, help="write every row and the summary as one JSON document")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    views = make_views(a.views, a.height, a.width, a.n_hyp, dev)
    rows = []
    for cell in a.cells.split(","):
        n_rand, ns, ni = (int(x) for x in cell.split(":"))
        arms = {"existing": make_trainer(ns, ni, n_rand, dev, False), "one_call": make_trainer(ns, ni, n_rand, dev, True)}
        dev_ms = {k: [] for k in arms}
        host_ms = {k: [] for k in arms}
        for rep in range(a.repeats):
            for name, ts in arms.items():
                for i in range(a.warmup):
                    ts.step_view(views, i % a.views, n_rand)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(a.host_steps):
                    ts.step_view(views, i % a.views, n_rand)
                host = time.perf_counter() - t0      # (the enqueue loop alone: the stream is still running)
                torch.cuda.synchronize()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for i in range(a.steps):
                    loss = ts.step_view(views, i % a.views, n_rand)[0]
                e.record()
                torch.cuda.synchronize()
                assert torch.isfinite(loss), (name, float(loss))
                dev_ms[name].append(s.elapsed_time(e) / a.steps)
                host_ms[name].append(1e3 * host / a.host_steps)
        assert arms["one_call"].one_call_steps == a.repeats * (a.warmup + a.host_steps + a.steps) and arms["existing"].one_call_steps == 0
        ex, oc = stats(dev_ms["existing"]), stats(dev_ms["one_call"])
        hex_, hoc = stats(host_ms["existing"]), stats(host_ms["one_call"])
        row = {"n_rand": n_rand, "n_samples": ns, "n_importance": ni, "precision": "f16x3", "n_hyp": a.n_hyp,
               "steps": a.steps, "host_steps": a.host_steps, "warmup": a.warmup, "repeats": a.repeats,
               "ms_per_step": {"existing": ex, "one_call": oc}, "host_ms_per_step": {"existing": hex_, "one_call": hoc},
               "aa_spread": spread(ex), "host_aa_spread": spread(hex_),
               "one_call_over_existing": oc["median"] / ex["median"], "host_one_call_over_existing": hoc["median"] / hex_["median"],
               "step_moved_beyond_spread": abs(oc["median"] / ex["median"] - 1.0) > spread(ex),
               "host_moved_beyond_spread": abs(hoc["median"] / hex_["median"] - 1.0) > spread(hex_),
               "rays_per_s": {"existing": 1e3 * n_rand / ex["median"], "one_call": 1e3 * n_rand / oc["median"]}}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del arms
        torch.cuda.empty_cache()
    summary = {"tool": "bench_depth_one_call", "device": torch.cuda.get_device_name(0), "rows": len(rows),
               "host_lower_everywhere": all(r["host_ms_per_step"]["one_call"]["median"] <
                                            r["host_ms_per_step"]["existing"]["median"] for r in rows),
               "one_call_over_existing": {f'{r["n_rand"]}:{r["n_samples"]}+{r["n_importance"]}':
                                          round(r["one_call_over_existing"], 4) for r in rows}}
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"summary": summary, "cells": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
