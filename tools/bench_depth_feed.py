"""The depth-supervised loop's data feed, timed: plnerf_select_depth_rays alone (DepthViews.select), and the full step
at bench.py's depth_128_64 (f16x3, 800 x 800 views, 4096 rays, three depth hypotheses per pixel) fed three ways:

  step_view   DepthTrainStep.step_view: the device feed, then the step (the depth script's own ray convention)
  bench_feed  bench.py's current route: select_view_rays (the NVS camera convention) + a torch gather of target_h
  host_feed   the reference-shaped route: depth.get_rays of the FULL image, then indexing at N_rand distinct pixels
              (get_ray_batch_from_one_image_hypothesis_idx, run_nerf_sample_based_depth.py:960-1001), all on the device

Each arm has its own networks and optimizer (same initial weights); the arms alternate within every repeat (warm-up, then
HIP-event timing of --steps steps), and the spread over the repeats is reported.  The feed-only legs time the feed
itself: select (one launch), and the host route's ray grid + gathers.  One JSON line per leg."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
import plnerf_amd as P
from plnerf_amd import depth as Dp


def make_trainer(a, dev):
    ns = argparse.Namespace(n_samples=128, n_importance=64)
    args = bench.depth_args(ns, "f16x3")
    args.N_rand = a.rays
    torch.manual_seed(0)
    kw, _, _, grad_vars, opt = Dp.create_nerf(args, device=dev)
    return Dp.DepthTrainStep(args, kw, opt, grad_vars, distributed=False, seed=0)


def timed(fn, i0, warmup, steps):
    for k in range(warmup):
        fn(i0 + k)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for k in range(steps):
        fn(i0 + warmup + k)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--feed-steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    scene = bench.Scene(P, "depth_128_64", a.views, dev)
    H, W, R = scene.H, scene.W, a.rays
    f = scene.K[0][0]
    intr = torch.tensor([[f, f, W / 2, H / 2]] * a.views, device=dev)
    poses = torch.stack([p.to(dev) for p in scene.poses])
    hyp = torch.stack(scene.hyp)                         # [V, 3, H, W]
    valid = torch.ones(a.views, H, W, dtype=torch.bool, device=dev)
    views = P.DepthViews(torch.stack(scene.images), poses, intr, hyp, valid, scene.near, scene.far)
    rng = np.random.default_rng(0)

    def host_batch(i):
        """get_ray_batch_from_one_image_hypothesis_idx on device tensors (the reference's select_coordinates draws with
        np.random.choice on the host and indexes the full grids)."""
        v = i % a.views
        rays_o, rays_d = Dp.get_rays(H, W, intr[v], poses[v])
        sel = torch.from_numpy(rng.choice(H * W, size=[R], replace=False)).to(dev)
        r, c = sel // W, sel % W
        o, d = rays_o[r, c], rays_d[r, c]
        vd = d / torch.norm(d, dim=-1, keepdim=True)
        cols = P.RayColumns(o.contiguous(), d.contiguous(), torch.full((R,), scene.near, device=dev),
                            torch.full((R,), scene.far, device=dev), vd.contiguous())
        return cols, views.images[v][r, c], views.hypotheses[v][:, r, c].unsqueeze(-1), valid[v][r, c].float()

    def bench_batch(i):
        v = i % a.views
        cols, target, pix = P.select_view_rays(H, W, scene.K, scene.poses[v], scene.images[v], R, scene.near, scene.far,
                                               seed=0, step=i, want_pixels=True)
        return cols, target, scene.hyp[v][:, pix[:, 0].long(), pix[:, 1].long()].unsqueeze(-1), None

    ts = {k: make_trainer(a, dev) for k in ("step_view", "bench_feed", "host_feed")}
    steps = {
        "step_view": lambda i: ts["step_view"].step_view(views, i % a.views),
        "bench_feed": lambda i: ts["bench_feed"](*bench_batch(i)),
        "host_feed": lambda i: ts["host_feed"](*host_batch(i)),
    }
    feeds = {
        "feed_select": lambda i: views.select(i % a.views, i, R, 0, seed=0),
        "feed_bench_route": bench_batch,
        "feed_host_route": host_batch,
    }
    ms = {k: [] for k in list(feeds) + list(steps)}
    i = 0
    for rep in range(a.repeats):
        for group, n in ((feeds, a.feed_steps), (steps, a.steps)):
            order = list(group) if rep % 2 == 0 else list(group)[::-1]
            for name in order:
                ms[name].append(timed(group[name], i, a.warmup, n))
                i += a.warmup + n
    for name, v in ms.items():
        print(json.dumps({"leg": name, "rays": R, "H": H, "W": W, "views": a.views, "n_hyp": 3,
                          "steps": a.feed_steps if name in feeds else a.steps, "warmup": a.warmup,
                          "ms": {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}}), flush=True)


if __name__ == "__main__":
    main()
