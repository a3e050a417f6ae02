"""Test-time camera-code optimisation: the cached route (camcode.CameraCodeOptimizer: plnerf_camcode_sweep +
plnerf_camcode_update) against the plain route (the reference's loop on the autograd path), interleaved on one GPU.

    python tools/bench_camopt.py [--H 96 --W 128 --N_samples 64 --N_importance 64 --N_rand 1024] [--out FILE.json]

Reports, per route, ms per iteration; the cache-build time; the sweep's bytes per iteration (A of the rows with a non-zero
coefficient, coef, targets, weights) over its time, beside the 5.9 TB/s read ceiling of DESIGN.md section 4; and the host's
enqueue time per iteration.  The comparison that counts: cache build + 100 cached iterations against 100 plain iterations."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

READ_CEILING_TBS = 5.9      # the measured HBM read ceiling


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=96)
    ap.add_argument("--W", type=int, default=128)
    ap.add_argument("--N_samples", type=int, default=64)
    ap.add_argument("--N_importance", type=int, default=64)
    ap.add_argument("--N_rand", type=int, default=1024)
    ap.add_argument("--n_cam", type=int, default=4)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--plain_iters", type=int, default=5, help="plain iterations timed per round (scaled to 100)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import plnerf_amd as P
    from plnerf_amd import camcode, depth as Dp
    dev = torch.device("cuda:0")
    args = argparse.Namespace(multires=9, i_embed=0, use_viewdirs=True, multires_views=0, input_ch_cam=a.n_cam,
                              N_importance=a.N_importance, N_samples=a.N_samples, netdepth=8, netwidth=256, netdepth_fine=8,
                              netwidth_fine=256, netchunk=65536, lrate=5e-4, perturb=0.0, white_bkgd=True, raw_noise_std=0.0,
                              mode="linear", color_mode="midpoint", lindisp=False, no_reload=True, precision=a.precision,
                              bb_center=0.0, bb_scale=1.0, chunk=32768, N_rand=a.N_rand)
    torch.manual_seed(0)
    _, kw, _, _, _ = Dp.create_nerf(args, device=dev)
    with torch.no_grad():
        for net in (kw["network_fn"], kw["network_fine"]):
            net.alpha_linear.weight.mul_(20.0)
            net.requires_grad_(False)
    kw.update(near=2.0, far=6.0)
    pose = P.rays.pose_spherical(30.0, -30.0, 4.0)[:3, :4].to(dev)
    intrinsic = torch.tensor([a.W * 0.9, a.W * 0.9, a.W / 2, a.H / 2], device=dev)
    with torch.no_grad():
        image = Dp.render(a.H, a.W, intrinsic, chunk=args.chunk, c2w=pose,
                          **dict(kw, embedded_cam=torch.full((a.n_cam,), 0.6, device=dev)))[0]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    reason = camcode.CameraCodeOptimizer.unsupported_reason(kw, args, a.H, a.W, 32 << 30)
    assert reason is None, reason
    fast = camcode.CameraCodeOptimizer(kw, a.H, a.W, args)
    fast.build(image, pose, intrinsic).run(3)                                                    # warm-up, both routes
    camcode.optimize_camera_embedding(image, pose, a.H, a.W, intrinsic, args, dict(kw), route="plain", n_iters=1)
    cam0 = torch.zeros(a.n_cam, device=dev)
    rounds = []
    for _ in range(a.rounds):
        _, t_build = timed(lambda: fast.build(image, pose, intrinsic))
        rec_host = None

        def run():
            nonlocal rec_host
            rec_host = fast.run(100)
        _, t_fast = timed(run)
        # the sweep alone, at the zero code: 100 launches enqueued (the host's time for that), then waited for
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(100):
            fast._sweep(P._lib.dptr(cam0))
        t_enqueue = time.perf_counter() - t1
        torch.cuda.synchronize()
        t_sweeps = time.perf_counter() - t1
        rec_plain, t_plain = timed(lambda: camcode.optimize_camera_embedding(
            image, pose, a.H, a.W, intrinsic, args, dict(kw), route="plain", n_iters=a.plain_iters))
        rounds.append(dict(cache_build_ms=t_build * 1e3, fast_100_iters_ms=t_fast * 1e3, sweep_ms=t_sweeps * 10.0,
                           sweep_enqueue_us=t_enqueue * 1e4, plain_ms_per_iter=t_plain * 1e3 / a.plain_iters,
                           fast_best_psnr=rec_host["best_psnr"], plain_first_psnr=rec_plain["psnr"][0],
                           fast_first_psnr=rec_host["psnr"][0]))
    best = lambda k: min(r[k] for r in rounds)
    n_rows = fast.A.shape[0]
    live = int((fast.coef != 0).sum())
    bytes_per_iter = live * fast.width * 4 + n_rows * 4 + fast.n_rays * (3 + 1 + 1) * 4
    sweep_s = best("sweep_ms") * 1e-3
    result = dict(
        view=[a.H, a.W], samples=[a.N_samples, a.N_importance], N_rand=a.N_rand, n_cam=a.n_cam, precision=a.precision,
        batches=len(fast.sizes), rows=n_rows, rows_with_nonzero_coef=live, cache_bytes=n_rows * fast.width * 4,
        cache_build_ms=best("cache_build_ms"), fast_ms_per_iter=best("fast_100_iters_ms") / 100.0,
        sweep_ms=best("sweep_ms"), sweep_bytes_per_iter=bytes_per_iter, sweep_TB_per_s=bytes_per_iter / sweep_s / 1e12,
        read_ceiling_TB_per_s=READ_CEILING_TBS, host_enqueue_us_per_sweep=best("sweep_enqueue_us"),
        plain_ms_per_iter=best("plain_ms_per_iter"), fast_total_100_ms=best("cache_build_ms") + best("fast_100_iters_ms"),
        plain_total_100_ms=best("plain_ms_per_iter") * 100.0, rounds=rounds)
    result["fast_is_faster_including_cache_build"] = result["fast_total_100_ms"] < result["plain_total_100_ms"]
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
