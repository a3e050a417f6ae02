"""A/B of the two routes to a rendered frame of the depth-supervised variant: DepthViewRenderer -- every frame one
plnerf_depth_render_view call -- against depth.render() (get_rays, pack_rays, then ~8 launches per chunk reached through
Python, ctypes and torch), on an 800 x 800 view with depth_128_64-style networks at chunk 32,768 in f16x3 under the test-time
settings (perturb 0, no density noise).  A frame of either route is first checked to be the other's, bit for bit; if it is
not, the tool says so and exits with status 1 before anything is timed.  depth.render() is handed device-resident poses
and intrinsics (it builds its rays where they live, and only the device's rays are the call's) and the call host ones (it
reads 16 host floats): the host times compare each route on the input it takes.  The arms alternate A / B / A / B within one
process, and every leg measures, after its warm-up,

  ms_per_frame       HIP events around --frames frames (the frame as the GPU sees it), and
  host_ms_per_frame  the wall time of an enqueue loop of --host-frames frames with the stream left to run, started on an
                     idle device.

Min, median and max over the legs are reported per arm, and `aa_spread` = (max - min) / median over the parent route's own
legs.  The frame is bound by the two MLP launches of each chunk, which both routes share, so no speed-up is expected:
`verdict` says whether the one-call frame is slower than the parent route's median by more than that spread.

The second run ("score") is the `test_samples_error` view: the call with valid + error_row (no hypothesis plane) against
depth.test_images_samples' present route on one view, under the same protocol, their rows compared first, plus each route's
peak allocation above what is resident before it runs (torch.cuda.max_memory_allocated; the one-call route's figure
includes the renderer it builds: planes, workspace, packed buffers).  One JSON line (also written to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import bench
import plnerf_amd as P
from plnerf_amd import depth as Dp


def stats(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v), "all": [round(x, 4) for x in v]}


def legs(arms, a):
    """The interleaved protocol: per leg and arm, warm-up, the host enqueue loop on an idle device, then HIP events."""
    dev_ms = {k: [] for k in arms}
    host_ms = {k: [] for k in arms}
    for rep in range(a.repeats):
        for name, fn in arms.items():
            for i in range(a.warmup):
                fn(i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.host_frames):
                fn(i)
            host = time.perf_counter() - t0      # (the enqueue loop alone: the stream is still running)
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for i in range(a.frames):
                fn(i)
            e.record()
            torch.cuda.synchronize()
            dev_ms[name].append(s.elapsed_time(e) / a.frames)
            host_ms[name].append(1e3 * host / a.host_frames)
    return dev_ms, host_ms


def summary(dev_ms, host_ms, parent, call):
    ex, oc = stats(dev_ms[parent]), stats(dev_ms[call])
    spread = (ex["max"] - ex["min"]) / ex["median"]
    return {"ms_per_frame": {parent: ex, call: oc},
            "host_ms_per_frame": {parent: stats(host_ms[parent]), call: stats(host_ms[call])},
            "aa_spread": spread, "one_call_over_parent": oc["median"] / ex["median"],
            "verdict": "not slower" if oc["median"] <= ex["median"] * (1.0 + spread) else "slower"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800, help="H = W")
    ap.add_argument("--chunk", type=int, default=32768)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3, help="legs per arm (A / B alternate)")
    ap.add_argument("--export", action="store_true", help="the one-call arm also quantises each frame (rgb8, depth16, depth_mm16)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ns, ni, _ = bench.WORKLOADS["depth_128_64"]
    args = bench.depth_args(argparse.Namespace(n_samples=ns, n_importance=ni), a.precision)
    args.chunk = a.chunk
    torch.manual_seed(0)
    _, kw, _, _, _ = Dp.create_nerf(args, device=dev)      # (render_kwargs_test: perturb 0, no noise)
    H = W = a.size
    near, far = 2.0, 6.0
    focal = .5 * W / 0.36002
    host_intr = torch.tensor([focal, focal * 1.01, W / 2 - 0.25, H / 2 + 0.5])
    host_poses = [P.rays.pose_spherical(-180.0 + 45.0 * i, -30.0, 4.0)[:3, :4] for i in range(8)]
    intr, poses = host_intr.to(dev), [p.to(dev) for p in host_poses]      # (depth.render() builds its rays where they live)
    gen = torch.Generator().manual_seed(1)
    valid = (torch.rand(1, H, W, generator=gen) < 0.5).to(dev)
    render_kw = dict(kw, near=near, far=far)
    torch.cuda.synchronize()

    # ---- peak allocation of the present test_samples_error route, before the renderer exists ----
    def present_rows(i):
        return Dp.test_images_samples(None, [0], None, None, valid, poses[i % len(poses)][None], H, W, intr[None], None, args,
                                      render_kw)

    with torch.no_grad():
        resident = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        want_error = present_rows(1).get("importance_sampling_error")
        torch.cuda.synchronize()
        peak_present = torch.cuda.max_memory_allocated() - resident
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        vr = P.DepthViewRenderer(kw, H, W, a.chunk, near, far, seed=0)
        row = vr.render(host_poses[1], host_intr, valid=valid)[3]["sample_error_row"].tolist()
        torch.cuda.synchronize()
        peak_call = torch.cuda.max_memory_allocated() - resident

        # ---- the frames are one frame ----
        def frame_render(i):
            return Dp.render(H, W, intr, chunk=a.chunk, c2w=poses[i % len(poses)], **render_kw)

        def frame_view(i):
            vr.enqueue(host_poses[i % len(poses)], host_intr, step=i, export=a.export)
            return vr.planes["rgb"]

        def score_view(i):
            vr.error_row.zero_()
            vr.enqueue(host_poses[i % len(poses)], host_intr, step=i, valid=valid)
            return vr.error_row

        ref = frame_render(1)
        got = frame_view(1).view(H, W, 3)
        same = bool(torch.equal(got, ref[0])) and bool(torch.equal(vr.planes["depth"].view(H, W), ref[3]["depth_map"]))
        same_row = row[1] > 0 and row[0] / row[1] == want_error
        if not (same and same_row):
            print(json.dumps({"tool": "bench_depth_render_view", "frames_bit_identical": same, "rows_identical": same_row,
                              "error": "the one-call frame (or its error row) is not the parent route's: nothing was timed"}),
                  flush=True)
            sys.exit(1)
        frame = summary(*legs({"render": frame_render, "one_call": frame_view}, a), "render", "one_call")
        score = summary(*legs({"test_images_samples": present_rows, "one_call": score_view}, a), "test_images_samples", "one_call")
    vr.check_range()
    for net in vr.nets:
        net.check_range()
    score["peak_bytes_above_resident"] = {"test_images_samples": peak_present, "one_call": peak_call,
                                          "one_call_workspace": vr.workspace_bytes}
    line = json.dumps({"tool": "bench_depth_render_view", "device": torch.cuda.get_device_name(0), "H": H, "W": W,
                      "chunk": a.chunk, "precision": a.precision, "n_samples": ns, "n_importance": ni, "export": a.export,
                      "frames": a.frames, "host_frames": a.host_frames, "warmup": a.warmup, "repeats": a.repeats,
                      "frames_bit_identical": same, "rows_identical": same_row,
                      "inputs": {"parent": "device-resident pose and intrinsics", "one_call": "host"},
                      "frame": frame, "score": score, "verdict": frame["verdict"]})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
