"""A/B of the two routes to a rendered frame: ViewRenderer -- every frame one plnerf_render_view call -- against render()
(get_rays, pack_rays, then ~10 launches per chunk reached through Python, ctypes and torch), on an 800 x 800 Blender-style
view at chunk 32,768 in f16x3, both under the same counter-based draws.  A frame of either route is first checked to be
the other's, bit for bit; if it is not, the tool says so and exits with status 1 before anything is timed.  render() is
handed device-resident poses (it builds its rays where the pose lives, and only the device's rays are the call's) and the call
host poses (it reads 12 host floats): the host times compare each route on the input it takes.  The arms alternate A / B / A / B within one process, and every leg measures, after its warm-up,

  ms_per_frame       HIP events around --frames frames (the frame as the GPU sees it), and
  host_ms_per_frame  the wall time of an enqueue loop of --host-frames frames with the stream left to run, started on an
                     idle device.

Min, median and max over the legs are reported per arm, and `aa_spread` = (max - min) / median over render()'s own legs.
The frame is bound by the two MLP launches of each chunk, which both routes share, so no speed-up is expected: `verdict`
says whether the one-call frame is slower than render()'s median by more than that spread.  One JSON line (also written
to --out)."""
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
from plnerf_amd import functional as Fn


def stats(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v), "all": [round(x, 4) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="blender_64_128")
    ap.add_argument("--size", type=int, default=800, help="H = W")
    ap.add_argument("--chunk", type=int, default=32768)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3, help="legs per arm (A / B alternate)")
    ap.add_argument("--export", action="store_true", help="the one-call arm also quantises each frame (rgb8, depth16)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ck = tempfile.mkdtemp()
    os.makedirs(os.path.join(ck, "exp"))
    ns, ni, _ = bench.WORKLOADS[a.workload]
    args = bench.make_args(argparse.Namespace(workload=a.workload, n_samples=ns, n_importance=ni, rays=4096), ck, a.precision)
    torch.manual_seed(0)
    _stdout = sys.stdout
    sys.stdout = open(os.devnull, "w")
    try:
        _, kw, _, _, _, _ = P.create_nerf(args, device=dev)
    finally:
        sys.stdout = _stdout
    H = W = a.size
    focal = .5 * W / 0.36002      # (camera_angle_x = 0.6911112: NeRF-synthetic's)
    K = [[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]]
    near, far = 2.0, 6.0
    host_poses = [P.rays.pose_spherical(-180.0 + 45.0 * i, -30.0, 4.0)[:3, :4] for i in range(8)]
    poses = [p.to(dev) for p in host_poses]      # (render() builds its rays where the pose lives)
    ndc = bool(kw.get("ndc", True))
    render_kw = dict(kw, ndc=ndc)
    view_kw = {k: v for k, v in kw.items() if k != "ndc"}
    vr = P.ViewRenderer(view_kw, H, W, K, a.chunk, near, far, ndc=ndc, seed=0)

    def frame_render(i):
        prev = Fn.set_draw_source(Fn.DrawSource(0, 0, i))
        try:
            return P.render(H, W, K, chunk=a.chunk, c2w=poses[i % len(poses)], near=near, far=far, **render_kw)
        finally:
            Fn.set_draw_source(prev)

    def frame_view(i):
        vr.enqueue(host_poses[i % len(poses)], step=i, export=a.export)
        return vr.planes["rgb"]

    with torch.no_grad():
        ref = frame_render(1)
        got = frame_view(1).view(H, W, 3)
        same = bool(torch.equal(got, ref[0])) and bool(torch.equal(vr.planes["depth"].view(H, W), ref[3]["depth_map"]))
        if not same:
            print(json.dumps({"tool": "bench_render_view", "frames_bit_identical": False,
                              "error": "the one-call frame is not render()'s: nothing was timed"}), flush=True)
            sys.exit(1)
        arms = {"render": frame_render, "one_call": frame_view}
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
    vr.check_range()
    for net in vr.nets:
        net.check_range()
    ex, oc = stats(dev_ms["render"]), stats(dev_ms["one_call"])
    spread = (ex["max"] - ex["min"]) / ex["median"]
    line = json.dumps({"tool": "bench_render_view", "device": torch.cuda.get_device_name(0), "H": H, "W": W, "chunk": a.chunk,
                      "precision": a.precision, "n_samples": ns, "n_importance": ni, "export": a.export,
                      "frames": a.frames, "host_frames": a.host_frames, "warmup": a.warmup, "repeats": a.repeats,
                      "frames_bit_identical": same,
                      "ms_per_frame": {"render": ex, "one_call": oc},
                      "host_ms_per_frame": {"render": stats(host_ms["render"]), "one_call": stats(host_ms["one_call"])},
                      "aa_spread": spread, "one_call_over_render": oc["median"] / ex["median"],
                      "poses": {"render": "device-resident", "one_call": "host"},
                      "verdict": "not slower" if oc["median"] <= ex["median"] * (1.0 + spread) else "slower"})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
