"""A/B of the two routes to a rendered frame of a MIXED pair of networks -- the coarse one on the fused 8 x 256 trunk, the fine
one outside it (netdepth 8 at netwidth 512: --netwidth 256 --netwidth_fine 512) --: AnyViewRenderer, every frame one
plnerf_render_view_any call, against render() (get_rays, pack_rays, then per chunk the glue launches, plnerf_embed_rows and the
layer-by-layer route reached through Python, ctypes and torch), on an 800 x 800 Blender-style view at chunk 32,768 with 64 + 128
samples, both under the same counter-based draws.

--route picks how the fine network runs, on both sides alike:
  layers32   the switches of generic.py off (the default): exact-fp32 layers whatever `precision` says
  chain16    generic.HONOUR_PRECISION and generic.CHAIN_INFERENCE on, set before create_nerf: render()'s best existing route
             (one plnerf_generic_fwd call per netchunk), the one call's CHAIN16 slot
render()'s netchunk is --net-rows, the one call's max_net_rows: both sides hand the fine network the same sub-blocks.

A frame of either route is first checked to be the other's, bit for bit; if it is not, the tool says so and exits with status
1 before anything is timed.  render() is handed device-resident poses and the call host poses, as tools/bench_render_view.py
says.  The arms alternate A / B / A / B within one process, and every leg measures, after its warm-up,

  ms_per_frame        HIP events around --frames frames (the frame as the GPU sees it),
  host_ms_per_frame   the wall time of an enqueue loop of --host-frames frames with the stream left to run, started on an
                      idle device, and
  peak_alloc_mib      torch's peak allocation over the leg (the one call's workspace is a torch allocation too; the renderer's
                      own planes and workspace, which sit idle while render() runs, are taken off render()'s figure).

Min, median and max over the legs are reported per arm, and `aa_spread` = (max - min) / median over render()'s own legs.  The
claim under test: the one-call frame is not slower on the device than render()'s median beyond that spread, and its host
enqueue time is smaller.  One JSON line (also written to --out)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import bench
import plnerf_amd as P
from plnerf_amd import functional as Fn
from plnerf_amd import generic


def stats(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v), "all": [round(x, 4) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="blender_64_128")
    ap.add_argument("--size", type=int, default=800, help="H = W")
    ap.add_argument("--chunk", type=int, default=32768)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--route", default="layers32", choices=["layers32", "chain16"])
    ap.add_argument("--netwidth-fine", type=int, default=512)
    ap.add_argument("--net-rows", type=int, default=1 << 21, help="render()'s netchunk and the one call's max_net_rows")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--host-frames", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=2, help="legs per arm (A / B alternate)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ck = tempfile.mkdtemp()
    os.makedirs(os.path.join(ck, "exp"))
    ns, ni, _ = bench.WORKLOADS[a.workload]
    args = bench.make_args(argparse.Namespace(workload=a.workload, n_samples=ns, n_importance=ni, rays=4096), ck, a.precision)
    args.netwidth_fine, args.netchunk = a.netwidth_fine, a.net_rows
    if a.route == "chain16":      # (before create_nerf: generic.py says why)
        generic.HONOUR_PRECISION = generic.CHAIN_INFERENCE = True
    torch.manual_seed(0)
    _stdout = sys.stdout
    sys.stdout = open(os.devnull, "w")
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)      # (create_nerf says once that the fine network is outside the trunk)
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
    assert not P.ViewRenderer.supported(view_kw), "the fine network is on the fused trunk: tools/bench_render_view.py measures that"
    resident = torch.cuda.memory_allocated()
    vr = P.AnyViewRenderer(view_kw, H, W, K, a.chunk, near, far, ndc=ndc, seed=0, max_net_rows=a.net_rows)
    resident = (torch.cuda.memory_allocated() - resident) / 2 ** 20      # the renderer's planes and workspace: idle under render()
    routes = [P.anyview.ROUTES[r] for r in vr.routes]
    assert routes == ["fused", a.route], routes

    def frame_render(i):
        prev = Fn.set_draw_source(Fn.DrawSource(0, 0, i))
        try:
            return P.render(H, W, K, chunk=a.chunk, c2w=poses[i % len(poses)], near=near, far=far, **render_kw)
        finally:
            Fn.set_draw_source(prev)

    def frame_view(i):
        vr.enqueue(host_poses[i % len(poses)], step=i)
        return vr.planes["rgb"]

    with torch.no_grad():
        ref = frame_render(1)
        got = frame_view(1).view(H, W, 3)
        same = bool(torch.equal(got, ref[0])) and bool(torch.equal(vr.planes["depth"].view(H, W), ref[3]["depth_map"]))
        if not same:
            print(json.dumps({"tool": "bench_any_view", "route": a.route, "frames_bit_identical": False,
                              "error": "the one-call frame is not render()'s: nothing was timed"}), flush=True)
            sys.exit(1)
        del ref, got
        arms = {"render": frame_render, "one_call": frame_view}
        dev_ms = {k: [] for k in arms}
        host_ms = {k: [] for k in arms}
        peak = {k: [] for k in arms}
        for rep in range(a.repeats):
            for name, fn in arms.items():
                for i in range(a.warmup):
                    fn(i)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
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
                peak[name].append(torch.cuda.max_memory_allocated() / 2 ** 20)
                print(f"leg {rep} {name}: {dev_ms[name][-1]:.2f} ms / frame, host {host_ms[name][-1]:.2f} ms, peak "
                      f"{peak[name][-1]:.0f} MiB", file=sys.stderr, flush=True)
    vr.check_range()
    ex, oc = stats(dev_ms["render"]), stats(dev_ms["one_call"])
    hx, hc = stats(host_ms["render"]), stats(host_ms["one_call"])
    spread = (ex["max"] - ex["min"]) / ex["median"]
    not_slower, less_host = oc["median"] <= ex["median"] * (1.0 + spread), hc["median"] < hx["median"]
    line = json.dumps({"tool": "bench_any_view", "device": torch.cuda.get_device_name(0), "H": H, "W": W, "chunk": a.chunk,
                      "precision": a.precision, "route": a.route, "routes": routes, "netwidth_fine": a.netwidth_fine,
                      "net_rows": a.net_rows, "n_samples": ns, "n_importance": ni, "frames": a.frames,
                      "host_frames": a.host_frames, "warmup": a.warmup, "repeats": a.repeats, "frames_bit_identical": same,
                      "workspace_mib": vr.workspace_bytes / 2 ** 20,
                      "ms_per_frame": {"render": ex, "one_call": oc},
                      "host_ms_per_frame": {"render": hx, "one_call": hc},
                      "peak_alloc_mib": {"render": max(peak["render"]) - resident, "one_call": max(peak["one_call"]),
                                         "renderer_resident": resident},
                      "aa_spread": spread, "one_call_over_render": oc["median"] / ex["median"],
                      "host_one_call_over_render": hc["median"] / hx["median"],
                      "poses": {"render": "device-resident", "one_call": "host"},
                      "verdict": {"device": "not slower" if not_slower else "slower",
                                  "host_enqueue": "smaller" if less_host else "not smaller"}})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
