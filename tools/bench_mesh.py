"""A/B of the two routes to extract_fields' density lattice, and the cost of marching cubes on it, on a fused 8 x 256 network:

  (a) the reference-shaped route that exists without plnerf_density_grid: 64^3 blocks through the render kwargs'
      network_query_fn (run_network -> NeRF.query), relu, a copy of every block to the host, assembled into the numpy volume
      (plnerf_amd.mesh._block_loop: nerf_extract_mesh.py:531-562 statement by statement);
  (b) plnerf_density_grid: one library call for the whole lattice (plnerf_amd.mesh.density_grid), the field left on the device;

then plnerf_mc_count + plnerf_mc_emit on (b)'s field at the median of its positive values.

Before anything is timed (b)'s field is checked to be (a)'s bit for bit; if it is not, the tool says so and exits with status 1.
Per --resolution (256 and 512) and --precision (f16x3 and fp32) the legs alternate a / b / a / b within one process; every leg
measures, after one warm-up, the wall time of the whole route on an idle device with a synchronisation at the end ((a) ends on
the host by construction; (b)'s figure includes no copy: the field stays where marching cubes reads it), (b) and the two
marching-cubes calls also under HIP events, and the host enqueue time of each call (the wall time until the call returns, the
stream left to run).  Min, median and max over the legs, `aa_spread` = (max - min) / median over (a)'s own legs, the ratio
(b) / (a) of the medians, and the workspaces' bytes.  One JSON line per configuration, all written to --out."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import plnerf_amd as P
from plnerf_amd import _lib as L
from plnerf_amd import mesh


def stats(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v), "all": [round(x, 4) for x in v]}


def timed(fn):
    """(result, wall ms with a synchronisation at the end, device ms between HIP events, host ms until fn returned)."""
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    start.record()
    out = fn()
    t1 = time.perf_counter()
    end.record()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return out, (t2 - t0) * 1e3, start.elapsed_time(end), (t1 - t0) * 1e3


def one(resolution, precision, legs, max_rows, seed):
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    net = P.NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True, precision=precision).to(dev)
    emb, embd = P.get_embedder(10, 0)[0], P.get_embedder(4, 0)[0]

    def query(inputs, viewdirs, fn):
        return P.run_network(inputs, viewdirs, fn, emb, embd)
    query.embedders = (emb, embd)
    lo, hi = np.array([-1.25, -1.25, -1.25]), np.array([1.25, 1.25, 1.25])
    route = mesh._served_route(query, net)
    assert route == L.ANYVIEW_FUSED
    xs, ys, zs = mesh._linspaces(lo, hi, resolution)

    def route_a():
        return mesh._block_loop(lo, hi, resolution, query, net)

    def route_b():
        return mesh.density_grid(net, route, xs, ys, zs, max_rows=max_rows, stats=True)
    u = route_a()
    field, _ = route_b()
    same = np.array_equal(field.cpu().numpy().view(np.int32), u.view(np.int32))
    if not same:
        print(f"bench_mesh: resolution {resolution} {precision}: plnerf_density_grid's field is NOT the block loop's", file=sys.stderr)
        sys.exit(1)
    positive = field[field > 0]
    iso = float(positive.median()) if positive.numel() else 0.0
    lib = L.lib()
    n = resolution
    mc_bytes = lib.plnerf_mc_workspace_bytes(n, n, n)
    ws = torch.empty(mc_bytes, device=dev, dtype=torch.uint8)
    counts = torch.zeros(2, device=dev, dtype=torch.int32)
    wsp = ctypes.c_void_p(ws.data_ptr())

    def count():
        L.check(lib.plnerf_mc_count(L.dptr(field), n, n, n, iso, wsp, mc_bytes, L.dptr(counts, "counts", torch.int32), L.stream()), "count")
    count()
    n_v, n_t = (int(c) for c in counts.cpu().tolist())
    vertices = torch.empty(max(n_v, 1), 3, device=dev, dtype=torch.float64)
    triangles = torch.empty(max(n_t, 1), 3, device=dev, dtype=torch.int32)

    def emit():
        L.check(lib.plnerf_mc_emit(L.dptr(field), n, n, n, iso, wsp, mc_bytes, ctypes.c_void_p(vertices.data_ptr()), n_v,
                                   ctypes.c_void_p(triangles.data_ptr()), n_t, L.stream()), "emit")
    emit()
    a_wall, b_wall, b_dev, b_host, c_dev, c_host, e_dev, e_host = ([] for _ in range(8))
    for _ in range(legs):      # a / b / a / b
        a_wall.append(timed(route_a)[1])
        _, wall, devms, host = timed(route_b)
        b_wall.append(wall), b_dev.append(devms), b_host.append(host)
        _, _, devms, host = timed(count)
        c_dev.append(devms), c_host.append(host)
        _, _, devms, host = timed(emit)
        e_dev.append(devms), e_host.append(host)
    a, b = stats(a_wall), stats(b_wall)
    spread = (a["max"] - a["min"]) / a["median"]
    ratio = b["median"] / a["median"]
    slot = L.AnyViewNet()
    keep = []
    _, code, in_ch, view_ch = mesh._fill_slot(slot, net, route, dev, keep)
    grid_bytes = lib.plnerf_density_grid_workspace_bytes(ctypes.byref(slot), code, in_ch, view_ch, n, max_rows)
    return {"resolution": resolution, "precision": precision, "rows": n ** 3, "max_rows": max_rows, "legs": legs,
            "field_is_block_loop_bit_for_bit": same, "iso": iso, "n_vertices": n_v, "n_triangles": n_t,
            "block_loop_ms": a, "density_grid_ms": b, "density_grid_device_ms": stats(b_dev), "density_grid_host_enqueue_ms": stats(b_host),
            "mc_count_device_ms": stats(c_dev), "mc_count_host_enqueue_ms": stats(c_host),
            "mc_emit_device_ms": stats(e_dev), "mc_emit_host_enqueue_ms": stats(e_host),
            "aa_spread": spread, "density_grid_over_block_loop": ratio,
            "verdict": "faster" if ratio < 1.0 - spread else ("slower" if ratio > 1.0 + spread else "within the A/A spread"),
            "density_grid_workspace_bytes": grid_bytes, "mc_workspace_bytes": mc_bytes, "mc_bytes_per_point": mc_bytes / n ** 3,
            "field_bytes": 4 * n ** 3, "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--precision", nargs="+", default=["f16x3", "fp32"])
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--max-rows", type=int, default=1 << 21)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh.json"))
    args = ap.parse_args()
    rows = []
    for resolution in args.resolution:
        for precision in args.precision:
            rows.append(one(resolution, precision, args.legs, args.max_rows, args.seed))
            print(json.dumps(rows[-1]), flush=True)
            with open(args.out, "w") as f:
                json.dump(rows, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
