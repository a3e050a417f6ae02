"""Which fp32 expression do torch's device kernels evaluate for rays.get_rays and raybatch.unit_directions?

render() builds a full view's rays with those two where the pose lives -- on the GPU -- and plnerf_view_rays has to equal
them bit for bit.  For views from 1 x 1 to 800 x 800 (intrinsics that are not fp32 numbers, a generic rotation) this evaluates
candidate expressions on the host in numpy fp32 -- the camera direction by division or by a multiply with the fp32
reciprocal of the focal length, the three terms of the rotation and of the norm in each of the three associations -- and
counts the elements in which each differs from the device's result and from the host's own get_rays.  One JSON line (also
written to --out): per view the mismatch counts, and `device_expression` / `host_expression`, the candidates with no mismatch
in any view."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import plnerf_amd as P
from plnerf_amd import raybatch as RB

f32 = np.float32
ORDERS = ("(t0+t1)+t2", "(t0+t2)+t1", "(t1+t2)+t0")


def sums(t0, t1, t2):
    return {"(t0+t1)+t2": (t0 + t1) + t2, "(t0+t2)+t1": (t0 + t2) + t1, "(t1+t2)+t0": (t1 + t2) + t0}


def rotation(th, ph, ps):
    rx = np.array([[1, 0, 0], [0, np.cos(ph), -np.sin(ph)], [0, np.sin(ph), np.cos(ph)]])
    ry = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    rz = np.array([[np.cos(ps), -np.sin(ps), 0], [np.sin(ps), np.cos(ps), 0], [0, 0, 1]])
    return rz @ ry @ rx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    views = ((9, 13, 11.3, 9.7, 6.1, 4.3), (13, 9, 10.0, 10.0, 4.5, 6.5), (8, 12, 7.7, 7.7, 6.0, 4.0), (12, 16, 13.1, 12.9, 8.2, 5.9),
             (800, 800, 1111.111, 1111.111, 400.0, 400.0), (1, 1, 3.0, 2.0, 0.3, 0.1))
    c2w = np.concatenate([rotation(0.4, -0.7, 0.25), np.array([[0.3], [-1.2], [2.5]])], 1).astype(f32)
    rows = []
    for H, W, fx, fy, cx, cy in views:
        K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]
        _, d_dev = P.get_rays(H, W, K, torch.from_numpy(c2w).to(dev))
        _, d_host = P.get_rays(H, W, K, torch.from_numpy(c2w))
        v_dev = RB.unit_directions(d_dev).cpu().numpy()
        d_dev, d_host = d_dev.cpu().numpy(), d_host.numpy()
        col = np.broadcast_to(np.arange(W, dtype=f32)[None, :], (H, W))
        row = np.broadcast_to(np.arange(H, dtype=f32)[:, None], (H, W))
        cams = {"divide": ((col - f32(cx)) / f32(fx), -(row - f32(cy)) / f32(fy)),
                "reciprocal": ((col - f32(cx)) * (f32(1) / f32(fx)), -(row - f32(cy)) * (f32(1) / f32(fy)))}
        directions = {}
        for cam, (d0, d1) in cams.items():
            d2 = -np.ones_like(d0)
            t = [[d0 * c2w[k, 0], d1 * c2w[k, 1], d2 * c2w[k, 2]] for k in range(3)]
            for order in ORDERS:
                cand = np.stack([sums(*t[k])[order] for k in range(3)], -1).astype(f32)
                directions[f"{cam}, {order}"] = {"vs_device": int((cand != d_dev).sum()), "vs_host": int((cand != d_host).sum())}
        flat = d_dev.reshape(-1, 3)
        squares = [flat[:, k] * flat[:, k] for k in range(3)]
        norms = {order: int(((flat / np.sqrt(s.astype(f32)).astype(f32)[:, None]).astype(f32) != v_dev).sum())
                 for order, s in sums(*squares).items()}
        rows.append({"H": H, "W": W, "components": int(d_dev.size), "device_vs_host_get_rays": int((d_dev != d_host).sum()),
                     "rays_d_mismatches": directions, "unit_directions_mismatches_vs_device": norms})
    multi = [r for r in rows if r["components"] > 3]      # (a single pixel cannot tell the candidates apart)
    exact = lambda key, side: [c for c in rows[0]["rays_d_mismatches"] if all(r["rays_d_mismatches"][c][side] == 0 for r in multi)]
    line = json.dumps({"tool": "probe_ray_arithmetic", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                       "views": rows, "device_expression": exact(None, "vs_device"), "host_expression": exact(None, "vs_host"),
                       "device_norm_order": [o for o in ORDERS if all(r["unit_directions_mismatches_vs_device"][o] == 0 for r in multi)]})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
