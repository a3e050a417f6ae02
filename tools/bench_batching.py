"""A/B of the two ray sources of the training step: TrainStep.step_batch (RayBank: random rays of all training views,
the reference's use_batching branch) against TrainStep.step_view (N_rand pixels of one view, its no_batching branch), on
bench.py's synthetic llff_ndc and blender_128_64 scenes at N_rand 1024 and 4096, f16x3.  Each arm has its own networks
and optimizers (same initial weights); the arms alternate within every repeat (warm-up, then HIP-event timing of
--steps steps), and the spread over the repeats is reported.  One JSON line per (workload, N_rand).
The ray-selection kernels' own time: run this under `rocprofv3 --kernel-trace --stats` (with --repeats 1)."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import bench
import plnerf_amd as P


def make_trainer(a, workload, n_rand, dev):
    ck = tempfile.mkdtemp()
    os.makedirs(os.path.join(ck, "exp"))
    ns, ni, _ = bench.WORKLOADS[workload]
    args = bench.make_args(argparse.Namespace(workload=workload, n_samples=ns, n_importance=ni, rays=n_rand), ck, "f16x3")
    torch.manual_seed(0)
    _stdout = sys.stdout
    sys.stdout = open(os.devnull, "w")
    try:
        kw, _, _, _, opt, opt_c = P.create_nerf(args, device=dev)
    finally:
        sys.stdout = _stdout
    return P.TrainStep(args, kw, opt, opt_c, distributed=False, seed=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="llff_ndc,blender_128_64")
    ap.add_argument("--rays", default="1024,4096")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for workload in a.workloads.split(","):
        scene = bench.Scene(P, workload, a.views, dev)
        bank = P.RayBank(torch.stack(scene.images), torch.stack([p[:3, :4] for p in scene.poses]), scene.K,
                         list(range(a.views)), scene.near, scene.far, seed=0, device=dev)
        for n_rand in (int(r) for r in a.rays.split(",")):
            ts_view, ts_batch = make_trainer(a, workload, n_rand, dev), make_trainer(a, workload, n_rand, dev)

            def view_step(i):
                v = i % a.views
                return ts_view.step_view(scene.H, scene.W, scene.K, scene.poses[v], scene.images[v], near=scene.near,
                                         far=scene.far, n_rand=n_rand)

            def batch_step(i):
                return ts_batch.step_batch(bank, n_rand)

            arms = {"step_view": view_step, "step_batch": batch_step}
            ms = {k: [] for k in arms}
            i = 0
            for rep in range(a.repeats):
                order = list(arms) if rep % 2 == 0 else list(arms)[::-1]
                for name in order:
                    fn = arms[name]
                    for _ in range(a.warmup):
                        fn(i)
                        i += 1
                    torch.cuda.synchronize()
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for _ in range(a.steps):
                        loss = fn(i)[0]
                        i += 1
                    e.record()
                    torch.cuda.synchronize()
                    assert torch.isfinite(loss), (name, float(loss))
                    ms[name].append(s.elapsed_time(e) / a.steps)
            out = {"workload": workload, "n_rand": n_rand, "views": a.views, "bank_rays": bank.M, "steps": a.steps,
                   "warmup": a.warmup, "repeats": a.repeats}
            for name, v in ms.items():
                out[name + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}
            out["batch_over_view"] = statistics.median(ms["step_batch"]) / statistics.median(ms["step_view"])
            print(json.dumps(out), flush=True)
            del ts_view, ts_batch
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
