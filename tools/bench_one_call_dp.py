"""A/B of the two routes of a DATA-PARALLEL training step: TrainStep(distributed=True, one_call=True) with train.ONE_CALL_DP on
-- two library calls around the one gradient all-reduce (plnerf_train_step_grads, plnerf_train_step_apply) -- against the
same object with the switch off, which is the Python-driven route every rank took before (~23 launches reached through
Python, ctypes and torch.autograd).  N ranks time-share ONE GPU over gloo, the way the suite's distributed tests run: what
this measures is the ranks' HOST side (N interpreters on one host, as in an N-GPU job) and that the step is not slower; the
RCCL wire over several GPUs is NOT measured here.

Every rank: 4096 rays of bench.py's synthetic Blender scene (view source), 64 + 128 samples, f16x3.  Each arm has its own
networks and optimizers (same initial weights); the arms alternate off / on / off / on within the same processes, every rank
issuing its collectives in the same order, and every leg measures, after its warm-up,

  ms_per_step       wall time of --steps steps between two device synchronisations, and
  host_ms_per_step  the host's own share of those steps: the loop's wall time minus the time spent inside the gradient
                    exchange (GradientBucket.finish / reduce_block).  Over gloo the exchange BLOCKS the host until the
                    GPU has produced the gradients and the ranks have summed them through host memory, so the loop's wall
                    time alone would be the step time on either route; what is left after taking the exchange out is the
                    Python, ctypes and autograd time a rank spends enqueueing -- the quantity the one-call entries remove.

Min and median over the legs are reported per arm (rank 0's and the mean over ranks), and `aa_spread` = (max - min) /
median over the off arm's own legs: a difference between the arms inside it is no difference.  Run without --worker this
starts the ranks (one fresh process each, under a time limit) for every N of --ranks and prints one JSON line per N."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v), "all": [round(x, 5) for x in v]}


def worker(a):
    import torch
    import torch.distributed as dist

    import bench
    import plnerf_amd as P
    from plnerf_amd import dp, train
    rank, world, _ = dp.init_from_env(backend="gloo")      # every rank on cuda:0; gloo moves CUDA tensors through the host
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    workload = a.workload
    ns, ni, _ = bench.WORKLOADS[workload]

    def make_trainer():
        ck = tempfile.mkdtemp()
        os.makedirs(os.path.join(ck, "exp"))
        args = bench.make_args(argparse.Namespace(workload=workload, n_samples=ns, n_importance=ni, rays=a.rays), ck, "f16x3")
        torch.manual_seed(0)
        _stdout = sys.stdout
        sys.stdout = open(os.devnull, "w")
        try:
            kw, _, _, _, opt, opt_c = P.create_nerf(args, device=dev)
        finally:
            sys.stdout = _stdout
        ts = P.TrainStep(args, kw, opt, opt_c, distributed=True, seed=0, one_call=True, range_check_every=0)
        ts.exchange_s = 0.0
        for name in ("finish", "reduce_block"):      # time spent inside the exchange, taken out of the host's share
            inner = getattr(ts.bucket, name)

            def timed(*args, _inner=inner, **kw):
                t0 = time.perf_counter()
                try:
                    return _inner(*args, **kw)
                finally:
                    ts.exchange_s += time.perf_counter() - t0
            setattr(ts.bucket, name, timed)
        return ts

    scene = bench.Scene(P, workload, a.views, dev)
    arms = {"off": make_trainer(), "on": make_trainer()}

    def step(name, i):
        train.ONE_CALL_DP = name == "on"
        v = i % a.views
        return arms[name].step_view(scene.H, scene.W, scene.K, scene.poses[v], scene.images[v], near=scene.near, far=scene.far,
                                    n_rand=a.rays)
    wall_ms = {k: [] for k in arms}
    host_ms = {k: [] for k in arms}
    for rep in range(a.repeats):
        for name, ts in arms.items():
            for i in range(a.warmup):
                step(name, i)
            torch.cuda.synchronize()
            dist.barrier()
            ts.exchange_s = 0.0
            t0 = time.perf_counter()
            for i in range(a.steps):
                loss = step(name, i)[0]
            loop = time.perf_counter() - t0
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            assert torch.isfinite(loss), (name, float(loss))
            wall_ms[name].append(1e3 * wall / a.steps)
            host_ms[name].append(1e3 * (loop - ts.exchange_s) / a.steps)
    total = a.repeats * (a.warmup + a.steps)
    assert arms["on"].one_call_steps == total and arms["off"].one_call_steps == 0 and arms["off"].merged_steps == total
    mine = {"rank": rank, "ms_per_step": {k: stats(v) for k, v in wall_ms.items()},
            "host_ms_per_step": {k: stats(v) for k, v in host_ms.items()}}
    every = [None] * world
    dist.all_gather_object(every, mine)
    if rank == 0:
        off, on = mine["ms_per_step"]["off"], mine["ms_per_step"]["on"]
        mean = lambda what, arm: statistics.mean(r[what][arm]["median"] for r in every)
        print(json.dumps({
            "tool": "bench_one_call_dp", "device": torch.cuda.get_device_name(0), "backend": "gloo, every rank on one GPU",
            "ranks": world, "rays_per_rank": a.rays, "n_samples": ns, "n_importance": ni, "precision": "f16x3", "source": "view",
            "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
            "ms_per_step": {"off": off, "on": on}, "host_ms_per_step": mine["host_ms_per_step"],
            "mean_over_ranks": {"ms_per_step": {k: mean("ms_per_step", k) for k in arms},
                                "host_ms_per_step": {k: mean("host_ms_per_step", k) for k in arms}},
            "aa_spread": (off["max"] - off["min"]) / off["median"], "on_over_off": on["median"] / off["median"],
            "host_on_over_off": mine["host_ms_per_step"]["on"]["median"] / mine["host_ms_per_step"]["off"]["median"]}), flush=True)
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", default="2,8", help="world sizes, comma separated: one run each")
    ap.add_argument("--rays", type=int, default=4096, help="rays per rank")
    ap.add_argument("--workload", default="blender_64_128")
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3, help="legs per arm (off / on alternate)")
    ap.add_argument("--limit", type=int, default=420, help="seconds a rank may take")
    ap.add_argument("--worker", action="store_true", help="(internal) this process is one rank")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    for world in (int(n) for n in a.ranks.split(",")):
        port = 26300 + (os.getpid() % 200) + world
        flags = ["--worker", "--rays", str(a.rays), "--workload", a.workload, "--views", str(a.views), "--warmup", str(a.warmup),
                 "--steps", str(a.steps), "--repeats", str(a.repeats)]
        procs = []
        for rank in range(world):
            env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port))
            procs.append(subprocess.Popen(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__)] + flags,
                                          env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        outs = [p.communicate()[0] for p in procs]
        bad = [(rank, p.returncode, out[-2000:]) for rank, (p, out) in enumerate(zip(procs, outs)) if p.returncode != 0]
        if bad:      # (a rank that failed or ran into its limit: nothing further is started)
            raise SystemExit(f"{world} ranks: rank {bad[0][0]} exited with {bad[0][1]}:\n{bad[0][2]}")
        for line in outs[0].splitlines():
            if line.startswith("{"):
                print(line, flush=True)


if __name__ == "__main__":
    main()
