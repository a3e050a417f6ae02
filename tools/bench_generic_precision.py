"""Same-box interleaved A/B of the layer-by-layer route's forward: plnerf_gemm_f32 (what runs with generic.HONOUR_PRECISION off)
against plnerf_gemm_h16 in each 16-bit mode (what runs with it on).

Two workloads: one 512 x 512 layer (bias + ReLU) at 262,144 rows, called through the raw entries; and a render() chunk (4096
rays, 64 + 128 samples, no gradient) of a D = 8, W = 512 network pair.  Every leg is warmed up, then the legs take turns
round by round -- fp32 twice per round (legs "fp32" and "fp32_again": their ratio is the A/A spread a difference has to
exceed) -- each sample timed with device events around `--calls` back-to-back calls.  Per leg: the median, the fastest and
the slowest sample; per 16-bit mode the ratio of medians fp32 / mode.  Writes profiles/generic_precision.json (or --out).

    python tools/bench_generic_precision.py [--rounds 12] [--calls 10] [--out profiles/generic_precision.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plnerf_amd as P                      # noqa: E402
from plnerf_amd import _lib as L            # noqa: E402
from plnerf_amd import generic              # noqa: E402

MODES = ("f16x3", "bf16x3", "f16", "bf16")


def timed(fn, calls):
    """Milliseconds per call over `calls` back-to-back calls, by device events."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def interleave(legs, rounds, calls, warmup=3):
    """legs: {name: callable}.  Warm every leg up, then `rounds` rounds in which the legs take turns."""
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            samples[name].append(timed(fn, calls))
    return {name: dict(median_ms=statistics.median(s), min_ms=min(s), max_ms=max(s), samples=len(s))
            for name, s in samples.items()}


def summarise(stats, flop):
    out = dict(legs=stats)
    base = stats["fp32"]["median_ms"]
    out["aa_spread"] = abs(stats["fp32_again"]["median_ms"] / base - 1.0)
    out["ratio_fp32_over_mode"] = {m: base / stats[m]["median_ms"] for m in MODES}
    if flop:
        out["tflops"] = {name: flop / (s["median_ms"] * 1e-3) / 1e12 for name, s in stats.items()}
    return out


def layer_legs(dev, M, N, K):
    gen = torch.Generator(device="cpu").manual_seed(1)
    a = torch.randn(M, K, generator=gen).to(dev)
    w = (torch.randn(N, K, generator=gen) / K ** 0.5).to(dev)
    b = torch.randn(N, generator=gen).to(dev)
    c = torch.empty(M, N, device=dev)
    lib, st = L.lib(), L.stream()
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def f32():
        L.check(lib.plnerf_gemm_f32(p(a), K, 1, p(w), 1, K, p(b), None, M, N, K, 1, 0, 0, p(c), N, 1, None, st), "plnerf_gemm_f32")

    def h16(mode):
        code = L.PRECISION[mode]
        return lambda: L.check(lib.plnerf_gemm_h16(p(a), K, p(w), K, p(b), M, N, K, 1, code, p(c), N, None, st), "plnerf_gemm_h16")
    legs = {"fp32": f32}
    legs.update({m: h16(m) for m in MODES})
    legs["fp32_again"] = f32
    return legs


def render_legs(dev, rays, n_samples, n_importance):
    emb, ic = P.get_embedder(10, 0)
    embd, icv = P.get_embedder(4, 0)
    torch.manual_seed(2)
    nets = [P.NeRF(D=8, W=512, input_ch=ic, input_ch_views=icv, output_ch=5, skips=[4], use_viewdirs=True,
                   precision="fp32").to(dev) for _ in range(2)]
    qfn = lambda inputs, viewdirs, fn: P.run_network(inputs, viewdirs, fn, emb, embd)
    gen = torch.Generator(device="cpu").manual_seed(3)
    o = (torch.tensor([0.0, 0.0, 4.0]) + 0.1 * torch.randn(rays, 3, generator=gen)).to(dev)
    d = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, -1.0]) + 0.3 * torch.randn(rays, 3, generator=gen), dim=-1).to(dev)
    K = [[1111.111, 0, 400], [0, 1111.111, 400], [0, 0, 1]]
    kw = dict(network_query_fn=qfn, perturb=0.0, N_samples=n_samples, N_importance=n_importance, network_fn=nets[0],
              network_fine=nets[1], white_bkgd=True, raw_noise_std=0.0, mode="linear", color_mode="midpoint", use_viewdirs=True,
              ndc=False)

    def leg(mode):
        def run():
            found = generic.HONOUR_PRECISION
            generic.HONOUR_PRECISION = mode != "fp32"
            for net in nets:
                net.precision = mode
            try:
                with torch.no_grad():
                    P.render(800, 800, K, chunk=rays, rays=(o, d), near=2.0, far=6.0, **kw)
            finally:
                generic.HONOUR_PRECISION = found
        return run
    legs = {"fp32": leg("fp32")}
    legs.update({m: leg(m) for m in MODES})
    legs["fp32_again"] = leg("fp32")
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generic_precision.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generic_precision.py measures on the GPU; there is none here (no fallback)")
    dev = torch.device("cuda:0")
    M, N, K = args.rows, 512, 512
    result = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, calls_per_sample=args.calls)
    result["layer"] = dict(shape=dict(M=M, N=N, K=K, bias=True, relu=True),
                           **summarise(interleave(layer_legs(dev, M, N, K), args.rounds, args.calls), 2.0 * M * N * K))
    result["render_chunk"] = dict(shape=dict(D=8, W=512, rays=args.rays, N_samples=64, N_importance=128),
                                  **summarise(interleave(render_legs(dev, args.rays, 64, 128), args.rounds, max(1, args.calls // 5)),
                                              0.0))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    for what in ("layer", "render_chunk"):
        r = result[what]
        print(f"{what}: fp32 {r['legs']['fp32']['median_ms']:.3f} ms, A/A spread {r['aa_spread']:.2%}; " +
              ", ".join(f"{m} {r['legs'][m]['median_ms']:.3f} ms (x{r['ratio_fp32_over_mode'][m]:.2f})" for m in MODES))


if __name__ == "__main__":
    main()
