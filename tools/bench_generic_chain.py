"""Same-box interleaved A/B of the layer-by-layer route's no-grad forward in the 16-bit modes: one plnerf_gemm_h16 per layer
with fp32 activations between the layers (generic.CHAIN_INFERENCE off) against ONE plnerf_generic_fwd call on 16-bit
activation planes (on).  tools/bench_generic_precision.py's protocol: every leg is warmed up, then the legs take turns round
by round -- the off-route twice per round (legs "off" and "off_again": their ratio is the A/A spread a difference has to
exceed) -- each sample timed with device events around `--calls` back-to-back calls.

Three workloads, each in every mode:
  network       a D = 8, W = 512 network (skip behind layer 4, view directions), no gradient, 196,608 embedded rows
  layer         one 512 x 512 layer (bias + ReLU) at 262,144 rows: plnerf_gemm_h16 (fp32 rows in, fp32 rows out) against the
                packed -> packed layer of plnerf_generic_fwd.  The library exports no single packed layer, so that one is
                the DIFFERENCE of two calls: a trunk of three layers minus a trunk of two (no skip, no view directions, a
                four-column head) -- one packed -> packed layer and the pack of its 512 x 512 weights
  render_chunk  render() of 4096 rays at 64 + 128 samples through a D = 8, W = 512 pair

Also reported: the bytes of workspace the one call takes for the network workload against the layered route's peak
allocation over one forward (torch.cuda.max_memory_allocated above what was allocated before it).
Writes profiles/generic_chain.json (or --out).

    python tools/bench_generic_chain.py [--rounds 10] [--calls 5] [--out profiles/generic_chain.json]"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plnerf_amd as P                      # noqa: E402
from plnerf_amd import _lib as L            # noqa: E402
from plnerf_amd import generic              # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_generic_precision import interleave              # noqa: E402

MODES = ("f16x3", "bf16x3", "f16", "bf16")


def summarise(stats):
    base = stats["off"]["median_ms"]
    return dict(legs=stats, aa_spread=abs(stats["off_again"]["median_ms"] / base - 1.0),
                ratio_off_over_on=base / stats["on"]["median_ms"])


def switched(chain, fn):
    def run():
        found = generic.HONOUR_PRECISION, generic.CHAIN_INFERENCE
        generic.HONOUR_PRECISION, generic.CHAIN_INFERENCE = True, chain
        try:
            with torch.no_grad():
                fn()
        finally:
            generic.HONOUR_PRECISION, generic.CHAIN_INFERENCE = found
    return run


def network_workload(dev, mode, rows, rounds, calls):
    emb, ic = P.get_embedder(10, 0)
    embd, icv = P.get_embedder(4, 0)
    torch.manual_seed(2)
    net = P.NeRF(D=8, W=512, input_ch=ic, input_ch_views=icv, output_ch=5, skips=[4], use_viewdirs=True, precision=mode).to(dev)
    gen = torch.Generator(device="cpu").manual_seed(3)
    x = torch.cat([emb((torch.rand(rows, 3, generator=gen) * 2 - 1).to(dev)),
                   embd(torch.nn.functional.normalize(torch.randn(rows, 3, generator=gen), dim=-1).to(dev))], -1).contiguous()
    off, on = switched(False, lambda: generic.forward(net, x)), switched(True, lambda: generic.forward(net, x))
    # the layered route's peak allocation over one forward, the one call's workspace
    off()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    off()
    torch.cuda.synchronize()
    layered_peak = torch.cuda.max_memory_allocated() - before
    on()
    out = summarise(interleave({"off": off, "on": on, "off_again": off}, rounds, calls))
    out.update(shape=dict(D=8, W=512, rows=rows), layered_peak_bytes=int(layered_peak),
               workspace_bytes=int(net.__dict__["_chain_workspace"].numel()), output_bytes=rows * 4 * 4)
    bits = []
    switched(True, lambda: bits.append(net.range_status()))()
    assert bits == [0], bits
    return out


def layer_workload(dev, mode, M, rounds, calls):
    N = K = 512
    gen = torch.Generator(device="cpu").manual_seed(1)
    a = torch.randn(M, K, generator=gen).to(dev)
    w = (torch.randn(N, K, generator=gen) / K ** 0.5).to(dev)
    b = torch.randn(N, generator=gen).to(dev)
    c = torch.empty(M, N, device=dev)
    lib, st, code = L.lib(), L.stream(), L.PRECISION[mode]
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def gemm():
        L.check(lib.plnerf_gemm_h16(p(a), K, p(w), K, p(b), M, N, K, 1, code, p(c), N, None, st), "plnerf_gemm_h16")

    def trunk(depth):
        shape = L.GenericShape(D=depth, W=N, input_ch=K, view_ch=0, use_viewdirs=0, output_ch=4, n_view_layers=0, n_skips=0)
        head_w, head_b = (torch.randn(4, N, generator=gen) / N ** 0.5).to(dev), torch.zeros(4, device=dev)
        tensors = [w, b] * depth + [head_w, head_b]
        params = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        nbytes = lib.plnerf_generic_fwd_workspace_bytes(ctypes.byref(shape), M, code)
        ws, out = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(M, 4, device=dev)

        def run(keep=(tensors, ws, out)):
            L.check(lib.plnerf_generic_fwd(ctypes.byref(shape), params, p(a), K, M, code, p(ws), nbytes, p(out), 4, None, st),
                    "plnerf_generic_fwd")
        return run
    stats = interleave({"off": gemm, "trunk2": trunk(2), "trunk3": trunk(3), "off_again": gemm}, rounds, calls)
    packed = stats["trunk3"]["median_ms"] - stats["trunk2"]["median_ms"]
    base = stats["off"]["median_ms"]
    return dict(shape=dict(M=M, N=N, K=K, bias=True, relu=True), legs=stats, packed_layer_ms=packed,
                aa_spread=abs(stats["off_again"]["median_ms"] / base - 1.0), ratio_off_over_on=base / packed,
                tflops=dict(off=2.0 * M * N * K / (base * 1e-3) / 1e12, on=2.0 * M * N * K / (packed * 1e-3) / 1e12))


def render_workload(dev, mode, rays, rounds, calls):
    emb, ic = P.get_embedder(10, 0)
    embd, icv = P.get_embedder(4, 0)
    torch.manual_seed(2)
    nets = [P.NeRF(D=8, W=512, input_ch=ic, input_ch_views=icv, output_ch=5, skips=[4], use_viewdirs=True,
                   precision=mode).to(dev) for _ in range(2)]
    qfn = lambda inputs, viewdirs, fn: P.run_network(inputs, viewdirs, fn, emb, embd)
    gen = torch.Generator(device="cpu").manual_seed(3)
    o = (torch.tensor([0.0, 0.0, 4.0]) + 0.1 * torch.randn(rays, 3, generator=gen)).to(dev)
    d = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, -1.0]) + 0.3 * torch.randn(rays, 3, generator=gen), dim=-1).to(dev)
    K = [[1111.111, 0, 400], [0, 1111.111, 400], [0, 0, 1]]
    kw = dict(network_query_fn=qfn, perturb=0.0, N_samples=64, N_importance=128, network_fn=nets[0], network_fine=nets[1],
              white_bkgd=True, raw_noise_std=0.0, mode="linear", color_mode="midpoint", use_viewdirs=True, ndc=False)
    run = lambda: P.render(800, 800, K, chunk=rays, rays=(o, d), near=2.0, far=6.0, **kw)
    off, on = switched(False, run), switched(True, run)
    out = summarise(interleave({"off": off, "on": on, "off_again": off}, rounds, calls))
    out.update(shape=dict(D=8, W=512, rays=rays, N_samples=64, N_importance=128))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rows", type=int, default=196608)
    ap.add_argument("--layer-rows", type=int, default=262144)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generic_chain.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generic_chain.py measures on the GPU; there is none here (no fallback)")
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, calls_per_sample=args.calls, network={}, layer={},
                  render_chunk={})
    for mode in MODES:
        result["network"][mode] = network_workload(dev, mode, args.rows, args.rounds, args.calls)
        result["layer"][mode] = layer_workload(dev, mode, args.layer_rows, args.rounds, args.calls)
        result["render_chunk"][mode] = render_workload(dev, mode, args.rays, args.rounds, max(1, args.calls // 3))
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    for what in ("network", "layer", "render_chunk"):
        for mode in MODES:
            r = result[what][mode]
            on = r["packed_layer_ms"] if what == "layer" else r["legs"]["on"]["median_ms"]
            print(f"{what} {mode}: off {r['legs']['off']['median_ms']:.3f} ms, on {on:.3f} ms (x{r['ratio_off_over_on']:.2f}), "
                  f"A/A spread {r['aa_spread']:.2%}" +
                  (f", workspace {r['workspace_bytes'] / 2 ** 20:.0f} MiB against a layered peak of "
                   f"{r['layered_peak_bytes'] / 2 ** 20:.0f} MiB" if what == "network" else ""))


if __name__ == "__main__":
    main()
