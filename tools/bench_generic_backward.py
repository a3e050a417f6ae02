"""Same-box interleaved A/B of the layer-by-layer route's backward: the two plnerf_gemm_f32 products of a layer (what runs
with generic.HONOUR_PRECISION_BACKWARD off) against plnerf_gemm_h16_dgrad / _wgrad in each 16-bit mode (what runs with both
switches on).

(a) raw products: dX = gate(G) W and [dW | db] = gate(G)^T [X | 1] at N = K = 512, M = 262,144 rows, through the raw entries
    (the IEEE-half modes with the max |g| word, the bf16 modes without, as the route passes it) against the same product on
    plnerf_gemm_f32 as generic._gemm issues it (its split rule for both sides);
(b) training step: forward + backward of a D = 8, W = 512 network through run_network at 196,608 rows -- both switches off
    (fp32), the forward switch alone, both switches, per mode.

Every leg is warmed up, then the legs take turns round by round -- fp32 twice per round (legs "fp32" and "fp32_again": their
ratio is the A/A spread a difference has to exceed) -- each sample timed with device events.  Per leg: the median, the
fastest and the slowest sample; per mode the ratio of medians fp32 / mode.  Writes profiles/generic_backward.json (or --out).

    python tools/bench_generic_backward.py [--rounds 10] [--calls 5] [--out profiles/generic_backward.json]"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plnerf_amd as P                                      # noqa: E402
from plnerf_amd import _lib as L                            # noqa: E402
from plnerf_amd import generic                              # noqa: E402
from bench_generic_precision import interleave              # noqa: E402

MODES = ("f16x3", "bf16x3", "f16", "bf16")
HALF = ("f16x3", "f16")


def summarise(stats, names, flop=0.0):
    """`names`: {label: leg name} whose ratio fp32 / leg is reported."""
    out = dict(legs=stats)
    base = stats["fp32"]["median_ms"]
    out["aa_spread"] = abs(stats["fp32_again"]["median_ms"] / base - 1.0)
    out["ratio_fp32_over_mode"] = {label: base / stats[leg]["median_ms"] for label, leg in names.items()}
    out["slower_than_fp32_beyond_aa"] = sorted(label for label, leg in names.items()
                                               if stats[leg]["median_ms"] > base * (1.0 + out["aa_spread"]))
    if flop:
        out["tflops"] = {name: flop / (s["median_ms"] * 1e-3) / 1e12 for name, s in stats.items()}
    return out


def product_legs(dev, M, N, K):
    """({leg: callable} for dgrad, the same for wgrad)."""
    gen = torch.Generator(device="cpu").manual_seed(1)
    grad = (torch.randn(M, N, generator=gen) * 1e-6).to(dev)
    y = torch.randn(M, N, generator=gen).to(dev)
    x = torch.randn(M, K, generator=gen).to(dev)
    w = (torch.randn(N, K, generator=gen) / K ** 0.5).to(dev)
    absmax = torch.linalg.vector_norm(grad, ord=float("inf"))
    dx, dwb = torch.empty(M, K, device=dev), torch.empty(N, K + 1, device=dev)
    splits = generic._splits(N, K + 1, M)
    partials = torch.empty(splits * N * (K + 1), device=dev)
    lib, st = L.lib(), L.stream()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def d32():
        generic._gemm(grad, N, 1, w, K, 1, M, K, N, gate=y, out=dx)

    def w32():
        generic._gemm(grad, 1, N, x, K, 1, N, K + 1, M, gate=y, ones_col=True, out=dwb)

    def d16(mode):
        code, word = L.PRECISION[mode], p(absmax if mode in HALF else None)
        return lambda: L.check(lib.plnerf_gemm_h16_dgrad(p(grad), N, p(y), N, p(w), K, M, N, K, code, word, p(dx), K, None, st),
                               "plnerf_gemm_h16_dgrad")

    def w16(mode):
        code, word = L.PRECISION[mode], p(absmax if mode in HALF else None)
        return lambda: L.check(lib.plnerf_gemm_h16_wgrad(p(grad), N, p(y), N, p(x), K, M, N, K, code, word, p(dwb), K + 1, splits,
                                                         p(partials), None, st), "plnerf_gemm_h16_wgrad")
    dlegs, wlegs = {"fp32": d32}, {"fp32": w32}
    dlegs.update({m: d16(m) for m in MODES})
    wlegs.update({m: w16(m) for m in MODES})
    dlegs["fp32_again"], wlegs["fp32_again"] = d32, w32
    return dlegs, wlegs, splits


def step_legs(dev, rows, samples=192):
    emb, ic = P.get_embedder(10, 0)
    embd, icv = P.get_embedder(4, 0)
    torch.manual_seed(2)
    net = P.NeRF(D=8, W=512, input_ch=ic, input_ch_views=icv, output_ch=5, skips=[4], use_viewdirs=True, precision="fp32").to(dev)
    rays = rows // samples
    gen = torch.Generator(device="cpu").manual_seed(3)
    pts = ((torch.rand(rays, samples, 3, generator=gen) * 2 - 1) * 1.5).to(dev)
    vd = torch.nn.functional.normalize(torch.randn(rays, 3, generator=gen), dim=-1).to(dev)
    cot = (torch.randn(rays, samples, 4, generator=gen) / (rays * samples)).to(dev)

    def leg(mode, forward_switch, backward_switch):
        def run():
            found = generic.HONOUR_PRECISION, generic.HONOUR_PRECISION_BACKWARD
            generic.HONOUR_PRECISION, generic.HONOUR_PRECISION_BACKWARD = forward_switch, backward_switch
            net.precision = mode
            try:
                net.zero_grad(set_to_none=True)
                out = P.run_network(pts, vd, net, emb, embd, netchunk=rays * samples)
                (out[..., :4] * cot).sum().backward()
            finally:
                generic.HONOUR_PRECISION, generic.HONOUR_PRECISION_BACKWARD = found
                net.precision = "fp32"
        return run
    legs = {"fp32": leg("fp32", False, False)}
    for m in MODES:
        legs[f"{m}_forward"] = leg(m, True, False)
        legs[f"{m}_both"] = leg(m, True, True)
    legs["fp32_again"] = leg("fp32", False, False)
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--step-rows", type=int, default=196608)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generic_backward.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generic_backward.py measures on the GPU; there is none here (no fallback)")
    dev = torch.device("cuda:0")
    M, N, K = args.rows, 512, 512
    result = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, calls_per_sample=args.calls)
    dlegs, wlegs, splits = product_legs(dev, M, N, K)
    same = {m: m for m in MODES}
    result["dgrad"] = dict(shape=dict(M=M, N=N, K=K, gate=True),
                           **summarise(interleave(dlegs, args.rounds, args.calls), same, 2.0 * M * N * K))
    result["wgrad"] = dict(shape=dict(M=M, N=N, K=K, gate=True, ones_column=True, k_splits=splits),
                           **summarise(interleave(wlegs, args.rounds, args.calls), same, 2.0 * M * N * (K + 1)))
    del dlegs, wlegs
    torch.cuda.empty_cache()
    names = {f"{m}_{which}": f"{m}_{which}" for m in MODES for which in ("forward", "both")}
    result["training_step"] = dict(shape=dict(D=8, W=512, rows=args.step_rows),
                                   **summarise(interleave(step_legs(dev, args.step_rows), args.rounds, max(1, args.calls // 2)), names))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    for what in ("dgrad", "wgrad", "training_step"):
        r = result[what]
        print(f"{what}: fp32 {r['legs']['fp32']['median_ms']:.3f} ms, A/A spread {r['aa_spread']:.2%}; " +
              ", ".join(f"{k} x{v:.2f}" for k, v in r["ratio_fp32_over_mode"].items()) +
              (f"; slower than fp32 beyond the spread: {r['slower_than_fp32_beyond_aa']}" if r["slower_than_fp32_beyond_aa"] else ""))


if __name__ == "__main__":
    main()
