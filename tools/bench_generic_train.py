"""Same-box interleaved A/B of one TRAINING step's network part on the layer-by-layer route in the 16-bit modes: forward and
backward of a D = 8, W = 512 network (skip behind layer 4, view directions) at 196,608 embedded rows, with both opt-ins of the
layered 16-bit route on (generic.HONOUR_PRECISION, generic.HONOUR_PRECISION_BACKWARD) and generic.CHAIN_TRAINING off -- one
autograd.Function per layer, fp32 activations split again by every tile -- against on: ONE plnerf_generic_train_fwd and ONE
plnerf_generic_train_bwd call on the saved 16-bit planes.  tools/bench_generic_chain.py's protocol: every leg is warmed up, then
the legs take turns round by round -- the off-route twice per round (legs "off" and "off_again": their ratio is the A/A spread
a difference has to exceed) -- each sample timed with device events around `--calls` back-to-back steps.

Also reported per mode and route: the host time to ENQUEUE one step (wall clock around the step without a synchronisation,
the queue drained before and after, median over the rounds), torch.cuda.max_memory_allocated over one step above what was
allocated before it, and the saved-state and workspace sizes from the entries' size queries against the fp32 activations the
layered route keeps (4 bytes per hidden element).
Writes profiles/generic_train.json (or --out).

    python tools/bench_generic_train.py [--rounds 10] [--calls 3] [--out profiles/generic_train.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plnerf_amd as P                      # noqa: E402
from plnerf_amd import _lib as L            # noqa: E402
from plnerf_amd import generic              # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_generic_precision import interleave              # noqa: E402

MODES = ("f16x3", "bf16x3", "f16", "bf16")
D, W, SKIPS = 8, 512, [4]


def switched(chain, fn):
    def run():
        found = generic.HONOUR_PRECISION, generic.HONOUR_PRECISION_BACKWARD, generic.CHAIN_TRAINING
        generic.HONOUR_PRECISION, generic.HONOUR_PRECISION_BACKWARD, generic.CHAIN_TRAINING = True, True, chain
        try:
            return fn()
        finally:
            generic.HONOUR_PRECISION, generic.HONOUR_PRECISION_BACKWARD, generic.CHAIN_TRAINING = found
    return run


def enqueue_ms(step, rounds):
    times = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        times.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
    return statistics.median(times)


def peak_bytes(step):
    step()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - before)


def workload(dev, mode, rows, rounds, calls):
    emb, ic = P.get_embedder(10, 0)
    embd, icv = P.get_embedder(4, 0)
    torch.manual_seed(2)
    net = P.NeRF(D=D, W=W, input_ch=ic, input_ch_views=icv, output_ch=5, skips=SKIPS, use_viewdirs=True, precision=mode).to(dev)
    gen = torch.Generator(device="cpu").manual_seed(3)
    x = torch.cat([emb((torch.rand(rows, 3, generator=gen) * 2 - 1).to(dev)),
                   embd(torch.nn.functional.normalize(torch.randn(rows, 3, generator=gen), dim=-1).to(dev))], -1).contiguous()
    cot = (torch.randn(rows, 4, generator=gen) * 1.0e-6).to(dev)

    def step(expect):
        def run():
            assert generic.chains_training(net, x) is expect
            net.zero_grad(set_to_none=True)
            (generic.forward(net, x) * cot).sum().backward()
        return run
    off, on = switched(False, step(False)), switched(True, step(True))
    out = dict(legs=interleave({"off": off, "on": on, "off_again": off}, rounds, calls))
    base = out["legs"]["off"]["median_ms"]
    out.update(aa_spread=abs(out["legs"]["off_again"]["median_ms"] / base - 1.0),
               ratio_off_over_on=base / out["legs"]["on"]["median_ms"],
               enqueue_ms=dict(off=enqueue_ms(off, rounds), on=enqueue_ms(on, rounds)),
               peak_bytes=dict(off=peak_bytes(off), on=peak_bytes(on)))
    shape = L.GenericShape(D=D, W=W, input_ch=ic, view_ch=icv, use_viewdirs=1, output_ch=0, n_view_layers=1, n_skips=1)
    shape.skips[0] = SKIPS[0]
    code = L.PRECISION[mode]
    hidden = rows * (D * W + W // 2)
    out.update(shape=dict(D=D, W=W, skips=SKIPS, rows=rows),
               saved_bytes=int(L.lib().plnerf_generic_train_saved_bytes(ctypes.byref(shape), rows, code)),
               workspace_bytes=int(L.lib().plnerf_generic_train_workspace_bytes(ctypes.byref(shape), rows, code)),
               layered_fp32_activation_bytes=hidden * 4, hidden_elements=hidden)
    bits = switched(True, lambda: net.range_status())()
    assert bits == 0, bits
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rows", type=int, default=196608)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generic_train.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generic_train.py measures on the GPU; there is none here (no fallback)")
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, calls_per_sample=args.calls, step={})
    for mode in MODES:
        result["step"][mode] = workload(dev, mode, args.rows, args.rounds, args.calls)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    for mode in MODES:
        r = result["step"][mode]
        print(f"{mode}: off {r['legs']['off']['median_ms']:.3f} ms, on {r['legs']['on']['median_ms']:.3f} ms "
              f"(x{r['ratio_off_over_on']:.2f}), A/A spread {r['aa_spread']:.2%}; enqueue {r['enqueue_ms']['off']:.2f} -> "
              f"{r['enqueue_ms']['on']:.2f} ms; peak {r['peak_bytes']['off'] / 2 ** 20:.0f} -> {r['peak_bytes']['on'] / 2 ** 20:.0f} MiB; "
              f"saved {r['saved_bytes'] / 2 ** 20:.0f} MiB + workspace {r['workspace_bytes'] / 2 ** 20:.0f} MiB against "
              f"{r['layered_fp32_activation_bytes'] / 2 ** 20:.0f} MiB of fp32 activations")


if __name__ == "__main__":
    main()
