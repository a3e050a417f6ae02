"""Guard-band cases of the experimental header include/experimental/plnerf_hip_camcode.h, described with the machinery of
tests/containment.py (imported, not edited: that table is the registered ABI's), as tests/depthview_cases.py does for its
header.  tests/test_gpu_camcode.py runs each through containment.run_case; tests/test_camcode_abi.py builds them on the CPU,
holds every call to its prototype and requires a case for every entry of the header that takes a stream."""
import math

import torch

import containment as C
from containment import IN, OUT, SCRATCH, Call, given, out

NO_DEVICE_WRITES = {"plnerf_camcode_sweep_workspace_bytes"}      # takes no stream: it cannot enqueue anything
KEPT = 7.5                                                       # the word in front of an input handed over at an offset


def sweep_inputs(n_rays, rows_per_ray, width, n_cam, tag, stride_extra=3, bkgd=True, gen=None):
    """Random inputs of one sweep (CPU tensors, fp32): A, coef (a quarter exact zeros, ray 0 all zero when there are several),
    cam, the weight matrix the code's columns sit in ([width, stride] with the columns at its end), w_rgb, b_rgb, target,
    bkgd, ray_weight (unequal; one ray of weight zero when there are three or more)."""
    gen = gen or C._gen(f"camcode-{tag}")
    n_rows = n_rays * rows_per_ray
    A = torch.randn(n_rows, width, generator=gen)
    coef = torch.rand(n_rows, generator=gen) / rows_per_ray
    coef[torch.rand(n_rows, generator=gen) < 0.25] = 0.0
    if n_rays > 1:
        coef[:rows_per_ray] = 0.0
    stride = width + 3 + n_cam if stride_extra else n_cam
    view_w = torch.randn(width, stride, generator=gen) * 0.5
    lam = (0.5 + torch.rand(n_rays, generator=gen)) / (3.0 * n_rays)
    if n_rays >= 3:
        lam[n_rays // 2] = 0.0
    return dict(A=A, coef=coef, cam=torch.randn(n_cam, generator=gen) * 0.7, view_w=view_w,
                w_rgb=torch.randn(3, width, generator=gen) / math.sqrt(width), b_rgb=torch.randn(3, generator=gen) * 0.3,
                target=torch.rand(n_rays, 3, generator=gen), bkgd=torch.rand(n_rays, generator=gen) * 0.2 if bkgd else None,
                ray_weight=lam, stride=stride)


def sweep_case(L, n_rays, rows_per_ray, width, n_cam, odd=False):
    """plnerf_camcode_sweep with a workspace of exactly the size query's bytes (scratch: it need not be zeroed).  odd: A and
    every fp32 input 4 bytes off their buffers' starts (the header asks fp32 pointers for 4-byte alignment only; A then
    takes the 4-byte loads) and g_cam in the middle of a buffer whose other words must stay untouched."""
    tag = f"{n_rays}x{rows_per_ray}x{width}x{n_cam}{'odd' if odd else ''}"
    d = sweep_inputs(n_rays, rows_per_ray, width, n_cam, tag)
    nbytes = int(L.lib().plnerf_camcode_sweep_workspace_bytes(n_rays))
    assert nbytes > 0 and nbytes % 256 == 0
    ws = out(f"cc_ws_{tag}", "u8", nbytes, align=256, opaque=True)
    off = 4 if odd else 0

    def inp(name, t):
        if odd:      # one word of padding in front: the pointer handed over is 4 bytes into the buffer
            t = torch.cat([torch.full((1,), KEPT), t.reshape(-1)])
        return IN(given(f"cc_{name}_{tag}", "f32", t, align=16), offset=off)
    n_cols = d["stride"]
    w_cam_offset = off + 4 * (n_cols - n_cam)
    loss = out(f"cc_loss_{tag}", "f64", 1, align=8)
    if odd:
        untouched = torch.ones(n_cam + 2, dtype=torch.bool)
        untouched[1:1 + n_cam] = False
        g_cam = OUT(out(f"cc_g_cam_{tag}", "f32", n_cam + 2, untouched=untouched), offset=4)
    else:
        g_cam = OUT(out(f"cc_g_cam_{tag}", "f32", n_cam))
    view_w = inp("view_w", d["view_w"])
    view_w.offset = w_cam_offset
    return [Call("plnerf_camcode_sweep", inp("A", d["A"]), inp("coef", d["coef"]), n_rays * rows_per_ray, rows_per_ray, width,
                 inp("cam", d["cam"]), n_cam, view_w, n_cols, inp("w_rgb", d["w_rgb"]), inp("b_rgb", d["b_rgb"]),
                 inp("target", d["target"]), inp("bkgd", d["bkgd"]), inp("ray_weight", d["ray_weight"]), SCRATCH(ws), nbytes,
                 OUT(loss), g_cam)]


def state_bytes(L, n_cam, lr=0.5):
    """A fresh plnerf_camcode_state as a uint8 tensor."""
    host = L.CamcodeState(lr=lr, best=-math.inf, best_iter=-1)
    return torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).clone()


def update_case(L, n_cam, n_history):
    """plnerf_camcode_update, two iterations on one state: the histories get entries 0 and 1 and no others (with
    n_history = 1: entry 0 alone), the state's bytes behind best_iter do not exist."""
    tag = f"{n_cam}h{n_history}"
    gen = C._gen(f"camcode-update-{tag}")
    state = given(f"cu_state_{tag}", "u8", state_bytes(L, n_cam), align=4)
    grads = [given(f"cu_grad{k}_{tag}", "f32", torch.randn(n_cam, generator=gen)) for k in range(2)]
    losses = [given(f"cu_loss{k}_{tag}", "f64", torch.tensor([0.02 / (k + 1)], dtype=torch.float64), align=8) for k in range(2)]
    untouched = torch.ones(n_history + 1, dtype=torch.bool)
    untouched[1:1 + min(2, n_history)] = False
    hist = [out(f"cu_{name}_{tag}", "f32", n_history + 1, untouched=untouched) for name in ("psnr", "lr")]
    return [Call("plnerf_camcode_update", C.INOUT(state), n_cam, IN(losses[k]), IN(grads[k]), 2, 0.9, 0.999, 1e-8, 0.5, 3,
                 OUT(hist[0], offset=4), OUT(hist[1], offset=4), n_history) for k in range(2)]


def all_cases():
    """(case id, builder taking the binding) of every guard-band case of the header."""
    return ([(f"camcode_sweep-{r}x{s}x{w}x{c}{'-odd' if odd else ''}", lambda L, a=(r, s, w, c, odd): sweep_case(L, *a))
             for r, s, w, c, odd in ((1, 1, 128, 4, False), (1, 1, 4, 1, True), (5, 3, 7, 29, True), (37, 65, 32, 4, False))] +
            [(f"camcode_update-c{c}-h{h}", lambda L, a=(c, h): update_case(L, *a)) for c, h in ((1, 1), (32, 5))])
