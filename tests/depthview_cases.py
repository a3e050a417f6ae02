"""Guard-band cases of the experimental header include/experimental/plnerf_hip_depthview.h, described with the machinery of
tests/containment.py (imported, not edited: that table is the registered ABI's).  tests/test_gpu_depth_view.py runs each
through containment.run_case; tests/test_depthview_abi.py builds them on the CPU, holds every call to its prototype and
requires a case for every experimental entry that takes a stream."""
import ctypes

import torch

import containment as C
from containment import IN, OUT, SCRATCH, Call, HostArray, Struct, given, out

H, W = C.ONE_CALL_H, C.ONE_CALL_W      # 9 x 11: 99 pixels
INTRINSIC = (12.5, 11.5, 5.5, 4.5)
KEPT = 0x1234                          # what export_case's second output holds before the call
NO_DEVICE_WRITES = {"plnerf_depth_render_view_workspace_bytes"}      # takes no stream: it cannot enqueue anything


def rays_case(R):
    """plnerf_depth_view_rays on the last R pixels with every output, and on the first R without view directions."""
    rays = lambda t: [OUT(out(f"{t}rays_o", "f32", R, 3)), OUT(out(f"{t}rays_d", "f32", R, 3))]
    nf = lambda t: [OUT(out(f"{t}near", "f32", R)), OUT(out(f"{t}far", "f32", R))]
    c2w = HostArray(ctypes.c_float, C.ONE_CALL_C2W)
    return [
        Call("plnerf_depth_view_rays", H, W, *INTRINSIC, c2w, H * W - R, R, 2.0, 6.0, *rays("dv_"),
             OUT(out("dv_viewdirs", "f32", R, 3)), *nf("dv_")),
        Call("plnerf_depth_view_rays", H, W, *INTRINSIC, c2w, 0, R, 2.0, 6.0, *rays("dvn_"), None, *nf("dvn_")),
    ]


def export_case(n):
    """plnerf_frame_export_u16 into exactly 2 n bytes at a word-aligned address, and 2 bytes off one: into a buffer of n + 1
    values that starts as KEPT everywhere, whose first value the call must leave alone."""
    gray = given("gray", "f32", torch.linspace(-1.0, 70.0, n) if n > 1 else torch.tensor([3.25]))
    odd = given("mm16_odd", "u16", torch.full((n + 1,), KEPT, dtype=torch.int16), align=4)
    return [Call("plnerf_frame_export_u16", IN(gray), 1000.0, OUT(out("mm16", "u16", n, align=4)), n),
            Call("plnerf_frame_export_u16", IN(gray), 1000.0, C.INOUT(odd, offset=2), n)]


def view_config(L, mode, precision="f16x3", max_rays=32, draws=False):
    cfg = L.DepthViewConfig()
    cfg.max_rays, cfg.n_samples, cfg.n_importance = max_rays, C.ONE_CALL_SAMPLES, C.ONE_CALL_IMPORTANCE
    cfg.mode, cfg.color_mode, cfg.lindisp, cfg.perturb, cfg.white_bkgd = mode, 0, 0, 1 if draws else 0, 1
    cfg.raw_noise_std, cfg.zero_tol, cfg.epsilon = 0.5 if draws else 0.0, C.ZERO_TOL, C.EPSILON
    cfg.H, cfg.W, cfg.near, cfg.far = H, W, 2.0, 6.0
    cfg.precision, cfg.fwd_kernel, cfg.input_ch, cfg.input_ch_views = C.PRECISIONS[precision], 0, 63, 27
    cfg.input_scale, cfg.density_beta, cfg.seed = 1.0, 10.0, C.SEED
    return cfg


def view_case(L, mode, precision="f16x3", draws=False):
    """plnerf_depth_render_view on the 9 x 11 view in blocks of 32 pixels (99 = 3 * 32 + 3): the whole frame with every
    plane, the hypotheses, valid + error_row and the three exports, then pixels [5, 45) with every nullable plane left out
    but valid + error_row (the hypotheses then live in the workspace only) -- the frame's other pixels stay untouched.  The
    workspace is exactly the size query's bytes, and need not be zeroed: scratch.  draws: jitter and density noise 0.5 on, so
    the noise planes of the workspace, the scaling launch and the draws inside the kernels are under the guard bands too."""
    cfg = view_config(L, mode, precision, draws=draws)
    nbytes = int(L.lib().plnerf_depth_render_view_workspace_bytes(ctypes.byref(cfg)))
    assert nbytes > 0
    ws = out("workspace", "u8", nbytes, align=256, opaque=True)
    coarse, fine = C._Net(L, "c_", precision, train=False), C._Net(L, "f_", precision, train=False)
    t_vals = given("t_vals", "f32", torch.linspace(0., 1., C.ONE_CALL_SAMPLES))
    u_vals = given("u_vals", "f32", torch.linspace(0., 1., C.ONE_CALL_IMPORTANCE))
    n, N = H * W, C.ONE_CALL_IMPORTANCE
    planes = {name: out(f"plane_{name}", "f32", *((n, 3) if name in ("rgb", "rgb0") else (n,))) for name in L.VIEW_PLANES}
    hyp = out("plane_pred_hyp", "f32", n, N)
    valid = given("valid", "u8", torch.rand(n, generator=C._gen("dv_valid")) > 0.3)
    rows = [given(f"error_row{k}", "f64", torch.zeros(2, dtype=torch.float64), align=8) for k in range(2)]
    rgb8, depth16, mm16 = out("rgb8", "u8", n, 3), out("depth16", "u16", n), out("depth_mm16", "u16", n)
    outside = torch.ones(n, 3, dtype=torch.bool)
    outside[5:45] = False
    part = out("part_rgb", "f32", n, 3, untouched=outside)
    nets = coarse.view_refs() + fine.view_refs() + [IN(t_vals), IN(u_vals), IN(valid)]

    def build_io(addr, full):
        io = L.DepthViewIo()
        coarse.fill_view_net(io.coarse, addr)
        fine.fill_view_net(io.fine, addr)
        io.t_vals, io.u_vals, io.valid = addr(IN(t_vals)), addr(IN(u_vals)), addr(IN(valid))
        io.error_row = addr(C.INOUT(rows[0 if full else 1]))
        if full:
            for name in L.VIEW_PLANES:
                setattr(io, name, addr(OUT(planes[name])))
            io.pred_hyp = addr(OUT(hyp))
            io.rgb8, io.depth16, io.depth_mm16 = addr(OUT(rgb8)), addr(OUT(depth16)), addr(OUT(mm16))
        else:
            io.rgb = addr(OUT(part))
        return io

    def build_args(addr, full):
        a = L.DepthViewArgs()
        a.c2w[:] = C.ONE_CALL_C2W
        a.fx, a.fy, a.cx, a.cy = INTRINSIC
        a.step, a.pix0, a.n_pix, a.pack_weights = 3, 0 if full else 5, n if full else 40, 1
        a.depth16_scale, a.depth_mm_mult = 1.0 / 6.0, 1000.0
        return a

    return [
        Call("plnerf_depth_render_view", Struct([], lambda addr: cfg),
             Struct(nets + [OUT(p) for p in planes.values()] + [OUT(hyp), C.INOUT(rows[0]), OUT(rgb8), OUT(depth16), OUT(mm16)],
                    lambda addr: build_io(addr, True)),
             Struct([], lambda addr: build_args(addr, True)), SCRATCH(ws), nbytes),
        Call("plnerf_depth_render_view", Struct([], lambda addr: cfg),
             Struct(nets + [OUT(part), C.INOUT(rows[1])], lambda addr: build_io(addr, False)),
             Struct([], lambda addr: build_args(addr, False)), SCRATCH(ws), nbytes),
    ]


def all_cases():
    """(case id, builder taking the binding) of every guard-band case of the experimental header."""
    return ([(f"depth_view_rays-R{R}", lambda L, R=R: rays_case(R)) for R in (1, 5, 67)] +
            [(f"frame_export_u16-n{n}", lambda L, n=n: export_case(n)) for n in (1, 1003)] +
            [("depth_render_view-linear", lambda L: view_case(L, C.MODE_LINEAR)),
             ("depth_render_view-linear-draws", lambda L: view_case(L, C.MODE_LINEAR, draws=True)),
             ("depth_render_view-constant", lambda L: view_case(L, C.MODE_CONSTANT))])
