"""Test-time camera-code optimisation on a real MI355X: plnerf_camcode_sweep and plnerf_camcode_update
(include/experimental/plnerf_hip_camcode.h), the cache build of camcode.CameraCodeOptimizer, both routes of
camcode.optimize_camera_embedding against fixture g10_camera_code_opt.npz (the reference's own run), the hooks in the depth
script's two evaluation loops, and the guard bands of tests/camcode_cases.py.

Bounds.  The sweep: its distance from fp64 autograd on identical inputs is at most 4 x the distance of the same expression
evaluated by torch in fp32 on the device (loss relative to the loss, gradient relative to its largest entry); inputs are
nudged so that no |A + W_cam cam| lies below 1e-4 and relu's mask is the same in every arithmetic.  The cache: the generic
route's bound of tests/test_gpu_modes.py, 1e-5 (1 + max |reference|); the sample depths bit for bit.  The update kernel: the
learning rates and the best index exactly, the codes within tests/test_gpu_step.py's Adam tolerance 2e-6.  The routes against
the fixture: tests/test_camopt_host.py's bounds."""
import ctypes
import json
import math
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import camcode_cases as cases
import camopt_fp64 as R
import containment as C
from camopt_fp64 import CODE_TOL, GRAD_BOUND, LOSS_BOUND
from gpu_support import P, dev      # (not its helper g: `g` is this file's fixture)
from run_args import depth_args

pytestmark = pytest.mark.gpu
GENERIC_TOL = 1e-5      # tests/test_gpu_modes.py: the generic route against fp64, times (1 + max |reference|)
BOUNDS = {}             # what the sweep cases measured; written to $PLNERF_CAMCODE_BOUNDS_OUT when that is set


@pytest.fixture(scope="module")
def g():
    return R.fixture()


# ----------------------------------------------------------------------------- 4. the sweep against fp64 autograd
GROUPS = 2048      # PLNERF_CAMCODE_MAX_GROUPS: rays are dealt round-robin over at most this many workgroups
SWEEP_SHAPES = [   # (n_rays, rows_per_ray, width, n_cam, bkgd)
    (1, 1, 4, 1, True), (37, 1, 128, 29, False), (1, 2, 32, 4, False), (37, 2, 4, 29, True), (1, 63, 128, 4, True),
    (37, 63, 32, 1, False), (1, 64, 32, 29, False), (37, 64, 128, 1, True), (1, 65, 4, 4, False), (37, 65, 128, 4, True),
    (1, 192, 128, 29, True), (37, 192, 32, 4, False), (1, 1024, 32, 1, True), (37, 1024, 128, 4, False),
    (GROUPS + 1, 2, 32, 4, True), (GROUPS + 1, 65, 4, 29, False)]


def _sweep_call(L, t, n_rays, rows_per_ray, width, n_cam):
    ws = torch.empty(L.lib().plnerf_camcode_sweep_workspace_bytes(n_rays), dtype=torch.uint8, device=dev())
    loss = torch.full((1,), float("nan"), dtype=torch.float64, device=dev())
    g_cam = torch.full((n_cam,), float("nan"), device=dev())
    w_cam = ctypes.c_void_p(t["view_w"].data_ptr() + 4 * (t["view_w"].shape[1] - n_cam))
    L.check(L.lib().plnerf_camcode_sweep(
        L.dptr(t["A"]), L.dptr(t["coef"]), n_rays * rows_per_ray, rows_per_ray, width, L.dptr(t["cam"]), n_cam, w_cam,
        t["view_w"].shape[1], L.dptr(t["w_rgb"]), L.dptr(t["b_rgb"]), L.dptr(t["target"]), L.dptr(t["bkgd"]),
        L.dptr(t["ray_weight"]), L.dptr(ws, "ws", torch.uint8), ws.numel(), L.dptr(loss, "loss", torch.float64), L.dptr(g_cam),
        L.stream()), "plnerf_camcode_sweep")
    return loss, g_cam


def _torch_objective(d, dtype, device, n_rays, rows_per_ray, width, n_cam):
    to = lambda x: None if x is None else x.to(device=device, dtype=dtype)
    cam = to(d["cam"]).clone().requires_grad_(True)
    loss = R.objective(to(d["A"]).reshape(n_rays, rows_per_ray, width), to(d["coef"]).reshape(n_rays, rows_per_ray),
                       to(d["view_w"])[:, -n_cam:], to(d["w_rgb"]), to(d["b_rgb"]), to(d["target"]), to(d["bkgd"]),
                       to(d["ray_weight"]), cam)
    loss.backward()
    return loss.detach().cpu().double(), cam.grad.detach().cpu().double()


@pytest.mark.parametrize("n_rays,rows_per_ray,width,n_cam,bkgd", SWEEP_SHAPES, ids=lambda v: str(v))
def test_sweep_against_fp64_autograd(P, n_rays, rows_per_ray, width, n_cam, bkgd):
    L = P._lib
    d = cases.sweep_inputs(n_rays, rows_per_ray, width, n_cam, "gpu", bkgd=bkgd,
                           gen=torch.Generator().manual_seed(1000 * n_rays + 10 * rows_per_ray + width + n_cam))
    assert bool((d["coef"] == 0).any()) or n_rays * rows_per_ray < 4
    if n_rays > 1:
        assert not d["coef"][:rows_per_ray].any()                  # one all-zero ray
    if n_rays >= 3:
        assert int((d["ray_weight"] == 0).sum()) == 1                # one ray of weight zero
    assert n_rays == 1 or float(d["ray_weight"].max()) > float(d["ray_weight"][d["ray_weight"] > 0].min())
    # no pre-activation within 1e-4 of zero: nudge the offenders, then assert in fp64 that none is left
    shift = (d["view_w"][:, -n_cam:].double() @ d["cam"].double())
    z = d["A"].double() + shift
    near = z.abs() < 2e-4
    d["A"][near] = (d["A"].double()[near] + torch.where(z[near] >= 0, 1e-3, -1e-3)).float()
    assert float((d["A"].double() + shift).abs().min()) >= 1e-4

    l64, g64 = _torch_objective(d, torch.float64, "cpu", n_rays, rows_per_ray, width, n_cam)
    l32, g32 = _torch_objective(d, torch.float32, dev(), n_rays, rows_per_ray, width, n_cam)
    t = {k: (v.to(dev()).contiguous() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    loss, g_cam = _sweep_call(L, t, n_rays, rows_per_ray, width, n_cam)
    loss2, g_cam2 = _sweep_call(L, t, n_rays, rows_per_ray, width, n_cam)
    torch.cuda.synchronize()
    assert torch.equal(loss.view(torch.int64), loss2.view(torch.int64))                  # two launches: the same bits
    assert torch.equal(g_cam.view(torch.int32), g_cam2.view(torch.int32))
    g_scale = max(float(g64.abs().max()), 1e-300)
    l_scale = max(abs(float(l64)), 1e-300)
    kernel = (abs(float(loss.cpu()[0]) - float(l64)) / l_scale, float((g_cam.cpu().double() - g64).abs().max()) / g_scale)
    torch32 = (abs(float(l32) - float(l64)) / l_scale, float((g32 - g64).abs().max()) / g_scale)
    BOUNDS[f"{n_rays}x{rows_per_ray}x{width}x{n_cam}{'+bkgd' if bkgd else ''}"] = {
        "kernel_loss": kernel[0], "torch_fp32_loss": torch32[0], "kernel_grad": kernel[1], "torch_fp32_grad": torch32[1]}
    print(f"sweep {n_rays} x {rows_per_ray} x {width}, n_cam {n_cam}: kernel loss {kernel[0]:.2e} grad {kernel[1]:.2e}; "
          f"torch fp32 loss {torch32[0]:.2e} grad {torch32[1]:.2e}")
    path = os.environ.get("PLNERF_CAMCODE_BOUNDS_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(BOUNDS, f, indent=1, sort_keys=True)
    assert kernel[0] <= 4 * torch32[0] and kernel[1] <= 4 * torch32[1]


def test_sweep_zero_rays_and_refusals(P):
    L = P._lib
    p = ctypes.c_void_p(256)
    loss = torch.full((1,), 3.0, dtype=torch.float64, device=dev())
    g_cam = torch.full((4,), 3.0, device=dev())
    rc = L.lib().plnerf_camcode_sweep(None, None, 0, 8, 64, None, 4, None, 71, None, None, None, None, None, None, 0,
                                      L.dptr(loss, "loss", torch.float64), L.dptr(g_cam), L.stream())
    torch.cuda.synchronize()
    assert rc == 0 and float(loss[0]) == 3.0 and bool((g_cam == 3.0).all())      # nothing launched, nothing written
    assert L.lib().plnerf_camcode_sweep(p, p, 16, 8, 129, p, 4, p, 71, p, p, p, None, p, p, 1 << 21, p, p, L.stream()) == -1


# ----------------------------------------------------------------------------- the fixture's scene on the device
def _args(**over):
    """The fixture's run: a 4-wide camera code, 8 + 8 samples without jitter, exact fp32; no loss fields."""
    at = dict(input_ch_cam=4, N_importance=8, N_samples=8, perturb=0.0, precision="fp32", chunk=1024, N_rand=6, dataset="scannet")
    return depth_args(train=False, **dict(at, **over))


def _fixture_scene(P, g, **over):
    from plnerf_amd import depth as Dp
    args = _args(**over)
    _, kw, _, _, _ = Dp.create_nerf(args, device=dev())
    for net, sd in zip((kw["network_fn"], kw["network_fine"]), R.state_dicts(g, torch.float32)):
        net.load_state_dict(sd)
        net.requires_grad_(False)
    kw.update(near=float(g["near"]), far=float(g["far"]))
    pose = torch.from_numpy(g["pose"]).to(dev())
    intrinsic = torch.from_numpy(g["intrinsic"]).to(dev())
    image = torch.from_numpy(g["image"]).to(dev())
    return Dp, args, kw, pose, intrinsic, image


@pytest.fixture(scope="module")
def scene(P, g):
    return _fixture_scene(P, g)


@pytest.fixture(scope="module")
def fast(P, g, scene):
    Dp, args, kw, pose, intrinsic, image = scene
    return P.CameraCodeOptimizer(kw, int(g["H"]), int(g["W"]), args).build(image, pose, intrinsic)


# ----------------------------------------------------------------------------- 5. the cache build
def _check_cache(P, Dp, args, kw, opt, pose, intrinsic, H, W):
    net = kw["network_fine"]
    n_cam, width = net.input_ch_cam, net.W // 2
    S = args.N_samples + args.N_importance
    with torch.no_grad():
        rays_o, rays_d = Dp.get_rays(H, W, intrinsic, pose)
        from plnerf_amd import raybatch as RB
        rows, _ = RB.pack_rays(rays_o, rays_d, kw["near"], kw["far"], [RB.unit_directions(rays_d)])
        rr = {k: v for k, v in kw.items() if k not in ("near", "far", "use_viewdirs", "embedded_cam")}
        gen = torch.Generator().manual_seed(3)
        worst_rgb = 0.0
        for _ in range(2):
            cam = (torch.randn(n_cam, generator=gen) * 0.8).to(dev())
            ret = Dp.render_rays(rows, True, embedded_cam=cam, retraw=True, **rr)
            assert torch.equal(ret["z_vals"].view(torch.int32), opt.z_vals.view(torch.int32))      # depths: bit for bit
            vw = net.views_linears[0].weight
            z = opt.A + vw[:, vw.shape[1] - n_cam:] @ cam
            rgb = torch.relu(z) @ net.rgb_linear.weight.T + net.rgb_linear.bias
            # net.forward in precision "fp32" on the same rows: the first three columns of raw
            ref = ret["raw"][..., :3].reshape(-1, 3)
            err = float((rgb - ref).abs().max())
            worst_rgb = max(worst_rgb, err)
            assert err <= GENERIC_TOL * (1.0 + float(ref.abs().max())), err
            full = Dp.raw2outputs(ret["raw"], ret["z_vals"], rows[:, 6:7], rows[:, 7:8], rows[:, 3:6].contiguous(),
                                  args.mode, args.color_mode, white_bkgd=args.white_bkgd)
            coef = P.camcode.coef_from_weights(full[3], args.mode, args.color_mode).reshape(-1)
            cerr = float((opt.coef - coef).abs().max())
            assert cerr <= GENERIC_TOL * (1.0 + float(coef.abs().max())), cerr
            if args.white_bkgd:
                assert float((opt.bkgd - (1.0 - full[2])).abs().max()) <= GENERIC_TOL * 2
    assert opt.A.shape == (H * W * S, width) and opt.coef.shape == (H * W * S,)
    return worst_rgb


def test_cache_build_fixture_scene(P, g, scene, fast):
    Dp, args, kw, pose, intrinsic, image = scene
    worst = _check_cache(P, Dp, args, kw, fast, pose, intrinsic, int(g["H"]), int(g["W"]))
    print(f"cache, netwidth 256: head rebuilt from A against net.forward {worst:.2e}")


def test_cache_build_netwidth_64(P, g):
    from plnerf_amd import depth as Dp
    args = _args(netwidth=64, netwidth_fine=64, N_samples=7, N_importance=6, color_mode="left", white_bkgd=False)
    torch.manual_seed(11)
    _, kw, _, _, _ = Dp.create_nerf(args, device=dev())
    with torch.no_grad():
        for net in (kw["network_fn"], kw["network_fine"]):      # biases off zero, a density that meets something
            for prm in net.parameters():
                if prm.dim() == 1:
                    prm.add_(torch.randn_like(prm) * 0.05)
            net.alpha_linear.weight.mul_(20.0)
            net.requires_grad_(False)
    kw.update(near=2.0, far=6.0)
    H, W = 5, 7
    pose = torch.from_numpy(g["pose"]).to(dev())
    intrinsic = torch.tensor([6.3, 5.9, 3.4, 2.6], device=dev())
    image = torch.rand(H, W, 3, device=dev())
    assert P.CameraCodeOptimizer.unsupported_reason(kw, args, H, W, 32 << 30) is None
    opt = P.CameraCodeOptimizer(kw, H, W, args).build(image, pose, intrinsic)
    worst = _check_cache(P, Dp, args, kw, opt, pose, intrinsic, H, W)
    print(f"cache, netwidth 64: head rebuilt from A against net.forward {worst:.2e}")
    # the sweep on this cache against the plain route's autograd, at a random code
    cam = torch.tensor([0.3, -0.5, 0.2, 0.7])
    lf, gf = opt.loss_and_grad(cam)
    lp, gp = P.camcode.plain_loss_and_grad(cam, image, pose, H, W, intrinsic, args, kw)
    assert abs(lf - float(lp)) <= 1e-4 * abs(float(lp))
    assert float((gf - gp).abs().max()) <= 1e-3 * float(gp.abs().max())


def test_routes_refuse_what_they_do_not_serve(P, scene, g):
    Dp, args, kw, pose, intrinsic, image = scene
    H, W = int(g["H"]), int(g["W"])
    reason = P.CameraCodeOptimizer.unsupported_reason
    assert reason(kw, args, H, W, 32 << 30) is None
    assert "cache_bytes_limit" in reason(kw, args, H, W, 1000)
    assert "pytest" in reason(dict(kw, pytest=True), args, H, W, 32 << 30)
    assert "c2w_staticcam" in reason(dict(kw, c2w_staticcam=pose), args, H, W, 32 << 30)
    assert "draws" in reason(dict(kw, perturb=1.0), args, H, W, 32 << 30)
    with pytest.raises(NotImplementedError, match="cache_bytes_limit"):
        P.optimize_camera_embedding(image, pose, H, W, intrinsic, args, dict(kw), route="fast", cache_bytes_limit=1000)
    assert 28.0e9 < 468 * 624 * 192 * 128 * 4 < (32 << 30)      # the 468 x 624 view at 64 + 128 samples is admitted


# ----------------------------------------------------------------------------- 6. the update kernel
def _run_updates(P, grads, losses, n_batches, n_cam):
    """The update kernel fed a gradient and loss sequence: (codes after every step [n, n_cam], lr [n], psnr [n], state)."""
    L = P._lib
    n = grads.shape[0]
    state = cases.state_bytes(L, n_cam).to(dev())
    gd, ld = grads.to(dev()).float().contiguous(), losses.to(dev()).double().contiguous()
    psnr, lrs = torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    codes = torch.zeros(n, n_cam, device=dev())
    for i in range(n):
        L.check(L.lib().plnerf_camcode_update(ctypes.c_void_p(state.data_ptr()), n_cam, ctypes.c_void_p(ld.data_ptr() + 8 * i),
                                              ctypes.c_void_p(gd.data_ptr() + 4 * n_cam * i), n_batches, 0.9, 0.999, 1e-8, 0.5,
                                              3, L.dptr(psnr), L.dptr(lrs), n, L.stream()), "plnerf_camcode_update")
        codes[i].copy_(state[:4 * n_cam].view(torch.float32))
    back = L.CamcodeState.from_buffer_copy(state.cpu().numpy().tobytes())
    return codes.cpu(), lrs.cpu(), psnr.cpu(), back


def test_update_kernel_on_the_recorded_run(P, g):
    n_cam = int(g["n_cam"])
    codes, lrs, psnr, back = _run_updates(P, torch.from_numpy(g["grad"]), torch.from_numpy(g["loss_sum"]), int(g["n_batches"]),
                                          n_cam)
    assert np.array_equal(lrs.double().numpy(), g["lr"])                                  # exactly
    assert back.best_iter == int(g["best_iter"]) and back.step == 100                       # exactly
    worst = float((codes[:-1] - torch.from_numpy(g["cam"][1:])).abs().max())
    print(f"update kernel against the recorded codes: {worst:.2e}; psnr {float((psnr - torch.from_numpy(g['psnr'])).abs().max()):.2e}")
    assert worst <= CODE_TOL
    assert float((torch.tensor(list(back.best_cam)[:n_cam]) - torch.from_numpy(g["best_cam"])).abs().max()) <= CODE_TOL
    assert torch.equal(torch.tensor(list(back.best_cam)[:n_cam]), codes[back.best_iter])    # the code AFTER that step
    assert abs(back.max_psnr - float(g["best_psnr"])) <= 1e-4
    assert float((psnr - torch.from_numpy(g["psnr"])).abs().max()) <= 1e-4


def test_update_kernel_on_a_plateau_against_torch(P):
    """A synthetic run whose PSNR climbs, sits on a plateau until the learning rate has halved twice, climbs again and
    plateaus again; the gaps are 0 or 1 dB, well clear of the scheduler's relative threshold 1e-4."""
    n_cam, n_batches, n = 7, 3, 40
    levels = [20.0 + 2.0 * i for i in range(5)] + [28.0] * 10 + [29.0 + i for i in range(5)] + [33.0] * 20
    losses = torch.tensor([n_batches * 10.0 ** (-p / 10.0) for p in levels], dtype=torch.float64)
    grads = torch.randn(n, n_cam, generator=torch.Generator().manual_seed(9))
    cam = torch.zeros(n_cam, requires_grad=True)
    opt = torch.optim.Adam(params=(cam,), lr=0.5)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, 'max', factor=0.5, patience=3)
    want_lr, want_codes, max_psnr, best_iter = [], [], 0.0, -1
    for i in range(n):
        cam.grad = grads[i].clone()
        want_lr.append(opt.param_groups[0]["lr"])
        opt.step()
        want_codes.append(cam.detach().clone())
        mse = losses[i].float() / n_batches
        p = -10.0 * torch.log(mse) / torch.log(torch.tensor([10.0]))[0]
        sched.step(p)
        if float(p) > max_psnr:
            max_psnr, best_iter = float(p), i
    assert want_lr[-1] <= 0.5 / 4      # halved at least twice
    codes, lrs, psnr, back = _run_updates(P, grads, losses, n_batches, n_cam)
    assert lrs.double().tolist() == want_lr                                                # exactly
    assert back.best_iter == best_iter
    assert float((codes - torch.stack(want_codes)).abs().max()) <= CODE_TOL
    assert float(back.lr) == opt.param_groups[0]["lr"]


# ----------------------------------------------------------------------------- 7. both routes against the fixture
def test_fast_route_matches_the_reference_at_every_recorded_code(P, g, fast):
    l_scale, g_scale = float(g["loss_sum"].max()), float(np.abs(g["grad"]).max())
    worst_l = worst_g = 0.0
    for i in range(g["cam"].shape[0]):
        loss, grad = fast.loss_and_grad(torch.from_numpy(g["cam"][i]))
        worst_l = max(worst_l, abs(loss - float(g["loss_sum"][i])) / l_scale)
        worst_g = max(worst_g, float((grad.cpu() - torch.from_numpy(g["grad"][i])).abs().max()) / g_scale)
    print(f"fast route against the fixture: loss {worst_l:.3e} (bound {LOSS_BOUND:.3e}), gradient {worst_g:.3e} "
          f"(bound {GRAD_BOUND:.3e})")
    assert worst_l <= LOSS_BOUND and worst_g <= GRAD_BOUND


def test_plain_route_matches_the_reference_at_every_recorded_code(P, g, scene):
    Dp, args, kw, pose, intrinsic, image = scene
    H, W = int(g["H"]), int(g["W"])
    l_scale, g_scale = float(g["loss_sum"].max()), float(np.abs(g["grad"]).max())
    worst_l = worst_g = 0.0
    for i in range(g["cam"].shape[0]):
        loss, grad = P.camcode.plain_loss_and_grad(torch.from_numpy(g["cam"][i]), image, pose, H, W, intrinsic, args, kw)
        worst_l = max(worst_l, abs(float(loss) - float(g["loss_sum"][i])) / l_scale)
        worst_g = max(worst_g, float((grad.cpu() - torch.from_numpy(g["grad"][i])).abs().max()) / g_scale)
    print(f"plain route against the fixture: loss {worst_l:.3e} (bound {LOSS_BOUND:.3e}), gradient {worst_g:.3e} "
          f"(bound {GRAD_BOUND:.3e})")
    assert worst_l <= LOSS_BOUND and worst_g <= GRAD_BOUND


def test_fast_route_run_improves_on_the_zero_code(P, g, scene):
    Dp, args, kw, pose, intrinsic, image = scene
    kw = dict(kw)
    record = P.optimize_camera_embedding(image, pose, int(g["H"]), int(g["W"]), intrinsic, args, kw, route="fast")
    assert record["route"] == "fast" and len(record["psnr"]) == 100 and len(record["lr"]) == 100
    assert record["best_psnr"] > record["psnr"][0]                      # strictly better than the code 0 it started from
    assert record["best_psnr"] == max(record["psnr"]) and record["best_iter"] == int(np.argmax(record["psnr"]))
    assert torch.equal(kw["embedded_cam"], record["best_cam"]) and not kw["embedded_cam"].requires_grad
    assert kw["embedded_cam"].shape == (4,) and bool(kw["embedded_cam"].any())
    assert record["lr"][0] == 0.5 and record["lr"][-1] < 0.5
    print(f"fast route: PSNR {record['psnr'][0]:.2f} at the zero code, best {record['best_psnr']:.2f} at iteration "
          f"{record['best_iter']} (the reference's run: {float(g['psnr'][0]):.2f}, {float(g['best_psnr']):.2f} at {int(g['best_iter'])})")
    # auto takes the fast route here; a few plain iterations land on the same first PSNR
    plain = P.optimize_camera_embedding(image, pose, int(g["H"]), int(g["W"]), intrinsic, args, dict(kw), route="plain", n_iters=3)
    assert plain["route"] == "plain" and abs(plain["psnr"][0] - record["psnr"][0]) <= 1e-2


# ----------------------------------------------------------------------------- 8. the hooks
def _two_views(P, g, scene, H, W):
    """Two H x W views of the fixture's networks, each one's target the scene rendered at a non-zero code of its own."""
    Dp, args, kw, pose, _, _ = scene
    poses = torch.stack([pose, P.rays.pose_spherical(75.0, -25.0, 4.0)[:3, :4].to(dev())])
    intrinsic = torch.tensor([W * 0.85, W * 0.8, W / 2 + 0.25, H / 2 - 0.25], device=dev())
    codes = torch.tensor([[0.8, -0.6, 0.5, -0.9], [-0.7, 0.4, 0.9, -0.3]], device=dev())
    with torch.no_grad():
        images = torch.stack([Dp.render(H, W, intrinsic, chunk=args.chunk, c2w=poses[i], **dict(kw, embedded_cam=codes[i]))[0]
                              for i in range(2)])
    intrinsics = torch.stack([intrinsic, intrinsic])
    depths = torch.full((2, H, W, 1), 4.0, device=dev())
    valid = torch.ones(2, H, W, dtype=torch.bool, device=dev())
    return Dp, args, dict(kw), images, depths, valid, poses, intrinsics


def test_render_images_with_metrics_optimises_the_code(P, g, scene):
    """Two 7 x 9 views, not 4 x 6: the frame metrics hold SSIM, whose 7 x 7 window plnerf_eval_metrics (like skimage in the
    reference) refuses on a smaller image -- 7 x 9 is the smallest shape of that aspect the loop can score.  63 pixels at
    N_rand = 6 are five batches of 12, 12, 13, 13, 13: unequal sizes on both routes' weights."""
    H, W = 7, 9
    Dp, args, kw, images, depths, valid, poses, intrinsics = _two_views(P, g, scene, H, W)
    assert sorted(set(P.camcode.batch_sizes(H * W, args.N_rand))) == [12, 13]
    base, _ = Dp.render_images_with_metrics(None, [0, 1], images, depths, valid, poses, H, W, intrinsics, None, args, kw)
    assert not bool(kw["embedded_cam"].any())      # zeros without the flag
    tuned, _ = Dp.render_images_with_metrics(None, [0, 1], images, depths, valid, poses, H, W, intrinsics, None, args, kw,
                                             with_test_time_optimization=True)
    print(f"render_images_with_metrics: psnr {base.get('psnr'):.2f} -> {tuned.get('psnr'):.2f} with the flag")
    assert tuned.get("psnr") >= base.get("psnr")
    assert kw["embedded_cam"].shape == (4,) and bool(kw["embedded_cam"].any()) and not kw["embedded_cam"].requires_grad
    with pytest.raises(NotImplementedError, match="no code to optimise"):
        Dp.render_images_with_metrics(None, [0], images, depths, valid, poses, H, W, intrinsics, None,
                                      Namespace(**dict(vars(args), input_ch_cam=0)), kw, with_test_time_optimization=True)


def test_test_images_samples_optimises_the_code(P, g, scene):
    H, W = int(g["H"]), int(g["W"])      # two 4 x 6 views
    Dp, args, kw, images, depths, valid, poses, intrinsics = _two_views(P, g, scene, H, W)
    base = Dp.test_images_samples(None, [0, 1], images, depths, valid, poses, H, W, intrinsics, None, args, kw)
    tuned = Dp.test_images_samples(None, [0, 1], images, depths, valid, poses, H, W, intrinsics, None, args, kw,
                                   with_test_time_optimization=True)
    assert tuned.total_weight == base.total_weight == 2
    assert math.isfinite(tuned.get("importance_sampling_error"))
    # (the hypotheses are drawn from densities, which the code does not reach: the error is the same number)
    assert abs(tuned.get("importance_sampling_error") - base.get("importance_sampling_error")) <= 1e-6
    assert kw["embedded_cam"].shape == (4,) and bool(kw["embedded_cam"].any())


# ----------------------------------------------------------------------------- 9. guard bands
@pytest.mark.parametrize("case_id,build", cases.all_cases(), ids=[c for c, _ in cases.all_cases()])
def test_no_entry_writes_outside_its_buffers(P, case_id, build):
    C.run_case(P._lib, build(P._lib), dev())
